"""Prompt-embedding builder of the Qwen3-TTS talker (VERDICT r1 missing #4): request -> the talker's prefill
embeddings, its queue of per-step text embeddings (`tailing_text_hidden`) and `tts_pad_embed`.

Mirrors `Qwen3TTSTalkerForConditionalGeneration._build_prompt_embeds` / `_generate_icl_prompt`
(/root/reference/vllm_omni/model_executor/models/qwen3_tts/qwen3_tts_talker.py:1160-1209, 1211-1567) for the three task types
(CustomVoice, VoiceDesign, Base incl. x-vector-only and in-context voice cloning), streaming and non-streaming text, language
tags with the dialect override, and the instruct prefix.  MI355X shape of it: every token id that needs the text projection
(instruct, role header, text, reference text, the three TTS markers) is gathered into ONE batch and goes through
`omni_resize_mlp` once (the reference runs up to six small projection chains per request); the codec rows are table gathers,
the in-context codec sum is accumulated in fp32 in group order on the device; assembly is row slicing.  A row's projection
does not depend on its batch mates, so the outputs are the reference's.

Out of scope, and taken as inputs: the text tokenizer (a checkpoint asset: pass token ids, or a `tokenize` callable) and
the reference-audio codec of in-context voice cloning (pass `ref_code`).  The speaker embedding of a Base request is either passed
(`ref_spk_embedding`) or computed from `ref_audio` by the builder's `speaker_encoder` (speaker.SpeakerEncoder, 24 kHz audio;
qwen3_tts_talker.py:1376-1386).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Callable

import numpy as np
import torch

from . import ops

BF16 = torch.bfloat16


@dataclass(frozen=True)
class TTSPromptIds:
    """Token ids the builder keys on: Qwen3TTSConfig.tts_*_token_id and Qwen3TTSTalkerConfig.codec_* / codec_language_id /
    spk_id / spk_is_dialect (configuration_qwen3_tts.py:376-409; a checkpoint's config.json overrides the defaults)."""
    tts_bos: int
    tts_eos: int
    tts_pad: int
    codec_nothink: int = 4203
    codec_think: int = 4202
    codec_think_bos: int = 4204
    codec_think_eos: int = 4205
    codec_pad: int = 4196
    codec_bos: int = 4197
    language_ids: dict = field(default_factory=dict)      # codec_language_id: language name (lower case) -> codec token id
    speaker_ids: dict = field(default_factory=dict)       # spk_id: voice name -> codec token id
    spk_is_dialect: dict = field(default_factory=dict)    # voice name (lower case) -> dialect language name

    @classmethod
    def from_hf_config(cls, cfg: Any) -> "TTSPromptIds":
        tc = cfg.talker_config
        return cls(tts_bos=cfg.tts_bos_token_id, tts_eos=cfg.tts_eos_token_id, tts_pad=cfg.tts_pad_token_id,
                   codec_nothink=tc.codec_nothink_id, codec_think=tc.codec_think_id, codec_think_bos=tc.codec_think_bos_id,
                   codec_think_eos=tc.codec_think_eos_id, codec_pad=tc.codec_pad_id, codec_bos=tc.codec_bos_id,
                   language_ids=dict(getattr(tc, "codec_language_id", None) or {}), speaker_ids=dict(getattr(tc, "spk_id", None) or {}),
                   spk_is_dialect=dict(getattr(tc, "spk_is_dialect", None) or {}))


@dataclass
class TTSPrompt:
    embeds: torch.Tensor                 # bf16 [P, H] (device)
    trailing_text_hidden: torch.Tensor   # bf16 [T, H] (device)
    tts_pad: torch.Tensor                # bf16 [1, H] (device)
    ref_code_len: int | None = None
    ref_code: torch.Tensor | None = None


def _first(x: Any) -> Any:
    return (x[0] if x else None) if isinstance(x, list) else x


def assistant_text(text: str) -> str:      # qwen3_tts_talker.py:670-680
    return f"<|im_start|>assistant\n{text}<|im_end|>\n<|im_start|>assistant\n"


def ref_text(text: str) -> str:
    return f"<|im_start|>assistant\n{text}<|im_end|>\n"


def instruct_text(instruct: str) -> str:
    return f"<|im_start|>user\n{instruct}<|im_end|>\n"


class TTSTalkerPromptBuilder:
    def __init__(self, weights: dict, ids: TTSPromptIds, device: str | torch.device = "cuda", tokenize: Callable[[str], list[int]] | None = None,
                 speaker_encoder=None):
        """weights: {"text_embedding" [Vt, Ht], "text_projection" {fc1_w, fc1_b, fc2_w, fc2_b}, "codec_embed" [V, H] (the talker's
        codec embedding = engine `embed`), "cp_embed" [Q-1, Vc, H]} -- checkpoint.load_talker_checkpoint's extras / weights."""
        self.dev = torch.device(device)
        up = lambda t: t.to(device=self.dev, dtype=BF16).contiguous()      # noqa: E731
        self.text_embedding = up(weights["text_embedding"])
        self.w_proj = {k: up(v) for k, v in weights["text_projection"].items()}
        self.codec_embed = up(weights["codec_embed"])
        self.cp_embed = up(weights["cp_embed"])
        self.ids, self.tokenize, self.speaker_encoder = ids, tokenize, speaker_encoder
        self.hidden = int(self.codec_embed.shape[1])

    @classmethod
    def from_checkpoint(cls, extras: dict, codec_embed: torch.Tensor, cp_embed: torch.Tensor, ids: TTSPromptIds, device="cuda", tokenize=None,
                        speaker_encoder_config: Any = None) -> "TTSTalkerPromptBuilder":
        """The builder over checkpoint.load_talker_checkpoint's extras: the text tables, and -- where the checkpoint ships
        `speaker_encoder.*` tensors (the Base variants) -- the speaker encoder, so that a Base request may carry `ref_audio`."""
        tp = "text_projection.linear_fc"
        w = {"text_embedding": extras["text_embedding.weight"], "codec_embed": codec_embed, "cp_embed": cp_embed,
             "text_projection": {"fc1_w": extras[tp + "1.weight"], "fc1_b": extras[tp + "1.bias"], "fc2_w": extras[tp + "2.weight"], "fc2_b": extras[tp + "2.bias"]}}
        enc = None
        if any(k.startswith("speaker_encoder.") for k in extras):
            from .speaker import SpeakerEncoder
            enc = SpeakerEncoder.from_state_dict(extras, speaker_encoder_config, device)
        return cls(w, ids, device, tokenize, speaker_encoder=enc)

    # ---- request-level resolution (talker.py:1254-1269, 1458-1466, 1226-1230)
    def resolve(self, task_type: str, info: dict) -> dict:
        language = _first(info.get("language")) or "Auto"
        language_id = None
        if isinstance(language, str) and language.lower() != "auto":
            language_id = self.ids.language_ids.get(language.lower())
        speaker_id = None
        if task_type == "CustomVoice":
            spk = str(_first(info.get("speaker")) or "").lower().strip()
            if not spk:
                raise ValueError("CustomVoice requires additional_information.speaker.")
            table = {k.lower(): v for k, v in self.ids.speaker_ids.items()}
            if spk not in table:
                raise ValueError(f"Unsupported speaker: {spk}")
            speaker_id = int(table[spk])
            if language_id is None and isinstance(language, str) and language.lower() in ("chinese", "auto"):
                dialect = self.ids.spk_is_dialect.get(spk)
                if isinstance(dialect, str) and dialect:
                    language_id = self.ids.language_ids.get(dialect)
        nsm = _first(info.get("non_streaming_mode"))
        return dict(language_id=language_id, speaker_id=speaker_id, non_streaming_mode=nsm if isinstance(nsm, bool) else None)

    def from_info(self, info: dict) -> TTSPrompt:
        """The request's additional_information -> prompt (the keys preprocess reads, talker.py:530-560); text fields are
        tokenised with `tokenize`, or arrive tokenised as `input_ids` / `instruct_ids` / `ref_ids`."""
        task = _first(info.get("task_type")) or "CustomVoice"
        kw = self.resolve(task, info)

        def ids_of(key_ids, key_text, template):
            v = info.get(key_ids)
            if v is not None:
                return [int(t) for t in (v.tolist() if hasattr(v, "tolist") else v)]
            txt = _first(info.get(key_text))
            if isinstance(txt, str) and txt.strip():
                if self.tokenize is None:
                    raise ValueError(f"{key_text} given as text but the builder has no tokenizer: pass {key_ids}")
                return list(self.tokenize(template(txt)))
            return None

        input_ids = ids_of("input_ids", "text", assistant_text)
        if not input_ids:
            raise ValueError("Missing additional_information.text for Qwen3-TTS AR talker.")
        vcp = _first(info.get("voice_clone_prompt"))
        vcp = vcp if isinstance(vcp, dict) else {}
        xvec_only = bool(_first(info.get("x_vector_only_mode")) or False)
        icl = not xvec_only
        if isinstance(_first(vcp.get("icl_mode")), bool):
            icl = _first(vcp.get("icl_mode"))
        ref_code = _first(vcp.get("ref_code"))
        spk = vcp.get("ref_spk_embedding")
        if task == "Base":
            ref_audio = info.get("ref_audio")
            if spk is None and self.speaker_encoder is not None and ref_audio is not None:
                spk = self.speaker_encoder.embed_audio(ref_audio)      # 24 kHz only: any other rate is a ValueError (resampling is upstream)
            if spk is None:
                raise ValueError("Base requires a speaker embedding (voice_clone_prompt.ref_spk_embedding): the speaker encoder runs upstream")
            if icl and ref_code is None:
                raise ValueError("Base in-context voice cloning requires voice_clone_prompt.ref_code: the audio codec runs upstream")
        return self.build(task, input_ids, speaker_embed=spk, instruct_ids=ids_of("instruct_ids", "instruct", instruct_text),
                          ref_ids=ids_of("ref_ids", "ref_text", ref_text) if task == "Base" and icl else None,
                          ref_code=ref_code if task == "Base" and icl else None, in_context_mode=task == "Base" and icl, **kw)

    # ---- id-level builder
    def build(self, task_type: str, input_ids, *, language_id=None, speaker_id=None, speaker_embed=None, instruct_ids=None,
              ref_ids=None, ref_code=None, in_context_mode: bool = False, non_streaming_mode: bool | None = None) -> TTSPrompt:
        ids, dev = self.ids, self.dev
        if task_type not in ("CustomVoice", "VoiceDesign", "Base"):
            raise ValueError(f"Unsupported task_type={task_type}")
        if non_streaming_mode is None:
            non_streaming_mode = task_type in ("CustomVoice", "VoiceDesign")
        a = [int(t) for t in input_ids]
        if len(a) < 9:
            raise ValueError("assistant template too short: <|im_start|>assistant\\n + text + 5 closing tokens expected")
        icl = task_type == "Base" and in_context_mode
        # ---- ONE projection batch: [instruct | tts markers | role header | (ref text) text]
        ins = [int(t) for t in instruct_ids] if instruct_ids is not None and len(instruct_ids) else []
        body = a[3:-5]
        if icl:
            r = [int(t) for t in (ref_ids.tolist() if hasattr(ref_ids, "tolist") else ref_ids)]
            r = r[0] if r and isinstance(r[0], list) else r
            body = r[3:-2] + body
        batch = ins + [ids.tts_bos, ids.tts_eos, ids.tts_pad] + a[:3] + body
        rows = self.text_embedding[torch.as_tensor(batch, dtype=torch.long, device=dev)]
        proj = ops.resize_mlp(rows.contiguous(), self.w_proj)
        o = len(ins)
        ins_e, tts_bos, tts_eos, tts_pad = proj[:o], proj[o:o + 1], proj[o + 1:o + 2], proj[o + 2:o + 3]
        role, text_e = proj[o + 3:o + 6], proj[o + 6:]
        emb = lambda t: self.codec_embed[torch.as_tensor(t, dtype=torch.long, device=dev)]     # noqa: E731
        pre = ([ids.codec_nothink, ids.codec_think_bos, ids.codec_think_eos] if language_id is None
               else [ids.codec_think, ids.codec_think_bos, int(language_id), ids.codec_think_eos])
        parts = [emb(pre)]
        if task_type == "Base":
            se = speaker_embed if isinstance(speaker_embed, torch.Tensor) else torch.as_tensor(np.asarray(speaker_embed, dtype=np.float32))
            parts.append(se.to(device=dev, dtype=BF16).reshape(1, -1))
        elif task_type == "CustomVoice":
            if speaker_id is None:
                raise ValueError("CustomVoice requires a speaker id")
            parts.append(emb([int(speaker_id)]))
        parts.append(emb([ids.codec_pad, ids.codec_bos]))
        codec_input = torch.cat(parts, 0)
        n = codec_input.shape[0]
        add = lambda x, y: (x.float() + y.float()).to(BF16)              # noqa: E731  bf16 tensor add
        prefix = add(torch.cat([tts_pad.expand(n - 2, -1), tts_bos], 0), codec_input[:-1])
        prompt = [role, prefix]
        ref_len, ref_t = None, None
        if icl:
            ref_t = torch.as_tensor(np.asarray(ref_code.cpu() if isinstance(ref_code, torch.Tensor) else ref_code), dtype=torch.long, device=dev)
            if ref_t.ndim == 3:
                ref_t = ref_t[0]
            ref_len = int(ref_t.shape[0])
            text_embed = torch.cat([text_e, tts_eos], 0)
            # codec rows: embed(code 0) + sum of the group embeddings, fp32 accumulate in group order, one rounding
            acc = emb(ref_t[:, 0]).float()
            for i in range(1, ref_t.shape[1]):
                acc = acc + self.cp_embed[i - 1][ref_t[:, i]].float()
            codec_sum = torch.cat([emb([ids.codec_bos]), acc.to(BF16)], 0)
            tl, cl = text_embed.shape[0], codec_sum.shape[0]
            if non_streaming_mode:
                prompt += [add(text_embed, emb([ids.codec_pad] * tl)), add(codec_sum, tts_pad)]
                trailing = tts_pad
            elif tl > cl:
                prompt.append(add(text_embed[:cl], codec_sum))
                trailing = text_embed[cl:]
            else:
                prompt.append(add(torch.cat([text_embed, tts_pad.expand(cl - tl, -1)], 0), codec_sum))
                trailing = tts_pad
        elif non_streaming_mode:
            text_all = torch.cat([text_e, tts_eos], 0)
            prompt += [add(text_all, emb([ids.codec_pad] * text_all.shape[0])), add(tts_pad, emb([ids.codec_bos]))]
            trailing = tts_pad
        else:
            prompt.append(add(text_e[:1], codec_input[-1:]))
            trailing = torch.cat([text_e[1:], tts_eos], 0)
        if o:
            prompt = [ins_e] + prompt
        return TTSPrompt(embeds=torch.cat(prompt, 0).contiguous(), trailing_text_hidden=trailing.contiguous(), tts_pad=tts_pad.contiguous(),
                         ref_code_len=ref_len, ref_code=None if ref_t is None else ref_t.cpu())
