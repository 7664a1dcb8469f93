"""Speaker encoder of the Qwen3-TTS Base checkpoints on the HIP path (csrc/spk_encoder.hip): reference audio -> log-mel (host) ->
ECAPA-TDNN embedding (device) -- what the reference's talker does for a request that carries `ref_audio`
(Qwen3TTSSpeakerEncoder, qwen3_tts_talker.py:57-239; mel_spectrogram :249-285; _extract_speaker_embedding :1069-1105).

    enc = SpeakerEncoder.from_state_dict(extras, hf_config.speaker_encoder_config)     # checkpoint.load_talker_checkpoint's extras
    emb = enc.encode(log_mel_24k(wav))                                                 # bf16 [enc_dim]

The weights are rounded to bf16 and laid out for the kernels once; `encode` is one C call of ~26 launches on the current stream.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any

import numpy as np
import torch

from . import _lib

BF16 = torch.bfloat16
SAMPLE_RATE = 24000
N_FFT, HOP, N_MELS, FMIN, FMAX = 1024, 256, 128, 0.0, 12000.0       # qwen3_tts_talker.py:1094-1103
_DEFAULTS = dict(mel_dim=128, enc_dim=1024, enc_channels=[512, 512, 512, 512, 1536], enc_kernel_sizes=[5, 3, 3, 3, 1], enc_dilations=[1, 2, 3, 4, 1],
                 enc_attention_channels=128, enc_res2net_scale=8, enc_se_channels=128)      # configuration_qwen3_tts.py:49-69


# ---------------------------------------------------------------- host front end
def slaney_mel_filterbank(sr: int = SAMPLE_RATE, n_fft: int = N_FFT, n_mels: int = N_MELS, fmin: float = FMIN, fmax: float = FMAX) -> torch.Tensor:
    """[n_mels, n_fft / 2 + 1] triangular filters on the Slaney mel scale (linear below 1 kHz, logarithmic above), each scaled
    to unit area (2 / bandwidth) -- the formula behind the filterbank the reference takes from librosa."""
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, math.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp

    def hz_to_mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f < min_log_hz, f / f_sp, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep)

    def mel_to_hz(m):
        m = np.asarray(m, dtype=np.float64)
        return np.where(m < min_log_mel, m * f_sp, min_log_hz * np.exp(logstep * (m - min_log_mel)))

    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fft_f = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    ramps = mel_f[:, None] - fft_f[None, :]
    fdiff = np.diff(mel_f)
    w = np.maximum(0.0, np.minimum(-ramps[:-2] / fdiff[:-1, None], ramps[2:] / fdiff[1:, None]))
    w *= (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]
    return torch.from_numpy(w.astype(np.float32))


def mel_band_centres(n_mels: int = N_MELS, fmin: float = FMIN, fmax: float = FMAX) -> np.ndarray:
    """Centre frequency (Hz) of every filter of slaney_mel_filterbank."""
    fb = slaney_mel_filterbank(n_mels=n_mels, fmin=fmin, fmax=fmax)
    return (fb.argmax(1).numpy() * (SAMPLE_RATE / N_FFT)).astype(np.float64)


def log_mel_frames(num_samples: int) -> int:
    """Frames log_mel_24k returns: the signal is reflect-padded by (n_fft - hop) / 2 per side and framed without centring."""
    return 1 + (num_samples + 2 * ((N_FFT - HOP) // 2) - N_FFT) // HOP


def log_mel_24k(wav) -> torch.Tensor:
    """24 kHz waveform [L] (floats in [-1, 1]) -> fp32 log-mel [T, 128] in the reference's arithmetic (mel_spectrogram): reflect pad,
    torch.stft with a Hann window (n_fft = win = 1024, hop 256, not centred), magnitude sqrt(re^2 + im^2 + 1e-9), mel projection,
    log(clamp(., 1e-5)).  Host code, as in the reference."""
    y = torch.as_tensor(np.asarray(wav, dtype=np.float32) if not isinstance(wav, torch.Tensor) else wav.detach().cpu().float()).reshape(1, -1)
    if y.shape[1] < N_FFT:
        raise ValueError(f"ref_audio waveform too short: {y.shape[1]} samples")
    pad = (N_FFT - HOP) // 2
    y = torch.nn.functional.pad(y.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    spec = torch.stft(y, N_FFT, hop_length=HOP, win_length=N_FFT, window=torch.hann_window(N_FFT), center=False, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True)
    mag = torch.sqrt(torch.view_as_real(spec).pow(2).sum(-1) + 1e-9)
    mel = torch.matmul(slaney_mel_filterbank(), mag)
    return torch.log(torch.clamp(mel, min=1e-5))[0].transpose(0, 1).contiguous()


def normalize_ref_audio(ref_audio: Any) -> tuple[np.ndarray, int]:
    """The request's `ref_audio` -> (mono fp32 waveform, sample rate).  Accepted: (wav, sr) / [wav, sr] (also nested in singleton
    lists), or a dict with array | wav | audio and sampling_rate | sr | sample_rate; wav a numpy array, tensor or list of numbers."""
    x = ref_audio
    while isinstance(x, (list, tuple)) and len(x) == 1:
        x = x[0]
    wav = sr = None
    if isinstance(x, dict):
        wav = next((x[k] for k in ("array", "wav", "audio") if x.get(k) is not None), None)
        sr = next((x[k] for k in ("sampling_rate", "sr", "sample_rate") if x.get(k) is not None), None)
    elif isinstance(x, (list, tuple)) and len(x) == 2:
        a, b = x
        wav, sr = (b, a) if isinstance(a, (int, float)) and not isinstance(b, (int, float)) else (a, b)
    if wav is None or not isinstance(sr, (int, float, np.integer, np.floating)):
        raise TypeError("ref_audio must be a (waveform, sample_rate) pair or a dict with a waveform and a sampling rate")
    wav = wav.detach().cpu().float().numpy() if isinstance(wav, torch.Tensor) else np.asarray(wav, dtype=np.float32)
    return wav.reshape(-1), int(sr)


# ---------------------------------------------------------------- weight layout
def frag_pack(w2d: torch.Tensor, kw: int) -> torch.Tensor:
    """bf16 [N, K] -> the MFMA tile order of include/omni_talker.h (tile (n / 16, k / kw), element ((kk / E) * 16 + row) * E + kk % E)."""
    n, k = w2d.shape
    e = kw // 4
    return w2d.reshape(n // 16, 16, k // kw, 4, e).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)


def conv_matrix(w: torch.Tensor) -> torch.Tensor:
    """torch conv1d weight [N, C_in, k] -> bf16 tile-ordered [N, k * C_in] (K index = tap * C_in + channel)."""
    n, cin, k = w.shape
    return frag_pack(w.to(BF16).permute(0, 2, 1).reshape(n, k * cin), 32 if cin % 32 == 0 else 16)


def _cfg(config: Any) -> dict:
    get = (lambda k: config.get(k)) if isinstance(config, dict) else (lambda k: getattr(config, k, None))
    return {k: (get(k) if config is not None and get(k) is not None else v) for k, v in _DEFAULTS.items()}


class SpeakerEncoder:
    def __init__(self, cfg: dict, tensors: dict, device):
        self.cfg, self.dev, self._t = cfg, torch.device(device), tensors
        self.lib = _lib.load()
        ch = list(cfg["enc_channels"])
        if not 3 <= len(ch) <= _lib.SPK_MAX_LAYERS:
            raise ValueError(f"speaker encoder: {len(ch)} layers (3 .. {_lib.SPK_MAX_LAYERS} supported)")
        self.mel_dim, self.enc_dim, self.C, self.C3 = int(cfg["mel_dim"]), int(cfg["enc_dim"]), int(ch[0]), int(ch[-1])
        d = _lib.SpkDesc()
        d.mel_dim, d.enc_dim, d.layers, d.scale = self.mel_dim, self.enc_dim, len(ch), int(cfg["enc_res2net_scale"])
        d.se_channels, d.att_channels = int(cfg["enc_se_channels"]), int(cfg["enc_attention_channels"])
        for i in range(len(ch)):
            d.channels[i], d.kernels[i], d.dilations[i] = int(ch[i]), int(cfg["enc_kernel_sizes"][i]), int(cfg["enc_dilations"][i])
        p = lambda n: tensors[n].data_ptr()      # noqa: E731
        d.conv0_w, d.conv0_b = p("conv0_w"), p("conv0_b")
        for i in range(len(ch) - 2):
            for n in ("tdnn1_w", "tdnn1_b", "res_w", "res_b", "tdnn2_w", "tdnn2_b", "se1_w", "se1_b", "se2_w", "se2_b"):
                setattr(d.blocks[i], n, p(f"b{i}.{n}"))
        for n in ("mfa_w", "mfa_b", "att_wh", "att_wms", "att_b", "att_conv_w", "att_conv_b", "fc_w", "fc_b"):
            setattr(d, n, p(n))
        self.desc = d
        self._scratch = None

    @classmethod
    def from_state_dict(cls, extras: dict, config: Any = None, device="cuda") -> "SpeakerEncoder":
        """extras: the checkpoint's `speaker_encoder.*` tensors (the prefix is optional); config: Qwen3TTSSpeakerEncoderConfig, a dict
        of its fields, or None for the shipped shapes."""
        cfg = _cfg(config)
        sd = {k[len("speaker_encoder."):] if k.startswith("speaker_encoder.") else k: v for k, v in extras.items()
              if k.startswith("speaker_encoder.") or k.split(".")[0] in ("blocks", "mfa", "asp", "fc")}
        if "blocks.0.conv.weight" not in sd:
            raise ValueError("no speaker_encoder.* tensors in the checkpoint extras: this checkpoint cannot clone a voice from ref_audio")
        dev = torch.device(device)
        up = lambda t, dt: t.detach().to(device=dev, dtype=dt).contiguous()      # noqa: E731
        cm = lambda n: up(conv_matrix(sd[n + ".weight"].detach().float()), BF16)   # noqa: E731
        fb = lambda n: up(sd[n + ".bias"].float(), torch.float32)                  # noqa: E731
        mv = lambda w: up(w.detach().float().squeeze(-1), BF16)                    # noqa: E731
        t = {"conv0_w": cm("blocks.0.conv"), "conv0_b": fb("blocks.0.conv")}
        nl, scale = len(cfg["enc_channels"]), int(cfg["enc_res2net_scale"])
        for i in range(nl - 2):
            b = f"blocks.{i + 1}."
            t[f"b{i}.tdnn1_w"], t[f"b{i}.tdnn1_b"] = cm(b + "tdnn1.conv"), fb(b + "tdnn1.conv")
            t[f"b{i}.tdnn2_w"], t[f"b{i}.tdnn2_b"] = cm(b + "tdnn2.conv"), fb(b + "tdnn2.conv")
            t[f"b{i}.res_w"] = torch.cat([cm(f"{b}res2net_block.blocks.{j}.conv") for j in range(scale - 1)])
            t[f"b{i}.res_b"] = torch.cat([fb(f"{b}res2net_block.blocks.{j}.conv") for j in range(scale - 1)])
            t[f"b{i}.se1_w"], t[f"b{i}.se1_b"] = mv(sd[b + "se_block.conv1.weight"]), fb(b + "se_block.conv1")
            t[f"b{i}.se2_w"], t[f"b{i}.se2_b"] = mv(sd[b + "se_block.conv2.weight"]), fb(b + "se_block.conv2")
        c3 = int(cfg["enc_channels"][-1])
        aw = sd["asp.tdnn.conv.weight"].detach().float()            # [A, 3 C3, 1]: columns [h | mean | std]
        t["mfa_w"], t["mfa_b"] = cm("mfa.conv"), fb("mfa.conv")
        t["att_wh"], t["att_wms"], t["att_b"] = up(conv_matrix(aw[:, :c3]), BF16), mv(aw[:, c3:]), fb("asp.tdnn.conv")
        t["att_conv_w"], t["att_conv_b"] = cm("asp.conv"), fb("asp.conv")
        t["fc_w"], t["fc_b"] = mv(sd["fc.weight"]), fb("fc")
        return cls(cfg, t, dev)

    # ---- calls
    def _scratch_for(self, T: int) -> torch.Tensor:
        need = int(self.lib.omni_spk_scratch_bytes(C.byref(self.desc), T))
        if need < 0:
            _lib.check(need, "omni_spk_scratch_bytes")
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.dev)
        return self._scratch

    def _rows(self, x, width: int) -> torch.Tensor:
        x = torch.as_tensor(x).to(device=self.dev, dtype=BF16).contiguous()
        if x.ndim != 2 or x.shape[1] != width:
            raise ValueError(f"expected [T, {width}], got {tuple(x.shape)}")
        return x

    def encode(self, mel, out: torch.Tensor | None = None) -> torch.Tensor:
        """log-mel [T, mel_dim] -> bf16 [enc_dim] on the device (stream-ordered; `out` for a caller-held buffer)."""
        mel = self._rows(mel, self.mel_dim)
        out = torch.empty(self.enc_dim, dtype=BF16, device=self.dev) if out is None else out
        scratch = self._scratch_for(mel.shape[0])
        _lib.check(self.lib.omni_spk_encode(C.byref(self.desc), mel.data_ptr(), mel.shape[0], out.data_ptr(), scratch.data_ptr(), _lib.current_stream()),
                   "omni_spk_encode")
        return out

    def res2net(self, block: int, x) -> torch.Tensor:
        """The Res2Net stage of SE-Res2Net block `block` (1-based, as config indexes layers) alone: bf16 [T, C] -> bf16 [T, C]."""
        x = self._rows(x, self.C)
        out = torch.empty_like(x)
        t = self._t
        _lib.check(self.lib.omni_spk_res2net(x.data_ptr(), self.C, t[f"b{block - 1}.res_w"].data_ptr(), t[f"b{block - 1}.res_b"].data_ptr(), out.data_ptr(), self.C,
                                             x.shape[0], self.C, self.desc.scale, self.desc.kernels[block], self.desc.dilations[block], _lib.current_stream()),
                   "omni_spk_res2net")
        return out

    def pool(self, h) -> torch.Tensor:
        """Attentive statistics pooling alone: bf16 [T, C3] -> fp32 [2 C3] = [mean | std]."""
        h = self._rows(h, self.C3)
        stats = torch.empty(2 * self.C3, dtype=torch.float32, device=self.dev)
        scratch = self._scratch_for(h.shape[0])
        _lib.check(self.lib.omni_spk_asp(C.byref(self.desc), h.data_ptr(), h.shape[0], stats.data_ptr(), scratch.data_ptr(), _lib.current_stream()), "omni_spk_asp")
        return stats

    def embed_audio(self, ref_audio: Any) -> torch.Tensor:
        """`ref_audio` of a request -> embedding; 24 kHz only."""
        wav, sr = normalize_ref_audio(ref_audio)
        if sr != SAMPLE_RATE:
            raise ValueError(f"ref_audio sample rate {sr} Hz: the speaker encoder takes {SAMPLE_RATE} Hz, resampling is upstream")
        return self.encode(log_mel_24k(wav))
