#!/usr/bin/env python3
"""Mint tests/golden/speaker_encoder_tiny.npz (authoring container only: needs the reference tree, read in place).

The reference's Qwen3TTSSpeakerEncoder (qwen3_tts_talker.py:183-239) is imported by path with make_fixtures' stubs for the
imports it does not have here, built for a reduced config with seeded weights, and run on a seeded [37, 32] log-mel twice: in
fp32, and in bf16 as the reference deploys it (_extract_speaker_embedding moves the module to bf16).  Only data is saved: the
state dict (bf16 bit patterns as uint16), the mel, both outputs and the config's fields.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf  # noqa: E402

CFG = dict(mel_dim=32, enc_dim=64, enc_channels=[128, 128, 128, 128, 384], enc_kernel_sizes=[5, 3, 3, 3, 1], enc_dilations=[1, 2, 3, 4, 1],
           enc_attention_channels=32, enc_res2net_scale=8, enc_se_channels=32)


def main():
    mf.install_auto_stubs()
    pkg = "refq3tts_spk_pkg"
    pm = types.ModuleType(pkg)
    pm.__path__ = [os.path.join(mf.V, "model_executor/models/qwen3_tts")]
    sys.modules[pkg] = pm
    mf._stub(pkg + ".qwen3_tts_tokenizer", Qwen3TTSTokenizer=object)
    mod = mf.load_by_path(pkg + ".qwen3_tts_talker", os.path.join(pm.__path__[0], "qwen3_tts_talker.py"), package=pkg)
    cfgm = sys.modules[pkg + ".configuration_qwen3_tts"]
    torch.manual_seed(2024)
    enc = mod.Qwen3TTSSpeakerEncoder(cfgm.Qwen3TTSSpeakerEncoderConfig(**CFG)).eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in enc.parameters():      # weights on the bf16 grid (the checkpoint's dtype); biases large enough to matter
            p.copy_((torch.randn(p.shape, generator=g) * (0.08 if p.ndim == 3 else 0.05)).bfloat16().float())
        mel = (torch.randn(37, CFG["mel_dim"], generator=g) * 2.0 - 4.0).bfloat16().float()      # log-mel-like range, on the bf16 grid
        out32 = enc(mel.unsqueeze(0))[0]
        sd = {k: v.clone() for k, v in enc.state_dict().items()}
        out16 = enc.to(torch.bfloat16)(mel.unsqueeze(0).bfloat16())[0].float()
    arrays = {"sd." + k: mf.np16(v.bfloat16()) for k, v in sd.items()}      # bf16 bit patterns (the values are on that grid)
    arrays.update(mel=mel.numpy(), out_fp32=out32.numpy(), out_bf16=out16.numpy())
    arrays.update({"cfg." + k: np.asarray(v) for k, v in CFG.items()})
    path = os.path.join(HERE, "speaker_encoder_tiny.npz")
    np.savez_compressed(path, **arrays)
    d = (out16 - out32).abs()
    print("speaker_encoder_tiny.npz", os.path.getsize(path), "bytes; bf16 module vs fp32 module: mean abs", float(d.mean()), "max abs", float(d.max()),
          "; |out| mean", float(out32.abs().mean()))


if __name__ == "__main__":
    main()
