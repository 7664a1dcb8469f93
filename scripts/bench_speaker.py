#!/usr/bin/env python3
"""A/B of the speaker encoder at the shipped shapes on a 10 s reference (940 frames): the HIP path (speaker.SpeakerEncoder.encode)
against the same network as torch ops in bf16 on the same GPU, and the one-launch Res2Net block against seven windowed conv launches
(omni_spk_conv per stage + a torch add).  Arms alternate in one process; device events around `iters` calls after warm-up.

    python scripts/bench_speaker.py [--frames 940] [--iters 50] [--rounds 5] [--out profiles/speaker_encoder_ab.txt]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ht_vllm_omni_amd import _lib, speaker  # noqa: E402

BF16 = torch.bfloat16
CFG = speaker._DEFAULTS


def state_dict(seed=3, std=0.05):
    g = torch.Generator().manual_seed(seed)
    ch, k, s, a, se = CFG["enc_channels"], CFG["enc_kernel_sizes"], CFG["enc_res2net_scale"], CFG["enc_attention_channels"], CFG["enc_se_channels"]
    shapes = {"blocks.0.conv": (ch[0], CFG["mel_dim"], k[0]), "mfa.conv": (ch[-1], ch[-1], 1), "asp.tdnn.conv": (a, 3 * ch[-1], 1), "asp.conv": (ch[-1], a, 1),
              "fc": (CFG["enc_dim"], 2 * ch[-1], 1)}
    for i in range(1, len(ch) - 1):
        b = f"blocks.{i}."
        shapes.update({b + "tdnn1.conv": (ch[i], ch[i - 1], 1), b + "tdnn2.conv": (ch[i], ch[i], 1), b + "se_block.conv1": (se, ch[i], 1), b + "se_block.conv2": (ch[i], se, 1)})
        shapes.update({f"{b}res2net_block.blocks.{j}.conv": (ch[i] // s, ch[i] // s, k[i]) for j in range(s - 1)})
    sd = {}
    for n, shp in shapes.items():
        sd[n + ".weight"] = (torch.randn(shp, generator=g) * std).to(BF16)
        sd[n + ".bias"] = (torch.randn(shp[0], generator=g) * std).to(BF16)
    return sd


def conv(x, sd, n, d=1, act=F.relu):
    w = sd[n + ".weight"]
    p = d * (w.shape[-1] - 1) // 2
    y = F.conv1d(F.pad(x, (p, p), mode="reflect") if p else x, w, sd[n + ".bias"], dilation=d)
    return act(y) if act else y


def torch_encoder(sd, mel):
    """The reference's forward as torch ops (bf16 tensors on the GPU: what its module runs after .to(bfloat16))."""
    x = conv(mel.T.unsqueeze(0), sd, "blocks.0.conv", CFG["enc_dilations"][0])
    outs = []
    for i in range(1, len(CFG["enc_channels"]) - 1):
        b = f"blocks.{i}."
        h, parts = conv(x, sd, b + "tdnn1.conv"), []
        for j, part in enumerate(torch.chunk(h, CFG["enc_res2net_scale"], 1)):
            if j:
                part = conv(part if j == 1 else part + parts[-1], sd, f"{b}res2net_block.blocks.{j - 1}.conv", CFG["enc_dilations"][i])
            parts.append(part)
        h = conv(torch.cat(parts, 1), sd, b + "tdnn2.conv")
        x = h * conv(conv(h.mean(2, keepdim=True), sd, b + "se_block.conv1"), sd, b + "se_block.conv2", act=torch.sigmoid) + x
        outs.append(x)
    h = conv(torch.cat(outs, 1), sd, "mfa.conv")
    mean = h.mean(2, keepdim=True)
    std = ((h - mean) ** 2).mean(2, keepdim=True).clamp(1e-12).sqrt()
    att = conv(conv(torch.cat([h, mean.expand_as(h), std.expand_as(h)], 1), sd, "asp.tdnn.conv").tanh(), sd, "asp.conv", act=None).softmax(2)
    m = (att * h).sum(2)
    s = (att * (h - m.unsqueeze(2)) ** 2).sum(2).clamp(1e-12).sqrt()
    return conv(torch.cat([m, s], 1).unsqueeze(2), sd, "fc", act=None)[0, :, 0]


def res2net_unfused(enc, block, x, bufs):
    """Seven windowed conv launches + the adds in torch: the intermediate chunks go through HBM."""
    lib, C, s = enc.lib, enc.C, enc.desc.scale
    w = C // s
    wt, bt = enc._t[f"b{block - 1}.res_w"], enc._t[f"b{block - 1}.res_b"]
    k, d, T = enc.desc.kernels[block], enc.desc.dilations[block], x.shape[0]
    out, tmp = bufs
    out[:, :w] = x[:, :w]
    for j in range(1, s):
        src = x[:, j * w:] if j == 1 else tmp
        if j > 1:
            torch.add(x[:, j * w:(j + 1) * w], out[:, (j - 1) * w:j * w], out=tmp)
        _lib.check(lib.omni_spk_conv(src.data_ptr(), C if j == 1 else w, wt.data_ptr() + (j - 1) * w * k * w * 2, bt.data_ptr() + (j - 1) * w * 4,
                                     out.data_ptr() + j * w * 2, C, T, w, w, k, d, _lib.SPK_ACT_RELU, _lib.current_stream()), "omni_spk_conv")
    return out


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters       # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=940)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_speaker.py measures on the GPU: none found")
    sd = state_dict()
    enc = speaker.SpeakerEncoder.from_state_dict({k: v.float() for k, v in sd.items()}, CFG)
    sd_dev = {k: v.cuda() for k, v in sd.items()}
    T, C, s = a.frames, enc.C, enc.desc.scale
    mel = (torch.randn(T, CFG["mel_dim"], generator=torch.Generator().manual_seed(1)) * 2 - 4).to(BF16).cuda()
    x = torch.randn(T, C, generator=torch.Generator().manual_seed(2)).to(BF16).cuda()
    bufs = (torch.empty(T, C, dtype=BF16, device="cuda"), torch.empty(T, C // s, dtype=BF16, device="cuda"))
    out = torch.empty(CFG["enc_dim"], dtype=BF16, device="cuda")
    r2 = (res2net_unfused(enc, 2, x, bufs).float() - enc.res2net(2, x).float()).abs().max()      # the unfused arm rounds y before the add: last-bit differences
    arms = {"encode: HIP path": lambda: enc.encode(mel, out=out), "encode: torch bf16": lambda: torch_encoder(sd_dev, mel),
            "res2net x3: one launch each": lambda: [enc.res2net(b, x) for b in (1, 2, 3)],
            "res2net x3: 7 conv launches each": lambda: [res2net_unfused(enc, b, x, bufs) for b in (1, 2, 3)]}
    with torch.no_grad():
        for fn in arms.values():
            timed(fn, 10)
        res = {n: [] for n in arms}
        for _ in range(a.rounds):
            for n, fn in arms.items():
                res[n].append(timed(fn, a.iters))
    err = (enc.encode(mel).float() - torch_encoder(sd_dev, mel).float()).abs()
    lines = [f"speaker encoder, shipped shapes, T = {T} frames, {a.rounds} alternating rounds x {a.iters} calls, us per call (median [min .. max])"]
    for n, v in res.items():
        v = sorted(v)
        lines.append(f"  {n:36s} {v[len(v) // 2]:9.1f}  [{v[0]:.1f} .. {v[-1]:.1f}]")
    med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
    lines.append(f"  Res2Net kernels' share of the HIP encode: {100 * med['res2net x3: one launch each'] / med['encode: HIP path']:.1f} %")
    lines.append(f"  HBM traffic the one-launch block avoids: {3 * (s - 1) * T * (C // s) * 2 * 2 / 1e6:.2f} MB per encode (7 chunks [T, C / 8] written and re-read, 3 blocks)")
    lines.append(f"  Res2Net arms, block 2: max |diff| {float(r2):.4f}")
    lines.append(f"  HIP vs torch bf16 output: mean |diff| {float(err.mean()):.4f}, max {float(err.max()):.4f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
