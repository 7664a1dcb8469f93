"""Speaker encoder on the HIP path (ht_vllm_omni_amd.speaker, csrc/spk_encoder.hip) against a plain torch functional reference of
the reference's ECAPA-TDNN (qwen3_tts_talker.py:57-239) in float64.

End to end the yardstick is the reference's own deployment: its module in bf16 against its module in fp32 (recorded in the fixture at
minting time; computed here on the CPU with the same functional reference in bf16 for the other shapes).  The HIP path keeps fp32 between
stored tensors, so it has fewer rounding points: mean |error| <= the yardstick's mean, max |error| <= 2 x the yardstick's max (a maximum
over enc_dim values is a single-sample statistic).

Per kernel the float64 reference rounds to bf16 exactly where the kernel stores (`rnd`), so what is left is (a) the rounding of the
output itself, (b) fp32 against float64 accumulation, (c) a stored bf16 operand that rounded the other way because of (b):
  Res2Net, per output y (bf16) over K = k * w products of |w| <= wmax, |in| <= xmax:
      |got - ref| <= 2^-7 |ref|              one bf16 ulp at the output's magnitude (8 significant bits)
                   + K 2^-22 wmax xmax        K fp32 accumulation steps, each <= 2^-24 of a partial sum <= K wmax xmax / 4 .. (4 x margin)
                   + 2^-7 wmax xmax           one operand of the window one ulp off (an operand flips with probability ~1e-4)
  pooling (fp32 output, h bf16 [T, C], attention width A): a logit deviates by at most d = 3 * 2^-8 wcmax (up to three of a row's A tanh
  values, |tanh| < 1 so ulp <= 2^-8, rounded the other way) + A 2^-24 wcmax; softmax weights then move by a factor e^(+-2d), so
      |mean - ref| <= 2 d hmax + T 2^-23 hmax,     |std^2 - ref^2| <= 2 hmax x that bound (d(var) = 2 (x - mean) d(mean) + ...).
An indexing error (wrong tap, wrong mirror row, stale halo row, wrong channel) moves outputs by O(xmax), far outside either bound.
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
F64, BF16 = torch.float64, torch.bfloat16
SHIPPED = dict(mel_dim=128, enc_dim=1024, enc_channels=[512, 512, 512, 512, 1536], enc_kernel_sizes=[5, 3, 3, 3, 1], enc_dilations=[1, 2, 3, 4, 1],
               enc_attention_channels=128, enc_res2net_scale=8, enc_se_channels=128)
TILE = 64                                   # the Res2Net kernel's time tile (R2_TT)
TS = [9, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
rnd = lambda t: t.to(BF16).to(t.dtype)      # noqa: E731


# ---------------------------------------------------------------- the reference (any dtype; x is [1, C, T])
def conv(x, w, b, d=1, act=F.relu):
    p = d * (w.shape[-1] - 1) // 2
    y = F.conv1d(F.pad(x, (p, p), mode="reflect") if p else x, w, b, dilation=d)
    return act(y) if act else y


def res2net(x, sd, pre, scale, d, rnd=lambda t: t):
    outs = []
    for i, part in enumerate(torch.chunk(x, scale, 1)):
        if i:
            part = conv(part if i == 1 else rnd(part + outs[-1]), sd[f"{pre}blocks.{i - 1}.conv.weight"], sd[f"{pre}blocks.{i - 1}.conv.bias"], d)
        outs.append(part)
    return torch.cat(outs, 1)


def asp(h, sd, rnd=lambda t: t, eps=1e-12):
    mean = h.mean(2, keepdim=True)
    std = ((h - mean) ** 2).mean(2, keepdim=True).clamp(eps).sqrt()
    att = rnd(conv(torch.cat([h, mean.expand_as(h), std.expand_as(h)], 1), sd["asp.tdnn.conv.weight"], sd["asp.tdnn.conv.bias"]).tanh())
    a = conv(att, sd["asp.conv.weight"], sd["asp.conv.bias"], act=None).softmax(2)
    m = (a * h).sum(2)
    return torch.cat([m, (a * (h - m.unsqueeze(2)) ** 2).sum(2).clamp(eps).sqrt()], 1)


def encoder(sd, cfg, mel, dtype):
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x = conv(mel.to(dtype).T.unsqueeze(0), sd["blocks.0.conv.weight"], sd["blocks.0.conv.bias"], cfg["enc_dilations"][0])
    outs = []
    for i in range(1, len(cfg["enc_channels"]) - 1):
        b = f"blocks.{i}."
        h = conv(x, sd[b + "tdnn1.conv.weight"], sd[b + "tdnn1.conv.bias"])
        h = res2net(h, sd, b + "res2net_block.", cfg["enc_res2net_scale"], cfg["enc_dilations"][i])
        h = conv(h, sd[b + "tdnn2.conv.weight"], sd[b + "tdnn2.conv.bias"])
        g = conv(conv(h.mean(2, keepdim=True), sd[b + "se_block.conv1.weight"], sd[b + "se_block.conv1.bias"]), sd[b + "se_block.conv2.weight"],
                 sd[b + "se_block.conv2.bias"], act=torch.sigmoid)
        x = h * g + x
        outs.append(x)
    h = conv(torch.cat(outs, 1), sd["mfa.conv.weight"], sd["mfa.conv.bias"])
    return conv(asp(h, sd).unsqueeze(2), sd["fc.weight"], sd["fc.bias"], act=None)[0, :, 0].double()


# ---------------------------------------------------------------- weights and shared references
def seeded_state_dict(cfg, seed=3, std=0.05):
    g = torch.Generator().manual_seed(seed)
    ch, k, s = cfg["enc_channels"], cfg["enc_kernel_sizes"], cfg["enc_res2net_scale"]
    shapes = {"blocks.0.conv": (ch[0], cfg["mel_dim"], k[0]), "mfa.conv": (ch[-1], ch[-1], 1), "asp.tdnn.conv": (cfg["enc_attention_channels"], 3 * ch[-1], 1),
              "asp.conv": (ch[-1], cfg["enc_attention_channels"], 1), "fc": (cfg["enc_dim"], 2 * ch[-1], 1)}
    for i in range(1, len(ch) - 1):
        b = f"blocks.{i}."
        shapes.update({b + "tdnn1.conv": (ch[i], ch[i - 1], 1), b + "tdnn2.conv": (ch[i], ch[i], 1), b + "se_block.conv1": (cfg["enc_se_channels"], ch[i], 1),
                       b + "se_block.conv2": (ch[i], cfg["enc_se_channels"], 1)})
        shapes.update({f"{b}res2net_block.blocks.{j}.conv": (ch[i] // s, ch[i] // s, k[i]) for j in range(s - 1)})
    sd = {}
    for n, shp in shapes.items():
        sd[n + ".weight"] = (torch.randn(shp, generator=g) * std).to(BF16).float()
        sd[n + ".bias"] = (torch.randn(shp[0], generator=g) * std).to(BF16).float()
    return sd


@functools.lru_cache(maxsize=None)
def model(name):
    if name == "shipped":
        return SHIPPED, seeded_state_dict(SHIPPED), None
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "speaker_encoder_tiny.npz"))
    cfg = {k[4:]: z[k].tolist() for k in z.files if k.startswith("cfg.")}
    sd = {k[3:]: torch.from_numpy(z[k].view(np.int16)).view(BF16).float() for k in z.files if k.startswith("sd.")}
    return cfg, sd, z


@functools.lru_cache(maxsize=None)
def hip_encoder(name):
    from ht_vllm_omni_amd.speaker import SpeakerEncoder
    cfg, sd, _ = model(name)
    return SpeakerEncoder.from_state_dict({"speaker_encoder." + k: v for k, v in sd.items()}, cfg)


def seeded(shape, seed, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale + shift).to(BF16)


@functools.lru_cache(maxsize=None)
def e2e_case(name, T):
    """(mel, float64 output, the bf16 deployment's mean / max deviation from it)"""
    cfg, sd, _ = model(name)
    mel = seeded((T, cfg["mel_dim"]), 100 + T, 2.0, -4.0)
    ref = encoder(sd, cfg, mel, F64)
    dep = (encoder(sd, cfg, mel, BF16) - ref).abs()
    return mel, ref, float(dep.mean()), float(dep.max())


def check_e2e(got, ref, y_mean, y_max, what):
    err = (got.double().cpu() - ref).abs()
    print(f"{what}: mean |err| {float(err.mean()):.5f} (yardstick {y_mean:.5f}), max |err| {float(err.max()):.5f} (yardstick {y_max:.5f})")
    assert float(err.mean()) <= y_mean and float(err.max()) <= 2 * y_max, what


# ---------------------------------------------------------------- tests
def test_reference_equals_the_reference_module():
    """The float64 functional reference reproduces the fixture's fp32 module output to fp32 rounding: ~12 layers of up to 1152-term fp32
    sums, each within K * 2^-24 of exact relative to the output scale -> 2e-4 of max |out|."""
    cfg, sd, z = model("tiny")
    ref = encoder(sd, cfg, torch.from_numpy(z["mel"]), F64)
    out = torch.from_numpy(z["out_fp32"]).double()
    assert float((ref - out).abs().max()) <= 2e-4 * float(out.abs().max())


@gpu
def test_encode_fixture_within_the_deployments_error():
    cfg, sd, z = model("tiny")
    ref = encoder(sd, cfg, torch.from_numpy(z["mel"]), F64)
    dep = np.abs(z["out_bf16"].astype(np.float64) - z["out_fp32"])
    check_e2e(hip_encoder("tiny").encode(torch.from_numpy(z["mel"])), ref, float(dep.mean()), float(dep.max()), "fixture")


@gpu
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", ["tiny", "shipped"])
def test_encode_matches_reference(name, T):
    mel, ref, y_mean, y_max = e2e_case(name, T)
    check_e2e(hip_encoder(name).encode(mel), ref, y_mean, y_max, f"{name} T={T}")


@gpu
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("block", [1, 2, 3])            # dilations 2, 3, 4
@pytest.mark.parametrize("name", ["tiny", "shipped"])   # w = 16 (16-deep MFMA) and w = 64
def test_res2net_kernel(name, block, T):
    cfg, sd, _ = model(name)
    C, scale, k = cfg["enc_channels"][block], cfg["enc_res2net_scale"], cfg["enc_kernel_sizes"][block]
    x = seeded((T, C), 7 * T + block)
    pre = f"blocks.{block}.res2net_block."
    ref = rnd(res2net(x.double().T.unsqueeze(0), {n: v.double() for n, v in sd.items() if n.startswith(pre)}, pre, scale, cfg["enc_dilations"][block], rnd))[0].T
    got = hip_encoder(name).res2net(block, x).double().cpu()
    wmax = max(float(v.abs().max()) for n, v in sd.items() if n.startswith(pre))
    xmax = float(torch.maximum(ref.abs().max(), x.double().abs().max())) * 2          # an input of a stage is x chunk + the previous output
    K = k * C // scale
    tol = ref.abs() * 2.0 ** -7 + wmax * xmax * (K * 2.0 ** -22 + 2.0 ** -7)
    bad = (got - ref).abs() > tol
    assert not bad.any(), f"{int(bad.sum())} elements off, first at (t, c) = {bad.nonzero()[0].tolist()}, max |err| {float((got - ref).abs().max()):.4f}"


@gpu
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", ["tiny", "shipped"])
def test_pooling_kernel(name, T):
    cfg, sd, _ = model(name)
    C, A = cfg["enc_channels"][-1], cfg["enc_attention_channels"]
    h = F.relu(seeded((T, C), 11 * T)).to(BF16)
    ref = asp(h.double().T.unsqueeze(0), {n: v.double() for n, v in sd.items() if n.startswith("asp.")}, rnd)[0]
    got = hip_encoder(name).pool(h).double().cpu()
    hmax, wcmax = float(h.double().abs().max()), float(sd["asp.conv.weight"].abs().max())
    tol = hmax * (2 * (3 * 2.0 ** -8 * wcmax + A * 2.0 ** -24 * wcmax) + T * 2.0 ** -23)
    assert float((got[:C] - ref[:C]).abs().max()) <= tol, "weighted mean"
    assert float((got[C:] ** 2 - ref[C:] ** 2).abs().max()) <= 2 * hmax * tol, "weighted variance"


@gpu
def test_deterministic_and_graph_safe():
    enc, (mel, *_) = hip_encoder("tiny"), e2e_case("tiny", 3 * TILE + 5)
    mel = mel.cuda()
    a, b = enc.encode(mel).clone(), enc.encode(mel).clone()
    assert torch.equal(a, b), "two calls, different bits"
    out = torch.empty_like(a)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enc.encode(mel, out=out)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a), "graph replay differs from the eager call"


@gpu
def test_base_request_with_ref_audio_builds_the_same_prompt():
    from ht_vllm_omni_amd.prompt_builder_tts import TTSPromptIds, TTSTalkerPromptBuilder
    from ht_vllm_omni_amd.speaker import log_mel_24k
    enc, H = hip_encoder("shipped"), SHIPPED["enc_dim"]
    w = {"text_embedding": seeded((96, 64), 1, 0.5), "codec_embed": seeded((80, H), 2, 0.5), "cp_embed": seeded((3, 40, H), 3, 0.5),
         "text_projection": {"fc1_w": seeded((64, 64), 4, 0.2), "fc1_b": seeded((64,), 5, 0.1), "fc2_w": seeded((H, 64), 6, 0.2), "fc2_b": seeded((H,), 7, 0.1)}}
    ids = TTSPromptIds(tts_bos=90, tts_eos=91, tts_pad=92, codec_nothink=60, codec_think=61, codec_think_bos=62, codec_think_eos=63, codec_pad=64, codec_bos=65)
    wav = (0.3 * torch.sin(torch.arange(6000) * 0.05) + 0.05 * seeded((6000,), 8).float()).numpy()
    info = {"task_type": "Base", "x_vector_only_mode": True, "input_ids": [1, 2, 3, 10, 11, 12, 13, 4, 3, 1, 2, 3], "ref_audio": (wav, 24000)}
    p = TTSTalkerPromptBuilder(w, ids, "cuda", speaker_encoder=enc).from_info(info)
    passed = dict(info, voice_clone_prompt={"ref_spk_embedding": enc.encode(log_mel_24k(wav))})
    passed.pop("ref_audio")
    q = TTSTalkerPromptBuilder(w, ids, "cuda").from_info(passed)
    assert torch.equal(p.embeds, q.embeds) and torch.equal(p.trailing_text_hidden, q.trailing_text_hidden) and torch.equal(p.tts_pad, q.tts_pad)
    with pytest.raises(ValueError, match="the speaker encoder runs upstream"):
        TTSTalkerPromptBuilder(w, ids, "cuda").from_info(info)
