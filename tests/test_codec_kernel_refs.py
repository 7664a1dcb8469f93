"""tests/codec_kernel_refs.py against the project's existing oracle, so that a wrong reference cannot pass a wrong kernel
(tests/test_gpu_codec_kernels.py compares every Code2Wav kernel with these references).  oracle/code2wav_oracle.py is fp32 and
is itself pinned to the reference module's outputs (tests/test_code2wav_oracle.py); the references are fp64, so each comparison
holds to fp32 rounding of sums of at most a few thousand terms: 1e-5 of the tensor's largest magnitude.  Where the oracle's
configurations do not reach (GQA, head_dim 128) the attention reference is held to a literal triple loop instead."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle.code2wav_oracle import Code2WavOracle
from tests import codec_kernel_refs as R
from tests.codec_util import MID_CODEC, TINY_CODEC, make_codec_state

CFGS = {"tiny": TINY_CODEC, "mid": MID_CODEC}
both = pytest.mark.parametrize("size", ["tiny", "mid"])


@functools.lru_cache(maxsize=None)
def _oracle(size):
    return Code2WavOracle(CFGS[size], make_codec_state(CFGS[size], 5))


def _close(ref64, oracle32, what):
    scale = oracle32.abs().max().item()
    err = (ref64 - oracle32.double()).abs().max().item()
    assert ref64.shape == oracle32.shape, what
    assert err <= 1e-5 * scale, f"{what}: max |ref - oracle| {err:.3g} at a scale of {scale:.3g}"


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@both
def test_rmsnorm_is_the_oracles(size):
    orc = _oracle(size)
    H = orc.cfg["hidden_size"]
    x = _randn(11, H, seed=1) * 3.0
    name = "pre_transformer.layers.0.input_layernorm"
    _close(R.ref_rmsnorm(x, orc.sd[name + ".weight"], orc.cfg["rms_norm_eps"]), orc.rms_norm(x, name), "rmsnorm")


@both
def test_dwconv_ln_is_the_front_of_the_oracles_convnext(size):
    orc = _oracle(size)
    C = orc.cfg["latent_dim"]
    p = "upsample.0.1."
    x = _randn(19, C, seed=2)                                                # [T, C]: rows 0..5 see the zero padding
    y = orc.causal_conv(x.T.contiguous(), p + "dwconv", groups=C).T          # the first two lines of Code2WavOracle.convnext
    want = F.layer_norm(y, (C,), orc.sd[p + "norm.weight"], orc.sd[p + "norm.bias"], 1e-6)
    w = orc.sd[p + "dwconv.conv.weight"][:, 0]                               # [C, 7], the layout code2wav.py uploads
    got = R.ref_dwconv_ln(x, w, orc.sd[p + "dwconv.conv.bias"], orc.sd[p + "norm.weight"], orc.sd[p + "norm.bias"], 1e-6, w.shape[1])
    _close(got, want, "dwconv_ln")
    _close(got[:6], want[:6], "dwconv_ln, padded rows")


@both
def test_out_conv_is_causal_conv_plus_clamp(size):
    orc = _oracle(size)
    n = len(orc.cfg["upsample_rates"])
    name = f"decoder.{n + 2}"
    wt = orc.sd[name + ".conv.weight"]                                       # [1, C, 7]
    x = _randn(50, wt.shape[1], seed=3) * 4.0                                # some samples saturate
    want = orc.causal_conv(x.T.contiguous(), name)[0].clamp(min=-1, max=1)
    got = R.ref_out_conv(x, wt[0].T, float(orc.sd[name + ".conv.bias"][0]), wt.shape[2])
    assert 0 < int((want.abs() == 1).sum()) < want.numel()
    _close(got, want, "out_conv")


@both
def test_rvq_embed_is_quantizer_decode(size):
    orc = _oracle(size)
    c = orc.cfg
    Q, bins = c["num_quantizers"], c["codebook_size"]
    codes = torch.randint(0, bins, (Q, 9), generator=torch.Generator().manual_seed(4))
    tabs = []                                                                # the fold of code2wav.py::_build, restated
    for q in range(Q):
        part, i = ("rvq_first", 0) if q == 0 else ("rvq_rest", q - 1)
        p = f"quantizer.{part}.vq.layers.{i}._codebook."
        emb = orc.sd[p + "embedding_sum"].double() / orc.sd[p + "cluster_usage"].double().clamp(min=1e-5)[:, None]
        tabs.append((emb @ orc.sd[f"quantizer.{part}.output_proj.weight"].double()[:, :, 0].T).float())
    table = torch.stack(tabs)
    _close(R.ref_rvq_embed(codes, table).T, orc.quantizer_decode(codes), "rvq_embed")
    # out-of-range codes read the first / last entry
    wild = codes.clone()
    wild[0, 0], wild[1, 1] = -1, bins
    tame = codes.clone()
    tame[0, 0], tame[1, 1] = 0, bins - 1
    assert torch.equal(R.ref_rvq_embed(wild, table), R.ref_rvq_embed(tame, table))


@both
def test_rope_and_window_attn_are_the_oracles_attention(size):
    """Same q, k, v on both sides: the oracle projects x with its q / k / v weights, the references get those products packed as
    qkv rows; o_proj is the identity, so the oracle returns what it computed in front of it."""
    orc = _oracle(size)
    c = orc.cfg
    H, nh, nkv = c["hidden_size"], c["num_attention_heads"], c["num_key_value_heads"]
    hd = H // nh
    assert nkv == nh and hd == 64
    T = c["sliding_window"] + 9                                              # past the window
    p = "pre_transformer.layers.0.self_attn."
    x = _randn(T, H, seed=6)
    eye = Code2WavOracle(c, {**orc.sd, p + "o_proj.weight": torch.eye(H)})
    want = eye.attention(x, p)
    qkv = torch.cat([x @ orc.sd[p + f"{n}_proj.weight"].T for n in "qkv"], 1)
    pad = torch.full((T, 8), 7.0)                                            # a pad behind the packed row: carried, never read
    rot = R.ref_rope(torch.cat([qkv, pad], 1), nh, nkv, hd, c["rope_theta"])
    assert torch.equal(rot[:, (nh + nkv) * hd:], torch.cat([qkv[:, (nh + nkv) * hd:], pad], 1).double()), "v heads and pad unchanged"
    assert torch.equal(rot[0], torch.cat([qkv, pad], 1)[0].double()), "row 0: angle 0"
    got = R.ref_window_attn(rot, nh, nkv, hd, c["sliding_window"], hd ** -0.5)
    _close(got, want, "rope + window_attn")


def _loop_attn(qkv, nh, nkv, hd, window, scale):
    T = qkv.shape[0]
    out = torch.zeros(T, nh * hd, dtype=torch.float64)
    for t in range(T):
        for h in range(nh):
            g = h // (nh // nkv)
            q = qkv[t, h * hd:(h + 1) * hd]
            js = [j for j in range(T) if 0 <= t - j < window]
            sc = [scale * float(q @ qkv[j, (nh + g) * hd:(nh + g + 1) * hd]) for j in js]
            m = max(sc)
            e = [math.exp(v - m) for v in sc]
            for j, w in zip(js, e):
                out[t, h * hd:(h + 1) * hd] += w / sum(e) * qkv[j, (nh + nkv + g) * hd:(nh + nkv + g + 1) * hd]
    return out


@pytest.mark.parametrize("nh,nkv,hd", [(4, 2, 64), (4, 1, 64), (2, 2, 128), (4, 1, 128), (6, 2, 64)])
def test_window_attn_with_gqa_and_wide_heads_is_a_literal_loop(nh, nkv, hd):
    T, window = 9, 4
    qkv = _randn(T, (nh + 2 * nkv) * hd + 8, seed=nh * 100 + nkv * 10 + hd).double()
    got = R.ref_window_attn(qkv, nh, nkv, hd, window, hd ** -0.5)
    want = _loop_attn(qkv, nh, nkv, hd, window, hd ** -0.5)
    assert (got - want).abs().max().item() <= 1e-12
    # the window's edges, sharply: a key just outside does not count, a key just inside does
    t = 6
    far = qkv.clone()
    far[t - window, nh * hd:] = 1e3
    assert torch.equal(R.ref_window_attn(far, nh, nkv, hd, window, hd ** -0.5)[t], got[t])
    near = qkv.clone()
    near[t - window + 1, (nh + nkv) * hd:] += 1.0
    assert not torch.equal(R.ref_window_attn(near, nh, nkv, hd, window, hd ** -0.5)[t], got[t])


@pytest.mark.parametrize("hd", [64, 128])
def test_rope_rotates_every_q_and_k_head_by_the_same_angles(hd):
    T, qh, kh = 5, 3, 2
    qkv = _randn(T, (qh + 2 * kh) * hd, seed=hd).double()
    got = R.ref_rope(qkv, qh, kh, hd, 10000.0)
    for t in range(T):
        for h in range(qh + kh):
            for d in range(hd // 2):
                a = t * 10000.0 ** (-2.0 * d / hd)
                x1, x2 = float(qkv[t, h * hd + d]), float(qkv[t, h * hd + d + hd // 2])
                assert abs(float(got[t, h * hd + d]) - (x1 * math.cos(a) - x2 * math.sin(a))) <= 1e-12
                assert abs(float(got[t, h * hd + d + hd // 2]) - (x2 * math.cos(a) + x1 * math.sin(a))) <= 1e-12
    assert torch.equal(got[:, (qh + kh) * hd:], qkv[:, (qh + kh) * hd:])


@both
@pytest.mark.parametrize("dilation", [1, 3, 9])
def test_res_unit_is_the_oracles_residual_unit(size, dilation):
    """The unit of Code2WavOracle.forward, h + conv2(snake(conv1(snake(h)))) with s = snake(h) given: without the bf16 points it is
    the fp32 oracle's; with them the 1x1 conv's operand and s_next are bf16 values and nothing moves by more than that rounding."""
    orc = _oracle(size)
    q = "decoder.1.block.2."
    W1, W2 = orc.sd[q + "conv1.conv.weight"], orc.sd[q + "conv2.conv.weight"]
    C = W1.shape[0]
    T = 6 * dilation + 7                                                     # rows inside and past the causal halo
    h = _randn(T, C, seed=7 + dilation)
    s = _randn(T, C, seed=8 + dilation)
    t = orc.causal_conv(s.T.contiguous(), q + "conv1", dilation=dilation)
    want_h = h.T + orc.causal_conv(orc.snake(t, q + "act2"), q + "conv2")
    want_s = orc.snake(want_h, q + "act1")
    sn2 = R.snake_params(orc.sd[q + "act2.alpha"], orc.sd[q + "act2.beta"])
    snn = R.snake_params(orc.sd[q + "act1.alpha"], orc.sd[q + "act1.beta"])
    args = (s, h, W1, orc.sd[q + "conv1.conv.bias"], sn2, W2, orc.sd[q + "conv2.conv.bias"], snn, dilation)
    got_h, got_s = R.ref_res_unit(*args, bf16=False)
    _close(got_h.T, want_h, "res_unit h")
    _close(got_s.T, want_s, "res_unit s_next")
    rh, rs, parts = R.ref_res_unit(*args, parts=True)
    assert torch.equal(parts["u"], R.bf16_round(parts["u"])) and torch.equal(rs, R.bf16_round(rs))
    bound = 2.0 ** -8 * (parts["u"].abs() @ W2[:, :, 0].double().abs().T)
    assert bool(((rh - got_h).abs() <= bound + 1e-12).all()) and float((rh - got_h).abs().max()) > 0
