"""The Code2Wav kernels one by one (csrc/codec.hip: rvq_embed, rmsnorm, rope, window_attn, dwconv_ln, out_conv; csrc/conv_unit.hip:
res_unit) through the ctypes bindings, against the fp64 references of tests/codec_kernel_refs.py (pinned to the oracle by
tests/test_codec_kernel_refs.py) -- at the shapes, leading dimensions, head layouts and lengths the whole-decoder tests
(tests/test_gpu_code2wav.py) never drive: head_dim 128, GQA, ld wider than the row, channel counts off the block stride, T below /
at / one past a block, a window edge, dilations 2 and 5.  Inputs are seeded; the references get the uploaded bf16 / fp32 values
widened exactly, so only the kernel's own arithmetic is measured.

Tolerances, elementwise, from the number formats (2^-8 |v| bounds the rounding of v to bf16; fp32 sums of n terms err by a few
2^-24 of the sum of the terms' magnitudes), not from what the kernels give.  Every test prints its worst error as a fraction of
its tolerance; the first run on an MI355X is under "Measured" below.
  rvq_embed    2^-8 |ref| + 2^-20 sum_q |table entry|                                    (<= 16 fp32 terms)
  rmsnorm      2^-8 |ref| + 1e-6 |w| max|x| rstd
  rope         (2^-8 + A(t, d)) (|x1| + |x2|): A bounds the error of cos / sin.  t < 256: A = t 2^-20 (fp32 t * inv and a few
               ulps of inv).  t >= 256: A = 2 E32(t, d), E32 = the distance from the fp64 cos / sin of the reference model's fp32
               formulation (inv_freq = 1 / theta^(2d/hd), t * inv_freq, cos, sin, all fp32 torch on the CPU); the factor 2 covers
               exp2f against pow rounding the same quantity differently.  Row 0, v heads and pad columns: bit-identical.
  window_attn  2^-8 |ref| + 1e-4 max|v| over the window (a convex combination of v rows; fp32 dots and __expf at scores of O(1))
  dwconv_ln    2^-8 (|n ln_w| + |ln_b|) + 1e-5 |ln_w| rstd sum_j |w_j x_j|               (n the normalised value)
  out_conv     1e-5 sum |w x|; saturated samples exactly +-1
  res_unit     h: 2^-8 sum_c |W2[n, c] u_c| + 1e-5 S.  u = bf16(snake2(conv7)) is the unit's one rounding; S = the absolute
               products of both convs: sum_c |W2[n, c]| (|u_c| + D_c sum |W1 s|_c) + |b2| + |h|, D = 1 + a / b the snake's slope.
               s_next: one bf16 ulp (2^-7 |ref|: both sides are rounded) + the h bound times the snake's slope 1 + |sin(2 a h)| a / b.

Measured on an MI355X, worst case over each kernel's cases: error / tolerance, and for bf16 outputs how many elements are not the
fp64 reference rounded to bf16 (rounding alone takes up to all of the 2^-8 |ref| term, so the count is the sharper figure):
  rvq_embed    0.991   0 of 13 112 elements off the rounded reference
  rmsnorm      0.991   0 of 9 688
  rope         0.973   8 536 of 1 062 016 (nearly all in the T = 8000 case).  Against the fp32 formulation: no element at t >= 256
               left the bf16 term, so (error - 2^-8 (|x1| + |x2|)) / (E32 (|x1| + |x2|)) is 0 of the allowed 2; largest E32 3.0e-4.
  window_attn  0.944   294 of 1 330 560
  dwconv_ln    0.984   171 of 21 952
  out_conv     0.012
  res_unit     h 0.110, s_next 0.668 (434 of 1 124 736 off the rounded reference); halo rows and block-end rows no worse than others
With the window start moved to t - window, the 30 test_window_attn cases with T > window, all of test_window_attn_edge_of_the_window
and all of test_window_attn_of_one_key_is_the_v_row fail; with the depthwise conv's padding test `r > 0`, all six test_dwconv_ln cases.
"""
import ctypes as C
import functools
import math

import pytest
import torch

from tests import codec_kernel_refs as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"
EPS8 = 2.0 ** -8


@functools.lru_cache(maxsize=None)
def _api():
    from ht_vllm_omni_amd import _lib as L
    return L, L.load()


def _stream():
    return _api()[0].current_stream()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed, std=1.0):
    return torch.randn(*shape, generator=_gen(seed)) * std


def _guarded(rows, cols, dtype, fill, guard=3):
    """A device tensor of rows + guard rows filled with `fill`: the kernel gets the first `rows`; the rest must survive."""
    return torch.full((rows + guard, cols), fill, dtype=dtype, device=DEV)


def _untouched(full, rows, fill, what):
    assert bool((full[rows:] == fill).all()), f"{what}: rows past T were written"


def _assert_within(what, got, ref, tol, groups=None):
    """|got - ref| <= tol elementwise; prints the worst error as a fraction of the tolerance (overall and per named row group)
    and names the worst element and its group on failure."""
    err = (got.detach().double().cpu() - ref).abs()
    assert err.shape == tol.shape, (what, err.shape, tol.shape)
    assert bool(torch.isfinite(err).all()), f"{what}: non-finite output"
    frac = torch.where(err <= tol, err / tol.clamp_min(1e-300), torch.full_like(err, float("inf")))
    frac = torch.where((err == 0) & (tol == 0), torch.zeros_like(frac), frac)
    worst = float(frac.max())
    msg = f"{what}: worst error / tolerance {min(worst, 1e9):.3f}"
    if got.dtype == BF16:          # rounding alone uses up to all of 2^-8 |ref|: the sharper figure is how often the kernel rounds elsewhere
        msg += f" ({int((got.detach().double().cpu() != R.bf16_round(ref)).sum())} of {err.numel()} elements off the rounded reference)"
    bad = []
    for name, rows in (groups or {}).items():
        if rows.numel() and bool(rows.any()):
            w = float(frac[rows].max())
            msg += f"; {name} {min(w, 1e9):.3f}"
            if w > 1.0:
                bad.append(name)
    print(msg)
    if worst > 1.0:
        i, idx = int(torch.argmax((err - tol).flatten())), ()
        for n in reversed(err.shape):
            i, r = divmod(i, n)
            idx = (r,) + idx
        raise AssertionError(f"{msg}; {int((err > tol).sum())} of {err.numel()} elements out, worst at {idx}: got "
                             f"{float(got.detach().double().cpu()[idx]):.6g}, ref {float(ref[idx]):.6g}, tolerance {float(tol[idx]):.3g}"
                             + (f"; failing row groups: {bad}" if groups else ""))
    return worst


# ---------------------------------------------------------------------------------------------------------------- rvq_embed
def _rvq(codes_dev, ld, table_dev, T, Q, bins, Cc):
    out = _guarded(T, Cc, BF16, 9.0)
    rc = _api()[1].omni_codec_rvq_embed(codes_dev.data_ptr(), ld, table_dev.data_ptr(), out.data_ptr(), T, Q, bins, Cc, _stream())
    assert rc == 0, _api()[1].omni_last_error()
    torch.cuda.synchronize()
    _untouched(out, T, 9.0, "rvq_embed")
    return out[:T]


@pytest.mark.parametrize("Q,bins,Cc,T,how", [(1, 8, 4, 1, "plain"), (16, 64, 64, 13, "slice"), (16, 32, 1020, 5, "wild"),
                                             (4, 16, 1024, 3, "plain"), (16, 16, 2052, 2, "wild")])
def test_rvq_embed(Q, bins, Cc, T, how):
    """64 threads below C = 1024, 256 at and above it, C off 4 * blockDim; codes as a column slice of a wider tensor (ld_codes > T);
    codes -1 and `bins` read entries 0 and bins - 1."""
    table = _randn(Q, bins, Cc, seed=Cc + T)
    codes = torch.randint(0, bins, (Q, T), generator=_gen(Q * 7 + T))
    if how == "wild":
        codes[0, 0], codes[Q - 1, T - 1] = -1, bins
    table_dev = table.to(DEV)
    if how == "slice":
        wide = torch.randint(0, bins, (Q, 40), generator=_gen(1))
        wide[:, 5:5 + T] = codes
        view = wide.to(DEV)[:, 5:5 + T]
        got = _rvq(view, 40, table_dev, T, Q, bins, Cc)
    else:
        got = _rvq(codes.to(DEV), T, table_dev, T, Q, bins, Cc)
    ref = R.ref_rvq_embed(codes, table)
    tol = EPS8 * ref.abs() + 2.0 ** -20 * R.ref_rvq_embed(codes, table.abs())
    _assert_within(f"rvq_embed {Q, bins, Cc, T, how}", got, ref, tol)
    if how == "wild":
        tame = codes.clamp(0, bins - 1)
        assert torch.equal(got, _rvq(tame.to(DEV), T, table_dev, T, Q, bins, Cc)), "clamped codes read entries 0 and bins - 1"


def test_rvq_embed_rejects_a_channel_count_off_the_vector_width():
    out = torch.full((2, 6), 9.0, dtype=BF16, device=DEV)
    codes, table = torch.zeros(2, 2, dtype=torch.long, device=DEV), torch.zeros(2, 4, 6, device=DEV)
    rc = _api()[1].omni_codec_rvq_embed(codes.data_ptr(), 2, table.data_ptr(), out.data_ptr(), 2, 2, 4, 6, _stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"omni_codec_rvq_embed" in _api()[1].omni_last_error() and bool((out == 9.0).all())


# ---------------------------------------------------------------------------------------------------------------- rmsnorm
@pytest.mark.parametrize("T,H,ldx", [(1, 4, 4), (5, 260, 264), (4, 256, 256), (7, 1024, 1024), (3, 64, 128)])
def test_rmsnorm(T, H, ldx):
    """One wave per row, 4 rows per block: T off the block, H off the wave's 256-column stride, ldx > H with the pad poisoned, a
    row of zeros (exactly 0 out) and a row with one element of 1e4."""
    eps = 1e-5
    x = torch.full((T, ldx), 1e30)
    x[:, :H] = _randn(T, H, seed=H + T, std=2.0)
    if T >= 3:
        x[1, :H] = 0.0
        x[2, H // 2] = 1e4
    w = 1.0 + _randn(H, seed=H, std=0.1)
    out = _guarded(T, H, BF16, 9.0)
    x_dev, w_dev = x.to(DEV), w.to(DEV)
    rc = _api()[1].omni_codec_rmsnorm(x_dev.data_ptr(), ldx, w_dev.data_ptr(), eps, out.data_ptr(), T, H, _stream())
    assert rc == 0, _api()[1].omni_last_error()
    torch.cuda.synchronize()
    _untouched(out, T, 9.0, "rmsnorm")
    xs = x[:, :H].double()
    ref = R.ref_rmsnorm(xs, w, eps)
    rstd = torch.rsqrt(xs.pow(2).mean(-1, keepdim=True) + eps)
    tol = EPS8 * ref.abs() + 1e-6 * w.double().abs() * xs.abs().amax(-1, keepdim=True) * rstd
    _assert_within(f"rmsnorm {T, H, ldx}", out[:T], ref, tol)
    if T >= 3:
        assert bool((out[1] == 0).all()), "a row of zeros: rstd = eps^-1/2, output exactly 0"


# ---------------------------------------------------------------------------------------------------------------- rope
@pytest.mark.parametrize("T,qh,kh,hd,ld", [(1, 1, 1, 64, 192), (37, 4, 2, 64, 520), (37, 4, 1, 128, 768), (8000, 1, 1, 64, 192)])
def test_rope(T, qh, kh, hd, ld):
    theta, half, nrot = 10000.0, hd // 2, (qh + kh) * hd
    x = _randn(T, ld, seed=T + hd).to(BF16)
    dev = x.clone().to(DEV)                                                  # rotated in place
    rc = _api()[1].omni_codec_rope(dev.data_ptr(), ld, T, qh, kh, hd, theta, _stream())
    assert rc == 0, _api()[1].omni_last_error()
    torch.cuda.synchronize()
    got = dev.cpu()
    assert torch.equal(got[0].view(torch.int16), x[0].view(torch.int16)), "row 0 (angle 0) must be bit-identical to its input"
    assert torch.equal(got[:, nrot:].view(torch.int16), x[:, nrot:].view(torch.int16)), "v heads and pad columns must be bit-identical"
    ref = R.ref_rope(x, qh, kh, hd, theta)[:, :nrot]
    # the reference model's fp32 formulation of cos / sin, and its distance from fp64
    inv32 = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    ang32 = torch.arange(T, dtype=torch.float32)[:, None] * inv32[None]
    ang64 = R.rope_angles(T, hd, theta)
    e32 = torch.maximum((ang32.cos().double() - ang64.cos()).abs(), (ang32.sin().double() - ang64.sin()).abs())     # [T, half]
    t = torch.arange(T, dtype=torch.float64)[:, None]
    A = torch.where(t < 256, t * 2.0 ** -20, 2.0 * e32)
    xs = x[:, :nrot].double().reshape(T, qh + kh, 2, half)
    mag = (xs[:, :, 0].abs() + xs[:, :, 1].abs())[:, :, None, :].expand(T, qh + kh, 2, half)                         # |x1| + |x2|
    tol = ((EPS8 + A[:, None, None, :]) * mag).reshape(T, nrot)
    _assert_within(f"rope {T, qh, kh, hd, ld}", got[:, :nrot], ref, tol)
    if T > 256:
        err = (got[:, :nrot].double() - ref).abs().reshape(T, qh + kh, 2, half)
        over = (err - EPS8 * mag).clamp_min(0.0)[256:]
        allow = (e32[:, None, None, :] * mag)[256:]
        used = torch.where(over > 0, over / allow.clamp_min(1e-300), torch.zeros_like(over))
        print(f"rope: largest (error - bf16 rounding) / E32 over rows >= 256: {float(used.max()):.3f} (allowed 2); "
              f"max E32 {float(e32.max()):.3g}")


# ---------------------------------------------------------------------------------------------------------------- window_attn
HEADS = [(2, 2, 64), (4, 2, 64), (4, 1, 64), (2, 2, 128), (4, 1, 128)]
SPANS = [(1, 72), (5, 72), (72, 72), (73, 72), (200, 72), (70, 1), (130, 64), (130, 65), (200, 130), (64, 64)]
OUT_FILL, QKV_POISON = -77.0, 1e30


def _qkv(T, nh, nkv, hd, wide, seed):
    """q, k, v ~ N(0, 1) in bf16, packed [T, ld]; `wide`: ld 8 past the packed row, the pad poisoned."""
    packed = (nh + 2 * nkv) * hd
    x = torch.full((T, packed + (8 if wide else 0)), QKV_POISON).to(BF16)
    x[:, :packed] = _randn(T, packed, seed=seed).to(BF16)
    return x


def _attn(qkv_dev, T, nh, nkv, hd, window, wide):
    """Launches on a device qkv; returns the [T, nh * hd] output (device) after checking the output's pad columns survived."""
    ldo = nh * hd + (8 if wide else 0)
    out = torch.full((T, ldo), OUT_FILL, dtype=BF16, device=DEV)
    rc = _api()[1].omni_codec_window_attn(qkv_dev.data_ptr(), qkv_dev.stride(0), out.data_ptr(), ldo, T, nh, nkv, hd, window,
                                          hd ** -0.5, _stream())
    assert rc == 0, _api()[1].omni_last_error()
    torch.cuda.synchronize()
    assert bool((out[:, nh * hd:] == OUT_FILL).all()), "the output's pad columns were written"
    return out[:, :nh * hd]


def _attn_tol(x, ref, nh, nkv, hd, window):
    """2^-8 |ref| + 1e-4 max|v| over the query's window, per (t, head)."""
    T = x.shape[0]
    v = x[:, (nh + nkv) * hd:(nh + 2 * nkv) * hd].double().reshape(T, nkv, hd).abs().amax(-1)                       # [T, nkv]
    vmax = torch.stack([v[max(0, t - window + 1):t + 1].amax(0) for t in range(T)])                                  # [T, nkv]
    vmax = vmax[:, torch.arange(nh) // (nh // nkv)]                                                                   # [T, nh]
    return EPS8 * ref.abs() + 1e-4 * vmax[:, :, None].expand(T, nh, hd).reshape(T, nh * hd)


@pytest.mark.parametrize("hi", range(len(HEADS)), ids=[f"nh{a}-nkv{b}-hd{c}" for a, b, c in HEADS])
@pytest.mark.parametrize("si", range(len(SPANS)), ids=[f"T{a}-w{b}" for a, b in SPANS])
def test_window_attn(hi, si):
    """T below, at and past the window; window 1; the 64-key chunk at exactly one chunk, one chunk plus one key and three chunks;
    head_dim 64 and 128; GQA; in half of the cases ld and ldo wider than the packed rows."""
    (nh, nkv, hd), (T, window) = HEADS[hi], SPANS[si]
    wide = (hi + si) % 2 == 1
    x = _qkv(T, nh, nkv, hd, wide, seed=100 * hi + si)
    got = _attn(x.to(DEV), T, nh, nkv, hd, window, wide)
    ref = R.ref_window_attn(x, nh, nkv, hd, window, hd ** -0.5)
    _assert_within(f"window_attn {HEADS[hi]} {SPANS[si]} wide={wide}", got, ref, _attn_tol(x, ref, nh, nkv, hd, window))


def _aligned_key(x, t, h, hd):
    """64 q_t / |q_t| of query head h: a key whose score, 64 |q_t| hd^-0.5, buries every N(0, 1) key's."""
    q = x[t, h * hd:(h + 1) * hd].double()
    return (64.0 * q / q.norm()).to(BF16)


@pytest.mark.parametrize("nh,nkv,hd", HEADS)
@pytest.mark.parametrize("T,window", [(200, 72), (130, 64)])
def test_window_attn_edge_of_the_window(nh, nkv, hd, T, window):
    """Sharp, not a matter of tolerance: a key just outside the window (t - window), aligned with the query and carrying v = 1000,
    must not move the output; the same key just inside (t - window + 1) must own it.  Per query head, on its kv head."""
    x = _qkv(T, nh, nkv, hd, True, seed=T + nh + hd)
    base = x.to(DEV)
    ref = R.ref_window_attn(x, nh, nkv, hd, window, hd ** -0.5)
    tol = _attn_tol(x, ref, nh, nkv, hd, window)
    for t in sorted({window - 1, window, window + 63, T - 1}):
        for h in range(nh):
            g = h // (nh // nkv)
            cols = slice(h * hd, (h + 1) * hd)
            for j, inside in ((t - window, False), (t - window + 1, True)):
                if j < 0:
                    continue
                y = base.clone()
                y[j, (nh + g) * hd:(nh + g + 1) * hd] = _aligned_key(x, t, h, hd).to(DEV)
                y[j, (nh + nkv + g) * hd:(nh + nkv + g + 1) * hd] = 1000.0
                got = _attn(y, T, nh, nkv, hd, window, True)[t, cols].double().cpu()
                if inside:
                    assert bool(((got - 1000.0).abs() <= 10.0).all()), \
                        f"t={t} head {h}: key t - window + 1 = {j} is inside the window, output {float(got.min()):.4g}..{float(got.max()):.4g}"
                else:
                    bad = (got - ref[t, cols]).abs() > tol[t, cols]
                    assert not bool(bad.any()), \
                        f"t={t} head {h}: key t - window = {j} is outside the window, output up to {float(got.abs().max()):.4g}"


@pytest.mark.parametrize("nh,nkv,hd", HEADS)
@pytest.mark.parametrize("T,window", [(200, 72), (130, 64)])
def test_window_attn_is_causal(nh, nkv, hd, T, window):
    """Overwriting every k and v row behind t with aligned keys and v = 1000 leaves row t bit-identical."""
    x = _qkv(T, nh, nkv, hd, False, seed=T + nh + hd + 1)
    base = x.to(DEV)
    want = _attn(base, T, nh, nkv, hd, window, False)
    for t in (0, 62, 63, window, T - 2):
        y = base.clone()
        for g in range(nkv):
            y[t + 1:, (nh + g) * hd:(nh + g + 1) * hd] = _aligned_key(x, t, g * (nh // nkv), hd).to(DEV)
        y[t + 1:, (nh + nkv) * hd:] = 1000.0
        got = _attn(y, T, nh, nkv, hd, window, False)
        assert torch.equal(got[:t + 1].view(torch.int16), want[:t + 1].view(torch.int16)), f"rows <= {t} changed with rows > {t}"


@pytest.mark.parametrize("nh,nkv,hd", HEADS)
def test_window_attn_of_one_key_is_the_v_row(nh, nkv, hd):
    """window = 1: softmax over one key is 1, the output is the bf16 v row of the mapped kv head bit for bit (the GQA map and the
    per-lane value stride, exactly)."""
    T = 70
    x = _qkv(T, nh, nkv, hd, True, seed=nh + hd)
    got = _attn(x.to(DEV), T, nh, nkv, hd, 1, True).cpu()
    for h in range(nh):
        g = h // (nh // nkv)
        v = x[:, (nh + nkv + g) * hd:(nh + nkv + g + 1) * hd]
        assert torch.equal(got[:, h * hd:(h + 1) * hd].view(torch.int16), v.view(torch.int16)), f"head {h} is not v head {g}"


@pytest.mark.parametrize("nh,nkv,hd,pad,what", [(2, 2, 96, 0, "head_dim"), (3, 2, 64, 0, "bad shape"), (2, 2, 64, 4, "ld=")])
def test_window_attn_rejections(nh, nkv, hd, pad, what):
    T = 4
    ld = (nh + 2 * nkv) * hd + pad
    x = torch.zeros(T, ld + 8, dtype=BF16, device=DEV)
    out = torch.full((T, nh * hd), OUT_FILL, dtype=BF16, device=DEV)
    rc = _api()[1].omni_codec_window_attn(x.data_ptr(), ld, out.data_ptr(), nh * hd, T, nh, nkv, hd, 8, 0.125, _stream())
    torch.cuda.synchronize()
    assert rc != 0 and what.encode() in _api()[1].omni_last_error() and bool((out == OUT_FILL).all())


# ---------------------------------------------------------------------------------------------------------------- dwconv_ln
def _dwconv(x, ldx, w, b, ln_w, ln_b, eps, T, Cc, taps):
    out = _guarded(T, Cc, BF16, 9.0)
    d = [v.to(DEV).contiguous() for v in (x, w, b, ln_w, ln_b)]
    rc = _api()[1].omni_codec_dwconv_ln(d[0].data_ptr(), ldx, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), eps,
                                        out.data_ptr(), T, Cc, taps, _stream())
    assert rc == 0, _api()[1].omni_last_error()
    torch.cuda.synchronize()
    _untouched(out, T, 9.0, "dwconv_ln")
    return out[:T]


def _dwconv_check(what, x, ldx, w, b, ln_w, ln_b, T, Cc, taps, eps=1e-6):
    got = _dwconv(x, ldx, w, b, ln_w, ln_b, eps, T, Cc, taps)
    ref, p = R.ref_dwconv_ln(x[:, :Cc], w, b, ln_w, ln_b, eps, taps, parts=True)
    tol = EPS8 * ((p["n"] * ln_w.double()).abs() + ln_b.double().abs()) + 1e-5 * ln_w.double().abs() * p["rstd"] * p["abs_sum"]
    rows = torch.arange(T)
    _assert_within(what, got, ref, tol, {f"rows t < {taps - 1} (zero padding)": rows < taps - 1, "rows past the padding": rows >= taps - 1})
    return got, tol


@pytest.mark.parametrize("T,Cc,taps,ldx", [(1, 64, 7, 64), (3, 256, 7, 256), (20, 300, 7, 304), (9, 1024, 7, 1024), (9, 128, 1, 128),
                                           (9, 128, 3, 160)])
def test_dwconv_ln(T, Cc, taps, ldx):
    """T below the tap count, C off the 256-thread stride and at its limit, 1 and 3 taps, ldx > C with the pad poisoned."""
    x = torch.full((T, ldx), 1e30)
    x[:, :Cc] = _randn(T, Cc, seed=T + Cc)
    w = _randn(Cc, taps, seed=Cc + taps, std=1 / math.sqrt(taps))
    b = _randn(Cc, seed=1, std=0.02)
    ln_w, ln_b = 1.0 + _randn(Cc, seed=2, std=0.1), _randn(Cc, seed=3, std=0.05)
    _dwconv_check(f"dwconv_ln {T, Cc, taps, ldx}", x, ldx, w, b, ln_w, ln_b, T, Cc, taps)


def test_dwconv_ln_of_a_signal_constant_over_channels_is_the_layernorm_bias():
    """No variance over the channels: eps rules rstd, the normalised value is ~0 and the output is ln_b."""
    T, Cc, taps = 12, 300, 7
    x = _randn(T, 1, seed=5).expand(T, Cc).contiguous()
    w = _randn(1, taps, seed=6, std=0.4).expand(Cc, taps).contiguous()
    b = torch.full((Cc,), 0.03)
    ln_w, ln_b = 1.0 + _randn(Cc, seed=2, std=0.1), _randn(Cc, seed=3, std=0.05)
    got, tol = _dwconv_check("dwconv_ln, constant over channels", x, Cc, w, b, ln_w, ln_b, T, Cc, taps)
    assert bool(((got.double().cpu() - ln_b.double()).abs() <= tol).all())


def test_dwconv_ln_rejects_more_channels_than_a_block_holds():
    z = torch.zeros(2, 1025, device=DEV)
    out = torch.full((2, 1025), 9.0, dtype=BF16, device=DEV)
    rc = _api()[1].omni_codec_dwconv_ln(z.data_ptr(), 1025, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 1e-6, out.data_ptr(),
                                        2, 1025, 1, _stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"omni_codec_dwconv_ln" in _api()[1].omni_last_error() and bool((out == 9.0).all())


# ---------------------------------------------------------------------------------------------------------------- out_conv
@pytest.mark.parametrize("T,Cc,taps", [(1, 8, 7), (255, 96, 7), (257, 96, 7), (700, 24, 7), (300, 96, 1), (3, 512, 7)])
def test_out_conv(T, Cc, taps):
    """T off the 256-sample block on both sides, T below the tap count, 1 tap; about a tenth of the samples saturate: those are
    exactly +-1, the others within fp32 accumulation of the fp64 sum."""
    x = _randn(T, Cc, seed=T + Cc).to(BF16)
    w = _randn(taps, Cc, seed=Cc + taps, std=0.61 / math.sqrt(taps * Cc))     # raw ~ N(0, 0.61^2): P(|raw| > 1) = 0.1
    bias = float(torch.tensor(0.01, dtype=torch.float32))                    # the fp32 value the call passes
    wav = _guarded(T, 1, torch.float32, 9.0)
    x_dev, w_dev = x.to(DEV), w.to(DEV)
    rc = _api()[1].omni_codec_out_conv(x_dev.data_ptr(), w_dev.data_ptr(), bias, wav.data_ptr(), T, Cc, taps, _stream())
    assert rc == 0, _api()[1].omni_last_error()
    torch.cuda.synchronize()
    _untouched(wav, T, 9.0, "out_conv")
    got = wav[:T, 0].double().cpu()
    ref, p = R.ref_out_conv(x, w, bias, taps, parts=True)
    tol = 1e-5 * p["abs_sum"]
    sat = p["raw"].abs() > 1.0 + tol
    if T >= 255:
        assert 0.03 <= float(sat.double().mean()) <= 0.3, float(sat.double().mean())
    assert torch.equal(got[sat], torch.sign(p["raw"][sat])), "saturated samples must be exactly +-1"
    assert float(got.abs().max()) <= 1.0
    rows = torch.arange(T)
    _assert_within(f"out_conv {T, Cc, taps}", got, ref, tol, {f"rows t < {taps - 1} (zero padding)": rows < taps - 1,
                                                              "the last block's rows": rows >= (T - 1) // 256 * 256})


@pytest.mark.parametrize("Cc,taps", [(12, 7), (2048, 9)])
def test_out_conv_rejections(Cc, taps):
    """C off the 8-element vector, and weights (taps * C * 4 bytes) past the 64 KB of LDS: an error code, nothing launched."""
    T = 4
    x, w = torch.zeros(T, Cc, dtype=BF16, device=DEV), torch.zeros(taps, Cc, device=DEV)
    wav = torch.full((T,), 9.0, device=DEV)
    rc = _api()[1].omni_codec_out_conv(x.data_ptr(), w.data_ptr(), 0.0, wav.data_ptr(), T, Cc, taps, _stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"omni_codec_out_conv" in _api()[1].omni_last_error() and bool((wav == 9.0).all())


# ---------------------------------------------------------------------------------------------------------------- res_unit
@functools.lru_cache(maxsize=None)
def _unit_weights(Cc):
    """Random fp32 weights rounded to bf16 and per-channel snake parameters drawn as tests/codec_util.py::make_codec_state draws
    them; packed for the device as Code2WavDecoder._build packs them (frag_shuffle of [N, tap * C + channel])."""
    from ht_vllm_omni_amd.engine import frag_shuffle
    W1 = _randn(Cc, Cc, 7, seed=Cc, std=0.5 / math.sqrt(7 * Cc)).to(BF16)
    W2 = _randn(Cc, Cc, 1, seed=Cc + 1, std=0.3 / math.sqrt(Cc)).to(BF16)
    b1, b2 = _randn(Cc, seed=Cc + 2, std=0.02), _randn(Cc, seed=Cc + 3, std=0.02)
    sn2 = R.snake_params(_randn(Cc, seed=Cc + 4, std=0.3), _randn(Cc, seed=Cc + 5, std=0.3))
    snn = R.snake_params(_randn(Cc, seed=Cc + 6, std=0.3), _randn(Cc, seed=Cc + 7, std=0.3))
    host = dict(W1=W1, W2=W2, b1=b1, b2=b2, sn2=sn2, snn=snn)
    dev = dict(w1=frag_shuffle(W1.permute(0, 2, 1).reshape(Cc, 7 * Cc).to(DEV).contiguous()),
               w2=frag_shuffle(W2[:, :, 0].to(DEV).contiguous()), b1=b1.to(DEV), b2=b2.to(DEV),
               a2=sn2[0].to(DEV), ib2=sn2[1].to(DEV), an=snn[0].to(DEV), ibn=snn[1].to(DEV))
    return host, dev


def _unit_struct(dev, s, h, s_next, T, Cc, dil):
    ru = _api()[0].ResUnit()
    ru.s, ru.h, ru.s_next = s.data_ptr(), h.data_ptr(), s_next.data_ptr()
    ru.w1, ru.b1, ru.snake2_alpha, ru.snake2_inv_beta = dev["w1"].data_ptr(), dev["b1"].data_ptr(), dev["a2"].data_ptr(), dev["ib2"].data_ptr()
    ru.w2, ru.b2, ru.next_alpha, ru.next_inv_beta = dev["w2"].data_ptr(), dev["b2"].data_ptr(), dev["an"].data_ptr(), dev["ibn"].data_ptr()
    ru.T, ru.C, ru.dilation = T, Cc, dil
    return ru


UNITS = [(96, 1, 1), (96, 2, 256), (96, 3, 257), (96, 9, 1100), (96, 9, 53), (96, 9, 55), (96, 5, 255), (96, 1, 511), (96, 2, 513),
         (96, 5, 513), (192, 9, 1), (192, 1, 256), (192, 5, 257), (192, 3, 1100), (192, 9, 53), (192, 2, 55), (192, 3, 255),
         (192, 5, 511), (192, 9, 513), (192, 2, 1100)]


@pytest.mark.parametrize("Cc,dil,T", UNITS)
def test_res_unit(Cc, dil, T):
    """The fused unit on its own: every dilation 1..9 it accepts (the decoder gives it 1, 3, 9), T below the halo, at one row
    block and one past it (256 rows at C = 192, 512 at C = 96), ragged tails; rows past T neither read nor written."""
    host, dev = _unit_weights(Cc)
    assert _api()[1].omni_codec_res_unit_supported(Cc, 7, dil)
    s = _randn(T, Cc, seed=T + dil).to(BF16)
    h = _randn(T, Cc, seed=T + dil + 1)
    s_dev, h_dev, sn_dev = _guarded(T, Cc, BF16, 1e30), _guarded(T, Cc, torch.float32, 9.0), _guarded(T, Cc, BF16, 9.0)
    s_dev[:T], h_dev[:T] = s.to(DEV), h.to(DEV)
    ru = _unit_struct(dev, s_dev, h_dev, sn_dev, T, Cc, dil)
    rc = _api()[1].omni_codec_res_unit(C.byref(ru), _stream())
    assert rc == 0, _api()[1].omni_last_error()
    torch.cuda.synchronize()
    _untouched(h_dev, T, 9.0, "res_unit h")
    _untouched(sn_dev, T, 9.0, "res_unit s_next")
    assert torch.equal(s_dev[:T].cpu().view(torch.int16), s.view(torch.int16)), "s is read-only"
    ref_h, ref_s, p = R.ref_res_unit(s, h, host["W1"], host["b1"], host["sn2"], host["W2"], host["b2"], host["snn"], dil, parts=True)
    W2a = host["W2"][:, :, 0].double().abs()
    a2, ib2 = host["sn2"][0].double(), host["sn2"][1].double()
    an, ibn = host["snn"][0].double(), host["snn"][1].double()
    u_abs = p["u"].abs()
    S = (u_abs + (1.0 + a2 * ib2) * p["abs1"]) @ W2a.T + host["b2"].double().abs() + h.double().abs()
    tol_h = EPS8 * (u_abs @ W2a.T) + 1e-5 * S
    slope = 1.0 + torch.clamp((torch.sin(2.0 * an * ref_h)).abs() + 2.0 * an * tol_h, max=1.0) * an * ibn
    tol_s = 2.0 ** -7 * ref_s.abs() + tol_h * slope
    rows = torch.arange(T)
    groups = {f"rows t < {6 * dil} (causal halo)": rows < 6 * dil, "last row of each 256-row block": rows % 256 == 255,
              "other rows": (rows >= 6 * dil) & (rows % 256 != 255)}
    _assert_within(f"res_unit h {Cc, dil, T}", h_dev[:T], ref_h, tol_h, groups)
    _assert_within(f"res_unit s_next {Cc, dil, T}", sn_dev[:T], ref_s, tol_s, groups)


def test_res_unit_rejects_s_next_aliasing_s():
    host, dev = _unit_weights(96)
    s = torch.zeros(8, 96, dtype=BF16, device=DEV)
    h = torch.full((8, 96), 9.0, device=DEV)
    rc = _api()[1].omni_codec_res_unit(C.byref(_unit_struct(dev, s, h, s, 8, 96, 1)), _stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"aliases" in _api()[1].omni_last_error() and bool((h == 9.0).all())
