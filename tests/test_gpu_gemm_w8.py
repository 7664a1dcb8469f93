"""The W8 skinny GEMMs (csrc/gemm_w8.hip), W_eff = bf16(fp8 * row scale) rebuilt in registers: bit for bit the bf16 entry point on W_eff for
every k-step count the layout distinguishes (K = 96: three steps; 256: one per wave; 512: one pair per wave; 768: a pair and an unpaired step;
2048: the counted schedule), and one float64 statement per form at the bounds tests/test_gpu_ops.py holds the bf16 form to."""
import pytest
import torch

from ht_vllm_omni_amd import ops
from oracle import talker_oracle as O
from tests.util import BF16, assert_bf16_close

pytestmark = pytest.mark.gpu
EPS = 1e-6


def _weights(g, rows, K):
    """(fp8 bytes, scales, W_eff) of randn rows times 2^U(-6, 2) (scales span binades, no powers of two); row 1 zero; row 2 holds +-max (+-448)."""
    from ht_vllm_omni_amd.engine import fp8_dequant_rows, fp8_quant_rows
    w = torch.randn(rows, K, generator=g) * torch.exp2(torch.rand(rows, 1, generator=g) * 8 - 6)
    w[1] = 0
    w[2, 0], w[2, 1] = w[2].abs().max(), -w[2].abs().max()
    q8, sc = fp8_quant_rows(w.to(BF16))
    return q8, sc, fp8_dequant_rows(q8, sc)


def _inputs(g, M, K):
    """x [M, K] row-major and fragment-major, norm weight, sum(r^2) slabs of arbitrary positive values."""
    from ht_vllm_omni_amd.engine import frag_shuffle
    xp = torch.zeros((M + 15) // 16 * 16, K, dtype=BF16)
    xp[:M] = (torch.randn(M, K, generator=g)).to(BF16)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF16)
    part = torch.rand(K // 16, 64, generator=g) * 16 + 0.5
    return xp[:M].contiguous().cuda(), frag_shuffle(xp).cuda(), nw.cuda(), part.cuda()


def _both(form, M, N, K, g):
    from ht_vllm_omni_amd import _lib as L
    from ht_vllm_omni_amd.engine import frag_shuffle, frag_shuffle_w8, gu8_rows, gu8_shuffle
    rows = 2 * N if form == "gu8" else N
    q8, sc, weff = _weights(g, rows, K)
    x, xf, nw, part = _inputs(g, M, K)
    if form == "gu8":
        w8, scd, wf = frag_shuffle_w8(gu8_rows(q8)).cuda(), gu8_rows(sc).contiguous().cuda(), gu8_shuffle(weff).cuda()
    else:
        w8, scd, wf = frag_shuffle_w8(q8).cuda(), sc.cuda(), frag_shuffle(weff).cuda()
    out = []
    frags = (False, True) if N % 32 == 0 else (False,)
    if form == "plain":
        bias = (torch.randn(N, generator=g) * 0.1).to(BF16).cuda()
        for xin, xl in ((x, 0), (xf, L.LAYOUT_X_FRAG)):
            for of in frags:
                lay = xl | (L.LAYOUT_OUT_FRAG if of else 0)
                out.append((f"plain layout {lay}", ops.gemm_w8(xin, w8, scd, bias=bias, layout=lay, M=M),
                            ops.gemm(xin, wf, bias=bias, layout=lay | L.LAYOUT_W_FRAG, M=M)))
    elif form == "resid":
        r0 = frag_shuffle((torch.randn(xf.shape[0], N, generator=g)).to(BF16)).cuda()      # accumulate into a non-zero stream
        ra, rb = r0.clone(), r0.clone()
        pa, pb = torch.zeros(N // 16, 64, device="cuda"), torch.zeros(N // 16, 64, device="cuda")
        assert ops.gemm_resid_w8(xf, w8, scd, ra, pa, M=M) == ops.gemm_resid(xf, wf, rb, pb, M=M) == N // 16
        out += [("stream", ra, rb), ("slabs", pa[:, :M], pb[:, :M])]
    else:
        epi = L.EPI_SILU_MUL_GU8 if form == "gu8" else L.EPI_BF16
        for of in frags:
            out.append((f"{form} out_frag {of}", ops.gemm_xnorm_w8(xf, part, K // 16, nw, w8, scd, EPS, M=M, epilogue=epi, out_frag=of),
                        ops.gemm_xnorm(xf, part, K // 16, nw, wf, EPS, M=M, epilogue=epi, out_frag=of)))
    return out


@pytest.mark.parametrize("M", [1, 16, 37, 64])
@pytest.mark.parametrize("K", [96, 256, 512, 768, 2048])
@pytest.mark.parametrize("form", ["plain", "resid", "xnorm", "gu8"])
def test_w8_entry_point_is_the_bf16_entry_point_on_the_dequantised_matrix(form, K, M):
    g = torch.Generator().manual_seed(1000 * M + K)
    for N in ((96, 768) if form == "gu8" else (256,) if form == "resid" else (16, 48, 256)):      # the residual stream needs N % 32 == 0
        for what, got, ref in _both(form, M, N, K, g):
            assert torch.equal(got, ref), f"{form} N={N} K={K} M={M}: {what} differs from the bf16 kernel on W_eff"


@pytest.mark.parametrize("form", ["plain", "resid", "xnorm", "gu8"])
def test_w8_against_float64(form):
    """x . W_eff^T in float64 with the form's roundings, at tests/test_gpu_ops.py's bounds for the bf16 form (test_gemm 1 ulp / 2 %; norm-free stream:
    delta, xnorm 1 ulp / 6 %, silu 2 ulps / 6 %); a CPU fp32-accumulate result differs from it in 0.011 / 0 / 0.021 / 0.028 % of the values here."""
    from ht_vllm_omni_amd import _lib as L
    from ht_vllm_omni_amd.engine import frag_shuffle_w8, frag_unshuffle, gu8_rows
    M, N, K = 37, 96 if form == "gu8" else 256, 768
    g = torch.Generator().manual_seed(77)
    q8, sc, weff = _weights(g, 2 * N if form == "gu8" else N, K)
    x, xf, nw, part = _inputs(g, M, K)
    w8, scd = frag_shuffle_w8(q8).cuda(), sc.cuda()
    x64, w64 = x.cpu().double(), weff.double()
    if form == "plain":
        bias = (torch.randn(N, generator=g) * 0.1).to(BF16)
        got = ops.gemm_w8(x, w8, scd, bias=bias.cuda())
        assert_bf16_close(got, (x64 @ w64.t() + bias.double()).to(BF16), what="w8 gemm bf16+bias")
        return
    if form == "resid":
        r = torch.zeros(xf.shape[0], N, dtype=BF16, device="cuda")
        slabs = torch.zeros(N // 16, 64, device="cuda")
        ops.gemm_resid_w8(xf, w8, scd, r, slabs, accumulate=False, M=M)
        r = frag_unshuffle(r.cpu())[:M]
        assert_bf16_close(r, (x64 @ w64.t()).to(BF16), ulps=1, max_mismatch=0.06, what="w8 delta")
        torch.testing.assert_close(slabs[:, :M].sum(0).cpu(), r.float().pow(2).sum(-1), rtol=1e-5, atol=1e-6)
        return
    # deferred rstd: rstd * sum(W_eff * bf16(norm_w * r)), rstd from the slabs in fp32
    xw = (x.cpu().float() * nw.cpu().float()).to(BF16).double()
    rstd = (1.0 / torch.sqrt(part[:, :M].sum(0).cpu() / K + EPS)).double()[:, None]
    y = (xw @ w64.t()) * rstd
    if form == "xnorm":
        got = ops.gemm_xnorm_w8(xf, part, K // 16, nw, w8, scd, EPS, M=M)
        assert_bf16_close(got, y.to(BF16), ulps=1, max_mismatch=0.06, what="w8 xnorm gemm")
    else:
        got = ops.gemm_xnorm_w8(xf, part, K // 16, nw, frag_shuffle_w8(gu8_rows(q8)).cuda(), gu8_rows(sc).contiguous().cuda(), EPS, M=M,
                                epilogue=L.EPI_SILU_MUL_GU8)
        assert_bf16_close(got, O.silu_mul(y[:, :N].to(BF16), y[:, N:].to(BF16)), ulps=2, max_mismatch=0.06, what="w8 xnorm silu")


@pytest.mark.parametrize("M,N,K,scales", [(4, 32, 48, True), (4, 24, 64, True), (65, 32, 64, True), (4, 32, 64, False)],
                         ids=["K%32", "N%16", "M>64", "null-scales"])
def test_w8_rejections(M, N, K, scales):
    from ht_vllm_omni_amd import _lib as L
    lib = L.load()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p, s = buf.data_ptr(), buf.data_ptr() if scales else None
    assert lib.omni_gemm_w8(p, K, p, s, None, p, M, N, K, 0, None) == -1
    assert lib.omni_gemm_resid_w8(p, p, s, p, 1, p, M, N, K, None) == -1
    assert lib.omni_gemm_xnorm_w8(p, p, 1, p, EPS, p, s, p, M, N, K, L.EPI_BF16, 0, None) == -1
