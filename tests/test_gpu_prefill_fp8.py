"""W8A8 prefill on the fp8 MFMA (csrc/gemm_prefill_f8.hip): the row quantiser bit for bit against engine.fp8_quant_rows (IEEE division: on
the CPU), the tile GEMM against float64 on its own quantised operands at the bound of one bf16 rounding of an fp32 accumulation, every
tile geometry bit-identical, and prefill_wide(gemm="fp8") against the same layer loop with float64 GEMMs."""
import pytest
import torch

from ht_vllm_omni_amd import _lib as L
from ht_vllm_omni_amd import ops
from ht_vllm_omni_amd.engine import frag_shuffle_w8, frag_unshuffle_w8, fp8_quant_rows, gu8_rows
from tests.test_gpu_gemm_tile import _close
from tests.test_gpu_gemm_w8 import _weights
from tests.util import BF16, assert_e2e_close

pytestmark = pytest.mark.gpu
EPS = 1e-6
F8 = torch.float8_e4m3fn


def _rows(g, M, K):
    """randn rows times 2^U(-6, 2); one row with a x64 outlier, one all-zero row."""
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.rand(M, 1, generator=g) * 8 - 6)
    x[-1, K // 3] *= 64
    x[M // 2] = 0
    return x.to(BF16)


@pytest.mark.parametrize("K", [128, 512, 640])
@pytest.mark.parametrize("M", [1, 17, 300])
def test_row_quantiser_equals_fp8_quant_rows(M, K):
    g = torch.Generator().manual_seed(M * K)
    x = _rows(g, M, K)
    wide = torch.zeros(M, K + 8, dtype=BF16)
    wide[:, :K] = x
    q, s = ops.quant_rows_fp8(wide.cuda()[:, :K])                               # a row stride
    rq, rs = fp8_quant_rows(x)
    rm = frag_unshuffle_w8(q.cpu())
    assert torch.equal(rm[:M], rq) and torch.equal(s.cpu(), rs) and not rm[M:].any()
    # the norm prologue: omni_rmsnorm's rows, never stored
    w, r = (1 + 0.1 * torch.randn(K, generator=g)).to(BF16).cuda(), torch.randn(M, K, generator=g).to(BF16).cuda()
    r_ref = r.clone()
    rq, rs = fp8_quant_rows(ops.rmsnorm(None, w, EPS, delta=x.cuda(), residual=r_ref).cpu())
    q, s = ops.quant_rows_fp8(norm_w=w, eps=EPS, delta=x.cuda(), residual=r)
    rm = frag_unshuffle_w8(q.cpu())
    assert torch.equal(rm[:M], rq) and torch.equal(s.cpu(), rs) and not rm[M:].any() and torch.equal(r, r_ref)


def _operands(M, rows, K, gu8=False):
    g = torch.Generator().manual_seed(M + rows + K)
    q8, sc, _ = _weights(g, rows, K)
    if gu8:
        q8, sc = gu8_rows(q8), gu8_rows(sc).contiguous()
    qx, sx = ops.quant_rows_fp8(_rows(g, M, K).cuda())
    return qx, sx, frag_shuffle_w8(q8).cuda(), sc.cuda(), q8


# one remainder MFMA | a remainder only | one main group | main + remainder | the long loop | M tails across row blocks
@pytest.mark.parametrize("M,N,K", [(1, 16, 128), (17, 48, 256), (300, 256, 512), (300, 272, 640), (70, 1024, 2048), (513, 512, 768)])
def test_gemm_against_float64_and_every_tile_alike(M, N, K):
    qx, sx, w8, sw, q8 = _operands(M, N, K)
    a, b = frag_unshuffle_w8(qx.cpu())[:M].view(F8).double(), q8.view(F8).double()
    s = sx.cpu().double()[:, None] * sw.cpu().double()[None, :]
    got = ops.gemm_tile_fp8(qx, sx, w8, sw, M=M)
    _close(got, (a @ b.T) * s, (a.abs() @ b.abs().T) * s, f"fp8 tile GEMM {M}x{N}x{K}")
    for hint in (1, 2, 3, 4):
        if hint == 2 or N % 256 == 0:       # the 256-column tiles take N % 256 == 0
            assert torch.equal(ops.gemm_tile_fp8(qx, sx, w8, sw, M=M, tile_hint=hint), got), f"tile_hint {hint}"


@pytest.mark.parametrize("M,I,K,hint", [(100, 64, 128, 0), (333, 768, 512, 0), (333, 768, 512, 3)])
def test_gate_up_epilogue_equals_silu_mul_of_the_plain_gemm(M, I, K, hint):
    qx, sx, w8, sw, _ = _operands(M, 2 * I, K, gu8=True)
    plain = ops.gemm_tile_fp8(qx, sx, w8, sw, M=M)                              # columns in the GU8 order: back to [gate | up]
    plain = plain.reshape(M, I // 8, 2, 8).transpose(1, 2).reshape(M, 2 * I).contiguous()
    fused = ops.gemm_tile_fp8(qx, sx, w8, sw, M=M, act=L.TILE_ACT_SILU_MUL_GU8, tile_hint=hint)
    assert torch.equal(fused, ops.silu_mul(plain))


def _reference_prefill(eng, x, pos, req, slots):
    """prefill_wide's layer loop on the project's norm / rope / attention ops, the four GEMMs in float64 on fp8_quant_rows operands."""
    import torch.nn.functional as F
    d = eng.d

    def lin(a, w, n):
        qa, sa = fp8_quant_rows(a.cpu())
        qw = frag_unshuffle_w8(w[n + "_w8"].cpu()).view(F8).double()
        return (qa.view(F8).double() @ qw.T) * sa.double()[:, None] * w[n + "_w8_scale"].cpu().double()[None, :]

    kw = dict(q_heads=eng.hq_l, kv_heads=eng.hkv_l, head_dim=d.head_dim, kv_dtype=eng.kv_code)
    resid, delta = x.clone(), None
    for l in range(d.layers):
        w = eng.layer_w[l]
        kc, vc = torch.zeros_like(eng.kv_caches[l][0]), torch.zeros_like(eng.kv_caches[l][1])
        a = ops.rmsnorm(None, w["ln1"], d.eps, delta=delta, residual=resid)
        q = ops.qknorm_rope_kvwrite(lin(a, w, "wqkv").to(BF16).cuda(), w["qnorm"], w["knorm"], pos, eng.cos_sin, slots, kc, vc, eps=d.eps,
                                    k_scale=eng.k_scale_l[l], v_scale=eng.v_scale_l[l], **kw)
        o = ops.paged_attn_prefill(q, kc, vc, eng.block_table, req, pos, block_size=eng.block_size, k_scale=eng.k_scale_l[l],
                                   v_scale=eng.v_scale_l[l], **kw)
        o = lin(o, w, "wo").to(BF16).cuda()
        a = ops.rmsnorm(None, w["ln2"], d.eps, delta=o, residual=resid)
        gu = lin(a, w, "wgu").reshape(a.shape[0], -1, 2, 8).to(BF16)            # GU8 row order: [8 gate | 8 up] per 16 columns
        act = (F.silu(gu[:, :, 0]) * gu[:, :, 1]).reshape(a.shape[0], -1)
        delta = lin(act, w, "wdown").to(BF16).cuda()
    return ops.rmsnorm(None, eng.final_norm, d.eps, delta=delta, residual=resid)


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_engine_prefill_on_fp8_against_float64_gemms(kv):
    from ht_vllm_omni_amd.config import get_dims
    from ht_vllm_omni_amd.engine import TalkerEngine
    from ht_vllm_omni_amd.sched import BlockPool, slot_of
    from ht_vllm_omni_amd.weights import make_weights
    d, lens, bs = get_dims("tiny"), [3, 30, 7, 19, 12], 16
    B = len(lens)
    eng = TalkerEngine(d, make_weights(d, seed=23, std=0.06, norm_noise=0.1), dense_fp8=True, prefill_gemm="fp8", kv_dtype=kv, num_blocks=4 * B + 8,
                       block_size=bs, max_batch=B)
    pool = BlockPool(eng.num_blocks, bs)
    for r, n in enumerate(lens):
        pool.allocate(f"r{r}", n + 2)
    bts = [pool.block_ids(f"r{r}") for r in range(B)]
    for r in range(B):
        eng.block_table[r, :len(bts[r])] = torch.tensor(bts[r], dtype=torch.int32).cuda()
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.randn(n, d.hidden, generator=g).to(BF16) for n in lens]).cuda()
    pos = torch.cat([torch.arange(n) for n in lens]).to(torch.int32)
    req = torch.cat([torch.full((n,), r) for r, n in enumerate(lens)]).to(torch.int32)
    slots = torch.tensor([slot_of(bts[int(req[t])], int(pos[t]), bs) for t in range(x.shape[0])]).cuda()
    pos, req = pos.cuda(), req.cuda()
    last = (torch.tensor(lens).cumsum(0) - 1).cuda()
    hl = eng.prefill_wide(x, pos, req, slots)[last]
    ref = _reference_prefill(eng, x, pos, req, slots)[last]
    diff = (hl.float() - ref.float()).abs()
    print(f"fp8 prefill vs float64 GEMMs ({kv} KV): mean |diff| {diff.mean().item():.4g}, max {diff.max().item():.4g}, scale {ref.float().abs().max().item():.4g}")
    # Every stage agrees with its float64 counterpart up to 1-ulp flips in ~0.1 % of the elements (mean 1e-5), but a per-token fp8 quantiser is
    # discontinuous: behind one flipped element a row's bytes differ in a few codes of 2^-3 relative size, and two layers on both runs are two
    # realisations of the fp8 quantisation noise.  assert_e2e_close's defaults (2 ulps, mean 4e-3) do not hold: measured mean |diff| 0.0298 /
    # 0.0301 and max 0.1665 / 0.1484 (10.7 / 9.5 ulps) at scale 3.8 for bf16 / fp8 KV.  Bound: 2 x measured.
    assert_e2e_close(hl, ref, mean_tol=0.06, max_ulps=21.3, what=f"last-token hidden states, {kv} KV")
    # ... and the decode step runs on the cache this prefill wrote
    eng.input_ids[:B] = eng.compute_logits(hl).argmax(-1).to(torch.int32)
    eng.last_hidden[:B] = hl
    eng.positions[:B] = torch.tensor(lens, dtype=torch.int32).cuda()
    eng.seq_lens[:B] = (torch.tensor(lens, dtype=torch.int32) + 1).cuda()
    eng.steps[:B] = 1
    eng.decode_step(B)
    torch.cuda.synchronize()
    assert eng.status[:2].tolist() == [0, 0]
