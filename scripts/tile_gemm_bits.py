"""sha256 of the output bytes of a fixed-seed list of tile GEMM calls: ops.gemm_tile (plain, windowed conv, grouped with group_rows, GU8,
the residual / fp32 / snake epilogue; tile_hints 0, 1, 2, 5), ops.gemm_tile_fp8 (hints 0 - 4), ops.quant_rows_fp8 (with and without the
norm prologue) and ops.moe_prefill_experts on bf16 and fp8 experts at both block heights.  One line per call.  Run it in two trees (each
copy imports the package of ITS tree) and diff the text: a refactor of the tile GEMM family leaves it unchanged.  Shapes: the parameter
tuples of tests/test_gpu_gemm_tile.py, test_gpu_prefill_fp8.py, test_gpu_moe_prefill.py and test_gpu_moe_prefill_fp8.py; a few seconds."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ht_vllm_omni_amd import ops, _lib as L
from ht_vllm_omni_amd.engine import fp8_quant_rows, frag_shuffle, frag_shuffle_w8, gu8_shuffle

BF16 = torch.bfloat16


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def rnd(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF16)


def bf16_gemms():
    for M, N, K in ((300, 256, 128), (257, 192, 96), (513, 384, 672), (1111, 96, 672), (900, 272, 160), (70, 48, 32), (6400, 2048, 2048)):
        g = torch.Generator().manual_seed(M * 7 + N)
        x, w = rnd(g, M, K).cuda(), frag_shuffle(rnd(g, N, K, scale=0.05)).cuda()
        for hint in (0, 1, 2) + ((5,) if N % 256 == 0 else ()):
            yield f"gemm_tile plain {M}x{N}x{K} hint {hint}", sha(ops.gemm_tile(x, w, tile_hint=hint))
    for Cin, Cout, taps, dil, T in ((96, 96, 7, 9, 531), (512, 1024, 3, 1, 77), (768, 768, 7, 9, 290)):
        g = torch.Generator().manual_seed(Cin + taps * 13 + dil)
        x, w, b = rnd(g, T, Cin).cuda(), frag_shuffle(rnd(g, Cout, taps * Cin, scale=0.05)).cuda(), torch.randn(Cout, generator=g).cuda()
        for hint in (0, 1, 2):
            yield f"gemm_tile conv k{taps} d{dil} {Cin}->{Cout} T={T} hint {hint}", sha(ops.gemm_tile(x, w, bias=b, taps=taps, dilation=dil, tile_hint=hint))
    for E, cap, N, K in ((16, 128, 128, 256), (128, 448, 1024, 384), (5, 320, 192, 96)):
        g = torch.Generator().manual_seed(E * 31 + N)
        x, w = rnd(g, E * cap, K).cuda(), frag_shuffle(rnd(g, E, N, K, scale=0.05)).cuda()
        rows = torch.randint(0, cap + 1, (E,), generator=g).to(torch.int32)
        rows[0], rows[-1] = cap, 0
        for hint in (0, 1, 2):
            out = torch.full((E * cap, N), 7.0, dtype=BF16, device="cuda")
            ops.gemm_tile(x, w, out=out, groups=E, group_rows=rows.cuda(), tile_hint=hint)
            yield f"gemm_tile grouped E={E} cap={cap} {N}x{K} hint {hint}", sha(out, ops.gemm_tile(x, w, groups=E, tile_hint=hint))
    for M, I, K in ((333, 3072, 1024), (100, 64, 64)):
        g = torch.Generator().manual_seed(I)
        x, w = rnd(g, M, K).cuda(), gu8_shuffle(rnd(g, 2 * I, K, scale=0.03)).cuda()
        for hint in (0, 1, 2) + ((5,) if (2 * I) % 256 == 0 else ()):
            yield f"gemm_tile GU8 {M}x{I}x{K} hint {hint}", sha(ops.gemm_tile(x, w, act=L.TILE_ACT_SILU_MUL_GU8, tile_hint=hint))
    for M, N, K in ((700, 192, 192), (1234, 512, 1088)):
        g = torch.Generator().manual_seed(5 + N)
        x, w = rnd(g, M, K).cuda(), frag_shuffle(rnd(g, N, K, scale=0.08)).cuda()
        b, sc, r = torch.randn(N, generator=g).cuda(), (torch.rand(N, generator=g) + 0.5).cuda(), (torch.randn(M, N, generator=g) * 4).cuda()
        al, ib = (torch.rand(N, generator=g) + 0.5).cuda(), (torch.rand(N, generator=g) + 0.5).cuda()
        for hint in (0, 1, 2) + ((5,) if N % 256 == 0 else ()):
            f, o, s = ops.gemm_tile(x, w, bias=b, scale=sc, resid=r, snake=(al, ib), want="fbs", tile_hint=hint)
            yield f"gemm_tile resid / fp32 / snake {M}x{N}x{K} hint {hint}", sha(f, o, s)
            yield f"gemm_tile GELU * scale {M}x{N}x{K} hint {hint}", sha(ops.gemm_tile(x, w, bias=b, scale=sc, act=L.TILE_ACT_GELU, tile_hint=hint))


def fp8_rows(g, M, K):
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.rand(M, 1, generator=g) * 8 - 6)
    x[-1, K // 3] *= 64
    x[M // 2] = 0
    return x.to(BF16)


def fp8_gemms():
    for M, K in ((1, 128), (17, 512), (300, 640), (300, 2048), (40, 8192)):
        g = torch.Generator().manual_seed(M * K)
        x = fp8_rows(g, M, K).cuda()
        yield f"quant_rows_fp8 {M}x{K}", sha(*ops.quant_rows_fp8(x))
        if K <= 4096:
            w, r = (1 + 0.1 * torch.randn(K, generator=g)).to(BF16).cuda(), rnd(g, M, K).cuda()
            q, s = ops.quant_rows_fp8(norm_w=w, eps=1e-6, delta=x, residual=r)
            yield f"quant_rows_fp8 norm prologue {M}x{K}", sha(q, s, r)
    for M, N, K, gu8 in ((1, 16, 128, False), (17, 48, 256, False), (300, 256, 512, False), (300, 272, 640, False), (70, 1024, 2048, False),
                         (513, 512, 768, False), (100, 128, 128, True), (333, 1536, 512, True)):
        g = torch.Generator().manual_seed(M + N + K)
        q8, sw = fp8_quant_rows(rnd(g, N, K, scale=0.05))
        qx, sx = ops.quant_rows_fp8(fp8_rows(g, M, K).cuda())
        w8, sw = frag_shuffle_w8(q8).cuda(), sw.cuda()
        for hint in range(5):
            if hint in (0, 2) or N % 256 == 0:
                out = ops.gemm_tile_fp8(qx, sx, w8, sw, M=M, act=L.TILE_ACT_SILU_MUL_GU8 if gu8 else L.TILE_ACT_NONE, tile_hint=hint)
                yield f"gemm_tile_fp8{' GU8' if gu8 else ''} {M}x{N}x{K} hint {hint}", sha(out)


def moe_weights(H, E, I, seed):
    g = torch.Generator().manual_seed(seed)
    return rnd(g, E, H, scale=0.5), rnd(g, E, 2 * I, H, scale=0.08), rnd(g, E, H, I, scale=0.08)


def moe_blocks():
    # (64, 16, 4, 32, ...): I too narrow for the fused gate_up (MOE_GU_PLAIN + silu_mul)
    for H, E, k, I, T, e0, n_local in ((64, 16, 4, 64, 9, 0, 16), (64, 4, 2, 64, 150, 0, 4), (64, 16, 4, 32, 70, 0, 16), (256, 16, 4, 128, 40, 4, 4),
                                       (256, 4, 2, 384, 150, 0, 4), (1024, 128, 8, 384, 300, 0, 128)):
        router, gate_up, down = moe_weights(H, E, I, seed=5 * E + k)
        x = fp8_rows(torch.Generator().manual_seed(T + H), T, H).cuda()
        idx, wts = ops.moe_route(ops.gemm_tile(x, ops._frag(router.cuda()))[:, :E].contiguous(), k, False)
        win = slice(e0, e0 + n_local)
        gu_f, dn_f = frag_shuffle(gate_up).cuda()[win], frag_shuffle(down).cuda()[win]
        for block in (64, 256):
            yield f"moe_prefill_experts bf16 H={H} E={E} k={k} I={I} T={T} block {block}", sha(
                ops.moe_prefill_experts(x, idx, wts, gu_f, dn_f, E=E, e0=e0, block=block))
        if H % 128 == 0 and I % 128 == 0:
            (gq, gs), (dq, ds) = fp8_quant_rows(gate_up), fp8_quant_rows(down)
            for block in (64, 256):
                yield f"moe_prefill_experts fp8  H={H} E={E} k={k} I={I} T={T} block {block}", sha(
                    ops.moe_prefill_experts(x, idx, wts, frag_shuffle(gq).cuda()[win], frag_shuffle(dq).cuda()[win], E=E, e0=e0, block=block,
                                            gate_up_scale=gs.cuda()[win], down_scale=ds.cuda()[win]))


if __name__ == "__main__":
    for part in (bf16_gemms, fp8_gemms, moe_blocks):
        for name, digest in part():
            print(f"{digest[:32]}  {name}", flush=True)
