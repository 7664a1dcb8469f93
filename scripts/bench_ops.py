"""Per-op micro-benchmarks inside hipGraphs with rotating (cache-defeating) buffers (diagnostic)."""
import os as _os; _os.environ.setdefault("OMNI_TALKER_DEBUG", "1")   # omni_debug_* hooks live in libomni_talker_debug.so
import ctypes as C, os, sys, time, math
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ht_vllm_omni_amd import _lib as L, ops
lib = L.load()
lib.omni_debug_set.argtypes = [C.c_int, C.c_int, C.c_int]; lib.omni_debug_set.restype = None
dev = "cuda"
BF16 = torch.bfloat16

def graph_time(fn, reps=5):
    fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): g.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # us per graph

def bench_gemm(name, N, K, epi, M=64, hot=False):
    rows = 2 * N if epi == L.EPI_SILU_MUL else N
    wbytes = rows * K * 2
    R = 1 if hot else max(2, min(64, int(1.2e9 // wbytes)))
    Ws = [torch.randn(rows, K, device=dev, dtype=BF16) * 0.02 for _ in range(R)]
    x = torch.randn(M, K, device=dev, dtype=BF16)
    n_launch = R if not hot else 20
    frag = os.environ.get("OMNI_BENCH_FRAG", "1") == "1"
    lay = 0
    if frag:
        from ht_vllm_omni_amd.engine import frag_shuffle
        Ws = [frag_shuffle(w_) for w_ in Ws]
        xp = torch.zeros((M + 15) // 16 * 16, K, device=dev, dtype=BF16); xp[:M] = x
        x = frag_shuffle(xp)
        lay = L.LAYOUT_W_FRAG | L.LAYOUT_X_FRAG
    def fn():
        for i in range(n_launch):
            ops.gemm(x, Ws[i % R], epilogue=epi, layout=lay, M=M)
    res = []
    for nt, wgs in ((5, 256), (5, 128), (5, 512), (4, 256)):   # nt bit0 = non-temporal W, bit1 = static-K, bit2 = silu NT=2
        lib.omni_debug_set(nt, 0, wgs)
        us = graph_time(fn) / n_launch
        res.append(f"nt={nt} wgs={wgs}: {us:6.2f} us {wbytes / us / 1e6:5.2f} TB/s")
    lib.omni_debug_set(1, 0, 256)
    print(f"{name:22s} M={M} N={N:5d} K={K:5d} {wbytes/1e6:6.1f} MB {'hot' if hot else 'cold'} | " + " | ".join(res), flush=True)

def bench_norm(rows, hidden):
    R = 32
    xs = [torch.randn(rows, hidden, device=dev, dtype=BF16) for _ in range(R)]
    ds = [torch.randn(rows, hidden, device=dev, dtype=BF16) for _ in range(R)]
    w = torch.ones(hidden, device=dev, dtype=BF16)
    def fn():
        for i in range(R): ops.rmsnorm(None, w, 1e-6, delta=ds[i], residual=xs[i])
    print(f"rmsnorm+resid {rows}x{hidden}: {graph_time(fn)/R:6.2f} us", flush=True)

def bench_attn(name, B, hq, hkv, ctx, kv, layers, fused):
    D, bs = 128, 16
    nblk = B * ((ctx + bs) // bs + 1) + 1
    store = torch.uint8 if kv == "fp8" else BF16
    caches = [torch.randint(0, 100, (2, nblk, bs, hkv, D), device=dev, dtype=torch.uint8).view(store) if kv == "fp8"
              else torch.randn(2, nblk, bs, hkv, D, device=dev, dtype=BF16) for _ in range(layers)]
    per = (ctx + bs) // bs + 1
    bt = (torch.arange(B * per, dtype=torch.int32).view(B, per) + 1).to(dev)
    seq = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    pos = seq - 1
    q = torch.randn(B, hq * D, device=dev, dtype=BF16)
    qkv = torch.randn(B, (hq + 2 * hkv) * D, device=dev, dtype=BF16)
    nw = torch.ones(D, device=dev, dtype=BF16)
    cs = ops.rope_table(4096, D, 1e6).to(dev)
    code = L.KV_CODES[kv]
    def fn():
        for c in caches:
            if fused:
                ops.attn_decode_fused(qkv, nw, nw, pos, cs, c[0], c[1], bt, seq, q_heads=hq, kv_heads=hkv, head_dim=D,
                                      block_size=bs, kv_dtype=code, eps=1e-6, max_seq_len=4096)
            else:
                ops.paged_attn_decode(q, c[0], c[1], bt, seq, q_heads=hq, kv_heads=hkv, head_dim=D, block_size=bs,
                                      kv_dtype=code, max_seq_len=4096)
    us = graph_time(fn) / layers
    kvb = B * ctx * hkv * D * 2 * (1 if kv == "fp8" else 2)
    print(f"{name:26s} B={B} ctx={ctx} {kv} fused={fused}: {us:6.2f} us  {kvb/1e6:6.1f} MB {kvb/us/1e6:5.2f} TB/s", flush=True)

def bench_w8(rounds=9, reps=3, M=64):
    """The four 1.7B backbone GEMMs at M = 64 as the decode step launches them (qkv: deferred-rstd prologue; o / down: residual epilogue;
    gate_up: deferred-rstd + GU8): the W8 entry point against the bf16 entry point on W_eff.  Cold weights (rotating sets past the 256 MB
    of MALL in BOTH arms), caller-allocated outputs (no fill kernel in the graph), arms alternated round by round in this one process;
    prints median and min-max of every arm -- the bf16 arm's spread is the yardstick of the ratio."""
    from ht_vllm_omni_amd.engine import frag_shuffle, frag_shuffle_w8, gu8_shuffle, gu8_rows, fp8_quant_rows, fp8_dequant_rows
    st = L.current_stream
    for name, form, N, K in (("qkv", "xnorm", 4096, 2048), ("o_proj", "resid", 2048, 2048), ("gate_up", "gu8", 6144, 2048), ("down", "resid", 2048, 6144)):
        rows = 2 * N if form == "gu8" else N
        R = max(4, min(64, int(1.2e9 // (rows * K * 2))))
        sets = []
        for _ in range(R):
            q8, sc = fp8_quant_rows((torch.randn(rows, K, device=dev) * 0.02).to(BF16))
            weff = fp8_dequant_rows(q8, sc)
            if form == "gu8":
                sets.append((frag_shuffle_w8(gu8_rows(q8)), gu8_rows(sc).contiguous(), gu8_shuffle(weff)))
            else:
                sets.append((frag_shuffle_w8(q8), sc, frag_shuffle(weff)))
        x = frag_shuffle(torch.randn(M, K, device=dev, dtype=BF16))
        nw = torch.ones(K, device=dev, dtype=BF16)
        part = torch.rand(K // 16, 64, device=dev) + 0.5
        out = torch.zeros(M, N, device=dev, dtype=BF16)
        slabs = torch.zeros(N // 16, 64, device=dev)
        epi = L.EPI_SILU_MUL_GU8 if form == "gu8" else L.EPI_BF16
        def run(arm):
            for w8, sc, wf in sets:
                if form == "resid" and arm:
                    rc = lib.omni_gemm_resid_w8(x.data_ptr(), w8.data_ptr(), sc.data_ptr(), out.data_ptr(), 1, slabs.data_ptr(), M, N, K, st())
                elif form == "resid":
                    rc = lib.omni_gemm_resid(x.data_ptr(), K, wf.data_ptr(), None, out.data_ptr(), 1, slabs.data_ptr(), None, M, N, K,
                                             L.LAYOUT_W_FRAG | L.LAYOUT_X_FRAG, st())
                elif arm:
                    rc = lib.omni_gemm_xnorm_w8(x.data_ptr(), part.data_ptr(), K // 16, nw.data_ptr(), 1e-6, w8.data_ptr(), sc.data_ptr(), out.data_ptr(),
                                                M, N, K, epi, int(form == "gu8"), st())
                else:
                    rc = lib.omni_gemm_xnorm(x.data_ptr(), part.data_ptr(), K // 16, nw.data_ptr(), 1e-6, None, wf.data_ptr(), out.data_ptr(), M, N, K, epi,
                                             None, int(form == "gu8"), st())
                L.check(rc, name)
        graphs = []
        for arm in (0, 1):
            run(arm); torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run(arm)
            g.replay(); torch.cuda.synchronize()
            graphs.append(g)
        t = ([], [])
        for _ in range(rounds):
            for arm in (0, 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps): graphs[arm].replay()
                e1.record(); torch.cuda.synchronize()
                t[arm].append(e0.elapsed_time(e1) / (reps * R) * 1e3)
        med = [sorted(v)[len(v) // 2] for v in t]
        byts = [rows * K * 2, rows * K + rows * 4]
        print(f"{name:8s} {rows:5d} x {K:4d} M={M} sets={R} | " + " | ".join(
            f"{a}: {med[i]:6.2f} us (min {min(t[i]):6.2f} max {max(t[i]):6.2f}) {byts[i] / med[i] / 1e6:5.2f} TB/s" for i, a in enumerate(("bf16", "w8  "))) +
            f" | w8 / bf16 = {med[1] / med[0]:.3f}  (bf16 spread +-{(max(t[0]) - min(t[0])) / 2 / med[0]:.1%})", flush=True)
        del sets

if __name__ == "__main__":
    which = sys.argv[1:] or ["gemm", "norm", "attn"]
    if "w8" in which:
        bench_w8()
    if "gemm" in which:
        bench_gemm("bb qkv", 4096, 2048, L.EPI_BF16)
        bench_gemm("bb o_proj", 2048, 2048, L.EPI_BF16)
        bench_gemm("bb gate_up+silu", 6144, 2048, L.EPI_SILU_MUL)
        bench_gemm("bb down", 2048, 6144, L.EPI_BF16)
        bench_gemm("lm_head", 3072, 2048, L.EPI_F32_BF16RND)
        bench_gemm("cp qkv", 4096, 1024, L.EPI_BF16)
        bench_gemm("cp o_proj", 1024, 2048, L.EPI_BF16)
        bench_gemm("cp gate_up+silu", 3072, 1024, L.EPI_SILU_MUL)
        bench_gemm("cp down", 1024, 3072, L.EPI_BF16)
        bench_gemm("cp qkv hot", 4096, 1024, L.EPI_BF16, hot=True)
        bench_gemm("cp down hot", 1024, 3072, L.EPI_BF16, hot=True)
    if "norm" in which:
        bench_norm(64, 2048); bench_norm(64, 1024)
    if "attn" in which:
        for fused in (False, True):
            bench_attn("backbone", 64, 16, 8, 352, "fp8", 28, fused)
            bench_attn("backbone bf16", 64, 16, 8, 352, "bf16", 14, fused)
            bench_attn("backbone long", 64, 16, 8, 2048, "fp8", 6, fused)
            bench_attn("code predictor", 64, 16, 8, 9, "bf16", 5, fused)
