"""Whole decode step, W3 (tts-1.7b, B = 64, fp8 KV, one hipGraph per step): the product default (bf16, persistent chains), bf16 with the
backbone launch per op (omni_debug_bb_chain(0); the predictor keeps its chain, as under dense_fp8), dense_fp8 (W8 launch per op) and
dense_fp8="chain" (the W8 stage sets of bb_chain.hip) -- four graphs in one
process, timed round-robin over the same context window (mean context --ctx at its middle).  Report only: the default does not change.  usage: python scripts/ab_dense_w8.py [--steps 48] [--rounds 5]"""
import argparse, ctypes as C, os, sys, types
os.environ["OMNI_TALKER_DEBUG"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from ht_vllm_omni_amd.config import get_dims
from ht_vllm_omni_amd.engine import TalkerEngine, dense_fp8_weights
from ht_vllm_omni_amd.weights import make_weights

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=48)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--ctx", type=int, default=352)
a = ap.parse_args()
B = 64
args = types.SimpleNamespace(batch=B, num_blocks=4096, warmup=0, steps=a.steps + 64, ttfa_steps=0, ctx_extra=0, target_ctx=a.ctx)
torch.cuda.set_device(0)
d = get_dims("tts-1.7b")
w = make_weights(d, seed=1234, std=0.02, device="cuda")
kw = dict(kv_dtype="fp8", num_blocks=args.num_blocks, block_size=16, max_batch=B, allow_eos=False)
engines = {"bf16": TalkerEngine(d, dense_fp8_weights(d, w), **kw), "dense_fp8": TalkerEngine(d, w, dense_fp8=True, **kw),
           "dense_fp8 chain": TalkerEngine(d, w, dense_fp8="chain", **kw)}
del w
lib = engines["bf16"].lib
lib.omni_debug_bb_chain.argtypes = [C.c_int]; lib.omni_debug_bb_chain.restype = None
graphs = {}
for name, eng, bb in (("bf16 chains (default)", engines["bf16"], 1), ("bf16 launch per op", engines["bf16"], 0), ("dense_fp8", engines["dense_fp8"], 1),
                      ("dense_fp8 chain", engines["dense_fp8 chain"], 1)):
    if not hasattr(eng, "start"):
        eng.set_sampling(greedy=0, temperature=0.9, top_k=50, rep_penalty=1.05, seed=42, cp_greedy=0, cp_temperature=0.9, cp_top_k=50)
        bench.setup_requests(d, eng, args)
        for _ in range(a.ctx - int(eng.seq_lens[:B].float().mean().item()) - a.steps // 2):
            eng.decode_step(B)
        eng.start = (eng.positions.clone(), eng.seq_lens.clone())      # every timed window of every arm covers the same contexts
    lib.omni_debug_bb_chain(bb)
    eng.decode_step(B); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.decode_step(B)
    graphs[name] = (g, eng, eng.chains_ran())
lib.omni_debug_bb_chain(1)
res = {n: [] for n in graphs}
for r in range(a.rounds):
    for n, (g, eng, _) in graphs.items():
        g.replay()
        eng.positions.copy_(eng.start[0]); eng.seq_lens.copy_(eng.start[1]); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            g.replay()
        e1.record(); torch.cuda.synchronize()
        res[n].append(e0.elapsed_time(e1) / a.steps)
for n, (g, eng, ran) in graphs.items():
    v = sorted(res[n])
    print(f"{n:24s} chains_ran={ran} ms/step " + " ".join(f"{x:.4f}" for x in res[n]) + f"   median {v[len(v) // 2]:.4f} min {v[0]:.4f} max {v[-1]:.4f}"
          f"   mean ctx {float(eng.seq_lens[:B].float().mean()):.0f}  chain_error {eng.chain_error()}")
