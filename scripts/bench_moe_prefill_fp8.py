"""MoE prefill of the Omni talker on fp8 expert weights: the W8A8 grouped GEMMs (csrc/gemm_prefill_f8.hip, MOE instantiations; both
quantiser launches counted) against the bf16 tile arm on the dequantised W_eff copy, one layer at the real shape.

    python scripts/bench_moe_prefill_fp8.py [--tokens 700 6400] [--window 0.4]

One process, two moe_fp8 engines of one layer (prefill_gemm "tile" and "fp8"); per token count the arms alternate -- tile @ 64 | fp8 @ 64 |
tile @ 256 | fp8 @ 256 -- in rounds inside the same call, all warmed, device events around `reps` layer passes (router and shared expert
included in every arm) sized so that one window lasts about --window seconds.  Prints the weight bytes both engines keep on the device, then
one JSON line per token count: per-layer milliseconds (median over rounds, min .. max).  Never compare against a figure from another run.
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_moe_prefill_fp8.py --trace fp8 --tokens 700 [--block 64]
        a run of its own for the kernel times: `--trace ARM` runs ARM for --passes + 1 layer passes and nothing else."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ht_vllm_omni_amd.config import get_dims      # noqa: E402
from ht_vllm_omni_amd.engine import TalkerEngine  # noqa: E402
from ht_vllm_omni_amd.weights import make_weights  # noqa: E402

ARMS = (("tile", 64), ("fp8", 64), ("tile", 256), ("fp8", 256))


def timed(eng, a, block, reps):
    eng.moe_block = block
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        eng._moe_mlp_tile(a, eng.layer_w[0])
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[700, 6400])
    ap.add_argument("--window", type=float, default=0.4, help="seconds of device work per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", choices=["tile", "fp8"], default=None)
    ap.add_argument("--block", type=int, default=None)
    ap.add_argument("--passes", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_moe_prefill_fp8: needs an MI355X (no CPU fallback)")
    d = get_dims("omni-talker").with_(layers=1, cp_layers=1, num_code_groups=3, max_model_len=512)
    w = make_weights(d, seed=1, std=0.02)
    engs = {m: TalkerEngine(d, w, kv_dtype="bf16", num_blocks=8, block_size=16, max_batch=8, moe_fp8=True, prefill_gemm=m) for m in ("tile", "fp8")}
    held = {m: sum(t.numel() * t.element_size() for t in {t.data_ptr(): t for t in e._keep}.values()) for m, e in engs.items()}
    print(json.dumps({"weight_bytes_one_layer_engine": held, "saved_per_layer": held["tile"] - held["fp8"]}), flush=True)
    g = torch.Generator().manual_seed(0)
    for T in args.tokens:
        a = torch.randn(T, d.hidden, generator=g).to(torch.bfloat16).cuda()
        if args.trace:
            timed(engs[args.trace], a, args.block, args.passes + 1)
            continue
        for m, blk in ARMS:                                                 # warm-up: code objects, allocator
            timed(engs[m], a, blk, 2)
        reps = [max(2, int(args.window * 1e3 / max(timed(engs[m], a, blk, 3), 1e-3))) for m, blk in ARMS]
        ms = [[] for _ in ARMS]
        for _ in range(args.rounds):
            for i, (m, blk) in enumerate(ARMS):
                ms[i].append(timed(engs[m], a, blk, reps[i]))
        res = {"tokens": T, "mean_rows_per_expert": T * d.moe_top_k / d.moe_experts, "rounds": args.rounds}
        for i, (m, blk) in enumerate(ARMS):
            res[f"{m}{blk}"] = {"ms_per_layer": round(statistics.median(ms[i]), 4), "min": round(min(ms[i]), 4), "max": round(max(ms[i]), 4), "reps": reps[i]}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
