"""MoE prefill of the Omni talker: the device dispatch (csrc/moe_prefill.hip) against the padded dispatch, one layer at the real shape.

    python scripts/bench_moe_prefill.py [--tokens 700 6400] [--window 0.4]
        one process; per token count the arms alternate -- padded | device @ 64 | device @ 256 -- in rounds inside the same call, both
        warmed, device events around `reps` layer passes sized so that one window lasts about --window seconds; prints one JSON line
        per token count: per-layer milliseconds (median over rounds, min .. max) and whether the outputs are equal bit for bit.
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_moe_prefill.py --trace device --tokens 700 [--block 64]
        a run of its own for the launch count: `--trace ARM` runs ARM for --passes layer passes after one warm-up pass and nothing
        else; launches per layer = the kernel-stats total calls / (passes + 1).

The padded arm is the parent behaviour (one host read per layer); never compare against a figure from another run."""
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

ARMS = (("padded", None), ("device", 64), ("device", 256))


def run(eng, a, arm, block, reps):
    eng.moe_dispatch, eng.moe_block = arm, block
    w = eng.layer_w[0]
    out = None
    for _ in range(reps):
        out = eng._moe_mlp_tile(a, w)
    return out


def timed(eng, a, arm, block, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run(eng, a, arm, block, reps)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[700, 6400])
    ap.add_argument("--window", type=float, default=0.4, help="seconds of device work per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", choices=["padded", "device"], default=None)
    ap.add_argument("--block", type=int, default=None)
    ap.add_argument("--passes", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_moe_prefill: needs an MI355X (no CPU fallback)")
    d = get_dims("omni-talker").with_(layers=1, cp_layers=1, num_code_groups=3, max_model_len=512)
    eng = TalkerEngine(d, make_weights(d, seed=1, std=0.02), kv_dtype="bf16", num_blocks=8, block_size=16, max_batch=8)
    g = torch.Generator().manual_seed(0)
    for T in args.tokens:
        a = torch.randn(T, d.hidden, generator=g).to(torch.bfloat16).cuda()
        if args.trace:
            run(eng, a, args.trace, args.block, args.passes + 1)
            torch.cuda.synchronize()
            continue
        outs = [run(eng, a, arm, blk, 2) for arm, blk in ARMS]              # warm-up: code objects, allocator
        torch.cuda.synchronize()
        reps = [max(2, int(args.window * 1e3 / max(timed(eng, a, arm, blk, 3), 1e-3))) for arm, blk in ARMS]
        ms = [[] for _ in ARMS]
        for _ in range(args.rounds):
            for i, (arm, blk) in enumerate(ARMS):
                ms[i].append(timed(eng, a, arm, blk, reps[i]))
        res = {"tokens": T, "mean_rows_per_expert": T * d.moe_top_k / d.moe_experts, "rounds": args.rounds}
        for i, (arm, blk) in enumerate(ARMS):
            name = arm if blk is None else f"{arm}{blk}"
            res[name] = {"ms_per_layer": round(statistics.median(ms[i]), 4), "min": round(min(ms[i]), 4), "max": round(max(ms[i]), 4),
                         "reps": reps[i], "equals_padded": bool(torch.equal(outs[i], outs[0]))}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
