"""Accuracy gate for ALL 15 group logits of the code predictor's persistent chain (cp_pair_kernel + cp_chain_kernel, csrc/cp_chain.hip).

The reference keeps the HF-exact RMSNorm in the predictor on purpose: fused-norm numerics "compound across the 15 autoregressive steps"
(qwen3_tts_code_predictor_vllm.py:22-33).  Since round 6 the chain's qkv / gate_up stages apply the rstd to the fp32 sums (DEFER), so the
statement that licenses that for the backbone (tests/test_gpu_parity_full.py, three-way) is made here for the predictor, group by group:

  (1) HIP: the product library, chains on, greedy, the logits of every group;
  (2) the oracle with the reference's bf16 rounding points, greedy -- its codes are THE frame;
  (3) the oracle with fp32 activations end to end, teacher-forced onto (2)'s frame (forced_codes), i.e. the arithmetic both bf16
      pipelines approximate, evaluated on the inputs (2) read.

A row enters group g's statistics while HIP's codes of the groups before g equal the frame (otherwise it read another input); a row may
leave the frame only at a verified near-tie of the oracle's logits.  With e_hip = |HIP - fp32| and e_ref = |bf16 oracle - fp32| on those
rows: mean and p99 of e_hip within 1.3 x those of e_ref (the backbone's factor) for every group and pooled, and the pooled mean within
POOLED_DRIFT x e_ref's (below).  A stage that is wrong by an ulp or two at groups 2-15 -- which no other test reads -- fails here.

Shapes: B = 49 is the smallest batch on cp_chain_kernel<true> (32-row gate_up tiles; four 16-row groups live, the last with one row);
B = 17 runs cp_chain_kernel<false> with one row in its second row group and the pair kernel's Bp + B packing at its edge.  Weights: flat
N(0, 0.02) heads (rows fork at near-ties: at least half stay per group) and weights.peak_predictor_heads (wide margins: nearly every
row stays on the frame through group 15, so the late groups are measured on nearly all rows)."""
import json
import os

import pytest
import torch

from ht_vllm_omni_amd.config import get_dims
from ht_vllm_omni_amd.weights import make_weights, peak_predictor_heads
from oracle import talker_oracle as O
from tests.util import BF16, codes_on_the_oracles_frame, report_dir

pytestmark = pytest.mark.gpu

FACTOR = 1.3            # tests/test_gpu_parity_full.py closer_than_reference: the backbone's factor, not a new number
# Drift bound on the pooled mean: the claim behind the deferred rstd is "one rounding FEWER than the reference", i.e. a ratio
# mean(e_hip) / mean(e_ref) <= 1.0.  The bound is max(1.0, 1.1 x the largest pooled ratio measured over the four cases below) x the
# reference's own error -- anchored to e_ref, never to HIP's figure; the 10 % are for the rows a near-tie fork removes on another box.
# Measured pooled mean ratios (MI355X; per group 0.923 ... 0.960, p99 0.917 ... 0.967: DESIGN section 4) -- "one rounding fewer" holds:
POOLED_MEASURED = {"B49-flat": 0.9470, "B49-peaked": 0.9401, "B17-flat": 0.9456, "B17-peaked": 0.9368}
POOLED_DRIFT = max(1.0, 1.1 * max(POOLED_MEASURED.values()))          # 1.0417

_SEEDS = {49: (21, 5), 17: (23, 7)}          # (weights, inputs): margins of the peaked sets checked on the CPU oracle for these


def _case(B, kind):
    d = get_dims("tts-1.7b").with_(layers=1, max_model_len=256)          # the released predictor: 5 layers, 16 groups; one backbone layer
    w = make_weights(d, seed=_SEEDS[B][0], std=0.02)
    if kind == "peaked":
        w = peak_predictor_heads(d, w)
    g = torch.Generator().manual_seed(_SEEDS[B][1])
    code0 = torch.randint(1, d.codebook, (B,), generator=g)
    return d, w, code0, w["embed"][code0], torch.randn(B, d.hidden, generator=g).to(BF16)


def _oracle(d, w, code0, e0, lh, act_dtype, forced=None):
    keep = O.BF16
    O.BF16 = act_dtype                                 # every rounding point of the restatement is `.to(BF16)`
    try:
        return O.TalkerOracle(d, w).code_predictor(code0, e0.to(act_dtype), lh.to(act_dtype), do_sample=False, return_logits=True,
                                                   forced_codes=forced)
    finally:
        O.BF16 = keep


def margins_in_ulps(lg):
    top = torch.topk(lg.float(), 2, dim=-1).values
    return (top[..., 0] - top[..., 1]) / torch.exp2(torch.floor(torch.log2(top[..., 0].abs().clamp_min(1e-30))) - 7)


@pytest.mark.parametrize("kind", ["flat", "peaked"])
@pytest.mark.parametrize("B", [49, 17])
def test_predictor_chain_group_logits_three_way(B, kind):
    from ht_vllm_omni_amd.engine import TalkerEngine
    d, w, code0, e0, lh = _case(B, kind)
    Q = d.num_code_groups
    eng = TalkerEngine(d, w, kv_dtype="bf16", num_blocks=8, max_batch=64)
    codes, lg = eng.code_predictor(code0.to(torch.int32).cuda(), e0.cuda(), lh.cuda(), greedy=True, return_logits=True)
    torch.cuda.synchronize()
    assert eng.chain_error() == 0
    codes, lg = codes.cpu(), lg.cpu()
    ref_codes, lg16 = _oracle(d, w, code0, e0, lh, torch.bfloat16)
    codes32, lg32 = _oracle(d, w, code0, e0, lh, torch.float32, forced=ref_codes)
    assert torch.equal(codes32, ref_codes)
    # a fork off the frame must be a verified near-tie of the oracle's logits
    codes_on_the_oracles_frame(codes, ref_codes, lg16, what=f"B={B} {kind}")
    if kind == "peaked":
        wide = float((margins_in_ulps(lg16) >= 8).float().mean())
        assert wide >= 0.995, f"the construction must give wide margins: {wide:.4f} of the picks >= 8 ulps"

    q99 = lambda e: float(torch.quantile(e, 0.99))
    groups, pool_h, pool_r = [], [], []
    on = torch.ones(B, dtype=torch.bool)               # rows whose codes of the groups before g equal the frame
    for g in range(1, Q):
        n = int(on.sum())
        if kind == "flat":
            assert n >= B // 2, f"group {g}: only {n} of {B} rows still on the oracle's frame"
        e_hip = (lg[on, g - 1].float() - lg32[on, g - 1].float()).abs().flatten()
        e_ref = (lg16[on, g - 1].float() - lg32[on, g - 1].float()).abs().flatten()
        pool_h.append(e_hip); pool_r.append(e_ref)
        groups.append({"group": g, "hip_mean": float(e_hip.mean()), "ref_mean": float(e_ref.mean()), "hip_p99": q99(e_hip), "ref_p99": q99(e_ref),
                       "rows_compared": n, "scale": float(lg32[on, g - 1].abs().max())})
        on = on & (codes[:, g] == ref_codes[:, g])
    e_hip, e_ref = torch.cat(pool_h), torch.cat(pool_r)
    pooled = {"hip_mean": float(e_hip.mean()), "ref_mean": float(e_ref.mean()), "hip_p99": q99(e_hip), "ref_p99": q99(e_ref),
              "rows_compared": sum(r["rows_compared"] for r in groups), "scale": float(lg32.abs().max())}
    for r in groups + [pooled]:
        r["mean_ratio"], r["p99_ratio"] = r["hip_mean"] / r["ref_mean"], r["hip_p99"] / r["ref_p99"]
    path = os.path.join(report_dir(), "cp_three_way.json")
    report = json.load(open(path)) if os.path.exists(path) else {}
    report[f"B{B}-{kind}"] = {"groups": groups, "pooled": pooled}
    json.dump(report, open(path, "w"), indent=1)
    print(f"B{B}-{kind}: pooled {pooled}; per-group mean ratios {[round(r['mean_ratio'], 4) for r in groups]}; p99 ratios {[round(r['p99_ratio'], 4) for r in groups]}")

    if kind == "peaked":
        share = pooled["rows_compared"] / (B * (Q - 1))
        assert share >= 0.95, f"only {share:.3f} of the {B} x {Q - 1} (row, group) pairs were compared"
    for r in groups:
        assert r["hip_mean"] <= FACTOR * r["ref_mean"] and r["hip_p99"] <= FACTOR * r["ref_p99"], r
    assert pooled["hip_mean"] <= FACTOR * pooled["ref_mean"] and pooled["hip_p99"] <= FACTOR * pooled["ref_p99"], pooled
    assert pooled["hip_mean"] <= POOLED_DRIFT * pooled["ref_mean"], pooled
