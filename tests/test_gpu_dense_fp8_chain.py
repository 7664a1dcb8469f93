"""TalkerEngine(dense_fp8="chain"): the backbone's persistent launches on the fp8 bytes (csrc/bb_chain.hip W8 stage sets, chain_gemm WSRC 4)
against the same engine launch per op (dense_fp8=True, csrc/gemm_w8.hip) -- bit for bit -- and against the fp32-activation oracle."""
import functools

import pytest
import torch

import tests.test_gpu_dense_fp8 as base
from ht_vllm_omni_amd.config import get_dims
from ht_vllm_omni_amd.sched import BlockPool
from ht_vllm_omni_amd.weights import make_weights
from tests.util import BF16, assert_e2e_close

BS = base.BS
UNRELEASED = (("hidden", 1536), ("inter", 4608), ("q_heads", 12), ("kv_heads", 6))      # the second BB_SHAPES triple (tests/test_gpu_chain.py)


@functools.lru_cache(maxsize=None)
def _model(shape):
    d = get_dims("tts-1.7b").with_(layers=2, max_model_len=256, **dict(shape))
    return d, make_weights(d, seed=23, std=0.02, norm_noise=0.1)


def _steps(shape, B, dense_fp8, mode="eager", num_blocks=None, kv="fp8"):
    """Ragged prompts + decode steps (base._run) of one engine: the engine, the prompt lengths and what every step left."""
    from ht_vllm_omni_amd.engine import TalkerEngine
    d, w = _model(shape)
    eng = TalkerEngine(d, w, dense_fp8=dense_fp8, kv_dtype=kv, num_blocks=num_blocks or 4 * B + 8, block_size=BS, max_batch=B)
    lens = torch.randint(3, 30, (B,), generator=torch.Generator().manual_seed(B)).tolist()
    out = base._run(eng, d, lens, mode)
    assert eng.dense_fp8 is True and eng.chain_error() == 0 and eng.status[:2].tolist() == [0, 0], eng.status.tolist()
    assert eng.chains_ran() == (3 if dense_fp8 == "chain" else 1), (dense_fp8, eng.chains_ran())
    return eng, lens, out


@functools.lru_cache(maxsize=None)
def _launch_per_op(shape, B, num_blocks):      # the reference of a (shape, rows, cache size): computed once, kept on the host
    return [{k: v.cpu() for k, v in s.items()} for s in _steps(shape, B, True, "eager", num_blocks)[2]]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,B,mode", [((), 64, "eager"), ((), 40, "eager"), ((), 17, "eager"), ((), 3, "eager"), ((), 64, "graph"),
                                          ((), 64, "resize"), (UNRELEASED, 64, "eager")])
def test_w8_chain_equals_the_w8_launch_path(shape, B, mode):
    """64 / 40 rows: bb_chain_kernel (40: last row tile partly filled); 17 / 3 rows: bb_chain_b32_kernel with gate_up on 32 / 16 rows; two
    layers = the launch without the head stage (layer 0 -> qkv of layer 1) and the one with it.  Everything three steps leave is equal."""
    a, _, ra = _steps(shape, B, "chain", mode)
    for s, (sa, sb) in enumerate(zip(ra, _launch_per_op(shape, B, a.num_blocks))):
        for k in sa:
            assert torch.equal(sa[k].cpu(), sb[k]), f"step {s}: {k} of the W8 chain differs from the W8 launch path"


@pytest.mark.gpu
def test_w8_chain_logits_against_the_fp32_activation_oracle(monkeypatch):
    """First decode step at 64 rows against the oracle on dense_fp8_weights with fp32 activations end to end (no rounding between ops).
    Bounds: the default engine's two-layer real-dimension decode step (tests/test_gpu_engine.py test_unreleased_width_runs_both_chains_
    and_matches_oracle: mean 2e-3, 3 ulps, deferred-rstd floors).  Measured: mean 0.0051, max 0.029 (1.8 ulps) at scale 3.9."""
    from ht_vllm_omni_amd.engine import dense_fp8_weights
    from oracle import talker_oracle as O
    B, (d, w) = 64, _model(())
    monkeypatch.setattr(base, "STEPS", 1)
    a, lens, ra = _steps((), B, "chain", kv="bf16")
    x_t = a.inputs_embeds[:B].cpu()                          # the step's backbone input, as the engine's predictor assembled it
    pool = BlockPool(a.num_blocks, BS)                       # base._run's prompts and block tables
    for r, n in enumerate(lens):
        pool.allocate(f"r{r}", n + 2)
    bts = [pool.block_ids(f"r{r}") for r in range(B)]
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.randn(n, d.hidden, generator=g).to(BF16) for n in lens])
    pos, req = torch.cat([torch.arange(n) for n in lens]), [r for r, n in enumerate(lens) for _ in range(n)]
    monkeypatch.setattr(O, "BF16", torch.float32)            # every rounding point of the oracle is `.to(BF16)`
    orc = O.TalkerOracle(d, dense_fp8_weights(d, w), kv_dtype="bf16", num_blocks=a.num_blocks, block_size=BS)
    orc.backbone(x.float(), pos, req, bts, lens)
    ref = orc.compute_logits(orc.backbone(x_t.float(), torch.tensor(lens), list(range(B)), bts, [n + 1 for n in lens]))
    assert_e2e_close(ra[1]["logits"], ref, mean_tol=2e-3, max_ulps=3, what="W8 chain: first decode step's logits", deferred_rstd=True)


@pytest.mark.parametrize("preset,dense_fp8,kw,match", [("tiny", "chains", {}, "dense_fp8='chains'"), ("tiny", "on", {}, "dense_fp8='on'"),
                                                       ("tiny", "chain", dict(tp_size=2), "dense_fp8 needs"),
                                                       ("omni-moe-tiny", "chain", {}, "dense_fp8 needs")])
def test_dense_fp8_chain_refusals(preset, dense_fp8, kw, match):
    from ht_vllm_omni_amd.engine import TalkerEngine
    with pytest.raises(ValueError, match=match):
        TalkerEngine(get_dims(preset), {}, dense_fp8=dense_fp8, **kw)
