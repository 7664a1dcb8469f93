"""TalkerEngine(dense_fp8=True) (engine A: backbone decode GEMMs on fp8 bytes, csrc/gemm_w8.hip) against the default engine on
dense_fp8_weights(...) (engine B: the same W_eff as bf16): bit for bit everything a step leaves behind, whichever schedule B takes."""
import pytest
import torch

from ht_vllm_omni_amd.config import get_dims
from ht_vllm_omni_amd.sched import BlockPool, slot_of
from ht_vllm_omni_amd.weights import make_weights
from tests.util import BF16

pytestmark = pytest.mark.gpu
BS, STEPS = 16, 3


def _run(eng, d, lens, mode):
    """Prefill of ragged prompts + STEPS decode steps (mode "graph": each step one replay of a captured hipGraph); what every step left."""
    B = len(lens)
    if mode == "resize":
        eng.resize_kv_cache(eng.num_blocks + 8)
    pool = BlockPool(eng.num_blocks, BS)
    for r, n in enumerate(lens):
        pool.allocate(f"r{r}", n + STEPS + 1)
    bts = [pool.block_ids(f"r{r}") for r in range(B)]
    bt = torch.zeros(eng.max_batch, eng.bt_stride, dtype=torch.int32)
    for r in range(B):
        bt[r, :len(bts[r])] = torch.tensor(bts[r])
    eng.block_table.copy_(bt)
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.randn(n, d.hidden, generator=g).to(BF16) for n in lens])
    pos = torch.cat([torch.arange(n) for n in lens]).to(torch.int32)
    req = torch.cat([torch.full((n,), r) for r, n in enumerate(lens)]).to(torch.int32)
    slots = torch.tensor([slot_of(bts[int(req[t])], int(pos[t]), BS) for t in range(x.shape[0])])
    hid = eng.prefill(x.cuda(), pos.cuda(), req.cuda(), slots.cuda())
    hl = hid[(torch.tensor(lens).cumsum(0) - 1).cuda()]
    out = [dict(prefill=hl.clone())]
    eng.input_ids[:B] = eng.compute_logits(hl).argmax(-1).to(torch.int32)
    eng.last_hidden[:B] = hl
    eng.positions[:B] = torch.tensor(lens, dtype=torch.int32).cuda()
    eng.seq_lens[:B] = (torch.tensor(lens, dtype=torch.int32) + 1).cuda()
    eng.steps[:B] = 1
    eng.text_step[:B] = torch.randn(B, d.hidden, generator=g).to(BF16).cuda()
    gr = None
    if mode == "graph":
        keep = {n: getattr(eng, n).clone() for n in ("input_ids", "positions", "seq_lens", "last_hidden", "steps", "seen")}
        kv = [c.clone() for c in eng.kv_caches]
        eng.decode_step(B)                      # warm-up on a copy of the state, then capture, then restore
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            eng.decode_step(B)
        for n, v in keep.items():
            getattr(eng, n).copy_(v)
        for c, v in zip(eng.kv_caches, kv):
            c.copy_(v)
    for _ in range(STEPS):
        gr.replay() if gr is not None else eng.decode_step(B)
        torch.cuda.synchronize()
        out.append({n: getattr(eng, n)[:B].clone() for n in ("logits", "input_ids", "audio_codes", "slot_mapping", "last_hidden")}
                   | {f"kv{l}": c.view(torch.uint8).clone() for l, c in enumerate(eng.kv_caches)})
    return out


@pytest.mark.parametrize("preset,B,kv,mode", [("tiny", 3, "bf16", "eager"), ("tiny", 33, "fp8", "eager"), ("tts-1.7b", 64, "fp8", "eager"),
                                              ("tts-1.7b", 64, "fp8", "graph"), ("tiny", 3, "bf16", "resize")])
def test_dense_fp8_engine_equals_the_default_engine_on_the_dequantised_weights(preset, B, kv, mode):
    from ht_vllm_omni_amd.engine import TalkerEngine, dense_fp8_weights
    big = preset != "tiny"
    d = get_dims(preset).with_(layers=2, max_model_len=256) if big else get_dims(preset)
    w = make_weights(d, seed=23, std=0.02 if big else 0.06, norm_noise=0.1)
    lens = torch.randint(3, 30, (B,), generator=torch.Generator().manual_seed(B)).tolist()
    kw = dict(kv_dtype=kv, num_blocks=4 * B + 8, block_size=BS, max_batch=B)
    a = TalkerEngine(d, w, dense_fp8=True, **kw)
    ra = _run(a, d, lens, mode)
    assert a.chains_ran() & 2 == 0 and a.chain_error() == 0 and a.status[:2].tolist() == [0, 0], (a.chains_ran(), a.status.tolist())
    b = TalkerEngine(d, dense_fp8_weights(d, w), **(kw | dict(num_blocks=a.num_blocks)))      # (A's cache after its resize)
    rb = _run(b, d, lens, "eager")
    assert b.chain_error() == 0 and b.status[:2].tolist() == [0, 0]
    if big:      # both persistent chains in B, the predictor's in A: the tail predicate (who computes layer 0's qkv) is exercised
        assert a.chains_ran() == 1 and b.chains_ran() == 3, (a.chains_ran(), b.chains_ran())
    for s, (sa, sb) in enumerate(zip(ra, rb)):
        for k in sa:
            assert torch.equal(sa[k], sb[k]), f"step {s}: {k} of the dense_fp8 engine differs from the bf16 engine on W_eff"
