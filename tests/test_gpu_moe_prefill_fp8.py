"""MoE prefill on fp8 expert weights (the MOE instantiations of csrc/gemm_prefill_f8.hip; omni_moe_prefill_experts_fp8): every stage against
float64 on the device's own bytes, both block heights bit-identical, a graph capture, and prefill_wide of a moe_fp8 engine."""
import pytest
import torch

from ht_vllm_omni_amd import ops
from ht_vllm_omni_amd.engine import fp8_quant_rows, frag_shuffle, frag_unshuffle
from tests.test_gpu_prefill_fp8 import _rows
from tests.util import BF16, assert_e2e_close, make_moe_weights

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn


def _unperm(q):
    """Token-major rows with byte 32 q + 8 e + j of every 128-k chunk holding k = 32 e + 8 q + j -> k order."""
    return q.reshape(q.shape[0], -1, 4, 4, 8).transpose(2, 3).reshape(q.shape)


def _lin(qx, sx, qw, sw):
    return ((qx.view(F8).double() @ qw.view(F8).double().T) * sx.double()[:, None] * sw.double()[None, :]).to(BF16).double()


def _gu_ref(qx, sx, qw, sw):
    g, u = _lin(qx, sx, qw, sw).chunk(2, dim=1)      # omni_silu_mul's three roundings
    return ((g * torch.sigmoid(g)).to(BF16).double() * u).to(BF16)


def _down_ref(qa, sa, qw, sw, wgt):
    return (_lin(qa, sa, qw, sw) * wgt.double()[:, None]).to(BF16)


def _close(got, ref, what):
    assert_e2e_close(got, ref, mean_tol=5e-4 * max(1.0, ref.float().abs().max().item()), max_ulps=2, what=what)


def _fp8_weights(H, E, I, Is, seed):
    w = make_moe_weights(H, E, I, Is, seed=seed)
    d = {k: v.cuda() for k, v in w.items() if k not in ("gate_up", "down")}
    for n in ("gate_up", "down"):
        w[n + "_q"], w[n + "_s"] = fp8_quant_rows(w[n])
        d[n + "_f"], d[n + "_scale"] = frag_shuffle(w[n + "_q"]).cuda(), w[n + "_s"].cuda()
    return w, d


@pytest.mark.parametrize("H,E,k,I,Is,T,blocks,e0,n_local", [
    (128, 4, 2, 128, 0, 9, (64,), 0, 4),                # one MFMA per output, most blocks nearly empty
    (256, 4, 2, 384, 64, 150, (64, 256), 0, 4),         # groups longer than a block; a 3-chunk down, shorter than the ring's prologue
    (256, 16, 4, 128, 64, 40, (64,), 4, 4),             # expert-parallel window
    (1024, 128, 8, 384, 768, 300, (64, 256), 0, 128),   # the talker's shape
])
def test_stages_against_float64_on_the_devices_bytes_and_blocks_alike(H, E, k, I, Is, T, blocks, e0, n_local):
    w, d = _fp8_weights(H, E, I, Is, seed=5 * E + k)
    x = _rows(torch.Generator().manual_seed(T + H), T, H)
    xc, win, outs = x.cuda(), slice(e0, e0 + n_local), []
    idx, wts = ops.moe_route(ops.gemm_tile(xc, ops._frag(d["router"]))[:, :E].contiguous(), k, False)
    sh = gate = None
    if Is:
        sh = ops.gemm_tile(ops.silu_mul(ops.gemm_tile(xc, ops._frag(d["shared_gate_up"]))), ops._frag(d["shared_down"]))
        gate = ops.gemm_tile(xc, ops._frag(d["shared_gate"]))
    for block in blocks:
        out, st = ops.moe_prefill_experts(xc, idx, wts, d["gate_up_f"][win], d["down_f"][win], E=E, e0=e0, shared=sh, gate_logit=gate, block=block,
                                          gate_up_scale=d["gate_up_scale"][win], down_scale=d["down_scale"][win], return_stages=True)
        outs.append(out)
        st, (qx, sx) = {n: t.cpu() for n, t in st.items()}, fp8_quant_rows(x)
        assert torch.equal(_unperm(st["x8"]), qx) and torch.equal(st["x_scale"], sx), "(a) token quantiser"
        owner = st["block_expert"].long().repeat_interleave(block)                 # local expert of every batch row, -1: none
        tok, owned, live = st["row_token"].long(), owner >= 0, st["row_token"] >= 0
        qa, sa = fp8_quant_rows(st["act"][owned])
        assert torch.equal(_unperm(st["act8"])[owned], qa) and torch.equal(st["act_scale"][owned], sa), "(c) act quantiser"
        assert not st["act8"][owned & ~live].any() and not st["act"][owned & ~live].any(), "pad rows inside an expert's blocks"
        act_ref, y_ref = torch.zeros_like(st["act"]), torch.zeros_like(st["y"])
        for e in range(n_local):
            r = torch.where(live & (owner == e))[0]
            act_ref[r] = _gu_ref(qx[tok[r]], sx[tok[r]], w["gate_up_q"][e0 + e], w["gate_up_s"][e0 + e])
            y_ref[r] = _down_ref(_unperm(st["act8"])[r], st["act_scale"][r], w["down_q"][e0 + e], w["down_s"][e0 + e], st["row_weight"][r])
        _close(st["act"][live], act_ref[live], "(b) gate_up stage")
        _close(st["y"][live], y_ref[live], "(d) down stage")
        rows = st["slot_row"].long().view(T, k).gather(1, idx.cpu().long().argsort(1))      # (e) ascending expert index, bf16 accumulation
        acc = torch.zeros(T, H, dtype=BF16)
        for j in range(k):
            acc = (acc.float() + torch.where(rows[:, j, None] >= 0, st["y"][rows[:, j].clamp(min=0)], torch.zeros_like(acc)).float()).to(BF16)
        if Is:
            acc = (acc.float() + (torch.sigmoid(gate.cpu()[:, :1].float()).to(BF16).float() * sh.cpu().float()).to(BF16).float()).to(BF16)
        assert torch.equal(out.cpu(), acc), "(e) combine"
    assert all(torch.equal(o, outs[0]) for o in outs), "block height changed the bits"


def test_block_is_captured_in_a_graph_and_replays_on_other_routings():
    k, (_, d), g = 2, _fp8_weights(256, 4, 128, 64, seed=11), torch.Generator().manual_seed(4)
    x1, x2 = (torch.randn(40, 256, generator=g).to(BF16).cuda() for _ in range(2))
    eager = [ops.moe_block_prefill(x, d, k) for x in (x1, x2)]
    assert not torch.equal(eager[0][1], eager[1][1]), "the two inputs must route differently"
    xs = x1.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, idx, _ = ops.moe_block_prefill(xs, d, k)
    for x, (e_out, e_idx, _) in ((x1, eager[0]), (x2, eager[1]), (x1, eager[0])):
        xs.copy_(x)
        graph.replay()
        assert torch.equal(idx, e_idx) and torch.equal(out, e_out)


def _reference_prefill(eng, x, pos, req, slots):
    """prefill_wide's layer loop on the project's ops, the two expert GEMMs in float64 on fp8_quant_rows operands."""
    d = eng.d
    kw = dict(q_heads=eng.hq_l, kv_heads=eng.hkv_l, head_dim=d.head_dim, kv_dtype=eng.kv_code)
    resid, delta = x.clone(), None
    for l in range(d.layers):
        w = eng.layer_w[l]
        kc, vc = torch.zeros_like(eng.kv_caches[l][0]), torch.zeros_like(eng.kv_caches[l][1])
        a = ops.rmsnorm(None, w["ln1"], d.eps, delta=delta, residual=resid)
        q = ops.qknorm_rope_kvwrite(ops.gemm_tile(a, w["wqkv_f"]), w["qnorm"], w["knorm"], pos, eng.cos_sin, slots, kc, vc, eps=d.eps, **kw)
        o = ops.paged_attn_prefill(q, kc, vc, eng.block_table, req, pos, block_size=eng.block_size, **kw)
        a = ops.rmsnorm(None, w["ln2"], d.eps, delta=ops.gemm_tile(o, w["wo_f"]), residual=resid)
        idx, wts = ops.moe_route(ops.gemm_tile(a, w["moe_router_f"]), d.moe_top_k, d.moe_norm_topk)
        sh = ops.gemm_tile(ops.silu_mul(ops.gemm_tile(a, w["moe_shared_gate_up_f"])), w["moe_shared_down_f"])
        gate = ops.gemm_tile(a, w["moe_shared_gate_f"])[:, :1]
        qgu, qdn, sgu, sdn = frag_unshuffle(w["moe_gate_up_f"].cpu()), frag_unshuffle(w["moe_down_f"].cpu()), w["moe_gate_up_scale"].cpu(), w["moe_down_scale"].cpu()
        (qa, sa), idx, wts = fp8_quant_rows(a.cpu()), idx.cpu().long(), wts.cpu()
        out = torch.zeros(a.shape, dtype=BF16)
        for e in range(d.moe_experts):                   # ascending expert index: the combine's accumulation order
            t, j = torch.where(idx == e)
            if t.numel():
                out[t] = (out[t].float() + _down_ref(*fp8_quant_rows(_gu_ref(qa[t], sa[t], qgu[e], sgu[e])), qdn[e], sdn[e], wts[t, j]).float()).to(BF16)
        delta = (out.cuda() + (torch.sigmoid(gate.float()).to(BF16) * sh)).to(BF16)
    return ops.rmsnorm(None, eng.final_norm, d.eps, delta=delta, residual=resid)


def test_engine_prefill_on_fp8_experts_against_float64_expert_gemms():
    from ht_vllm_omni_amd.config import get_dims
    from ht_vllm_omni_amd.engine import TalkerEngine
    from ht_vllm_omni_amd.weights import make_weights
    d = get_dims("omni-talker").with_(layers=2, cp_layers=1, num_code_groups=3, max_model_len=512)
    lens, bs, B = [3, 30, 7, 19, 12], 16, 5
    eng = TalkerEngine(d, make_weights(d, seed=23, std=0.02), moe_fp8=True, prefill_gemm="fp8", kv_dtype="bf16", num_blocks=3 * B + 8, block_size=bs, max_batch=B)
    lw = eng.layer_w[0]
    assert lw["moe_gate_up_f"].dtype == torch.uint8 and lw["moe_down_f"].dtype == torch.uint8 and "moe_gate_up" not in lw and "moe_gate_up_t" not in lw
    eng.block_table[:B, :3] = torch.arange(3 * B, dtype=torch.int32).view(B, 3).cuda()      # three 16-token blocks per request
    x = torch.randn(sum(lens), d.hidden, generator=torch.Generator().manual_seed(5)).to(BF16).cuda()
    pos = torch.cat([torch.arange(n) for n in lens]).to(torch.int32).cuda()
    req = torch.repeat_interleave(torch.arange(B), torch.tensor(lens)).to(torch.int32).cuda()
    slots = eng.block_table[req.long(), (pos // bs).long()].long() * bs + pos % bs
    last = (torch.tensor(lens).cumsum(0) - 1).cuda()
    hl = eng.prefill_wide(x, pos, req, slots)[last]
    ref = _reference_prefill(eng, x, pos, req, slots)[last]
    diff = (hl.float() - ref.float()).abs()
    print(f"fp8 MoE prefill vs float64 expert GEMMs: mean |diff| {diff.mean():.4g}, max {diff.max():.4g}, scale {ref.float().abs().max():.4g}")
    # Two realisations of the act rows' fp8 quantisation noise.  Measured: mean |diff| 0.001954, max 0.01953 (1.25 ulps) at scale 3.72.  Bound: 2 x.
    assert_e2e_close(hl, ref, mean_tol=0.0039, max_ulps=2.5, what="last-token hidden states")
    eng.input_ids[:B], eng.last_hidden[:B] = eng.compute_logits(hl).argmax(-1).to(torch.int32), hl      # ... and the decode step runs on the cache this prefill wrote
    eng.positions[:B], eng.seq_lens[:B], eng.steps[:B] = pos[last] + 1, pos[last] + 2, 1
    eng.decode_step(B)
    assert eng.status[:2].tolist() == [0, 0]
