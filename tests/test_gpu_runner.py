"""The worker/runner contract end to end on the GPU: a mini scheduler (block pool, chunked prefill, staggered
arrivals, finish + KV transfer, hipGraph buckets) drives MI355XARWorker; every step is checked against the CPU
oracle driven the same way."""
import pytest
import torch

from ht_vllm_omni_amd.config import get_dims
from ht_vllm_omni_amd.connectors import InProcConnector, OmniKVTransferManager
from ht_vllm_omni_amd.payloads import (OmniCachedRequestData, OmniNewRequestData, OmniSchedulerOutput, SamplingParams,
                                       encode_tensor)
from ht_vllm_omni_amd.sched import BlockPool, truncate_blocks
from ht_vllm_omni_amd.weights import make_weights
from ht_vllm_omni_amd.worker import MI355XARWorker, make_config
from oracle import talker_oracle as O
from tests.util import codes_on_the_oracles_frame, assert_e2e_close

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.mark.parametrize("graphs", [False, True])
def test_worker_runner_matches_oracle(graphs):
    d = get_dims("tiny")
    w = make_weights(d, seed=9, std=0.06, norm_noise=0.1)
    bs, nb = 16, 64
    sp = SamplingParams(temperature=0.0, top_k=0, repetition_penalty=1.0)
    cfg = make_config(d, kv_cache_dtype="fp8", block_size=bs, max_num_seqs=4, num_gpu_blocks_override=nb, weights=w,
                      enforce_eager=not graphs, default_sampling_params=sp)
    wk = MI355XARWorker(cfg, local_rank=0, rank=0)
    wk.init_device(); wk.load_model()
    # measured, per process (round 6): the engine is built on a probe cache and profiled here, resized -- not rebuilt -- below
    budget = wk.determine_available_memory()
    probe_engine, probe_blocks = wk.engine, wk.engine.num_blocks
    assert budget > 0 and wk.memory_accounting in ("process-scoped (KFD)", "snapshot delta") and wk.process_memory_bytes > wk.engine.kv_cache_bytes()
    assert budget <= wk.init_total and probe_blocks >= 8192 // bs
    wk.initialize_from_config(None)
    assert wk.engine is probe_engine and wk.engine.num_blocks == nb and wk.engine.kv_caches[0].shape[1] == nb
    conn = InProcConnector()
    wk.model_runner.kv_transfer_manager = OmniKVTransferManager(conn)
    wk.engine.set_sampling(cp_greedy=1)
    wk.compile_or_warm_up_model()
    run, eng = wk.model_runner, wk.engine
    assert (len(run.graphs) > 0) == graphs

    orc = O.TalkerOracle(d, w, kv_dtype="fp8", num_blocks=nb, block_size=bs)
    pool = BlockPool(nb, bs)
    g = torch.Generator().manual_seed(3)
    spec = {"a": 5, "b": 40, "c": 12}
    prompts = {k: torch.randn(n, d.hidden, generator=g).to(BF16) for k, n in spec.items()}
    tails = {k: torch.randn(t, d.hidden, generator=g).to(BF16) for k, t in (("a", 2), ("b", 0), ("c", 4))}
    pads = {k: torch.randn(d.hidden, generator=g).to(BF16) for k in spec}
    ostate = {k: O.OracleState(tail_text=list(tails[k]), tts_pad=pads[k]) for k in spec}
    def new_req(k):
        pool.allocate(k, spec[k] + 1)
        info = {"talker_prompt_embeds": encode_tensor(prompts[k]), "tts_pad_embed": encode_tensor(pads[k])}
        if tails[k].shape[0]:
            info["tailing_text_hidden"] = encode_tensor(tails[k])
        return OmniNewRequestData(req_id=k, prompt_token_ids=[d.codec_pad_id] * spec[k], block_ids=(pool.block_ids(k),),
                                  sampling_params=sp, additional_information=info)

    def cached(keys):
        new_blocks = []
        for k in keys:
            st = run.requests[k]
            nb_new = pool.allocate(k, st.num_computed + 2)
            new_blocks.append((nb_new,) if nb_new else None)
        return OmniCachedRequestData(req_ids=list(keys), new_block_ids=new_blocks)

    def oracle_prefill(k):
        _, ids, h = orc.prefill([ostate[k]], [prompts[k]], [pool.block_ids(k)])
        return int(ids[0]), h[0]

    def force(k, tok, h):            # keep the GPU on the oracle's trajectory (1-ulp logit flips must not fork the run)
        r = run.rows.index(k)
        eng.input_ids[r] = tok
        eng.last_hidden[r] = h.cuda()

    def check_decode(keys, out):
        ol, oi, oh, oc, osl = orc.decode_step([ostate[k] for k in keys], [pool.block_ids(k) for k in keys])
        for j, k in enumerate(keys):
            i = out.req_id_to_index[k]
            if codes_on_the_oracles_frame(out.pooler_output[i]["audio_codes"], oc[j:j + 1], orc.last_cp_logits[j:j + 1], what=f"{k}: audio codes")[0]:
                assert_e2e_close(out.pooler_output[i]["hidden"], oh[j:j + 1], mean_tol=6e-3, what=f"{k} hidden", deferred_rstd=True)      # a decode step's qkv / gate_up (gemm.hip PRO 3)
            got = out.sampled_token_ids[i][0]
            if got != int(oi[j]):
                top = torch.topk(ol[j], 2).values
                assert (top[0] - top[1]).item() <= 2 ** -6, f"{k}: sampled id differs without a near-tie"
            force(k, int(oi[j]), oh[j])

    # step 1: a whole prompt, b first chunk of 32
    so = OmniSchedulerOutput(scheduled_new_reqs=[new_req("a"), new_req("b")], num_scheduled_tokens={"a": 5, "b": 32},
                             total_num_scheduled_tokens=37)
    assert wk.execute_model(so) is None
    out = wk.sample_tokens(None)
    tok, h = oracle_prefill("a")
    assert out.sampled_token_ids[out.req_id_to_index["a"]] == [tok] and out.sampled_token_ids[out.req_id_to_index["b"]] == []
    assert_e2e_close(out.pooler_output[out.req_id_to_index["a"]]["hidden"][-1:], h[None], mean_tol=6e-3, what="a prefill hidden")
    force("a", tok, h)
    # step 2: a decodes, b finishes its prompt
    so = OmniSchedulerOutput(scheduled_cached_reqs=cached(["a", "b"]), num_scheduled_tokens={"a": 1, "b": 8}, total_num_scheduled_tokens=9)
    wk.execute_model(so); out = wk.sample_tokens(None)
    check_decode(["a"], out)
    tok, h = oracle_prefill("b")
    assert out.sampled_token_ids[out.req_id_to_index["b"]] == [tok]
    force("b", tok, h)
    # step 3: a, b decode; c arrives
    so = OmniSchedulerOutput(scheduled_new_reqs=[new_req("c")], scheduled_cached_reqs=cached(["a", "b"]),
                             num_scheduled_tokens={"a": 1, "b": 1, "c": 12}, total_num_scheduled_tokens=14)
    wk.execute_model(so); out = wk.sample_tokens(None)
    check_decode(["a", "b"], out)
    tok, h = oracle_prefill("c")
    assert out.sampled_token_ids[out.req_id_to_index["c"]] == [tok]
    force("c", tok, h)
    # steps 4-6: all decode
    for _ in range(3):
        so = OmniSchedulerOutput(scheduled_cached_reqs=cached(["a", "b", "c"]), num_scheduled_tokens={"a": 1, "b": 1, "c": 1},
                                 total_num_scheduled_tokens=3)
        wk.execute_model(so); out = wk.sample_tokens(None)
        check_decode(["a", "b", "c"], out)
    # step 7: a finishes -> KV transfer, ack, row reuse; b, c keep decoding (batch condensed)
    seq_a = ostate["a"].seq_len
    fin = {"a": {"seq_len": seq_a, "block_ids": truncate_blocks(pool.block_ids("a"), seq_a, bs)}}
    so = OmniSchedulerOutput(finished_req_ids={"a"}, finished_requests_needing_kv_transfer=fin,
                             scheduled_cached_reqs=cached(["b", "c"]), num_scheduled_tokens={"b": 1, "c": 1}, total_num_scheduled_tokens=2)
    wk.execute_model(so); out = wk.sample_tokens(None)
    assert out.kv_extracted_req_ids == ["a"]
    check_decode(["b", "c"], out)
    kv, _ = conn.get("0", "1", "omni_0_to_1_kv_cache_a")
    k0 = kv["layer_blocks"]["key_cache"][0]
    assert k0.shape == (seq_a, d.kv_heads, d.head_dim) and k0.dtype == torch.uint8       # fp8 blocks travel as raw bytes
    ref_k, _ = O.extract_kv(orc.kv[0].data.view(torch.uint8), fin["a"]["block_ids"], seq_a)
    assert (k0 != ref_k).float().mean().item() < 0.1
    pool.free_request("a")
    if graphs:
        assert out.cudagraph_stats["replays"] >= 5 and out.cudagraph_stats["eager_steps"] == 0
    wk.shutdown()


@pytest.mark.parametrize("graphs", [False, True])
def test_mixed_sampling_batch_with_prefill_inside_padded_bucket(graphs):
    """Rows a2 / a3: four requests with four different SamplingParams share the
    captured step and each is sampled with ITS parameters and RNG key (oracle: sample_row per request); in the step where
    three of them decode while the fourth's prompt completes, the bucket-4 graph runs over the fourth's row too -- its KV
    blocks, first token, hidden state, position and counters must come out exactly as in eager mode / the oracle."""
    from ht_vllm_omni_amd.runner import request_seed
    d = get_dims("tiny")
    w = make_weights(d, seed=9, std=0.06, norm_noise=0.1)
    bs, nb = 16, 64
    cfg = make_config(d, kv_cache_dtype="fp8", block_size=bs, max_num_seqs=4, num_gpu_blocks_override=nb, weights=w,
                      enforce_eager=not graphs)
    wk = MI355XARWorker(cfg, local_rank=0, rank=0)
    wk.init_device(); wk.load_model(); wk.initialize_from_config(None)
    wk.engine.set_sampling(cp_greedy=1)
    wk.compile_or_warm_up_model()
    run, eng = wk.model_runner, wk.engine
    sps = {"a": SamplingParams(temperature=0.0, top_k=0, repetition_penalty=1.0),
           "b": SamplingParams(temperature=0.8, top_k=10, repetition_penalty=1.1, seed=7),
           "c": SamplingParams(temperature=1.2, top_k=0, repetition_penalty=1.0, seed=None),
           "d": SamplingParams(temperature=0.9, top_k=5, top_p=0.9, repetition_penalty=1.3, seed=3)}
    okw = {k: dict(greedy=sp.greedy, temperature=sp.temperature or 1.0, top_k=sp.top_k, top_p=sp.top_p,
                   rep_penalty=sp.repetition_penalty, seed=request_seed(k, sp)) for k, sp in sps.items()}
    orc = O.TalkerOracle(d, w, kv_dtype="fp8", num_blocks=nb, block_size=bs)
    pool = BlockPool(nb, bs)
    g = torch.Generator().manual_seed(31)
    spec = {"a": 5, "b": 19, "c": 12, "d": 23}
    prompts = {k: torch.randn(n, d.hidden, generator=g).to(BF16) for k, n in spec.items()}
    pads = {k: torch.randn(d.hidden, generator=g).to(BF16) for k in spec}
    ostate = {k: O.OracleState(tail_text=[], tts_pad=pads[k]) for k in spec}

    def new_req(k):
        pool.allocate(k, spec[k] + 1)
        info = {"talker_prompt_embeds": encode_tensor(prompts[k]), "tts_pad_embed": encode_tensor(pads[k])}
        return OmniNewRequestData(req_id=k, prompt_token_ids=[d.codec_pad_id] * spec[k], block_ids=(pool.block_ids(k),),
                                  sampling_params=sps[k], additional_information=info)

    def cached(keys):
        nbk = []
        for k in keys:
            new = pool.allocate(k, run.requests[k].num_computed + 2)
            nbk.append((new,) if new else None)
        return OmniCachedRequestData(req_ids=list(keys), new_block_ids=nbk)

    def force(k, tok, h, got):
        r = run.rows.index(k)
        eng.input_ids[r] = tok
        eng.last_hidden[r] = h.cuda()
        if got != tok:                                  # keep the repetition-penalty bitmap on the oracle's trajectory too
            eng.seen[r, got] = 0
            eng.seen[r, tok] = 1

    def check_token(k, got, tok, logits_row, step):
        if got != tok:
            m = O.sample_row_margin(logits_row, step=step, **okw[k])
            assert m <= 2e-2, f"{k}: sampled {got} != oracle {tok} with score margin {m}"

    def oracle_prefill(keys, out):
        for k in keys:
            lg, ids, h = orc.prefill([ostate[k]], [prompts[k]], [pool.block_ids(k)], sampling=[okw[k]])
            got = out.sampled_token_ids[out.req_id_to_index[k]]
            assert len(got) == 1
            check_token(k, got[0], int(ids[0]), lg[0], 0)
            force(k, int(ids[0]), h[0], got[0])

    def oracle_decode(keys, out):
        steps = [len(ostate[k].out_ids) for k in keys]
        ol, oi, oh, oc, osl = orc.decode_step([ostate[k] for k in keys], [pool.block_ids(k) for k in keys],
                                              sampling=[okw[k] for k in keys])
        for j, k in enumerate(keys):
            i = out.req_id_to_index[k]
            if codes_on_the_oracles_frame(out.pooler_output[i]["audio_codes"], oc[j:j + 1], orc.last_cp_logits[j:j + 1], what=f"{k}: audio codes")[0]:
                assert_e2e_close(out.pooler_output[i]["hidden"], oh[j:j + 1], mean_tol=6e-3, what=f"{k} hidden", deferred_rstd=True)      # a decode step's qkv / gate_up (gemm.hip PRO 3)
            got = out.sampled_token_ids[i][0]
            check_token(k, got, int(oi[j]), ol[j], steps[j])
            force(k, int(oi[j]), oh[j], got)
        return osl

    # step 1: a, b, c prefill whole prompts
    so = OmniSchedulerOutput(scheduled_new_reqs=[new_req(k) for k in "abc"], num_scheduled_tokens={k: spec[k] for k in "abc"},
                             total_num_scheduled_tokens=sum(spec[k] for k in "abc"))
    wk.execute_model(so); out = wk.sample_tokens(None)
    oracle_prefill("abc", out)
    # step 2: a, b, c decode (3 live rows in the bucket-4 graph) while d's prompt completes in the SAME step on row 3
    so = OmniSchedulerOutput(scheduled_new_reqs=[new_req("d")], scheduled_cached_reqs=cached("abc"),
                             num_scheduled_tokens={"a": 1, "b": 1, "c": 1, "d": spec["d"]}, total_num_scheduled_tokens=3 + spec["d"])
    wk.execute_model(so); out = wk.sample_tokens(None)
    oracle_decode("abc", out)
    oracle_prefill("d", out)
    rd = run.rows.index("d")
    assert rd == 3 and int(eng.positions[rd]) == spec["d"] and int(eng.seq_lens[rd]) == spec["d"] + 1 and int(eng.steps[rd]) == 1
    # d's prompt KV must be exactly what the oracle wrote (the padded row's "decode" must not have touched its blocks)
    for layer in (0, d.layers - 1):
        blk = pool.block_ids("d")
        got_k = eng.kv_caches[layer][0][blk].cpu().view(torch.uint8)
        ref_k = orc.kv[layer].data[0][blk].view(torch.uint8)
        assert (got_k[:, : , :, :].reshape(-1)[: spec["d"] * d.kv_heads * d.head_dim] != ref_k.reshape(-1)[: spec["d"] * d.kv_heads * d.head_dim]).float().mean().item() < 0.1
        tail_rows = got_k.reshape(len(blk) * bs, -1)[spec["d"]:]
        assert int(tail_rows.abs().sum()) == 0, "slots past d's prompt were written by the padded row's decode step"
    # steps 3-5: all four decode
    for _ in range(3):
        so = OmniSchedulerOutput(scheduled_cached_reqs=cached("abcd"), num_scheduled_tokens={k: 1 for k in "abcd"}, total_num_scheduled_tokens=4)
        wk.execute_model(so); out = wk.sample_tokens(None)
        osl = oracle_decode("abcd", out)
        assert torch.equal(eng.slot_mapping[:4].cpu(), osl)
    if graphs:
        assert out.cudagraph_stats["replays"] == 4 and out.cudagraph_stats["eager_steps"] == 0
    wk.shutdown()


def test_engine_core_loop_scheduler_worker_oracle():
    """Row a12 end to end on the GPU: MI355XARScheduler (admission under a token budget, chunked prefill, block
    allocation, stop at max_tokens, KV hand-off + ack) drives MI355XARWorker through TalkerStageEngine; the token
    streams and the per-step audio codes must be the oracle's, driven by the same schedule."""
    from ht_vllm_omni_amd.scheduler import MI355XARScheduler, Request, TalkerStageEngine
    d = get_dims("tiny")
    w = make_weights(d, seed=9, std=0.06, norm_noise=0.1)
    bs, nb = 16, 64
    sp = SamplingParams(temperature=0.0, top_k=0, repetition_penalty=1.0, max_tokens=5, stop_token_ids=())
    cfg = make_config(d, kv_cache_dtype="fp8", block_size=bs, max_num_seqs=4, num_gpu_blocks_override=nb, weights=w,
                      enforce_eager=False, default_sampling_params=sp)
    wk = MI355XARWorker(cfg, local_rank=0, rank=0)
    wk.init_device(); wk.load_model(); wk.initialize_from_config(None)
    conn = InProcConnector()
    wk.model_runner.kv_transfer_manager = OmniKVTransferManager(conn)
    wk.engine.set_sampling(cp_greedy=1)
    wk.compile_or_warm_up_model()
    run, eng = wk.model_runner, wk.engine
    sched = MI355XARScheduler(num_blocks=nb, block_size=bs, max_num_seqs=4, max_num_batched_tokens=48, max_model_len=d.max_model_len,
                              need_send_cache=True)
    core = TalkerStageEngine(wk, sched)
    orc = O.TalkerOracle(d, w, kv_dtype="fp8", num_blocks=nb, block_size=bs)
    g = torch.Generator().manual_seed(4)
    spec = {"a": 7, "b": 60, "c": 20}                     # b needs two prefill chunks under the 48-token budget
    prompts = {k: torch.randn(n, d.hidden, generator=g).to(BF16) for k, n in spec.items()}
    pads = {k: torch.randn(d.hidden, generator=g).to(BF16) for k in spec}
    ostate = {k: O.OracleState(tail_text=[], tts_pad=pads[k]) for k in spec}
    reqs = {}
    for k, n in spec.items():
        info = {"talker_prompt_embeds": encode_tensor(prompts[k]), "tts_pad_embed": encode_tensor(pads[k])}
        reqs[k] = Request(request_id=k, num_prompt_tokens=n, prompt_token_ids=[d.codec_pad_id] * n, sampling_params=sp,
                          additional_information=info)
        core.add_request(reqs[k])
    prefilled, streams, finished = set(), {k: [] for k in spec}, {}
    for step in range(40):
        outs = core.step()
        decoding = [o.request_id for o in outs if o.request_id in prefilled and o.new_token_ids]
        if decoding:                                    # the oracle takes the same decode step for the same requests
            ol, oi, oh, oc, _ = orc.decode_step([ostate[k] for k in decoding], [sched.pool.block_ids(k) for k in decoding])
        for o in outs:
            k = o.request_id
            if o.finished:
                finished[k] = o
            if not o.new_token_ids:
                continue
            if k not in prefilled:                      # the step that completed the prompt: oracle prefill of the whole prompt
                _, ids, h = orc.prefill([ostate[k]], [prompts[k]], [sched.pool.block_ids(k)])
                tok, hid = int(ids[0]), h[0]
                prefilled.add(k)
            else:
                j = decoding.index(k)
                tok, hid = int(oi[j]), oh[j]
                assert torch.equal(o.pooling_output["audio_codes"], oc[j:j + 1]), f"{k}: audio codes at step {step}"
            got = o.new_token_ids[0]
            streams[k].append(got)
            assert got == tok, f"{k}: token {got} != oracle {tok} at step {step}"
            if k in run.requests:                       # keep the device on the oracle's hidden state (1-ulp drift must not fork)
                r = run.rows.index(k)
                eng.last_hidden[r] = hid.cuda()
        if not sched.has_unfinished_requests() and not sched.waiting_for_transfer_free and not sched.requests_needing_kv_transfer:
            break
    assert all(len(v) == 5 for v in streams.values()), streams
    assert set(finished) == set(spec) and all(o.finish_reason == "length" for o in finished.values())
    assert not sched.requests and sched.pool.num_free == nb - 1 and run.rows == []
    for k, n in spec.items():                           # every finished request shipped ceil(seq / 16) blocks of KV
        kv, _ = conn.get("0", "1", f"omni_0_to_1_kv_cache_{k}")
        assert kv["metadata"]["seq_len"] == n + 4
    wk.shutdown()


def test_engine_core_loop_async_scheduling_is_bit_identical_to_the_synchronous_loop():
    """the async output path (sample_tokens -> AsyncStepOutput, get_output() after the next dispatch) hands
    on the same ids, code frames, hidden states and KV hand-offs as the synchronous loop the oracle test above pins -- at the
    1.7B width with sampling on, chunked prefill, a finishing request per few steps and late arrivals."""
    from ht_vllm_omni_amd.scheduler import MI355XARScheduler, Request, TalkerStageEngine
    from ht_vllm_omni_amd.runner import AsyncStepOutput
    d = get_dims("tts-1.7b").with_(layers=2, max_model_len=512)
    w = make_weights(d, seed=9, std=0.02)
    bs, nb = 16, 256

    def run_once(async_on):
        sp0 = SamplingParams(temperature=0.9, top_k=50, repetition_penalty=1.05, seed=5)
        cfg = make_config(d, kv_cache_dtype="fp8", block_size=bs, max_num_seqs=64, num_gpu_blocks_override=nb, weights=w,
                          default_sampling_params=sp0, async_scheduling=async_on)
        wk = MI355XARWorker(cfg, local_rank=0, rank=0)
        wk.init_device(); wk.load_model(); wk.initialize_from_config(None)
        conn = InProcConnector()
        wk.model_runner.kv_transfer_manager = OmniKVTransferManager(conn)
        wk.engine.set_sampling(cp_greedy=0, cp_temperature=0.9, cp_top_k=50)
        wk.compile_or_warm_up_model()
        sched = MI355XARScheduler(num_blocks=nb, block_size=bs, max_num_seqs=64, max_num_batched_tokens=512,
                                  max_model_len=d.max_model_len, need_send_cache=True, async_scheduling=async_on)
        core = TalkerStageEngine(wk, sched)
        g = torch.Generator().manual_seed(4)
        pending = []
        for i in range(72):
            n = int(torch.randint(3, 40, (1,), generator=g))
            m = int(torch.randint(2, 14, (1,), generator=g))
            sp = SamplingParams(temperature=0.9, top_k=50, repetition_penalty=1.05, seed=5 + i, max_tokens=m, stop_token_ids=())
            info = {"talker_prompt_embeds": encode_tensor((torch.randn(n, d.hidden, generator=g) * 0.5).to(BF16)),
                    "tts_pad_embed": encode_tensor((torch.randn(d.hidden, generator=g) * 0.02).to(BF16)),
                    "tailing_text_hidden": encode_tensor((torch.randn(3, d.hidden, generator=g) * 0.02).to(BF16))}
            pending.append(Request(request_id=f"r{i}", num_prompt_tokens=n, prompt_token_ids=[d.codec_pad_id] * n, sampling_params=sp,
                                   additional_information=info, ignore_eos=True))
        for r in pending[:60]:
            core.add_request(r)
        pending = pending[60:]
        streams, codes, hid, kvlen, steps, handles = {}, {}, {}, {}, 0, 0
        while (pending or core.has_work()) and steps < 400:
            if steps % 3 == 2 and pending:
                core.add_request(pending.pop(0))
            for o in core.step():
                streams.setdefault(o.request_id, []).extend(o.new_token_ids)
                if o.pooling_output is not None and o.new_token_ids:
                    codes.setdefault(o.request_id, []).append(o.pooling_output["audio_codes"].clone())
                    hid.setdefault(o.request_id, []).append(o.pooling_output["hidden"].clone())
                if o.finished and o.kv_transfer_params:
                    kvlen[o.request_id] = o.kv_transfer_params["kv_metadata"]["seq_len"]
            handles += sum(isinstance(h, AsyncStepOutput) for _, h in core.inflight)
            steps += 1
        core.step()
        chains = int(wk.engine.status[2])
        rows, free = list(wk.model_runner.rows), sched.pool.num_free
        wk.shutdown()
        return streams, codes, hid, kvlen, handles, rows, free, chains

    s0, c0, h0, k0, n0, rows0, free0, _ = run_once(False)
    s1, c1, h1, k1, n1, rows1, free1, _ = run_once(True)
    assert n0 == 0 and n1 > 0, "the async loop keeps AsyncStepOutput handles in flight"
    assert len(s0) == 72 and s0 == s1, "token streams"
    assert k0 == k1 and len(k0) == 72
    for k in s0:
        assert len(c0[k]) == len(c1[k]) and all(torch.equal(a, b) for a, b in zip(c0[k], c1[k])), f"{k}: code frames"
        assert all(torch.equal(a, b) for a, b in zip(h0[k], h1[k])), f"{k}: hidden states"
    assert rows0 == rows1 == [] and free0 == free1 == nb - 1


def test_omni_request_prompt_built_on_device_then_decodes_with_queued_text_steps():
    """A Qwen3-Omni style request carries the thinker's outputs, not ready talker embeddings: the runner's prompt builder
    (prompt_builder_omni = the reference's talker_preprocess_prefill) makes the prompt and the text-step queue on the
    device; prefill + decode then follow the oracle fed with the same prompt rows and queue (builder parity itself:
    tests/test_gpu_prompt_builder.py)."""
    from ht_vllm_omni_amd.prompt_builder_omni import OmniPromptIds
    d = get_dims("tiny")
    w = make_weights(d, seed=9, std=0.06, norm_noise=0.1)
    bs, nb, Ht, I = 16, 64, 64, 96
    g = torch.Generator().manual_seed(12)
    rnd = lambda *s, sc=0.15: (torch.randn(*s, generator=g) * sc).to(BF16)
    mlp = lambda: {"fc1_w": rnd(I, Ht), "fc1_b": rnd(I), "fc2_w": rnd(d.hidden, I), "fc2_b": rnd(d.hidden)}
    ids = OmniPromptIds(im_start=5, system=6, user=7, assistant=8, tts_pad_token=12, audio=9, image=10, video=11,
                        codec_nothink=140, codec_think_bos=141, codec_think_eos=142, codec_pad=d.codec_pad_id, codec_bos=149,
                        speaker_ids={"ethan": 160}, default_speaker="ethan")
    pbw = {"text": mlp(), "hidden": mlp()}
    sp = SamplingParams(temperature=0.0, top_k=0, repetition_penalty=1.0)
    cfg = make_config(d, kv_cache_dtype="fp8", block_size=bs, max_num_seqs=4, num_gpu_blocks_override=nb, weights=w,
                      enforce_eager=True, default_sampling_params=sp, prompt_builder={"weights": pbw, "ids": ids})
    wk = MI355XARWorker(cfg, local_rank=0, rank=0)
    wk.init_device(); wk.load_model(); wk.initialize_from_config(None)
    wk.engine.set_sampling(cp_greedy=1)
    wk.compile_or_warm_up_model()
    run, eng = wk.model_runner, wk.engine
    assert run.prompt_builder is not None and torch.equal(run.prompt_builder.codec_embed.cpu(), w["embed"])
    # thinker side: system + user (3 audio tokens) + assistant (7 generated tokens)
    chat = [5, 6, 30, 31] + [5, 7, 32, 9, 9, 9, 33] + [5, 8, 34]
    seq = chat + [35, 36, 37, 38, 39, 40, 41]
    T = len(seq)
    info = {"thinker_prefill_embeddings": encode_tensor(torch.randn(T, Ht, generator=g)),
            "thinker_hidden_states": encode_tensor(torch.randn(T, Ht, generator=g)),
            "thinker_sequences": seq, "thinker_input_ids": chat, "speaker": "Ethan",
            "tts_bos_embed": encode_tensor(torch.randn(1, 1, Ht, generator=g)), "tts_eos_embed": encode_tensor(torch.randn(1, 1, Ht, generator=g)),
            "tts_pad_embed": encode_tensor(torch.randn(1, 1, Ht, generator=g))}
    P = 7 + 9                                   # user segment rows + the 9-row assistant block (system is skipped)
    pool = BlockPool(nb, bs)
    pool.allocate("o", P + 1)
    nr = OmniNewRequestData(req_id="o", prompt_token_ids=[0] * P, block_ids=(pool.block_ids("o"),), sampling_params=sp,
                            additional_information=info)
    so = OmniSchedulerOutput(scheduled_new_reqs=[nr], num_scheduled_tokens={"o": P}, total_num_scheduled_tokens=P)
    assert wk.execute_model(so) is None
    out = wk.sample_tokens(None)
    st = run.requests["o"]
    assert st.prompt_embeds.shape == (P, d.hidden) and st.tail.shape == (7 - 1 + 1, d.hidden)      # generated[1:] + tts_eos
    assert st.info["prefill_consumed_text_tokens"] == 1
    orc = O.TalkerOracle(d, w, kv_dtype="fp8", num_blocks=nb, block_size=bs)
    ost = O.OracleState(tail_text=list(st.tail.cpu()), tts_pad=st.tts_pad.cpu())
    _, oids, oh = orc.prefill([ost], [st.prompt_embeds.clone()], [pool.block_ids("o")])
    assert out.sampled_token_ids[0] == [int(oids[0])]
    eng.input_ids[0] = int(oids[0]); eng.last_hidden[0] = oh[0].cuda()
    for stepno in range(9):                     # 7 queued text steps, then tts_pad
        nb_new = pool.allocate("o", st.num_computed + 2)
        so = OmniSchedulerOutput(scheduled_cached_reqs=OmniCachedRequestData(req_ids=["o"], new_block_ids=[(nb_new,) if nb_new else None]),
                                 num_scheduled_tokens={"o": 1}, total_num_scheduled_tokens=1)
        wk.execute_model(so); out = wk.sample_tokens(None)
        ol, oi, oh, oc, _ = orc.decode_step([ost], [pool.block_ids("o")])
        assert torch.equal(out.pooler_output[0]["audio_codes"], oc[0:1]), f"audio codes at decode step {stepno}"
        eng.input_ids[0] = int(oi[0]); eng.last_hidden[0] = oh[0].cuda()
    wk.shutdown()


def test_engine_core_soak_with_request_churn():
    """40 requests of mixed prompt / output lengths through an 8-row batch with a tight block pool (preemption by
    recompute included) and sampled decoding: every request finishes with its length, the pool and the persistent batch
    come back empty, the captured step is used throughout, and a second run of the same workload reproduces every token
    (hash RNG keyed by request step: no dependence on batch composition is allowed to leak into the streams... except
    through the positions of rows -- which the row-independent kernels must not let through)."""
    from ht_vllm_omni_amd.scheduler import MI355XARScheduler, Request, TalkerStageEngine
    d = get_dims("tiny")
    w = make_weights(d, seed=9, std=0.06, norm_noise=0.1)
    bs, nb = 16, 40
    dflt = SamplingParams(temperature=0.9, top_k=20, repetition_penalty=1.05, seed=5)

    def run_once(async_on=False):
        cfg = make_config(d, kv_cache_dtype="fp8", block_size=bs, max_num_seqs=8, num_gpu_blocks_override=nb, weights=w,
                          enforce_eager=False, default_sampling_params=dflt, async_scheduling=async_on)
        wk = MI355XARWorker(cfg, local_rank=0, rank=0)
        wk.init_device(); wk.load_model(); wk.initialize_from_config(None)
        wk.engine.set_sampling(cp_greedy=0, cp_temperature=0.9, cp_top_k=20)
        wk.compile_or_warm_up_model()
        sched = MI355XARScheduler(num_blocks=nb, block_size=bs, max_num_seqs=8, max_num_batched_tokens=64,
                                  max_model_len=d.max_model_len, need_send_cache=False, async_scheduling=async_on)
        core = TalkerStageEngine(wk, sched)
        g = torch.Generator().manual_seed(77)
        want = {}
        pending = []
        for i in range(40):
            n = int(torch.randint(3, 70, (1,), generator=g))
            m = int(torch.randint(1, 24, (1,), generator=g))
            sp = SamplingParams(temperature=0.9, top_k=20, repetition_penalty=1.05, seed=5, max_tokens=m, stop_token_ids=())
            pe = torch.randn(n, d.hidden, generator=g).to(BF16)
            pad = torch.randn(d.hidden, generator=g).to(BF16)
            info = {"talker_prompt_embeds": encode_tensor(pe), "tts_pad_embed": encode_tensor(pad)}
            pending.append(Request(request_id=f"r{i}", num_prompt_tokens=n, prompt_token_ids=[d.codec_pad_id] * n, sampling_params=sp,
                                   additional_information=info, ignore_eos=True))
            want[f"r{i}"] = m
        streams, finished, steps = {}, {}, 0
        while (pending or core.has_work()) and steps < 4000:
            for _ in range(2):                                   # requests keep arriving while others decode
                if pending:
                    core.add_request(pending.pop(0))
            for o in core.step():
                streams.setdefault(o.request_id, []).extend(o.new_token_ids)
                if o.finished:
                    finished[o.request_id] = o.finish_reason
            steps += 1
        core.step()                                              # delivers the last finished ids: the runner drops its rows
        stats = dict(wk.model_runner.cudagraph_stats)
        free, rows = sched.pool.num_free, list(wk.model_runner.rows)
        wk.shutdown()
        return want, streams, finished, steps, stats, free, rows

    want, streams, finished, steps, stats, free, rows = run_once()
    assert set(finished) == set(want) and all(r == "length" for r in finished.values()), (len(finished), steps)
    assert all(len(streams[k]) == want[k] for k in want), {k: (len(streams[k]), want[k]) for k in want if len(streams[k]) != want[k]}
    assert free == nb - 1 and rows == [], (free, rows)
    assert stats["replays"] > 0
    _, streams2, *_ = run_once()
    assert streams2 == streams, "same workload, same seeds -> same token streams"
    # async scheduling (stage_configs/qwen3_tts.yaml:16): every step is dispatched before its predecessor's outputs are read; the
    # arrival pattern relative to the steps shifts (outputs come one loop turn later), the requests' streams do not
    want3, streams3, finished3, _, stats3, free3, rows3 = run_once(async_on=True)
    assert set(finished3) == set(want) and all(r == "length" for r in finished3.values())
    assert streams3 == streams, "async scheduling changes no request's token stream"
    assert free3 == nb - 1 and rows3 == [] and stats3["replays"] > 0


def test_chunk_streamer_fed_by_the_real_runner_ships_the_oracles_frames():
    """SURVEY 8f rank 1 on the GPU (f1 had no -m gpu test): scheduler + worker + runner with graphs, the per-step
    audio codes of the native step go through CodecChunkStreamer and the connector under {req}_{stage}_{chunk}; every shipped
    window must hold exactly the ORACLE's frames of that request in the reference's layout (codebook-major, left context +
    new frames, chunk sizes by the load-dependent initial-chunk rule), the last chunk flagged finished."""
    from ht_vllm_omni_amd.scheduler import MI355XARScheduler, Request, TalkerStageEngine
    from ht_vllm_omni_amd.stage_input_processors import CodecChunkStreamer
    d = get_dims("tiny")
    Q = d.num_code_groups
    w = make_weights(d, seed=9, std=0.06, norm_noise=0.1)
    bs, nb = 16, 64
    n_out = {"a": 13, "b": 7, "c": 10}
    cfg = make_config(d, kv_cache_dtype="fp8", block_size=bs, max_num_seqs=4, num_gpu_blocks_override=nb, weights=w, enforce_eager=False)
    wk = MI355XARWorker(cfg, local_rank=0, rank=0)
    wk.init_device(); wk.load_model(); wk.initialize_from_config(None)
    wk.engine.set_sampling(cp_greedy=1)
    wk.compile_or_warm_up_model()
    run, eng = wk.model_runner, wk.engine
    chunk_conn = InProcConnector()
    streamer = CodecChunkStreamer(codec_chunk_frames=4, codec_left_context_frames=2, max_num_seqs=4, num_quantizers=Q, connector=chunk_conn)
    wk.model_runner.kv_transfer_manager = OmniKVTransferManager(InProcConnector())
    sched = MI355XARScheduler(num_blocks=nb, block_size=bs, max_num_seqs=4, max_num_batched_tokens=64, max_model_len=d.max_model_len,
                              chunk_streamer=streamer, need_send_cache=True)      # finished requests keep their blocks until acked
    core = TalkerStageEngine(wk, sched)
    orc = O.TalkerOracle(d, w, kv_dtype="fp8", num_blocks=nb, block_size=bs)
    g = torch.Generator().manual_seed(8)
    spec = {"a": 9, "b": 21, "c": 14}
    prompts = {k: torch.randn(n, d.hidden, generator=g).to(BF16) for k, n in spec.items()}
    pads = {k: torch.randn(d.hidden, generator=g).to(BF16) for k in spec}
    ostate = {k: O.OracleState(tail_text=[], tts_pad=pads[k]) for k in spec}
    for k, n in spec.items():
        sp = SamplingParams(temperature=0.0, top_k=0, repetition_penalty=1.0, max_tokens=n_out[k], stop_token_ids=())
        info = {"talker_prompt_embeds": encode_tensor(prompts[k]), "tts_pad_embed": encode_tensor(pads[k])}
        core.add_request(Request(request_id=k, num_prompt_tokens=n, prompt_token_ids=[d.codec_pad_id] * n, sampling_params=sp,
                                 additional_information=info))
    frames = {k: [] for k in spec}               # the runner's audio codes per decode step, each checked against the oracle's
    prefilled, forks = set(), 0
    for step in range(60):
        outs = core.step()
        decoding = [o.request_id for o in outs if o.request_id in prefilled and o.new_token_ids]
        if decoding:
            ol, oi, oh, oc, _ = orc.decode_step([ostate[k] for k in decoding], [sched.pool.block_ids(k) for k in decoding])
        for o in outs:
            k = o.request_id
            if not o.new_token_ids:
                continue
            on_frame = True
            if k not in prefilled:
                _, ids, h = orc.prefill([ostate[k]], [prompts[k]], [sched.pool.block_ids(k)])
                tok, hid = int(ids[0]), h[0]
                prefilled.add(k)
            else:
                j = decoding.index(k)
                tok, hid = int(oi[j]), oh[j]
                # the frame the runner produced is the frame that must be shipped; against the oracle's it may fork at a verified near-tie
                # (tests/util.py), after which this step's sampled id reads another input: the row is put back on the oracle's trajectory
                on_frame = bool(codes_on_the_oracles_frame(o.pooling_output["audio_codes"], oc[j:j + 1], orc.last_cp_logits[j:j + 1],
                                                           what=f"{k}: audio codes at step {step}")[0])
                frames[k].append(o.pooling_output["audio_codes"][0].tolist())
                forks += int(not on_frame)
            if on_frame and o.new_token_ids[0] != tok:      # same frame, another greedy id: only at a near-tie of the oracle's logits
                top = torch.topk(ol[decoding.index(k)], 2).values if k in decoding else None
                assert top is not None and (top[0] - top[1]).item() <= 2 ** -6, (k, step, "sampled id differs without a near-tie")
            if k in run.requests:
                eng.last_hidden[run.rows.index(k)] = hid.cuda()
                eng.input_ids[run.rows.index(k)] = tok
        if not sched.has_unfinished_requests() and not sched.waiting_for_transfer_free and not sched.requests_needing_kv_transfer:
            break
    assert all(len(frames[k]) == n_out[k] - 1 for k in spec)
    assert forks <= sum(n_out.values()) // 4, f"{forks} frames left the oracle's greedy path"
    # what the connector received: per request the chunks' NEW frames tile the oracle's frame sequence exactly (no gap, no
    # replay), each chunk's left context is the frames right before its new ones, the last chunk is flagged finished
    for k in spec:
        F = frames[k]
        covered, chunk_id, sent_finished = 0, 0, False
        while f"{k}_0_{chunk_id}" in chunk_conn.store:
            payload, _ = chunk_conn.get("0", "1", f"{k}_0_{chunk_id}")
            lc = payload["left_context_size"]
            codes = torch.tensor(payload["code_predictor_codes"]).reshape(Q, -1).t().tolist()     # codebook-major -> frames
            new = codes[lc:]
            assert 0 <= lc <= 2 and len(new) >= 1 and not sent_finished
            assert new == F[covered:covered + len(new)], f"{k} chunk {chunk_id}: new frames differ from the decoded ones"
            assert codes[:lc] == F[covered - lc:covered], f"{k} chunk {chunk_id}: left context"
            covered += len(new)
            sent_finished = bool(payload["finished"])
            chunk_id += 1
        assert covered == len(F) and chunk_id >= 2 and sent_finished, (k, covered, len(F), chunk_id)
        assert k not in streamer.code_prompt_token_ids          # state dropped when the request finished
    wk.shutdown()
