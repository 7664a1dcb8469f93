"""bench.py on the GPU, at the tiny shape: what a plain run does and prints, what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, STEPS = 5, 3


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    """ONE greedy run of the benchmark (the tiny preset, 5 rows), timed from wherever warm-up ends (the preset holds 512
    positions), shared by the tests below: (the JSON line, stderr, the dump)."""
    out = tmp_path_factory.mktemp("bench") / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--model", "tiny",
                        "--batch", str(B), "--num-blocks", "256", "--target-ctx", "0", "--greedy", "--dump-outputs", str(out)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0]), r.stderr, {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}


def test_a_plain_run_prints_the_headline_line_and_nothing_that_takes_a_run_of_its_own(plain_run):
    j, _, _ = plain_run
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int), ("ms_per_step", float),
                 ("higher_is_better", bool), ("dtype", str), ("config", dict), ("roofline", dict)):
        assert isinstance(j[k], t), (k, type(j[k]))
    assert j["metric"] == "speech-tokens/sec" and j["unit"] == "speech-tokens/s" and j["higher_is_better"] is True and j["dtype"] == "bf16"
    assert j["steps"] == STEPS and j["warmup"] == 1 and j["ms_per_step"] > 0
    assert abs(j["value"] - B * 1e3 / j["ms_per_step"]) / j["value"] < 1e-6      # the timed steps' tokens over the timed steps' wall time
    r = j["roofline"]
    assert abs(r["achieved"] * 1e9 * r["event_ms_per_step"] * 1e-3 - r["bytes_per_step"]["total"]) / r["bytes_per_step"]["total"] < 1e-6
    # the legs behind --full
    for k in ("cpu_baseline", "engine_loop", "p50_ttfa_ms", "ttfa", "replicas", "allreduce"):
        assert k not in j, k
    for k in ("families", "breakdown", "copy_probe_gbs"):
        assert k not in r, k


def test_dump_outputs_is_the_last_timed_steps_output_record(plain_run):
    """Greedy rows: every dumped id is a maximum of its dumped logits row (the dump is ONE step's record, taken before anything else
    ran), inside the codec's allowed ids; the code frames are codebook entries and the hidden states are bf16 values."""
    from ht_vllm_omni_amd.config import get_dims
    d = get_dims("tiny")
    _, _, a = plain_run
    assert sorted(a) == ["audio_codes", "last_hidden", "logits", "token_ids"]
    assert all(x.dtype in (np.float32, np.float64) and np.isfinite(x).all() for x in a.values())
    assert a["token_ids"].shape == (B,) and a["audio_codes"].shape == (B, d.num_code_groups)
    assert a["last_hidden"].shape == (B, d.hidden) and a["logits"].shape == (B, d.vocab)
    ids = a["token_ids"].astype(np.int64)
    assert np.array_equal(ids, a["token_ids"]) and ((ids >= 1) & (ids < d.codebook)).all()      # EOS is masked in the bench
    assert np.array_equal(a["logits"][np.arange(B), ids], a["logits"].max(axis=1))
    assert (a["logits"][:, d.codebook:] == -1e9).all() and (a["logits"][:, 1:d.codebook] > -1e9).all()
    codes = a["audio_codes"].astype(np.int64)
    assert np.array_equal(codes, a["audio_codes"]) and ((codes >= 0) & (codes < d.codebook)).all()
    import torch
    h = torch.from_numpy(a["last_hidden"])
    assert torch.equal(h.to(torch.bfloat16).float(), h) and float(h.abs().max()) > 0
