"""TalkerOracle.code_predictor(forced_codes=...): teacher forcing for the three-way accuracy test of the predictor
(tests/test_gpu_predictor_accuracy.py).  CPU only."""
import torch

from ht_vllm_omni_amd.config import get_dims
from ht_vllm_omni_amd.weights import make_weights
from oracle import talker_oracle as O
from tests.util import BF16


def _inputs(d, w, B, seed):
    g = torch.Generator().manual_seed(seed)
    code0 = torch.randint(1, d.codebook, (B,), generator=g)
    return code0, w["embed"][code0], torch.randn(B, d.hidden, generator=g).to(BF16)


def test_forcing_the_oracles_own_greedy_codes_reproduces_its_logits():
    d = get_dims("tiny")
    w = make_weights(d, seed=3, std=0.08, norm_noise=0.1)
    orc = O.TalkerOracle(d, w)
    code0, e0, lh = _inputs(d, w, 5, 1)
    codes, lg = orc.code_predictor(code0, e0, lh, do_sample=False, return_logits=True)
    f_codes, f_lg = orc.code_predictor(code0, e0, lh, do_sample=False, return_logits=True, forced_codes=codes)
    assert torch.equal(f_codes, codes) and torch.equal(f_lg, lg)


def test_forced_codes_replace_the_pick_and_feed_the_next_pass():
    d = get_dims("tiny")
    w = make_weights(d, seed=3, std=0.08, norm_noise=0.1)
    orc = O.TalkerOracle(d, w)
    code0, e0, lh = _inputs(d, w, 4, 2)
    codes, lg = orc.code_predictor(code0, e0, lh, do_sample=False, return_logits=True)
    Q = d.num_code_groups
    assert Q >= 3
    other = codes.clone()
    other[0, 1] = (codes[0, 1] + 1) % d.codebook          # row 0 leaves its greedy path at group 1
    f_codes, f_lg = orc.code_predictor(code0, e0, lh, do_sample=False, return_logits=True, forced_codes=other)
    assert torch.equal(f_codes, other), "the forced frame is what comes back, whatever the logits say"
    assert torch.equal(f_lg[:, 0], lg[:, 0]), "group 1 reads the same inputs"
    assert torch.equal(f_lg[1:], lg[1:]), "rows are independent"
    assert not torch.equal(f_lg[0, 1], lg[0, 1]), "group 2 of row 0 read the forced code's embedding"
