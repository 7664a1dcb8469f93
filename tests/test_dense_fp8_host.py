"""Host side of the dense fp8 backbone (no GPU): the W8 fragment layout of include/omni_talker.h, the worker's `quantization`, the refusals."""
import types

import pytest
import torch

from ht_vllm_omni_amd.config import get_dims


@pytest.mark.parametrize("K", [256, 512, 768])
def test_frag_shuffle_w8_is_the_documented_permutation(K):
    from ht_vllm_omni_amd.engine import frag_shuffle_w8, frag_unshuffle_w8
    N, P = 32, K // 512
    q = torch.arange(N * K, dtype=torch.int32).reshape(N, K)      # every element distinct: the formula is checked per byte
    s = frag_shuffle_w8(q)
    assert s.shape == q.shape and torch.equal(s.flatten().sort().values, q.flatten()) and torch.equal(frag_unshuffle_w8(s), q)
    row, k = torch.meshgrid(torch.arange(N), torch.arange(K), indexing="ij")
    st, lane = k // 32, (k % 32) // 8 * 16 + row % 16
    off = torch.where(st < 16 * P, ((st // 16) * 8 + st % 8) * 1024 + lane * 16 + (st % 16) // 8 * 8 + k % 8,
                      P * 8192 + (st - 16 * P) * 512 + lane * 8 + k % 8)
    assert torch.equal(s.reshape(N // 16, 16 * K)[row // 16, off], q)


def test_quantization_maps_to_the_engine_flags():
    from ht_vllm_omni_amd.worker import config_from_vllm, make_config
    c = make_config("tiny")
    assert (c.quantization, c.dense_fp8, c.moe_fp8) == (None, False, False)
    c = make_config("tiny", quantization="fp8")
    assert (c.quantization, c.dense_fp8, c.moe_fp8) == ("fp8", True, False)
    c = make_config("omni-moe-tiny", quantization="fp8")
    assert (c.dense_fp8, c.moe_fp8) == (False, True)
    v = types.SimpleNamespace(model_config=types.SimpleNamespace(model="tiny", quantization="fp8"))
    assert config_from_vllm(v).dense_fp8 and not config_from_vllm(v).moe_fp8
    v.model_config.quantization = None
    assert not config_from_vllm(v).dense_fp8
    v.model_config.quantization = "awq"
    for refused in (lambda: make_config("tiny", quantization="int8"), lambda: config_from_vllm(v)):
        with pytest.raises(ValueError):
            refused()


@pytest.mark.parametrize("dims,kw", [("moe", {}), ("tiny", {"tp_size": 2}), ("tiny", {"fused_norm": False})], ids=["moe", "tp", "separate-norm"])
def test_dense_fp8_refuses_what_the_w8_path_does_not_serve(dims, kw):
    from ht_vllm_omni_amd.engine import TalkerEngine
    d = get_dims("omni-talker" if dims == "moe" else dims)
    assert (d.moe_experts > 0) == (dims == "moe")
    with pytest.raises(ValueError, match="dense_fp8"):
        TalkerEngine(d, {}, dense_fp8=True, **kw)

