"""TalkerEngine(moe_fp8=True, prefill_gemm="fp8") on an MoE model: what the option accepts and refuses, in front of the GPU check."""
import pytest
import torch

from ht_vllm_omni_amd import _lib
from ht_vllm_omni_amd.config import get_dims
from ht_vllm_omni_amd.engine import TalkerEngine


@pytest.mark.parametrize("preset,kw,err", [
    pytest.param("omni-talker", {}, _lib.OmniError, marks=pytest.mark.skipif(torch.cuda.is_available(), reason="GPU present")),      # accepted: the next stop is the GPU check
    ("omni-talker", dict(moe_dispatch="padded"), ValueError), ("omni-talker", dict(tp_size=2), ValueError),
    ("omni-moe-tiny", {}, ValueError)])      # the tiny model's expert width 64 is no multiple of 128
def test_moe_prefill_fp8_option_check(preset, kw, err):
    with pytest.raises(err, match="prefill_gemm" if err is ValueError else None):
        TalkerEngine(get_dims(preset), {}, moe_fp8=True, prefill_gemm="fp8", **kw)
