"""TalkerEngine(prefill_gemm="fp8"): what the option refuses and accepts, checked in front of the GPU check (no GPU needed)."""
import pytest
import torch

from ht_vllm_omni_amd import _lib
from ht_vllm_omni_amd.config import get_dims
from ht_vllm_omni_amd.engine import TalkerEngine


@pytest.mark.parametrize("preset,kw", [("tiny", {}), ("tiny", dict(dense_fp8=True, frag_layout=False)), ("omni-moe-tiny", {}),
                                       ("omni-moe-tiny", dict(dense_fp8=True))])
def test_prefill_fp8_needs_a_dense_fp8_engine(preset, kw):
    with pytest.raises(ValueError, match="prefill_gemm"):
        TalkerEngine(get_dims(preset), {}, prefill_gemm="fp8", **kw)


def test_prefill_fp8_passes_the_option_check():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.OmniError):      # accepted: the next stop is the GPU check
        TalkerEngine(get_dims("tiny"), {}, prefill_gemm="fp8", dense_fp8=True)
