"""Host side of voice cloning from reference audio (ht_vllm_omni_amd.speaker): the log-mel front end and the builder's input checks."""
import math

import numpy as np
import pytest
import torch

from ht_vllm_omni_amd import speaker as S


@pytest.mark.parametrize("n", [1024, 6000, 24000, 24001])
def test_log_mel_frame_count_is_the_reference_formula(n):
    """mel_spectrogram pads (n_fft - hop) / 2 = 384 samples per side and frames without centring: 1 + (n + 768 - 1024) // 256."""
    mel = S.log_mel_24k(np.zeros(n, dtype=np.float32))
    assert mel.shape == (1 + (n + 768 - 1024) // 256, 128) == (S.log_mel_frames(n), 128)
    assert torch.allclose(mel, torch.full_like(mel, math.log(1e-5))), "silence sits on the clamp"


def test_sine_peaks_in_the_band_that_brackets_it():
    wav = np.sin(2 * np.pi * 1000.0 * np.arange(24000) / 24000.0).astype(np.float32)
    band = int(S.log_mel_24k(wav).mean(0).argmax())
    centres = S.mel_band_centres()
    assert centres[band - 1] < 1000.0 < centres[band + 1] and abs(centres[band] - 1000.0) == np.abs(centres - 1000.0).min()


@pytest.mark.parametrize("ref_audio", [(np.zeros(16000, dtype=np.float32), 16000), {"array": np.zeros(44100, dtype=np.float32), "sampling_rate": 44100}])
def test_builder_refuses_other_sample_rates(ref_audio):
    """The rate is checked before anything touches the device (resampling is out of scope)."""
    from ht_vllm_omni_amd.prompt_builder_tts import TTSPromptIds, TTSTalkerPromptBuilder
    z = torch.zeros(8, 16)
    w = {"text_embedding": z, "codec_embed": z, "cp_embed": z[None], "text_projection": {}}
    b = TTSTalkerPromptBuilder(w, TTSPromptIds(1, 2, 3), "cpu", speaker_encoder=S.SpeakerEncoder.__new__(S.SpeakerEncoder))
    with pytest.raises(ValueError, match="resampling is upstream"):
        b.from_info({"task_type": "Base", "x_vector_only_mode": True, "input_ids": list(range(12)), "ref_audio": ref_audio})
