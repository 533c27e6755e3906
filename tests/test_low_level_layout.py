"""The state_dict of eeg_image_decode_amd.low_level.LowLevelEncoder against the fp32 restatement (tests/low_level_ref.py) of the reference's
encoder_low_level: same keys in the same order, same shapes, and the restatement's state dict loads strictly.  The published widths are built on the `meta`
device (the first transposed convolution alone is 8064 x 1024 x 16 weights); the load runs at a small `hidden`."""
import pytest
import torch

from eeg_image_decode_amd.low_level import LowLevelEncoder
from eeg_image_decode_amd._lib import EegclipError
from low_level_ref import EncoderLowLevelRef


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_published_widths_keys_and_shapes():
    with torch.device("meta"):
        ref = EncoderLowLevelRef()
    ours = LowLevelEncoder(device="meta")
    a, b = _shapes(ours), _shapes(ref)
    assert list(a) == list(b) and a == b
    assert a["upsampler.0.weight"] == (8064, 1024, 4, 4) and a["upsampler.15.weight"] == (64, 4, 4, 4)
    assert a["subject_wise_linear.0.weight"] == (128, 250) and a["upsampler.13.running_var"] == (64,)
    convs = [k for k in a if k.startswith("upsampler.") and k.endswith(".weight") and len(a[k]) == 4]
    assert convs == [f"upsampler.{i}.weight" for i in (0, 3, 6, 9, 12, 15)]
    assert ours.latent_size == 64 and not ours.training and ours.dtype == torch.float16


def test_restatement_state_dict_loads_strictly():
    ch = (63 * 64, 64, 64, 4)
    ref = EncoderLowLevelRef(num_subjects=2, hidden=64, channels=ch)
    ours = LowLevelEncoder(num_subjects=2, hidden=64, channels=ch, dtype=torch.bfloat16, seed=3)
    res = ours.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in ref.state_dict().items():
        got = ours.state_dict()[k]
        assert torch.equal(got.float(), v.to(got.dtype).float()), k
    assert ours.latent_size == 8
    with pytest.raises(RuntimeError):
        ours.load_state_dict({k: v for k, v in ref.state_dict().items() if k != "upsampler.1.running_var"})


def test_config_errors_and_no_eager_path():
    with pytest.raises(EegclipError):
        LowLevelEncoder(hidden=64, device="meta")                               # channels[0] != 63 * hidden
    with pytest.raises(EegclipError):
        LowLevelEncoder(hidden=64, channels=(4032, 100, 4), device="meta")      # an inner width that is no multiple of 64
    with pytest.raises(EegclipError):
        LowLevelEncoder(hidden=64, channels=(4032, 64, 16), device="meta")      # the last layer is the direct NCHW form: below 16 channels
    m = LowLevelEncoder(hidden=64, channels=(4032, 64, 4))
    if not torch.cuda.is_available():
        with pytest.raises(EegclipError):
            m(torch.zeros(1, 63, 250))                                           # CPU tensors: there is no eager path


def test_lazy_export():
    import eeg_image_decode_amd
    assert eeg_image_decode_amd.LowLevelEncoder is LowLevelEncoder
