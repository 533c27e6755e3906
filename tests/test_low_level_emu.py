"""The product's LowLevelEncoder host code with its kernels under the lane emulator (tests/emu_patch.py), against the fp32 restatement
(tests/low_level_ref.py): the CPU-side cover of low_level.py's forward (the K = 250 -> 256 staging, the 1 x 1 frame, the dead-tap descriptor of the first
layer, the folded BatchNorm, the NCHW last layer) beside tests/test_kernels_convt16.py.  hidden = 64, channels (4032, 64, 4): a 4 x 4 latent, B = 2."""
import pytest
import torch

from eeg_image_decode_amd import low_level          # noqa: F401  (before product_on_emulator(): it patches the modules already loaded)
from eeg_image_decode_amd._lib import EegclipError
from emu_patch import product_on_emulator
from low_level_ref import calibrated

pytestmark = pytest.mark.emu
CH = (4032, 64, 4)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_forward_on_emulator(dtype):
    """within 3 x the format's own error (the restatement with its activations rounded to the dtype at every layer boundary) of the fp32 restatement"""
    ref = calibrated(64, CH, dtype)
    model = low_level.LowLevelEncoder(hidden=64, channels=CH, dtype=dtype, seed=1)
    model.load_state_dict(ref.state_dict())
    x = torch.randn(2, 63, 250, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want, fmt = ref(x), ref(x, round_to=dtype)
    with product_on_emulator():
        got = model(x)
        again = model(x, subject_id=0)
        model.train()
        with pytest.raises(EegclipError):
            model(x)
        model.eval()
        with pytest.raises(EegclipError):
            model(x, subject_id=1)
    e_fmt, err = rel_l2(fmt, want), rel_l2(got.float(), want)
    print(f"emulator forward {dtype}: relative L2 {err:.3e}, format error {e_fmt:.3e}, allowance {3 * e_fmt:.3e}")
    assert got.dtype == dtype and tuple(got.shape) == (2, 4, 4, 4) and torch.equal(got, again)
    assert err < 3 * e_fmt
