"""The product's metrics host code (eeg_image_decode_amd/metrics.py, through preprocess.py and a small CLIP tower) with its kernels under the lane emulator
(tests/emu_patch.py), against tests/recon_metrics_ref.py: the checks are tests/recon_metrics_cases.py's, shared with tests/test_recon_metrics_gpu.py.  The
emulator runs them at size 32 (the device at the default 425)."""
import pytest
import torch

import recon_metrics_cases as cases
from eeg_image_decode_amd import clip_vision, metrics, preprocess   # noqa: F401  (before product_on_emulator(): it patches the loaded modules)
from emu_patch import product_on_emulator

pytestmark = pytest.mark.emu


def test_image_metrics_on_emulator():
    with product_on_emulator():
        cases.check_image_metrics("cpu", 32)


def test_two_way_on_emulator():
    with product_on_emulator():
        cases.check_two_way("cpu")


def test_reconstruction_metrics_on_emulator():
    with product_on_emulator():
        cases.check_reconstruction_metrics("cpu", 32)


def test_exported_from_the_package_and_no_cpu_path():
    """the public names resolve from the package; without the emulator patch a CPU tensor raises (there is no CPU path)"""
    import eeg_image_decode_amd as pkg
    from eeg_image_decode_amd._lib import EegclipError
    for name in ("pixcorr_ssim", "pixcorr", "ssim", "two_way_identification", "clip_two_way", "reconstruction_metrics"):
        assert getattr(pkg, name) is getattr(metrics, name) and name in pkg.__all__
    x = torch.rand(2, 3, 16, 20)
    with pytest.raises(EegclipError):
        metrics.pixcorr_ssim(x, x, size=None)
    with pytest.raises(EegclipError):
        metrics.two_way_identification(torch.rand(4, 8), torch.rand(4, 8))
