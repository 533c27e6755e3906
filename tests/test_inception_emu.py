"""The product's InceptionV3 host code (eeg_image_decode_amd/metric_nets.InceptionFeatures, metrics.inception_two_way through preprocess.py) with its kernels
under the lane emulator (tests/emu_patch.py), against tests/inception_ref.py: the checks are tests/inception_cases.py's, shared with
tests/test_metric_inception_gpu.py.  The emulator runs one fiber per work-item, so it takes shallow nets -- blocks = (1, 1, 1): one block of each of the five
kinds, Mixed_6a with 256 and Mixed_6b with 736 input channels -- at the smallest size 75 x 75 (7 x 7, 3 x 3, 1 x 1 in the three groups) and at 83 x 107 (sizes
83 -> 41 -> 39 -> 39 -> 19 -> 19 -> 17 -> 8 -> 3 -> 1 and 107 -> 53 -> 51 -> 51 -> 25 -> 25 -> 23 -> 11 -> 5 -> 2: tile tails in every stage), and (2, 1, 1)
once: Mixed_5c's 288 channels in a 320-channel frame.  The device runs full depth."""
import pytest
import torch

import inception_cases as cases
from eeg_image_decode_amd import metric_nets, metrics, preprocess   # noqa: F401  (before product_on_emulator(): it patches the loaded modules)
from emu_patch import product_on_emulator

pytestmark = pytest.mark.emu


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("H,W", [(75, 75), (83, 107)])
def test_shallow_features_on_emulator(H, W, dtype):
    with product_on_emulator():
        cases.check_features("cpu", H, W, 2, dtype, blocks=cases.SHALLOW)


def test_padded_concatenation_on_emulator():
    """(2, 1, 1) at 75 x 75: Mixed_5c and Mixed_6a read 288 channels of a 320-channel frame whose last 32 nobody writes"""
    with product_on_emulator():
        cases.check_features("cpu", 75, 75, 2, torch.float16, blocks=(2, 1, 1), extras=False)


def test_inception_row_on_emulator():
    with product_on_emulator():
        cases.check_inception_row("cpu", 83, 107, 3, blocks=cases.SHALLOW)


def test_exported_from_the_package_and_no_cpu_path():
    """the public names resolve from the package; without the emulator patch a CPU tensor raises (there is no CPU path)"""
    import eeg_image_decode_amd as pkg
    from eeg_image_decode_amd._lib import EegclipError
    for name, mod in (("InceptionFeatures", metric_nets), ("inception_v3", metric_nets), ("inception_two_way", metrics), ("inception_preprocess", preprocess)):
        assert getattr(pkg, name) is getattr(mod, name) and name in pkg.__all__
    net = metric_nets.InceptionFeatures(blocks=(1, 1, 1), device="cpu")
    with pytest.raises(EegclipError):
        net(torch.zeros(1, 3, 75, 75, dtype=torch.float16))
