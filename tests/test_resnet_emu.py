"""The product's ResNet host code (eeg_image_decode_amd/metric_nets.ResNetFeatures, metrics.swav_distance through preprocess.py) with its kernels under the
lane emulator (tests/emu_patch.py), against tests/resnet_ref.py: the checks are tests/resnet_cases.py's, shared with tests/test_resnet_gpu.py.  The emulator
runs a shallow net, layers = (1, 1, 1, 1), at 32 x 40 through the same code in both dtypes, and ONE full-depth forward at 33 x 47 (the device runs full depth
at 33 x 47 and 224 x 224)."""
import pytest
import torch

import resnet_cases as cases
from eeg_image_decode_amd import metric_nets, metrics, preprocess   # noqa: F401  (before product_on_emulator(): it patches the loaded modules)
from emu_patch import product_on_emulator

pytestmark = pytest.mark.emu


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_shallow_features_on_emulator(dtype):
    with product_on_emulator():
        cases.check_features("cpu", 32, 40, 2, dtype, layers=cases.SHALLOW)


def test_full_depth_forward_on_emulator():
    """(3, 4, 6, 3) at 33 x 47, N = 2, fp16: 17 x 24 behind the stem, 9 x 12 behind the pool, 5 x 6, 3 x 3 and 2 x 2 in layer2 .. layer4"""
    with product_on_emulator():
        cases.check_features("cpu", 33, 47, 2, torch.float16, layers=cases.FULL, extras=False)


def test_smallest_image_on_emulator():
    with product_on_emulator():
        cases.check_smallest("cpu", torch.float16)


def test_swav_row_on_emulator():
    with product_on_emulator():
        cases.check_swav_row("cpu", 32, 40, 3, layers=cases.SHALLOW)


def test_exported_from_the_package_and_no_cpu_path():
    """the public names resolve from the package; without the emulator patch a CPU tensor raises (there is no CPU path)"""
    import eeg_image_decode_amd as pkg
    from eeg_image_decode_amd._lib import EegclipError
    for name, mod in (("ResNetFeatures", metric_nets), ("swav_resnet50", metric_nets), ("swav_distance", metrics), ("correlation_distance", metrics),
                      ("swav_preprocess", preprocess)):
        assert getattr(pkg, name) is getattr(mod, name) and name in pkg.__all__
    net = metric_nets.ResNetFeatures(layers=(1, 1, 1, 1), device="cpu")
    with pytest.raises(EegclipError):
        net(torch.zeros(1, 3, 32, 32, dtype=torch.float16))
    with pytest.raises(EegclipError):
        metrics.correlation_distance(torch.zeros(2, 8), torch.ones(2, 8))
