"""The product's AlexNet host code (eeg_image_decode_amd/metric_nets.py, metrics.alexnet_two_way through preprocess.py) with its kernels under the lane
emulator (tests/emu_patch.py), against tests/metric_nets_ref.py: the checks are tests/metric_nets_cases.py's, shared with tests/test_metric_nets_gpu.py.
The emulator runs the smallest input that reaches `features.11`, 31 x 37 (the device runs 67 x 83 and 256 x 256)."""
import pytest
import torch

import metric_nets_cases as cases
from eeg_image_decode_amd import metric_nets, metrics, preprocess   # noqa: F401  (before product_on_emulator(): it patches the loaded modules)
from emu_patch import product_on_emulator

pytestmark = pytest.mark.emu


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_features_on_emulator(dtype):
    with product_on_emulator():
        cases.check_features("cpu", 31, 37, 2, dtype)


def test_two_way_rows_on_emulator():
    with product_on_emulator():
        cases.check_two_way_rows("cpu", 31, 37, 4)


def test_alexnet_preprocess_is_pil_resize_and_imagenet_normalize():
    """preprocess.alexnet_preprocess against PIL itself: Image.resize(BILINEAR) with the shortest side at `size` and no crop (landscape and portrait inputs),
    then (q / 255 - mean) / std with ImageNet's constants written out here.  The pixels are PIL's integers; the floats are within the three fp32 roundings of
    q * scale + shift (2^-21 of the two terms, the bound of tests/preprocess_cases.py)."""
    import numpy as np
    from PIL import Image
    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
    rng = np.random.default_rng(11)
    with product_on_emulator():
        for (H, W), (h, w) in (((40, 52), (32, 41)), ((52, 40), (41, 32)), ((32, 47), (32, 47))):
            a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            q = np.asarray(Image.fromarray(a).resize((w, h), Image.BILINEAR), np.float64).transpose(2, 0, 1)
            want = (q / 255 - mean[:, None, None]) / std[:, None, None]
            got = preprocess.alexnet_preprocess([a, Image.fromarray(a)], size=32, device="cpu")
            assert tuple(got.shape) == (2, 3, h, w) and got.dtype == torch.float32 and torch.equal(got[0], got[1])
            bound = 2.0 ** -21 * (np.abs(q / 255 / std[:, None, None]) + np.abs(mean / std)[:, None, None])
            assert (np.abs(got[0].double().numpy() - want) <= bound).all()
            half = preprocess.alexnet_preprocess(a, size=32, device="cpu", dtype=torch.float16)
            assert torch.equal(half, got[:1].half())
        assert tuple(preprocess.alexnet_preprocess(rng.integers(0, 256, (20, 30, 3), dtype=np.uint8), device="cpu").shape) == (1, 3, 256, 384)


def test_exported_from_the_package_and_no_cpu_path():
    """the public names resolve from the package; without the emulator patch a CPU tensor raises (there is no CPU path)"""
    import eeg_image_decode_amd as pkg
    from eeg_image_decode_amd._lib import EegclipError
    for name, mod in (("AlexNetFeatures", metric_nets), ("alexnet_two_way", metrics), ("alexnet_preprocess", preprocess)):
        assert getattr(pkg, name) is getattr(mod, name) and name in pkg.__all__
    net = metric_nets.AlexNetFeatures(device="cpu")
    x = torch.zeros(1, 3, 31, 31, dtype=torch.float16)
    with pytest.raises(EegclipError):
        net(x)
    with pytest.raises(EegclipError):
        net(x, nodes=("features.4",))
