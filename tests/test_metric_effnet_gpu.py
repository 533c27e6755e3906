"""eeg_image_decode_amd/metric_nets.EfficientNetFeatures and metrics.effnet_distance on the MI355X: tests/effnet_cases.py's checks at full depth, at 33 x 47
(odd sizes, tile tails in every stage) and 64 x 64 with N = 3 in fp16 and bf16, and at the notebooks' 255 x 255 (N = 2, fp16), then the EffNet-B row and the
table.  (The module's name sorts it behind the tests/test_kernels_*.py files: those run on the allocator state they have always run on.)"""
import pytest
import torch

import effnet_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("H,W", [(33, 47), (64, 64)], ids=["33x47", "64x64"])
def test_features_on_device(H, W, dtype):
    assert cases.check_features("cuda", H, W, 3, dtype, layers=cases.FULL) > 0


def test_features_at_the_notebooks_size_on_device():
    assert cases.check_features("cuda", 255, 255, 2, torch.float16, layers=cases.FULL, extras=False) > 0


def test_smallest_image_on_device():
    cases.check_smallest("cuda", torch.float16, layers=cases.FULL)


def test_cpu_tensor_raises_on_device_net():
    from eeg_image_decode_amd import metric_nets
    from eeg_image_decode_amd._lib import EegclipError
    net = metric_nets.efficientnet_b1()
    assert net.layers == (2, 3, 3, 4, 4, 5, 2)
    with pytest.raises(EegclipError):
        net(torch.zeros(1, 3, 32, 32, dtype=torch.float16))


def test_effnet_row_and_table_on_device():
    """fp16, 33 x 47, N = 6, mixed pairs, full depth: the row against scipy; then the table with swav= and effnet= has the four rows, the others unchanged"""
    from eeg_image_decode_amd import metric_nets
    images, recons, net = cases.check_effnet_row("cuda", 33, 47, 6)
    out = cases.check_table("cuda", images, recons, net, 33, swav=metric_nets.ResNetFeatures(layers=(1, 1, 1, 1), dtype=torch.float16))
    assert sorted(out) == ["EffNet-B", "PixCorr", "SSIM", "SwAV"]
