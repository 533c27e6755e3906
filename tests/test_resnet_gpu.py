"""eeg_image_decode_amd/metric_nets.ResNetFeatures and metrics.swav_distance on the MI355X: tests/resnet_cases.py's checks at full depth, at 33 x 47 (N = 4:
odd sizes, tile tails in every stage) and at the notebooks' 224 x 224 (N = 3), in fp16 and bf16, then the SwAV row and the table."""
import pytest
import torch

import resnet_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("H,W,N", [(33, 47, 4), (224, 224, 3)], ids=["33x47", "224x224"])
def test_features_on_device(H, W, N, dtype):
    assert cases.check_features("cuda", H, W, N, dtype, layers=cases.FULL) > 0


def test_smallest_image_on_device():
    cases.check_smallest("cuda", torch.float16, layers=cases.FULL)


def test_cpu_tensor_raises_on_device_net():
    from eeg_image_decode_amd import metric_nets
    from eeg_image_decode_amd._lib import EegclipError
    net = metric_nets.swav_resnet50()
    assert net.layers == (3, 4, 6, 3)
    with pytest.raises(EegclipError):
        net(torch.zeros(1, 3, 32, 32, dtype=torch.float16))


def test_swav_row_and_table_on_device():
    """fp16, 64 x 80, N = 8, mixed pairs, full depth: the row against scipy; then the table with alexnet= and swav= has the five rows, the others unchanged"""
    from eeg_image_decode_amd import metric_nets
    images, recons, net = cases.check_swav_row("cuda", 64, 80, 8)
    out = cases.check_table("cuda", images, recons, net, 64, alexnet=metric_nets.AlexNetFeatures(dtype=torch.float16))
    assert sorted(out) == ["AlexNet(2)", "AlexNet(5)", "PixCorr", "SSIM", "SwAV"]
