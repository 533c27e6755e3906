"""eeg_image_decode_amd/metric_nets.py and metrics.alexnet_two_way on the MI355X: tests/metric_nets_cases.py's checks at 67 x 83 (N = 8: odd sizes, several
M tiles, a tile tail in every layer) and at the notebooks' 256 x 256 (N = 2), in fp16 and bf16, and the two AlexNet rows of the table."""
import pytest
import torch

import metric_nets_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("H,W,N", [(67, 83, 8), (256, 256, 2)], ids=["67x83", "256x256"])
def test_features_on_device(H, W, N, dtype):
    """yardstick measured on the CPU (torch-default init, smooth images): 4.3e-4 / 5.1e-4 in fp16 and 3.5e-3 / 4.2e-3 in bf16 at both sizes"""
    ratios = cases.check_features("cuda", H, W, N, dtype)
    assert sorted(ratios) == ["features.11", "features.4"]
    if (H, W) == (256, 256):
        from eeg_image_decode_amd import metric_nets
        out = metric_nets.AlexNetFeatures(dtype=dtype)(torch.zeros(N, 3, H, W, dtype=dtype, device="cuda"))
        assert tuple(out["features.4"].shape) == (N, 192, 31, 31) and tuple(out["features.11"].shape) == (N, 256, 15, 15)


def test_cpu_tensor_raises_on_device_net():
    from eeg_image_decode_amd import metric_nets
    from eeg_image_decode_amd._lib import EegclipError
    net = metric_nets.AlexNetFeatures()
    with pytest.raises(EegclipError):
        net(torch.zeros(1, 3, 31, 31, dtype=torch.float16))


def test_two_way_rows_and_table_on_device():
    """fp16, 67 x 83, N = 8, mixed pairs: the counts of both rows are the reference's; then the table with alexnet= has the four keys and the same PixCorr / SSIM"""
    images, recons, net = cases.check_two_way_rows("cuda", 67, 83, 8)
    cases.check_table("cuda", images, recons, net, 67)
