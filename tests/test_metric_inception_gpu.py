"""eeg_image_decode_amd/metric_nets.InceptionFeatures and metrics.inception_two_way on the MI355X: tests/inception_cases.py's checks at full depth, at the
smallest size 75 x 75 and at 83 x 107 (odd sizes, tile tails in every stage) with N = 3 in fp16 and bf16, and at the notebooks' 342 x 342 (N = 2, fp16), then the
Inception row and the table.  (The module's name sorts it behind the tests/test_kernels_*.py files, as tests/test_metric_effnet_gpu.py's does.)"""
import pytest
import torch

import inception_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("H,W", [(75, 75), (83, 107)], ids=["75x75", "83x107"])
def test_features_on_device(H, W, dtype):
    assert cases.check_features("cuda", H, W, 3, dtype, blocks=cases.FULL) > 0


def test_features_at_the_notebooks_size_on_device():
    assert cases.check_features("cuda", 342, 342, 2, torch.float16, blocks=cases.FULL, extras=False) > 0


def test_too_small_an_image_and_a_cpu_tensor_raise():
    from eeg_image_decode_amd import metric_nets
    from eeg_image_decode_amd._lib import EegclipError
    net = metric_nets.inception_v3()
    assert net.blocks == (3, 4, 2)
    with pytest.raises(EegclipError):
        net(torch.zeros(1, 3, 74, 80, dtype=torch.float16, device="cuda"))
    with pytest.raises(EegclipError):
        net(torch.zeros(1, 3, 75, 75, dtype=torch.float16))


def test_inception_row_and_table_on_device():
    """fp16, 83 x 107, N = 6, mixed pairs, full depth: the row's counts against the reference's; then the table with effnet= and inception= has the four rows,
    the others unchanged"""
    from eeg_image_decode_amd import metric_nets
    images, recons, net = cases.check_inception_row("cuda", 83, 107, 6)
    out = cases.check_table("cuda", images, recons, net, 83, effnet=metric_nets.EfficientNetFeatures(layers=(1,) * 7, dtype=torch.float16))
    assert sorted(out) == ["EffNet-B", "Inception", "PixCorr", "SSIM"]
