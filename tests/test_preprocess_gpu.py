"""eeg_image_decode_amd/preprocess.py on the MI355X: tests/preprocess_cases.py's preset and feature-cache checks on the device, the workload's own batch
exact against PIL, a device-resident source, and run-to-run bit identity."""
import numpy as np
import pytest
import torch

import preprocess_cases as cases
import preprocess_ref as R

pytestmark = pytest.mark.gpu


def test_presets_on_device():
    cases.check_presets("cuda")


def test_feature_cache_on_device(tmp_path):
    cases.check_feature_cache(str(tmp_path), "cuda")


@pytest.fixture(scope="module")
def batch8():
    src = np.random.default_rng(11).integers(0, 256, (8, 500, 500, 3), dtype=np.uint8)
    return src, np.stack([R.pil_resize(s, 224, 224, "bicubic").transpose(2, 0, 1) for s in src])


def test_workload_batch_is_pil(batch8):
    """B = 8 at 500 x 500 -> 224 through open_clip_preprocess: the integer pixels (mean / std / rescale off) equal PIL's in every element, and the preset's
    floats are within the normalisation bound of them"""
    from eeg_image_decode_amd import preprocess as P
    src, want = batch8
    raw = P.resize_crop_normalize(src, 224, (224, 224), rescale=None)
    assert raw.is_cuda and raw.shape == (8, 3, 224, 224) and np.array_equal(raw.cpu().numpy().astype(np.int64), want)
    out = P.open_clip_preprocess(src).cpu()
    scale, shift = R.affine(R.CLIP_MEAN, R.CLIP_STD, 1 / 255)
    R.assert_normalized(out, want.transpose(0, 2, 3, 1).astype(np.uint8), scale, shift)


def test_device_source_and_two_runs(batch8):
    """a uint8 tensor already on the device takes the host array's path, bit for bit; two runs are bit-identical"""
    from eeg_image_decode_amd import preprocess as P
    src, _ = batch8
    a = P.open_clip_preprocess(src)
    b = P.open_clip_preprocess(torch.from_numpy(src).cuda())
    c = P.open_clip_preprocess([torch.from_numpy(s).cuda() for s in src])
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, P.open_clip_preprocess(src))
