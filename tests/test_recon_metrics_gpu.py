"""eeg_image_decode_amd/metrics.py on the MI355X: tests/recon_metrics_cases.py's checks at the reference's size 425, and run-to-run bit identity."""
import pytest
import torch

import recon_metrics_cases as cases
import recon_metrics_ref as R

pytestmark = pytest.mark.gpu


def test_image_metrics_on_device():
    """3 pairs through Resize(425): uint8 / PIL / float inputs, size=None against size=425; then two more runs of the same call give the same bits"""
    from eeg_image_decode_amd import metrics as M
    A, B, pix, ssm = cases.check_image_metrics("cuda", 425)
    assert A.shape == (3, 3, 425, 552)
    for _ in range(2):
        again = M.pixcorr_ssim(A, B, size=None)
        assert torch.equal(again[0], pix) and torch.equal(again[1], ssm)


def test_two_way_on_device():
    cases.check_two_way("cuda")


def test_two_way_runs_are_bit_identical():
    from eeg_image_decode_amd import metrics as M
    G, P = R.feature_pair(1, 33, 1000)
    g, p = torch.from_numpy(G).cuda(), torch.from_numpy(P).cuda()
    s0, c0 = M.two_way_identification(g, p, return_counts=True)
    s1, c1 = M.two_way_identification(g, p, return_counts=True)
    assert s0 == s1 == R.two_way(G, P)[2] and torch.equal(c0, c1)


def test_reconstruction_metrics_on_device():
    cases.check_reconstruction_metrics("cuda", 425)
