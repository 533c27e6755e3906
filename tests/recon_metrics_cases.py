"""What tests/test_recon_metrics_emu.py (product host code on the lane emulator, device "cpu") and tests/test_recon_metrics_gpu.py (the MI355X, device
"cuda") share: eeg_image_decode_amd/metrics.py against tests/recon_metrics_ref.py applied to preprocess.resize_crop_normalize's OWN output (the resize is
tested against PIL elsewhere).  Bounds: tests/test_kernels_recon_metrics.py's."""
import numpy as np
import torch

import recon_metrics_ref as R

SSIM_TOL, PIX_TOL = 1e-4, 1e-6


def image_pairs(n=3, H=40, W=52):
    """n uint8 image pairs (H, W, 3): a smooth image and a noisy version of it"""
    a, b = [], []
    for i in range(n):
        x, y = R.smooth_pair(20 + i, H, W, noise=0.08 + 0.05 * i)
        a.append((x.transpose(1, 2, 0) * 255).round().astype(np.uint8))
        b.append((y.transpose(1, 2, 0) * 255).round().astype(np.uint8))
    return a, b


def block_pairs(n=4, H=40, W=52):
    """n uint8 pairs of 5 x 4 random colour blocks and a noisy version: images a random tower tells apart (smooth ones all look alike to it)"""
    rng = np.random.default_rng(30)
    a = [np.kron(rng.integers(0, 256, (5, 4, 3), dtype=np.uint8), np.ones((H // 5, W // 4, 1), np.uint8)) for _ in range(n)]
    b = [np.clip(x.astype(np.int64) + rng.integers(-40, 41, x.shape), 0, 255).astype(np.uint8) for x in a]
    return a, b


def oracle(A, B):
    A, B = A.float().cpu().numpy(), B.float().cpu().numpy()
    return np.array([R.pixcorr(x, y) for x, y in zip(A, B)]), np.array([R.ssim(x, y) for x, y in zip(A, B)])


def close(pix, ssm, want, label):
    ep, es = np.abs(pix.cpu().numpy() - want[0]).max(), np.abs(ssm.cpu().numpy() - want[1]).max()
    print(f"\n[metrics] {label}: ssim {want[1].min():.4f}..{want[1].max():.4f} max err {es:.2e}; pixcorr max err {ep:.2e}", end=" ")
    assert pix.dtype == ssm.dtype == torch.float32 and es <= SSIM_TOL and ep <= PIX_TOL, (label, es, ep)


def check_image_metrics(device, size):
    """uint8 arrays, PIL images and float tensors through the resize to `size` (shortest side), size=None on the resized tensors, the thin wrappers, errors"""
    from PIL import Image
    from eeg_image_decode_amd import metrics as M, preprocess as P
    from eeg_image_decode_amd._lib import EegclipError
    a8, b8 = image_pairs()
    A = P.resize_crop_normalize(a8, size, filter="bilinear", rescale=1 / 255, device=device)
    B = P.resize_crop_normalize(b8, size, filter="bilinear", rescale=1 / 255, device=device)
    assert A.shape[2] == size and A.shape[3] == int(size * 52 / 40) and 0.0 <= float(A.min()) and float(A.max()) <= 1.0
    want = oracle(A, B)
    pix, ssm = M.pixcorr_ssim(a8, b8, size=size, device=device)
    assert pix.shape == ssm.shape == (3,) and pix.device.type == torch.device(device).type
    close(pix, ssm, want, f"uint8 lists -> {size}")
    for other in (M.pixcorr_ssim([Image.fromarray(x) for x in a8], [Image.fromarray(x) for x in b8], size=size, device=device),
                  M.pixcorr_ssim(np.stack(a8), torch.from_numpy(np.stack(b8)), size=size, device=device),
                  M.pixcorr_ssim(A, B, size=None), M.pixcorr_ssim(A, B, size=size), M.pixcorr_ssim(a8, B, size=size, device=device)):
        assert torch.equal(other[0], pix) and torch.equal(other[1], ssm)
    assert torch.equal(M.pixcorr(A, B, size=None), pix) and torch.equal(M.ssim(A, B, size=None), ssm)
    # float tensors of another size: quantised and resized as the uint8 images they stand for
    fa = torch.from_numpy(np.stack(a8)).permute(0, 3, 1, 2).float().div(255).to(device)
    fb = torch.from_numpy(np.stack(b8)).permute(0, 3, 1, 2).float().div(255).to(device)
    got = M.pixcorr_ssim(fa, fb, size=size, device=device)
    assert torch.equal(got[0], pix) and torch.equal(got[1], ssm)
    # fp16 tensors as they are: the oracle sees the quantised values
    hp, hs = M.pixcorr_ssim(A.half(), B.half(), size=None)
    close(hp, hs, oracle(A.half(), B.half()), "fp16 tensors, size=None")
    for bad in (lambda: M.pixcorr_ssim(a8, b8, size=None), lambda: M.pixcorr_ssim(A, B[:2], size=None), lambda: M.pixcorr_ssim(A[..., :10], B[..., :10], size=None),
                lambda: M.pixcorr_ssim(A, B[..., :-1], size=None)):
        try:
            bad()
        except EegclipError:
            continue
        raise AssertionError("no EegclipError")
    return A, B, pix, ssm


def check_two_way(device):
    """features with trailing dimensions (17, 5, 26 -> D = 130), flattened: score and counts are the oracle's"""
    from eeg_image_decode_amd import metrics as M
    from eeg_image_decode_amd._lib import EegclipError
    G, Pf = R.feature_pair(1, 17, 130)
    r, count, score = R.two_way(G, Pf)
    assert R.two_way_gap(r) > 1e-3
    g, p = torch.from_numpy(G).reshape(17, 5, 26).to(device), torch.from_numpy(Pf).reshape(17, 5, 26).to(device)
    got, c = M.two_way_identification(g, p, return_counts=True)
    assert c.dtype == torch.int32 and np.array_equal(c.cpu().numpy(), count) and abs(got - score) < 1e-12 and M.two_way_identification(g, p) == got
    assert abs(M.two_way_identification(g.half(), p.half()) - R.two_way(g.half().float().cpu().numpy(), p.half().float().cpu().numpy())[2]) < 1e-12
    for bad in (lambda: M.two_way_identification(g, p[:5]), lambda: M.two_way_identification(g[:1], p[:1]), lambda: M.two_way_identification(G, Pf)):
        try:
            bad()
        except EegclipError:
            continue
        raise AssertionError("no EegclipError")


def check_reconstruction_metrics(device, size):
    """the table with a small random CLIP tower as the feature net: PixCorr / SSIM are the means of pixcorr_ssim, the tower's entry is the oracle's two-way score
    on the tower's own features (asserted away from a tie first), and clip_two_way gives it too"""
    from eeg_image_decode_amd import clip_vision, metrics as M, preprocess as P
    a8, b8 = block_pairs()
    tower = clip_vision.CLIPVisionEncoder(128, 256, 1, 2, "gelu", 128, image_size=28, seed=7, device=device)
    net = lambda x: tower(P.clip_image_processor(x, size=28, dtype=tower.dtype, device=device)).image_embeds
    out = M.reconstruction_metrics(a8, b8, {"CLIP": net}, size=size, device=device)
    assert sorted(out) == ["CLIP", "PixCorr", "SSIM"] and all(isinstance(v, float) for v in out.values())
    pix, ssm = M.pixcorr_ssim(a8, b8, size=size, device=device)
    assert out["PixCorr"] == float(pix.mean()) and out["SSIM"] == float(ssm.mean())
    fa, fb = net(a8), net(b8)
    assert fa.shape == (4, 128)
    r, count, score = R.two_way(fa.float().cpu().numpy(), fb.float().cpu().numpy())
    gap = R.two_way_gap(r)
    print(f"\n[metrics] CLIP two-way on 4 pairs: score {score:.4f}, gap {gap:.1e}", end=" ")
    assert gap > 1e-4                                             # (the kernel's r is within 2e-5: tests/test_kernels_recon_metrics.py)
    assert abs(out["CLIP"] - score) < 1e-12 and abs(M.clip_two_way(a8, b8, tower, size=28) - score) < 1e-12
    assert sorted(M.reconstruction_metrics(a8, b8, size=size, device=device)) == ["PixCorr", "SSIM"]
