"""fp64 restatement (numpy + scipy) of the reconstruction metrics of MindEye's Reconstruction_Metrics, which the reference's notebooks copy: the oracle of
tests/test_kernels_recon_metrics.py, tests/test_recon_metrics_emu.py and tests/test_recon_metrics_gpu.py.

  pixcorr   np.corrcoef of the two flattened (3, H, W) images
  ssim      skimage's structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=1.0) on rgb2gray images, written out:
            the mean of S over the pixels at least 5 from every border.  Their 11 x 11 windows never leave the image, so no boundary rule takes part; ssim()
            ASSERTS that: scipy's gaussian_filter(truncate=3.5) with mode="reflect" (what skimage calls) and with mode="constant", and an explicit 11-tap
            correlate1d, give the same cropped mean.
  two_way   r = np.corrcoef(G, P)[:N, N:]; count[j] = #{ i != j : r[i, j] < r[j, j] }; score = mean(count) / (N - 1)
"""
import numpy as np
from scipy.ndimage import correlate1d, gaussian_filter

C1, C2, PAD = 0.01 ** 2, 0.03 ** 2, 5


def taps():
    i = np.arange(-PAD, PAD + 1, dtype=np.float64)
    w = np.exp(-i * i / (2 * 1.5 ** 2))
    return w / w.sum()


def gray(img):
    img = np.asarray(img, np.float64)
    return 0.2125 * img[0] + 0.7154 * img[1] + 0.0721 * img[2]


def pixcorr(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.corrcoef(np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel())[0, 1])


def _ssim_with(x, y, smooth):
    ux, uy = smooth(x), smooth(y)
    vx, vy, vxy = smooth(x * x) - ux * ux, smooth(y * y) - uy * uy, smooth(x * y) - ux * uy
    S = (2 * ux * uy + C1) * (2 * vxy + C2) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return float(S[PAD:-PAD, PAD:-PAD].mean())


def ssim(a, b):
    """a, b: (3, H, W) in [0, 1], H, W >= 11"""
    x, y = gray(a), gray(b)
    assert x.shape == y.shape and min(x.shape) >= 2 * PAD + 1
    w = taps()
    reflect = _ssim_with(x, y, lambda z: gaussian_filter(z, 1.5, truncate=3.5, mode="reflect"))
    const = _ssim_with(x, y, lambda z: gaussian_filter(z, 1.5, truncate=3.5, mode="constant"))
    explicit = _ssim_with(x, y, lambda z: correlate1d(correlate1d(z, w, axis=0, mode="constant"), w, axis=1, mode="constant"))
    assert abs(reflect - const) < 1e-12 and abs(reflect - explicit) < 1e-12, (reflect, const, explicit)
    return reflect


def two_way(G, P):
    """-> (r (N, N), count (N,) int, score)"""
    G, P = np.asarray(G, np.float64), np.asarray(P, np.float64)
    G, P = G.reshape(len(G), -1), P.reshape(len(P), -1)
    N = len(G)
    r = np.corrcoef(G, P)[:N, N:]
    off = ~np.eye(N, dtype=bool)
    count = ((r < np.diag(r)[None, :]) & off).sum(0)
    return r, count.astype(np.int64), float(count.mean() / (N - 1))


def two_way_gap(r):
    """the smallest |r[i, j] - r[j, j]| over i != j: how far every comparison is from a tie"""
    N = len(r)
    d = np.abs(r - np.diag(r)[None, :])
    return float(d[~np.eye(N, dtype=bool)].min())


# ---- the inputs the kernel tests and the Python-API tests share ----
def smooth_pair(seed, H, W, noise=0.1):
    """a smooth image and a noisy version of it, (3, H, W) fp32 in [0, 1]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    ph = rng.uniform(0, 2 * np.pi, (3, 2))
    a = np.stack([0.5 + 0.35 * np.sin(5 * xx + ph[c, 0]) * np.cos(4 * yy + ph[c, 1]) for c in range(3)])
    b = np.clip(a + noise * rng.standard_normal(a.shape), 0, 1)
    return a.astype(np.float32), b.astype(np.float32)


def low_contrast_pair(seed, H, W, mean=0.8, std=0.01):
    rng = np.random.default_rng(seed)
    a = mean + std * rng.standard_normal((3, H, W))
    b = a + 0.7 * std * rng.standard_normal((3, H, W))
    return a.astype(np.float32), b.astype(np.float32)


def feature_pair(seed, N, D):
    """P = 0.35 G + noise"""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((N, D))
    return G.astype(np.float32), (0.35 * G + rng.standard_normal((N, D))).astype(np.float32)
