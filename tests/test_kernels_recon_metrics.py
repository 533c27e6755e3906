"""csrc/recon_metrics.hip through the C ABI on both backends (CPU lane emulator / MI355X) against the fp64 oracle tests/recon_metrics_ref.py.

Bounds (set with the feature, not from the kernel): SSIM within 1e-4 absolute of the oracle (the metric is reported to three decimals; an fp32 evaluation of
the same formula on the CPU was at most 7.7e-6 off), PixCorr within 1e-6 absolute on every case (fp64 moments, one fp32 rounding), two-way counts EQUAL to
the oracle's after the oracle's own smallest |r[i, j] - r[j, j]| was asserted above 1e-3, the optional r within 2e-5.  Every output array has a sentinel
element behind it that must survive, and every workspace starts as NaN bytes (nothing has to be cleared).  fp16 / bf16 inputs: the oracle sees the quantised
values.

Largest measured |kernel - oracle| per case (the MI355X and the emulator give the same figures; each test prints its own with -s):
  case                      SSIM      PixCorr   |  case                     SSIM      PixCorr
  11 x 11 smooth + noise    1.9e-07   1.7e-08   |  11 x 11 low contrast     2.9e-06   2.4e-08
  12 x 27 smooth + noise    7.8e-09   2.5e-08   |  12 x 27 low contrast     3.0e-06   8.8e-09
  37 x 53 smooth + noise    1.5e-09   5.1e-09   |  37 x 53 low contrast     2.7e-07   3.6e-09
  full tiles, B = 43        8.2e-07   3.0e-08   |  the same pair, B = 1     1.7e-08   7.6e-09
  batch of three            5.9e-07   7.2e-09   |  fp16 / bf16 planes       2.0e-07 / 6.6e-07   1.9e-08 / 8.3e-09
  two-way r: 2 x 7 3.0e-08, 17 x 130 3.7e-08, 33 x 1000 7.5e-08, 55 x 200 5.5e-08; oracle gaps 4.3e-01, 9.1e-03, 2.0e-01, 1.4e-02; counts equal everywhere.
  All SSIM errors are below 2e-5, so DESIGN has nothing to explain beyond section 4.7's note on the moments about 0.5.
"""
import numpy as np
import pytest
import torch

import recon_metrics_ref as R
from backends import be, ok  # noqa: F401
from eeg_image_decode_amd import _abi

TH, TW = _abi.SSIM_TILE_H, _abi.SSIM_TILE_W
SSIM_TOL, PIX_TOL, R_TOL, GAP = 1e-4, 1e-6, 2e-5, 1e-3
SENT = np.float32(-77.0)
# H x W.  "tiles": 3 row tiles x 2 column tiles of the FULL tile with ragged last ones; run with B = 43 so that the launcher (which shrinks the tile while
# there are fewer workgroups than the 256 CUs) keeps it: 43 * 6 = 258 workgroups
SHAPES = {"one_window": (11, 11), "12x27": (12, 27), "37x53": (37, 53), "tiles": (2 * TH + 5, TW + 9)}
FULL_TILE_B = 43


def run(be, a, b, dt=_abi.DT_F32, expect_tiles=None):
    """a, b: (B, 3, H, W) as the arrays the device holds (fp32, or int16 bit patterns) -> (pixcorr (B,), ssim (B,)) fp32"""
    B, _, H, W = a.shape
    nbytes = be.lib.eegclip_pixcorr_ssim_workspace_bytes(B, H, W)
    assert nbytes > 0 and nbytes % (8 * B) == 0
    if expect_tiles is not None:
        assert nbytes == B * expect_tiles * 10 * 8, (nbytes, expect_tiles)
    WS = be.dev(np.full(nbytes, 0xFF, np.uint8))
    S, P = be.dev(np.full(B + 1, SENT, np.float32)), be.dev(np.full(B + 1, SENT, np.float32))
    A, Bm = be.dev(a), be.dev(b)
    ok(be.lib.eegclip_pixcorr_ssim(be.ptr(A), be.ptr(Bm), dt, B, H, W, be.ptr(S), be.ptr(P), be.ptr(WS), nbytes, be.stream))
    be.sync()
    s, p = be.host(S), be.host(P)
    assert s[B] == SENT and p[B] == SENT, "the element behind an output was written"
    return p[:B], s[:B]


def check_pairs(be, pairs, label, **kw):
    """pairs: [(a, b)] of (3, H, W) fp32 -> asserts both metrics of every pair against the oracle; returns (pixcorr, ssim)"""
    a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    pix, ssm = run(be, a, b, **kw)
    want_p = np.array([R.pixcorr(x, y) for x, y in pairs])
    want_s = np.array([R.ssim(x, y) for x, y in pairs])
    ep, es = np.abs(pix - want_p).max(), np.abs(ssm - want_s).max()
    print(f"\n[recon_metrics {be.name}] {label}: ssim {want_s.min():.4f}..{want_s.max():.4f} max err {es:.2e}; pixcorr max err {ep:.2e}", end=" ")
    assert np.isfinite(ssm).all() and es <= SSIM_TOL, (label, es)
    assert np.isfinite(pix).all() and ep <= PIX_TOL, (label, ep)
    return pix, ssm


@pytest.mark.parametrize("content", ["smooth_noise", "low_contrast"])
@pytest.mark.parametrize("shape", ["one_window", "12x27", "37x53"])
def test_single_pair(be, shape, content):
    """B = 1 (the launcher's smallest tiles: 37 x 53 is 10 x 4 of them): a smooth image against a noisy copy, and a low-contrast pair around mean 0.8 with
    std 0.01 -- raw fp32 moments are 1e-3 off there, shifted by 0.5 or not"""
    H, W = SHAPES[shape]
    pair = R.smooth_pair(3, H, W) if content == "smooth_noise" else R.low_contrast_pair(4, H, W)
    check_pairs(be, [pair], f"{shape} {content}")


@pytest.fixture(scope="module")
def full_tile_pairs():
    H, W = SHAPES["tiles"]
    return [R.smooth_pair(100 + i, H, W, noise=0.05 + 0.01 * i) if i % 3 else R.low_contrast_pair(100 + i, H, W) for i in range(FULL_TILE_B)]


def test_full_tiles_ragged_and_tiling_independence(be, full_tile_pairs):
    """(2 TH + 5) x (TW + 9) with B = 43: 3 x 2 full tiles per pair, the last row tile 5 high and the last column tile 9 wide; then pair 7 alone (B = 1: the
    smallest tiles) gives the same bits"""
    H, W = SHAPES["tiles"]
    pix, ssm = check_pairs(be, full_tile_pairs, "full tiles", expect_tiles=6)
    small = be.lib.eegclip_pixcorr_ssim_workspace_bytes(1, H, W) // 80
    assert small == ((H + 3) // 4) * ((W + 15) // 16)
    p1, s1 = check_pairs(be, full_tile_pairs[7:8], "the same pair on 4 x 16 tiles")
    assert p1[0] == pix[7] and s1[0] == ssm[7]


def test_batch_of_three_different_pairs(be):
    """B = 3 at 37 x 53: smooth + noise, low contrast, and an identical pair (SSIM 1, PixCorr 1) in one launch -- a wrong batch stride mixes them"""
    H, W = SHAPES["37x53"]
    a, _ = R.smooth_pair(5, H, W)
    pairs = [R.smooth_pair(6, H, W), R.low_contrast_pair(7, H, W), (a, a.copy())]
    pix, ssm = check_pairs(be, pairs, "batch of three")
    assert abs(ssm[2] - 1.0) <= 1e-6 and abs(pix[2] - 1.0) <= 1e-6
    assert 0.1 < ssm[0] < 0.9 and len({float(v) for v in ssm}) == 3


def test_constant_image_is_nan_pixcorr_finite_ssim(be):
    """a constant image (0.3: not a dyadic value, the raw moments do not cancel to zero by themselves): PixCorr NaN as np.corrcoef gives, SSIM finite
    and the oracle's"""
    H, W = SHAPES["12x27"]
    _, b = R.smooth_pair(8, H, W)
    const = np.full((3, H, W), 0.3, np.float32)
    assert np.isnan(R.pixcorr(const, b))
    for pair in ((const, b), (b, const), (const, const)):
        pix, ssm = run(be, pair[0][None], pair[1][None])
        assert np.isnan(pix[0]) and np.isfinite(ssm[0]) and abs(ssm[0] - R.ssim(*pair)) <= SSIM_TOL


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_half_inputs(be, dt):
    """fp16 / bf16 planes, B = 2 at 37 x 53: the oracle is applied to the quantised values"""
    H, W = SHAPES["37x53"]
    tdt, code = (torch.float16, _abi.DT_F16) if dt == "f16" else (torch.bfloat16, _abi.DT_BF16)
    pairs = [R.smooth_pair(9, H, W), R.low_contrast_pair(10, H, W)]
    q = [tuple(torch.from_numpy(x).to(tdt) for x in p) for p in pairs]
    a, b = torch.stack([p[0] for p in q]), torch.stack([p[1] for p in q])
    pix, ssm = run(be, a.view(torch.int16).numpy(), b.view(torch.int16).numpy(), dt=code)
    want_p = np.array([R.pixcorr(x.float().numpy(), y.float().numpy()) for x, y in q])
    want_s = np.array([R.ssim(x.float().numpy(), y.float().numpy()) for x, y in q])
    ep, es = np.abs(pix - want_p).max(), np.abs(ssm - want_s).max()
    print(f"\n[recon_metrics {be.name}] {dt}: ssim max err {es:.2e}; pixcorr max err {ep:.2e}", end=" ")
    assert es <= SSIM_TOL and ep <= PIX_TOL


def test_pixcorr_ssim_rejections(be):
    A = be.zeros((1, 3, 12, 27), np.float32)
    S, WS = be.zeros((4,), np.float32), be.zeros((4096,), np.float64)

    def call(a=None, dt=_abi.DT_F32, B=1, H=12, W=27, s=None, ws=None, nbytes=4096 * 8):
        return be.lib.eegclip_pixcorr_ssim(be.ptr(A) if a is None else a, be.ptr(A), dt, B, H, W, be.ptr(S) if s is None else s, be.ptr(S) + 8,
                                           be.ptr(WS) if ws is None else ws, nbytes, be.stream)

    assert call() == 0
    assert call(H=10, W=27) < 0 and call(H=12, W=10) < 0 and call(B=0) < 0 and call(dt=3) < 0 and call(dt=-1) < 0 and call(nbytes=8) < 0
    assert call(a=be.ptr(A) + 2) < 0 and call(s=be.ptr(S) + 2) < 0 and call(ws=be.ptr(WS) + 4) < 0
    q = be.lib.eegclip_pixcorr_ssim_workspace_bytes
    assert q(1, 10, 27) < 0 and q(1, 27, 10) < 0 and q(0, 12, 27) < 0 and q(1, 11, 11) > 0
    be.sync()


# ---- two-way identification ----
# (N, D, seed): D = 7 and 130 take the scalar loads (D % 4 != 0), 1000 and 200 the 16-byte ones; N = 55 is 4 row tiles x 4 column tiles, the last 7 wide;
# D = 200 leaves the four waves' k ranges unequal (3 steps of 64 and a part of a fourth)
TWO_WAY = {"2x7": (2, 7, 1), "17x130": (17, 130, 1), "33x1000": (33, 1000, 1), "tiles": (3 * 16 + 7, 200, 1)}


@pytest.mark.parametrize("case", list(TWO_WAY))
def test_two_way(be, case):
    N, D, seed = TWO_WAY[case]
    G, P = R.feature_pair(seed, N, D)
    r, count, score = R.two_way(G, P)
    gap = R.two_way_gap(r)
    assert gap > GAP, (case, gap)
    nbytes = be.lib.eegclip_two_way_workspace_bytes(N, D)
    assert nbytes > 0
    WS = be.dev(np.full(nbytes, 0xFF, np.uint8))
    C, Rm = be.dev(np.full(N + 1, -7, np.int32)), be.dev(np.full(N * N + 1, SENT, np.float32))
    Gd, Pd = be.dev(G), be.dev(P)
    ok(be.lib.eegclip_two_way(be.ptr(Gd), be.ptr(Pd), N, D, be.ptr(C), be.ptr(Rm), be.ptr(WS), nbytes, be.stream))
    be.sync()
    c, rm = be.host(C), be.host(Rm)
    assert c[N] == -7 and rm[N * N] == SENT
    err = np.abs(rm[:N * N].reshape(N, N) - r).max()
    print(f"\n[recon_metrics {be.name}] two-way {case}: gap {gap:.1e}, score {score:.4f}, r max err {err:.2e}", end=" ")
    assert np.array_equal(c[:N], count) and err <= R_TOL
    C2 = be.dev(np.full(N + 1, -7, np.int32))                          # without r: the same counts
    ok(be.lib.eegclip_two_way(be.ptr(Gd), be.ptr(Pd), N, D, be.ptr(C2), None, be.ptr(WS), nbytes, be.stream))
    be.sync()
    assert np.array_equal(be.host(C2), c)


def test_two_way_rejections(be):
    G, C, WS = be.zeros((4, 8), np.float32), be.zeros((8,), np.int32), be.zeros((256,), np.int32)

    def call(N=4, D=8, g=None, nbytes=1024):
        return be.lib.eegclip_two_way(be.ptr(G) if g is None else g, be.ptr(G), N, D, be.ptr(C), None, be.ptr(WS), nbytes, be.stream)

    assert call() == 0
    assert call(N=1) < 0 and call(D=1) < 0 and call(nbytes=16) < 0 and call(g=be.ptr(G) + 2) < 0
    q = be.lib.eegclip_two_way_workspace_bytes
    assert q(1, 8) < 0 and q(4, 1) < 0 and q(2, 2) > 0
    be.sync()
