"""csrc/image_resize.hip through the C ABI on both backends (CPU lane emulator / MI355X) against PIL itself (tests/preprocess_ref.py): every comparison covers
every output element and is exact on the integer values (scale = shift = NULL), no tolerance and no excluded share.  Sizes are written width x height, as PIL
writes them.  The NumPy restatement of the fixed-point algorithm is asserted equal to PIL first, and the host-only coefficient builder equal to it."""
import ctypes

import numpy as np
import pytest
import torch

import preprocess_ref as R
from backends import be, ok  # noqa: F401
from eeg_image_decode_amd import _abi

SENTINEL = -77.0
FILTERS = {"bicubic": _abi.RESIZE_BICUBIC, "bilinear": _abi.RESIZE_BILINEAR}
NP_OUT = {_abi.DT_F32: np.float32, _abi.DT_F16: np.int16, _abi.DT_BF16: np.int16}
T_OUT = {_abi.DT_F32: torch.float32, _abi.DT_F16: torch.float16, _abi.DT_BF16: torch.bfloat16}
_ip = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def tables(lib, in_size, out_size, first, count, filt, extra=0):
    """the host-only builder: (bounds (count, 2), coeffs (count, ksize + extra), ksize + extra)"""
    ks = lib.eegclip_resize_coeffs(in_size, out_size, 0, 0, FILTERS[filt], None, None, 0)
    assert ks >= 3
    ks += extra
    b, k = np.zeros((count, 2), np.int32), np.full((count, ks), 12345, np.int32)
    assert lib.eegclip_resize_coeffs(in_size, out_size, first, count, FILTERS[filt], _ip(b), _ip(k), ks) == ks - extra
    return b, k, ks


def resize(be, src, rh, rw, filt, window=None, out_dt=_abi.DT_F32, scale=None, shift=None, src_kind=_abi.SRC_U8_HWC, a=0.0, b=0.0, extra=0):
    """src: uint8 (B, H, W, 3), or (B, 3, H, W) planes as the array the device holds (fp32, or int16 bit patterns) with src_kind -> (B, 3, ch, cw) as a torch
    tensor of the output type; the element row behind the output must keep its sentinel"""
    B = src.shape[0]
    H, W = (src.shape[1], src.shape[2]) if src_kind == _abi.SRC_U8_HWC else (src.shape[2], src.shape[3])
    top, left, ch, cw = window if window is not None else (0, 0, rh, rw)
    hb, hk, kh = tables(be.lib, W, rw, left, cw, filt, extra)
    vb, vk, kv = tables(be.lib, H, rh, top, ch, filt, extra)
    sent = np.float32(SENTINEL) if out_dt == _abi.DT_F32 else np.int16(0x7BCD)
    OUT = be.dev(np.full((B * 3 * ch + 1, cw), sent, NP_OUT[out_dt]))
    SRC, HB, HK, VB, VK = be.dev(src), be.dev(hb), be.dev(hk), be.dev(vb), be.dev(vk)
    SC, SH = (be.dev(scale), be.dev(shift)) if scale is not None else (None, None)
    ok(be.lib.eegclip_resize_crop_normalize(be.ptr(SRC), src_kind, a, b, B, H, W, rh, rw, top, left, ch, cw, FILTERS[filt], be.ptr(HB), be.ptr(HK), kh, be.ptr(VB),
                                            be.ptr(VK), kv, be.ptr(SC), be.ptr(SH), be.ptr(OUT), out_dt, be.stream))
    be.sync()
    raw = be.host(OUT)
    assert (raw[B * 3 * ch:] == sent).all(), "the row behind the output was written"
    return torch.tensor(raw[:B * 3 * ch].reshape(B, 3, ch, cw)).view(T_OUT[out_dt])


def pil_batch(src, rh, rw, filt, window=None):
    """(B, H, W, 3) uint8 -> PIL's resize and the window, as (B, 3, ch, cw) integers"""
    top, left, ch, cw = window if window is not None else (0, 0, rh, rw)
    return np.stack([R.pil_resize(s, rh, rw, filt)[top:top + ch, left:left + cw].transpose(2, 0, 1) for s in src]).astype(np.int64)


def exact(be, src, rh, rw, filt, window=None, **kw):
    got = resize(be, src, rh, rw, filt, window, **kw)
    want = pil_batch(src, rh, rw, filt, window)
    assert np.array_equal(got.double().numpy().astype(np.int64), want), int((got.double().numpy() != want).sum())
    return got


def rand_u8(seed, B, H, W):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


# (width, height) -> (width, height), as the shapes are listed
SHAPES = {"down": ((61, 47), (24, 31)), "up": ((20, 23), (44, 51)), "one_axis": ((33, 33), (33, 20)), "strong_down": ((257, 300), (16, 16)),
          "lds_shrink": ((600, 650), (40, 40))}


@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("shape", list(SHAPES) + ["non_square"])
def test_numpy_restatement_is_pil(shape, filt):
    """the fixed-point algorithm as this repository states it == Image.resize, byte for byte (no kernel involved)"""
    (w0, h0), (w1, h1) = SHAPES.get(shape, ((37, 90), (16, 38)))
    a = rand_u8(1, 1, h0, w0)[0]
    assert np.array_equal(R.numpy_resize(a, h1, w1, filt), R.pil_resize(a, h1, w1, filt))


@pytest.mark.parametrize("filt", list(FILTERS))
def test_coefficient_builder_matches_the_restatement(be, filt):
    """eegclip_resize_coeffs (host code of the library under test) against preprocess_ref.coeffs: bounds and every coefficient equal, a sub-range is the
    rows of the whole, the tail of a wider row is zero; ksize 5 / 3 when up-scaling, 67 and 77 (bicubic) at 257 x 300 -> 16 x 16"""
    for in_size, out_size in ((47, 31), (61, 24), (20, 44), (23, 51), (33, 33), (300, 16), (257, 16), (500, 224)):
        rb, rk = R.coeffs(in_size, out_size, filt)
        b, k, ks = tables(be.lib, in_size, out_size, 0, out_size, filt)
        assert ks == rk.shape[1] and np.array_equal(b, rb) and np.array_equal(k, rk), (in_size, out_size)
        first, count = out_size // 3, out_size - out_size // 3 - 1
        if count >= 1:
            b2, k2, ks2 = tables(be.lib, in_size, out_size, first, count, filt, extra=2)
            assert np.array_equal(b2, rb[first:first + count]) and np.array_equal(k2[:, :ks], rk[first:first + count]) and not k2[:, ks:].any()
    want = {"bicubic": (5, 67, 77), "bilinear": (3, 35, 39)}[filt]
    assert tuple(be.lib.eegclip_resize_coeffs(i, o, 0, 0, FILTERS[filt], None, None, 0) for i, o in ((20, 44), (257, 16), (300, 16))) == want
    b, k = np.zeros((4, 2), np.int32), np.zeros((4, 16), np.int32)
    call = lambda i=47, o=31, f=0, c=4, fl=FILTERS[filt], ks=16: be.lib.eegclip_resize_coeffs(i, o, f, c, fl, _ip(b), _ip(k), ks)
    assert call() > 0
    assert call(i=0) < 0 and call(o=0) < 0 and call(f=-1) < 0 and call(f=28) < 0 and call(c=0) < 0 and call(fl=1) < 0 and call(ks=4) < 0


@pytest.mark.parametrize("filt", list(FILTERS))
def test_down_scaling_batch_of_three(be, filt):
    """61 x 47 -> 24 x 31, three different images in one launch"""
    (w0, h0), (w1, h1) = SHAPES["down"]
    src = rand_u8(2, 3, h0, w0)
    got = exact(be, src, h1, w1, filt)
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])


@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("shape", ["up", "one_axis", "strong_down", "lds_shrink"])
def test_other_scales(be, shape, filt):
    """up-scaling (ksize 5 / 3, bounds clipped at both borders); one axis unchanged (the identity pass); scale 16 and 18.75 (bicubic ksize 67 horizontally, 77
    vertically); scale 15 and 16.25 into a window 40 wide: the 64-column tile's strip of 16 rows (327 input rows x 192 bytes + 20 KB of bicubic coefficients)
    does not fit 64 KiB of LDS, the host halves the tile's height"""
    (w0, h0), (w1, h1) = SHAPES[shape]
    exact(be, rand_u8(3, 1, h0, w0), h1, w1, filt)


@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("to", [(24, 31), (122, 94)], ids=["down", "up"])
def test_clamp_both_ends(be, to, filt):
    """a random {0, 255} image: the unclamped horizontal sums leave 0..255 on both sides (bicubic; counted below on the restatement, which is PIL), so both
    ends of clip8 and the arithmetic shift of negative sums are exercised"""
    w0, h0 = 61, 47
    src = (np.random.default_rng(4).integers(0, 2, (1, h0, w0, 3)) * 255).astype(np.uint8)
    _, sums = R.numpy_resize(src[0], to[1], to[0], filt, return_sums=True)
    below, above = int((sums < 0).sum()), int(((sums >> R.BITS) > 255).sum())
    print(f"\n[clamp] {filt} -> {to}: {below} sums below 0, {above} above 255", end=" ")
    if filt == "bicubic":
        assert below > 100 and above > 100
    exact(be, src, to[1], to[0], filt)


@pytest.mark.parametrize("rounding", ["torchvision", "transformers"])
def test_window_with_offset(be, rounding):
    """shortest side 24 from 61 x 47 (-> 31 x 24), crop 24 x 24: the remainder 7 is odd, so the two rounding rules put the window at column 4 and 3; the
    window is the reference's resize-then-crop; coefficient rows one longer than needed (a row stride above ksize)"""
    src = rand_u8(5, 2, 47, 61)
    rh, rw = R.resized_size(47, 61, 24)
    assert (rh, rw) == (24, 31)
    top, left = R.crop_origin(rh, rw, 24, 24, rounding)
    assert (top, left) == ((0, 4) if rounding == "torchvision" else (0, 3))
    got = exact(be, src, rh, rw, "bicubic", window=(top, left, 24, 24), extra=1)
    want = np.stack([R.resize_crop(s, 24, (24, 24), "bicubic", rounding).transpose(2, 0, 1) for s in src])
    assert np.array_equal(got.numpy().astype(np.int64), want)
    exact(be, src.transpose(0, 2, 1, 3).copy(), 31, 24, "bilinear", window=(left, 0, 24, 24))        # (the tall image: the offset on the vertical axis)


@pytest.mark.parametrize("filt", list(FILTERS))
def test_full_tile_with_many_images(be, filt):
    """the launcher shrinks its 16 x 64 tile while there are fewer workgroups than CUs, so the cases above run on small tiles: 64 images of 10 x 9 -> 65 x 17
    make 2 x 2 x 64 = 256 workgroups of the full tile, with a ragged last column and row"""
    exact(be, rand_u8(10, 64, 9, 10), 17, 65, filt)


def test_workload_shape(be):
    """500 x 500 -> 224 x 224, B = 1, bicubic: the feature cache's own shape, once"""
    exact(be, rand_u8(6, 1, 500, 500), 224, 224, "bicubic")


@pytest.mark.parametrize("case", ["f32_half_half", "f16_half_half", "bf16_half_half", "f32_one_zero"])
def test_float_loader(be, case):
    """(B, 3, H, W) planes quantised on load as diffusers' postprocess(output_type="pil") does it: equal to PIL on
    ((x.float() / 2 + 0.5).clamp(0, 1).numpy() * 255).round().astype(uint8) (x / 2 is x * 0.5 exactly; both sides do the same fp32 operations)"""
    g = torch.Generator().manual_seed(7)
    B, H, W = 2, 47, 61
    if case == "f32_one_zero":
        x, a, b = torch.rand(B, 3, H, W, generator=g), 1.0, 0.0
        x[0, :, :4] = torch.tensor([0.0, 1.0, 0.5 / 255, 1.5 / 255])[None, :, None]                   # (ends and ties)
        q = (x.clamp(0, 1).numpy() * 255).round().astype(np.uint8)
    else:
        tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[case.split("_")[0]]
        x, a, b = (torch.rand(B, 3, H, W, generator=g) * 2.4 - 1.2).to(tdt), 0.5, 0.5
        q = ((x.float() / 2 + 0.5).clamp(0, 1).numpy() * 255).round().astype(np.uint8)
    assert q.min() == 0 and q.max() == 255
    kind = {torch.float32: _abi.DT_F32, torch.float16: _abi.DT_F16, torch.bfloat16: _abi.DT_BF16}[x.dtype]
    dev = x.numpy() if x.dtype == torch.float32 else x.view(torch.int16).numpy()
    for filt in FILTERS:
        got = resize(be, dev, 31, 24, filt, src_kind=kind, a=a, b=b)
        assert np.array_equal(got.numpy().astype(np.int64), pil_batch(np.ascontiguousarray(q.transpose(0, 2, 3, 1)), 31, 24, filt))


@pytest.mark.parametrize("out_dt", [_abi.DT_F32, _abi.DT_F16, _abi.DT_BF16], ids=["f32", "f16", "bf16"])
def test_normalisation(be, out_dt):
    """CLIP's mean / std, rescale 1 / 255: fp32 within 2^-23 (|q scale_c| + |shift_c|) of the fp64 value on the fp32 scale / shift; fp16 / bf16 within one unit
    in the last place of that value rounded once.  Without scale / shift every type holds the integers exactly."""
    src = rand_u8(8, 2, 47, 61)
    scale, shift = R.affine(R.CLIP_MEAN, R.CLIP_STD, 1 / 255)
    got = resize(be, src, 31, 24, "bicubic", out_dt=out_dt, scale=scale, shift=shift)
    q = np.stack([R.pil_resize(s, 31, 24, "bicubic") for s in src])
    R.assert_normalized(got, q, scale, shift)
    plain = resize(be, src, 31, 24, "bicubic", out_dt=out_dt)
    assert np.array_equal(plain.double().numpy().astype(np.int64), pil_batch(src, 31, 24, "bicubic"))


def test_rejections(be):
    """every error of the list returns < 0 beside the valid call, which returns 0"""
    B, H, W, rh, rw = 1, 47, 61, 31, 24
    hb, hk, kh = tables(be.lib, W, rw, 0, rw, "bicubic")
    vb, vk, kv = tables(be.lib, H, rh, 0, rh, "bicubic")
    SRC, HB, HK, VB, VK = be.dev(rand_u8(9, B, H, W)), be.dev(hb), be.dev(hk), be.dev(vb), be.dev(vk)
    F32 = be.zeros((B, 3, H, W), np.float32)
    OUT, SC = be.zeros((B * 3 * rh + 1, rw), np.float32), be.zeros((4,), np.float32)

    def call(src=None, kind=_abi.SRC_U8_HWC, B_=B, H_=H, W_=W, rh_=rh, rw_=rw, top=0, left=0, ch=rh, cw=rw, filt=_abi.RESIZE_BICUBIC, kh_=kh, kv_=kv, hb_=None,
             sc=None, sh=None, out=None, dt=_abi.DT_F32):
        return be.lib.eegclip_resize_crop_normalize(be.ptr(SRC) if src is None else src, kind, 0.5, 0.5, B_, H_, W_, rh_, rw_, top, left, ch, cw, filt,
                                                    be.ptr(HB) if hb_ is None else hb_, be.ptr(HK), kh_, be.ptr(VB), be.ptr(VK), kv_, sc, sh,
                                                    be.ptr(OUT) if out is None else out, dt, be.stream)

    assert call() == 0
    assert call(src=be.ptr(F32), kind=_abi.DT_F32) == 0 and call(sc=be.ptr(SC), sh=be.ptr(SC)) == 0 and call(top=3, ch=rh - 3, left=2, cw=rw - 2) == 0
    assert call(B_=0) < 0 and call(H_=0) < 0 and call(W_=0) < 0 and call(rh_=0) < 0 and call(rw_=0) < 0 and call(ch=0) < 0 and call(cw=0) < 0
    assert call(top=1) < 0 and call(left=1) < 0 and call(top=-1, ch=rh - 1) < 0 and call(left=-1, cw=rw - 1) < 0 and call(ch=rh + 1) < 0       # outside rh x rw
    assert call(kh_=kh - 1) < 0 and call(kv_=kv - 1) < 0
    assert call(filt=1) < 0 and call(filt=4) < 0 and call(kind=4) < 0 and call(kind=-1) < 0 and call(dt=3) < 0 and call(dt=-1) < 0
    assert call(sc=be.ptr(SC)) < 0 and call(sh=be.ptr(SC)) < 0                                         # scale without shift, and the reverse
    assert call(out=be.ptr(OUT) + 2) < 0 and call(hb_=be.ptr(HB) + 2) < 0 and call(src=be.ptr(F32) + 2, kind=_abi.DT_F32) < 0
    assert call(src=be.ptr(F32) + 1, kind=_abi.DT_F16) < 0 and call(sc=be.ptr(SC) + 2, sh=be.ptr(SC)) < 0
    assert call(src=be.ptr(SRC) + 1, B_=B, H_=H - 1) == 0                                              # (uint8 has no alignment)
    # a scale the smallest tile does not hold: 16384 -> 16 is 1024 x (coefficient rows of 4097); nothing is read before the rejection
    assert call(W_=16384, rw_=16, cw=16, kh_=8192) < 0
    be.sync()
