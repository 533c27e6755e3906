"""csrc/clip_vision.hip through the C ABI on both backends (CPU lane emulator / MI355X): patch_rows16 against torch.nn.functional.unfold on the CPU,
embed_ln16 (position row + LayerNorm) against fp64 at tests/test_kernels_unet.py's layernorm16 tolerances."""
import numpy as np
import pytest
import torch

from backends import be, ok  # noqa: F401
from eeg_image_decode_amd import _abi

SENTINEL = 0x7BCD
T16 = {_abi.DT_F16: torch.float16, _abi.DT_BF16: torch.bfloat16, _abi.DT_F32: torch.float32}


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().copy()


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "scale_shift"])
@pytest.mark.parametrize("out_dt", [_abi.DT_F16, _abi.DT_BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("pix_dt", [_abi.DT_F32, _abi.DT_F16, _abi.DT_BF16], ids=["px_f32", "px_f16", "px_bf16"])
def test_patch_rows16(be, pix_dt, out_dt, affine):
    """B = 2, image 28 x 42, patch 14: 6 patches + the class slot per image, K = 588 padded to 640.  Class rows and pad columns exactly zero; a 16-bit pixel of
    the output's own format is copied bit for bit, and every other pixel without scale / shift (fp32, or the other 16-bit format) is one correctly rounded
    conversion of an exact fp32 value: bit-exact equality with the reference rounded once.  With scale / shift the fp32 value pixel * scale + shift may be
    one fused or two separate operations: the bit patterns may be one unit in the last place apart, no more."""
    g = torch.Generator().manual_seed(100 * pix_dt + 10 * out_dt + int(affine))
    B, H, W, P = 2, 28, 42, 14
    px = (torch.rand(B, 3, H, W, generator=g) * (255.0 if affine else 2.0) - (0.0 if affine else 1.0)).to(T16[pix_dt])
    scale = torch.tensor([1 / (255 * 0.2686), 1 / (255 * 0.2613), 1 / (255 * 0.2758)], dtype=torch.float32)
    shift = torch.tensor([-0.4815 / 0.2686, -0.4578 / 0.2613, -0.4082 / 0.2758], dtype=torch.float32)
    K, Kpad, T = 3 * P * P, 640, 1 + (H // P) * (W // P)
    x32 = px.float()
    if affine:
        x32 = x32 * scale[None, :, None, None] + shift[None, :, None, None]
    ref = torch.zeros(B, T, Kpad)
    ref[:, 1:, :K] = torch.nn.functional.unfold(x32, kernel_size=P, stride=P).transpose(1, 2)       # (B, patches, (c, i, j))
    ref16 = _bits(ref.to(T16[out_dt])).reshape(B * T, Kpad)

    PX = be.dev(_bits(px) if pix_dt != _abi.DT_F32 else px.numpy())
    SC, SH = (be.dev(scale.numpy()), be.dev(shift.numpy())) if affine else (None, None)
    OUT = be.dev(np.full((B * T + 3, Kpad), SENTINEL, np.int16))
    ok(be.lib.eegclip_patch_rows16(be.ptr(PX), pix_dt, be.ptr(SC), be.ptr(SH), be.ptr(OUT), B, H, W, P, out_dt, be.stream))
    be.sync()
    raw = be.host(OUT)
    got = raw[:B * T]
    assert (raw[B * T:] == SENTINEL).all(), "rows behind the output were written"
    assert (got.reshape(B, T, Kpad)[:, 0] == 0).all(), "class rows must be zero"
    assert (got[:, K:] == 0).all(), "pad columns must be zero"
    if not affine:
        assert np.array_equal(got, ref16)
    else:
        assert np.abs(got.astype(np.int32) - ref16.astype(np.int32)).max() <= 1


def test_patch_rows16_rejections(be):
    B, H, W, P = 1, 28, 28, 14
    PX = be.zeros((B, 3, H, W), np.float32)
    OUT = be.zeros((B * 5, 640), np.int16)
    SC = be.zeros((3,), np.float32)

    def call(px=None, pdt=_abi.DT_F32, sc=None, sh=None, out=None, B_=B, H_=H, W_=W, P_=P, dt=_abi.DT_F16):
        return be.lib.eegclip_patch_rows16(be.ptr(PX) if px is None else px, pdt, sc, sh, be.ptr(OUT) if out is None else out, B_, H_, W_, P_, dt, be.stream)

    assert call() == 0
    assert call(H_=27) < 0 and call(W_=30) < 0 and call(P_=0) < 0 and call(B_=0) < 0
    assert call(pdt=5) < 0 and call(dt=_abi.DT_F32) < 0
    assert call(sc=be.ptr(SC)) < 0                                     # scale without shift
    assert call(out=be.ptr(OUT) + 2) < 0 and call(px=be.ptr(PX) + 2) < 0


def _embed_ln(be, C, dt):
    rng = np.random.default_rng(C + dt)
    T, B = 5, 2
    rows, ld = B * T, C + 64
    tdt = T16[dt]
    r16 = lambda a: torch.tensor(np.asarray(a, np.float32)).to(tdt)
    x, pos = r16(rng.standard_normal((rows, C)) * 2), r16(rng.standard_normal((T, C)) + 0.5)
    g, b = r16(1 + 0.3 * rng.standard_normal(C)), r16(0.3 * rng.standard_normal(C))
    xs = np.zeros((rows, ld), np.int16)
    xs[:, :C] = _bits(x)
    X, PS, GA, BE = be.dev(xs), be.dev(_bits(pos)), be.dev(_bits(g)), be.dev(_bits(b))
    Y = be.dev(np.full((rows + 1, C), SENTINEL, np.int16))
    ok(be.lib.eegclip_embed_ln16(be.ptr(X), ld, be.ptr(PS), T, be.ptr(GA), be.ptr(BE), be.ptr(Y), C, rows, C, 1e-5, dt, be.stream))
    be.sync()
    raw = be.host(Y)
    assert (raw[rows:] == SENTINEL).all()
    got = torch.tensor(raw[:rows]).view(tdt).double().numpy()
    xd = x.double().numpy() + np.tile(pos.double().numpy(), (B, 1))
    gd, bd = g.double().numpy(), b.double().numpy()
    ng = (xd - xd.mean(1, keepdims=True)) / np.sqrt(xd.var(1, keepdims=True) + 1e-5) * gd
    assert be.lib.eegclip_embed_ln16(be.ptr(X), ld, be.ptr(PS), T, be.ptr(GA), be.ptr(BE), be.ptr(Y), C, rows, C - 4, 1e-5, dt, be.stream) < 0     # C % 8
    assert be.lib.eegclip_embed_ln16(be.ptr(X), ld, be.ptr(PS), 0, be.ptr(GA), be.ptr(BE), be.ptr(Y), C, rows, C, 1e-5, dt, be.stream) < 0         # T < 1
    return got, ng, bd


@pytest.mark.parametrize("C", [128, 640])
def test_embed_ln16_bf16(be, C):
    """test_kernels_unet.py::test_layernorm16's tolerance (bf16: atol 3e-2, rtol 1e-2)"""
    got, ng, bd = _embed_ln(be, C, _abi.DT_BF16)
    np.testing.assert_allclose(got, ng + bd, atol=3e-2, rtol=1e-2)


@pytest.mark.parametrize("C", [128, 640])
def test_embed_ln16_fp16(be, C):
    """test_kernels_unet.py::test_layernorm16_fp16_against_fp64's bound: one fp16 ulp of the exact value plus 6e-5 of the summands' size"""
    got, ng, bd = _embed_ln(be, C, _abi.DT_F16)
    ref = ng + bd
    bound = np.spacing(np.abs(ref).astype(np.float16)).astype(np.float64) + 6e-5 * (np.abs(ng) + np.abs(bd))
    assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) / bound).max())
