"""The yardstick of the image preprocessing tests: PIL itself (Image.resize on 8-bit RGB), the size and crop rules of torchvision / transformers written
out, and beside it a NumPy restatement of PIL's fixed-point resampling (Pillow src/libImaging/Resample.c) that tests/test_kernels_resize.py asserts equal to
PIL first -- so the kernel is never the only witness of the algorithm.  Nothing here imports the product.

transformers' CLIPImageProcessor runs here without torchvision (it falls back to its PIL backend), so tests/test_preprocess_emu.py pins clip_image_processor
to the class itself as well (`hf_clip_image_processor`), beside the rules written out below."""
import numpy as np

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
BITS = 22


def pil_filter(name):
    from PIL import Image
    return {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}[name]


def pil_resize(a, h, w, filt):
    """uint8 (H, W, 3) -> uint8 (h, w, 3) with Image.resize"""
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(a)).resize((w, h), pil_filter(filt)))


def to_rgb_array(img):
    """a PIL image (any mode) or a uint8 (H, W, 3) array -> uint8 (H, W, 3)"""
    if isinstance(img, np.ndarray):
        return img
    return np.asarray(img.convert("RGB"))


# ---------------------------------------------------------------------------------------------------------------- size and crop rules
def resized_size(H, W, size):
    """int: shortest side -> size, the long side int(size * long / short) (torchvision.transforms.Resize and transformers' get_resize_output_image_size
    compute the same); (h, w): as given"""
    if isinstance(size, int):
        short, long = (H, W) if H <= W else (W, H)
        new_long = int(size * long / short)
        return (size, new_long) if H <= W else (new_long, size)
    return int(size[0]), int(size[1])


def crop_origin(Hr, Wr, h, w, rounding):
    """top-left of the centred (h, w) window in a (Hr, Wr) image: torchvision's int(round((Hr - h) / 2.0)) or transformers' (Hr - h) // 2"""
    if rounding == "torchvision":
        return int(round((Hr - h) / 2.0)), int(round((Wr - w) / 2.0))
    return (Hr - h) // 2, (Wr - w) // 2


def resize_crop(a, size, crop, filt, rounding):
    """uint8 (H, W, 3) -> PIL's resize, then the centred crop: uint8 (h, w, 3)"""
    Hr, Wr = resized_size(a.shape[0], a.shape[1], size)
    r = pil_resize(a, Hr, Wr, filt)
    if crop is None:
        return r
    top, left = crop_origin(Hr, Wr, crop[0], crop[1], rounding)
    return r[top:top + crop[0], left:left + crop[1]]


# ---------------------------------------------------------------------------------------------------------------- the fixed-point algorithm in NumPy
def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def coeffs(in_size, out_size, filt):
    """precompute_coeffs + normalize_coeffs_8bpc: (bounds (out, 2) int32, k (out, ksize) int32)"""
    f, S = (_bicubic, 2.0) if filt == "bicubic" else (_bilinear, 1.0)
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = S * fs
    ss = 1.0 / fs
    ksize = int(np.ceil(support)) * 2 + 1
    bounds, k = np.zeros((out_size, 2), np.int32), np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = np.array([f((x + xmin - center + 0.5) * ss) for x in range(n)], np.float64)
        ww = 0.0
        for v in w:                                               # (PIL's left-to-right sum)
            ww += v
        if ww != 0.0:
            w = w / ww
        k[xx, :n] = [int(-0.5 + v * (1 << BITS)) if v < 0 else int(0.5 + v * (1 << BITS)) for v in w]
        bounds[xx] = xmin, n
    return bounds, k


def _pass(a, bounds, k):
    """one pass along axis 1 of (R, n_in, C) uint8 -> (R, n_out, C) uint8; `sums` also returned (before the shift) for the clamp statistics"""
    out = np.zeros((a.shape[0], len(bounds), a.shape[2]), np.uint8)
    sums = np.zeros(out.shape, np.int64)
    for xx, (xmin, n) in enumerate(bounds):
        s = (1 << (BITS - 1)) + np.tensordot(a[:, xmin:xmin + n].astype(np.int64), k[xx, :n].astype(np.int64), axes=([1], [0]))
        assert np.abs(s).max() < 2 ** 31
        sums[:, xx] = s
        out[:, xx] = np.clip(s >> BITS, 0, 255)
    return out, sums


def numpy_resize(a, h, w, filt, return_sums=False):
    """PIL's ImagingResample on uint8 (H, W, 3): horizontal pass, rounding to uint8, vertical pass, rounding to uint8"""
    hb, hk = coeffs(a.shape[1], w, filt)
    vb, vk = coeffs(a.shape[0], h, filt)
    t, hsums = _pass(a, hb, hk)
    o, _ = _pass(np.ascontiguousarray(t.transpose(1, 0, 2)), vb, vk)
    o = np.ascontiguousarray(o.transpose(1, 0, 2))
    return (o, hsums) if return_sums else o


# ---------------------------------------------------------------------------------------------------------------- the affine and its bound
def affine(mean, std, rescale):
    """fp32 per-channel (scale, shift) of y = (q * rescale - mean) / std, each computed in double and rounded once"""
    m, s = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    return (rescale / s).astype(np.float32), (-m / s).astype(np.float32)


def range_affine(lo, hi):
    """y = lo + q / 255 * (hi - lo)"""
    return np.full(3, (hi - lo) / 255.0, np.float64).astype(np.float32), np.full(3, float(lo), np.float64).astype(np.float32)


def normalized(q, scale, shift):
    """q uint8 (.., h, w, 3) -> (fp64 value of q * scale_c + shift_c on the fp32 scale / shift as (.., 3, h, w), the fp32 bound: three roundings of at
    most half a unit in the last place each, on terms no larger than |q scale_c| and |shift_c|: 2^-23 (|q scale_c| + |shift_c|))"""
    qd = np.moveaxis(q.astype(np.float64), -1, -3)
    sc, sh = scale.astype(np.float64)[:, None, None], shift.astype(np.float64)[:, None, None]
    return qd * sc + sh, 2.0 ** -23 * (np.abs(qd * sc) + np.abs(sh))


def assert_normalized(got, q, scale, shift):
    """got: a torch tensor (.., 3, h, w) in fp32 / fp16 / bf16 against `normalized`: fp32 within the bound; 16-bit within one unit in the last place of the
    exact value rounded once (tests/test_kernels_clip_vision.py::test_patch_rows16's criterion for its scale_shift cases)"""
    import torch
    want, bound = normalized(q, scale, shift)
    assert tuple(got.shape) == want.shape, (tuple(got.shape), want.shape)
    if got.dtype == torch.float32:
        err = np.abs(got.double().numpy() - want)
        assert (err <= bound).all(), float((err / bound).max())
    else:
        ref16 = torch.tensor(want).to(got.dtype).contiguous().view(torch.int16).numpy().astype(np.int32)
        got16 = got.contiguous().view(torch.int16).numpy().astype(np.int32)
        assert np.abs(got16 - ref16).max() <= 1


# ---------------------------------------------------------------------------------------------------------------- the three presets
def open_clip_ref(img, size=224):
    """Resize(size, BICUBIC), CenterCrop(size) (torchvision's rounding), ToTensor, Normalize(CLIP mean / std): (q uint8 (size, size, 3), scale, shift)"""
    return (resize_crop(to_rgb_array(img), size, (size, size), "bicubic", "torchvision"),) + affine(CLIP_MEAN, CLIP_STD, 1 / 255)


def clip_image_processor_ref(img, size=224):
    """CLIPImageProcessor's defaults: shortest edge, bicubic, (H' - h) // 2 crop, rescale, normalise"""
    return (resize_crop(to_rgb_array(img), size, (size, size), "bicubic", "transformers"),) + affine(CLIP_MEAN, CLIP_STD, 1 / 255)


def vae_ref(img, size=512, filt="bilinear", out_range=(-1, 1)):
    """Resize((size, size)), ToTensor, then the VAE's range"""
    return (resize_crop(to_rgb_array(img), (size, size), None, filt, "torchvision"),) + range_affine(*out_range)


def hf_clip_image_processor(imgs, size=224):
    """transformers' CLIPImageProcessor itself (its PIL backend where torchvision is absent) at `size`: fp32 (B, 3, size, size)"""
    import logging
    logging.getLogger("transformers").setLevel(logging.ERROR)
    from transformers import CLIPImageProcessor
    proc = CLIPImageProcessor(size={"shortest_edge": size}, crop_size={"height": size, "width": size})
    return np.asarray(proc([im.convert("RGB") for im in imgs], return_tensors="np")["pixel_values"], np.float32)
