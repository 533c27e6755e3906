"""Image files' pixels -> the `pixel_values` every image consumer here takes, on the GPU and bit for bit what PIL gives: csrc/image_resize.hip resamples with
PIL's own 8-bit fixed-point arithmetic (antialiased bicubic / bilinear), keeps a centred crop window and applies the per-channel normalisation, in one launch
per group of equally sized images.  It is the one operation behind four preprocessors of the reference:

* open_clip_preprocess   open_clip's transform in front of the ViT-H/14 image tower (Retrieval/eegdatasets_leaveone.py:62-74, :108-135: Resize(224, BICUBIC),
                         CenterCrop(224), ToTensor, Normalize) -- what datasets.image_features_from_files / build_feature_cache feed the tower;
* clip_image_processor   transformers' CLIPImageProcessor with its defaults (the pipeline's feature_extractor in front of the IP-Adapter's image encoder,
                         Generation/custom_pipeline.py:365-373, and GIT's processor): shortest edge 224 bicubic, centre crop, rescale, normalise;
* alexnet_preprocess     the metrics notebooks' transform in front of AlexNet (Generation/..._metrics_sub8.ipynb: Resize(256, BILINEAR), Normalize with ImageNet's
                         mean / std), what metric_nets.AlexNetFeatures takes;
* vae_preprocess         the low-level script's Resize((512, 512)) + ToTensor in front of vae.encode (Generation/train_vae_latent_512_low_level_no_average.py),
                         bilinear (torchvision's default), to the range the VAE takes (diffusers' VaeImageProcessor.normalize: 2 x - 1).

On the host stay: decoding the files (PIL), .convert("RGB"), stacking equally sized images, the size / crop arithmetic and the coefficient tables (PIL's
precompute_coeffs in double, eegclip_resize_coeffs; cached per (in, out, window, filter) on the device).  No torch arithmetic touches a pixel, and there is no
CPU path: CPU tensors without the library raise as everywhere else.  `lib`, `require_cuda` and `raw_stream` are called as this module's globals
(tests/emu_patch.py swaps them).
"""
import ctypes

import numpy as np
import torch

from . import _abi
from ._lib import EegclipError, check, lib, raw_stream, require_cuda
from .clip_vision import CLIP_MEAN, CLIP_STD

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILTERS = {"bicubic": _abi.RESIZE_BICUBIC, "bilinear": _abi.RESIZE_BILINEAR}
_OUT_CODES = {torch.float32: _abi.DT_F32, torch.float16: _abi.DT_F16, torch.bfloat16: _abi.DT_BF16}
_tables = {}           # (in_size, out_size, first, count, filter, device) -> (bounds, coeffs, ksize) on the device
_affines = {}          # (scale values, shift values, device) -> (scale, shift) fp32 (3) on the device


def resized_size(H, W, size):
    """int: the shortest side becomes `size`, the long one int(size * long / short) (torchvision.transforms.Resize and transformers'
    get_resize_output_image_size compute the same); (h, w): as given"""
    if isinstance(size, (tuple, list)):
        if len(size) != 2:
            raise EegclipError(f"size must be an int or (h, w); got {size!r}")
        rh, rw = int(size[0]), int(size[1])
    else:
        size = int(size)
        short, long = (H, W) if H <= W else (W, H)
        new_long = int(size * long / short)
        rh, rw = (size, new_long) if H <= W else (new_long, size)
    if rh < 1 or rw < 1:
        raise EegclipError(f"size {size!r} gives an empty image")
    return rh, rw


def crop_origin(rh, rw, h, w, crop_rounding="torchvision"):
    """top-left of the centred (h, w) window of a (rh, rw) image: torchvision's CenterCrop int(round((rh - h) / 2.0)) (Python's round) or transformers'
    center_crop (rh - h) // 2"""
    if crop_rounding not in ("torchvision", "transformers"):
        raise EegclipError(f"crop_rounding must be 'torchvision' or 'transformers'; got {crop_rounding!r}")
    if h < 1 or w < 1 or h > rh or w > rw:
        raise EegclipError(f"crop ({h}, {w}) does not fit the resized image ({rh}, {rw}) (padding is not offered)")
    if crop_rounding == "torchvision":
        return int(round((rh - h) / 2.0)), int(round((rw - w) / 2.0))
    return (rh - h) // 2, (rw - w) // 2


def _table(in_size, out_size, first, count, filt, device):
    key = (in_size, out_size, first, count, filt, str(device))
    hit = _tables.get(key)
    if hit is None:
        L = lib()
        ks = L.eegclip_resize_coeffs(in_size, out_size, 0, 0, filt, None, None, 0)
        if ks < 1:
            raise EegclipError(f"resize_coeffs({in_size} -> {out_size}) failed with code {ks}")
        b, k = np.zeros((count, 2), np.int32), np.zeros((count, ks), np.int32)
        rc = L.eegclip_resize_coeffs(in_size, out_size, first, count, filt, b.ctypes.data_as(ctypes.c_void_p), k.ctypes.data_as(ctypes.c_void_p), ks)
        if rc != ks:
            raise EegclipError(f"resize_coeffs({in_size} -> {out_size}, rows {first} .. {first + count - 1}) failed with code {rc}")
        if len(_tables) >= 256:                                   # (a data set of many image sizes: the tables are cheap to rebuild)
            _tables.clear()
        hit = _tables[key] = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device), ks)
    return hit


def _affine(scale, shift, device):
    if scale is None:
        return None, None
    key = (tuple(float(v) for v in scale), tuple(float(v) for v in shift), str(device))
    hit = _affines.get(key)
    if hit is None:
        if len(_affines) >= 64:
            _affines.clear()
        hit = _affines[key] = (torch.from_numpy(np.asarray(scale, np.float32)).to(device), torch.from_numpy(np.asarray(shift, np.float32)).to(device))
    return hit


def _is_pil(x):
    return hasattr(x, "convert") and hasattr(x, "mode") and hasattr(x, "size")


def _one_u8(x):
    """one image -> uint8 (H, W, 3): a host array or a tensor where it lives"""
    if _is_pil(x):
        return np.asarray(x.convert("RGB"))
    if isinstance(x, np.ndarray) and x.dtype == np.uint8 and x.ndim == 3 and x.shape[2] == 3:
        return x
    if isinstance(x, torch.Tensor) and x.dtype == torch.uint8 and x.dim() == 3 and x.shape[2] == 3:
        return x
    raise EegclipError(f"an image is a PIL image or a uint8 (H, W, 3) array / tensor; got {type(x).__name__}"
                       + (f" {tuple(x.shape)} {x.dtype}" if hasattr(x, "shape") else ""))


def _groups(images, device):
    """images -> (number of images, [(positions, batch on the device, source kind)]): one batch per image size, positions in input order"""
    if isinstance(images, torch.Tensor) and images.is_floating_point():
        if images.dim() != 4 or images.shape[1] != 3 or images.numel() == 0 or images.dtype not in _OUT_CODES:
            raise EegclipError(f"a float image batch is (B, 3, H, W) in fp32, fp16 or bf16; got {tuple(images.shape)} {images.dtype}")
        return images.shape[0], [(None, images.to(device).contiguous(), _OUT_CODES[images.dtype])]
    if isinstance(images, (np.ndarray, torch.Tensor)) and images.ndim == 4:
        u8 = images.dtype == (torch.uint8 if isinstance(images, torch.Tensor) else np.uint8)
        if not u8 or images.shape[3] != 3 or images.shape[0] == 0:
            raise EegclipError(f"a uint8 image batch is (B, H, W, 3); got {tuple(images.shape)} {images.dtype}")
        t = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
        return t.shape[0], [(None, t.to(device).contiguous(), _abi.SRC_U8_HWC)]
    items = [_one_u8(x) for x in (images if isinstance(images, (list, tuple)) else [images])]
    if not items:
        raise EegclipError("no image given")
    by_size = {}
    for i, a in enumerate(items):
        by_size.setdefault((int(a.shape[0]), int(a.shape[1])), []).append(i)
    out = []
    for idx in by_size.values():
        part = [items[i] for i in idx]
        if all(isinstance(a, np.ndarray) for a in part):
            batch = torch.from_numpy(np.stack(part)).to(device)                                  # one upload per size
        else:
            batch = torch.stack([(a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(device) for a in part])
        out.append((idx if len(by_size) > 1 else None, batch.contiguous(), _abi.SRC_U8_HWC))
    return len(items), out


def _run(images, size, crop, filter, scale, shift, dtype, device, crop_rounding, in_range):
    if filter not in FILTERS:
        raise EegclipError(f"filter must be one of {sorted(FILTERS)}; got {filter!r}")
    if dtype not in _OUT_CODES:
        raise EegclipError(f"dtype must be fp32, fp16 or bf16; got {dtype!r}")
    if device is None:
        device = images.device if isinstance(images, torch.Tensor) and images.device.type != "cpu" else "cuda"
    device = torch.device(device)
    n, groups = _groups(images, device)
    a = b = 0.0
    if groups[0][2] != _abi.SRC_U8_HWC:
        if in_range is None or len(in_range) != 2 or not float(in_range[1]) > float(in_range[0]):
            raise EegclipError("a float image batch needs in_range=(lo, hi), the values that stand for black and white ((-1, 1) for a VAE decode, (0, 1))")
        lo, hi = float(in_range[0]), float(in_range[1])
        a, b = 1.0 / (hi - lo), -lo / (hi - lo)
    elif in_range is not None:
        raise EegclipError("in_range goes with a float image batch; uint8 pixels are 0..255")
    sc, sh = _affine(scale, shift, device)
    filt, L, result = FILTERS[filter], lib(), None
    for idx, batch, kind in groups:
        require_cuda(batch, "images")
        B = batch.shape[0]
        H, W = (batch.shape[1], batch.shape[2]) if kind == _abi.SRC_U8_HWC else (batch.shape[2], batch.shape[3])
        rh, rw = resized_size(H, W, size)
        ch, cw = (rh, rw) if crop is None else (int(crop[0]), int(crop[1]))
        top, left = (0, 0) if crop is None else crop_origin(rh, rw, ch, cw, crop_rounding)
        hb, hk, kh = _table(W, rw, left, cw, filt, device)
        vb, vk, kv = _table(H, rh, top, ch, filt, device)
        if result is None:
            result = torch.empty(n, 3, ch, cw, dtype=dtype, device=device)
        elif tuple(result.shape[2:]) != (ch, cw):
            raise EegclipError(f"images of different sizes give outputs of different sizes ({tuple(result.shape[2:])}, {(ch, cw)}): give a crop, or size=(h, w)")
        out = result if idx is None else torch.empty(B, 3, ch, cw, dtype=dtype, device=device)
        for b0 in range(0, B, 32768):                                 # (the image index is a grid dimension)
            nb = min(32768, B - b0)
            check(L.eegclip_resize_crop_normalize(batch[b0:b0 + nb].data_ptr(), kind, a, b, nb, H, W, rh, rw, top, left, ch, cw, filt, hb.data_ptr(), hk.data_ptr(),
                                                  kh, vb.data_ptr(), vk.data_ptr(), kv, sc.data_ptr() if sc is not None else None,
                                                  sh.data_ptr() if sh is not None else None, out[b0:b0 + nb].data_ptr(), _OUT_CODES[dtype], raw_stream()),
                  f"resize_crop_normalize ({H} x {W} -> {rh} x {rw}, window {ch} x {cw})")
        if idx is not None:
            result[torch.as_tensor(idx, device=device)] = out          # (a copy into the rows of the input order)
    return result


def resize_crop_normalize(images, size, crop=None, filter="bicubic", mean=None, std=None, rescale=1 / 255, dtype=torch.float32, device=None,
                          crop_rounding="torchvision", in_range=None):
    """PIL's Image.resize (8-bit, antialiased `filter`: "bicubic" or "bilinear"), a centred crop and (q * rescale - mean[c]) / std[c], on the GPU -> (B, 3, ch, cw)
    of `dtype` on `device` (default: a device tensor's own, else "cuda"), rows in input order.

    images: one or a list of PIL images (any mode: taken through .convert("RGB")) or uint8 (H, W, 3) arrays / tensors, a uint8 (B, H, W, 3) array / tensor on
    the host or the device, or a float (B, 3, H, W) tensor with in_range=(lo, hi) -- lo is black, hi white; it is quantised to 8 bits on load as diffusers'
    postprocess(output_type="pil") does, so a VAE decode gets the bytes the reference's PIL round trip would give it.  Images of different sizes are grouped
    by size, one launch per group.  size: an int (the shortest side -> size, the long one int(size * long / short)) or (h, w).  crop: (h, w), centred as
    crop_rounding says ("torchvision": int(round((H' - h) / 2.0)); "transformers": (H' - h) // 2); larger than the resized image raises.
    mean / std / rescale: each None is the identity; all three None give the integers 0..255 themselves."""
    scale = shift = None
    if mean is not None or std is not None or rescale is not None:
        m = np.asarray([0.0] * 3 if mean is None else [float(v) for v in mean], np.float64)
        s = np.asarray([1.0] * 3 if std is None else [float(v) for v in std], np.float64)
        if m.size != 3 or s.size != 3 or (s == 0).any():
            raise EegclipError("mean and std take three values, std non-zero")
        scale, shift = ((1.0 if rescale is None else float(rescale)) / s).astype(np.float32), (-m / s).astype(np.float32)
    return _run(images, size, crop, filter, scale, shift, dtype, device, crop_rounding, in_range)


def open_clip_preprocess(images, size=224, **kw):
    """open_clip's deterministic transform of ViT-H-14 (the reference's ImageEncoder input, eegdatasets_leaveone.py:108-135): Resize(size, BICUBIC),
    CenterCrop(size), ToTensor, Normalize(CLIP mean / std)"""
    return resize_crop_normalize(images, size, (size, size), "bicubic", CLIP_MEAN, CLIP_STD, 1 / 255, crop_rounding="torchvision", **kw)


def clip_image_processor(images, size=224, **kw):
    """transformers' CLIPImageProcessor with its defaults (the IP-Adapter's feature_extractor, GIT's processor): shortest edge `size` bicubic, centre crop
    (size, size), rescale 1 / 255, normalise with CLIP's mean / std"""
    return resize_crop_normalize(images, size, (size, size), "bicubic", CLIP_MEAN, CLIP_STD, 1 / 255, crop_rounding="transformers", **kw)


def alexnet_preprocess(images, size=256, **kw):
    """the metrics notebooks' transform in front of AlexNet: Resize(size, BILINEAR) -- the shortest side becomes `size`, no crop -- and Normalize with
    ImageNet's mean / std.  The notebooks resize float tensors; this is PIL's 8-bit antialiased resize (what Resize does to a PIL image), so the values can
    differ from the notebooks' in the last digits, as for metrics.pixcorr_ssim.  A float (B, 3, H, W) batch needs in_range (resize_crop_normalize)."""
    return resize_crop_normalize(images, size, None, "bilinear", IMAGENET_MEAN, IMAGENET_STD, 1 / 255, **kw)


def swav_preprocess(images, size=224, **kw):
    """the metrics notebooks' transform in front of the SwAV ResNet-50: Resize(size, BILINEAR) -- the shortest side becomes `size`, no crop -- and Normalize
    with ImageNet's mean / std: alexnet_preprocess at the SwAV row's size, with the same note on PIL's 8-bit resize"""
    return alexnet_preprocess(images, size=size, **kw)


def vae_preprocess(images, size=512, filter="bilinear", out_range=(-1, 1), **kw):
    """the low-level script's Resize((size, size)) + ToTensor in front of vae.encode, to out_range: q / 255 * (hi - lo) + lo.  The default (-1, 1) is the range
    diffusers' AutoencoderKL is trained on (VaeImageProcessor.normalize); out_range=(0, 1) is ToTensor alone."""
    lo, hi = float(out_range[0]), float(out_range[1])
    scale, shift = np.full(3, (hi - lo) / 255.0, np.float64).astype(np.float32), np.full(3, lo, np.float64).astype(np.float32)
    return _run(images, (size, size), None, filter, scale, shift, kw.pop("dtype", torch.float32), kw.pop("device", None), "torchvision", kw.pop("in_range", None), **kw)


def effnet_preprocess(images, size=255, **kw):
    """the metrics notebooks' transform in front of EfficientNet-B1: Resize(255, BILINEAR) -- the shortest side becomes `size`, no crop -- and Normalize with
    ImageNet's mean / std: alexnet_preprocess at the EffNet-B row's size, with the same note on PIL's 8-bit resize"""
    return alexnet_preprocess(images, size=size, **kw)


def inception_preprocess(images, size=342, **kw):
    """the metrics notebooks' transform in front of InceptionV3: Resize(342, BILINEAR) -- the shortest side becomes `size`, no crop -- and Normalize with
    ImageNet's mean / std: alexnet_preprocess at the Inception row's size, with the same note on PIL's 8-bit resize.  (torchvision's transform_input, which
    undoes this normalisation in favour of (x - 0.5) / 0.5, is part of the net: metric_nets.InceptionFeatures.)"""
    return alexnet_preprocess(images, size=size, **kw)
