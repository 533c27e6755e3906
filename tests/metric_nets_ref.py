"""fp64 restatement of torchvision's AlexNet up to `features.11` from torch.nn.functional.conv2d / relu / max_pool2d on the CPU (torchvision/models/alexnet.py;
torchvision itself is not a dependency), the oracle of tests/test_kernels_metric_nets.py, tests/test_metric_nets_emu.py and tests/test_metric_nets_gpu.py:

  features(x, sd)            {"features.4", "features.11"} in fp64 from a state dict with the ten keys features.{0,3,6,8,10}.{weight,bias}
  yardstick(x, sd, dtype)    the same chain in fp32 with the input, the weights, the biases and EVERY layer's output rounded to `dtype`: what any 16-bit
                             implementation of the net pays against features()
  conv_relu / conv_abs       one layer in fp64, and |x| (*) |w| = sum |x| |w| (the scale of its fp32 accumulation error)
  bits / values              16-bit patterns <-> fp64 values of either dtype; frame / first_frame / pack_weight: the layouts of include/eegclip.h
"""
import numpy as np
import torch
import torch.nn.functional as F

# (index in `features`, Cin, Cout, kernel, stride, padding)
LAYERS = [("0", 3, 64, 11, 4, 2), ("3", 64, 192, 5, 1, 2), ("6", 192, 384, 3, 1, 1), ("8", 384, 256, 3, 1, 1), ("10", 256, 256, 3, 1, 1)]
POOL_AFTER = ("0", "3")                       # MaxPool2d(3, 2) follows the ReLUs of features.0 and features.3 (features.12, the third, is never run)
NODE_AFTER = {"3": "features.4", "10": "features.11"}
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}          # half an ulp, relative: one rounding to nearest


def _chain(x, sd, rnd):
    out = {}
    x = rnd(x)
    for i, _, _, _, s, p in LAYERS:
        x = rnd(F.relu(F.conv2d(x, rnd(sd[f"features.{i}.weight"].to(x.dtype)), rnd(sd[f"features.{i}.bias"].to(x.dtype)), stride=s, padding=p)))
        if i in NODE_AFTER:
            out[NODE_AFTER[i]] = x
        if i in POOL_AFTER:
            x = F.max_pool2d(x, 3, 2)
    return out


def features(x, sd):
    return _chain(x.detach().cpu().double(), {k: v.detach().cpu().double() for k, v in sd.items()}, lambda t: t)


def yardstick(x, sd, dtype):
    return _chain(x.detach().cpu().float(), {k: v.detach().cpu().float() for k, v in sd.items()}, lambda t: t.to(dtype).float())


def rel_l2(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return float((a - ref).norm() / ref.norm())


def conv_relu(x, w, b, stride, pad):
    return F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad))


def conv_abs(x, w, stride, pad):
    return F.conv2d(x.double().abs(), w.double().abs(), None, stride=stride, padding=pad)


# ---- 16-bit patterns and the frames of include/eegclip.h ----
def bits(t, dtype):
    """values exact in `dtype` -> uint16 numpy array of their patterns"""
    return t.to(dtype).contiguous().view(torch.int16).numpy().view(np.uint16)


def values(u, dtype):
    """uint16 patterns -> fp64 tensor"""
    return torch.from_numpy(np.ascontiguousarray(u).view(np.int16)).view(dtype).double()


def exact(t, dtype):
    """round to `dtype`, returned in fp64: operands that are exact in the dtype"""
    return t.to(dtype).double()


def frame(x, pad, dtype):
    """(N, C, H, W) -> zero-bordered NHWC patterns (N, H + 2 pad, W + 2 pad, C)"""
    N, C, H, W = x.shape
    f = np.zeros((N, H + 2 * pad, W + 2 * pad, C), np.uint16)
    f[:, pad:pad + H, pad:pad + W, :] = bits(x.permute(0, 2, 3, 1), dtype)
    return f


def unframe(f, pad, dtype):
    """frame patterns -> (N, C, H, W) fp64 of the interior"""
    inner = f[:, pad:f.shape[1] - pad, pad:f.shape[2] - pad, :] if pad else f
    return values(inner, dtype).permute(0, 3, 1, 2)


def border_is_zero(f, pad):
    if not pad:
        return True
    return not (f[:, :pad].any() or f[:, -pad:].any() or f[:, :, :pad].any() or f[:, :, -pad:].any())


def first_frame(x, width, dtype):
    """(N, 3, H, W) -> the 3-channel layer's frame (N, H + 4, width, 4): pixel (y, x) at (y + 2, x + 2) as {c0, c1, c2, 0}"""
    N, _, H, W = x.shape
    f = np.zeros((N, H + 4, width, 4), np.uint16)
    f[:, 2:2 + H, 2:2 + W, :3] = bits(x.permute(0, 2, 3, 1), dtype)
    return f


def pack_weight(w, dtype):
    """(Cout, Cin, KS, KS) -> [Cout][KS * KS * Cin] in (ky, kx, ci) order; for Cin = 3, [Cout][KS][64] with element 4 kx + ci"""
    Cout, Cin, KS, _ = w.shape
    p = w.permute(0, 2, 3, 1)
    if Cin != 3:
        return bits(p.reshape(Cout, -1), dtype)
    q = torch.zeros(Cout, KS, 16, 4, dtype=w.dtype)
    q[:, :, :KS, :3] = p
    return bits(q.reshape(Cout, -1), dtype)


# ---- the inputs the network tests share ----
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def normalised_images(n, H, W):
    """recon_metrics_ref.smooth_pair(s, H, W)'s smooth images, s = 0 .. n - 1, through Normalize(ImageNet mean / std): (n, 3, H, W) fp32"""
    import recon_metrics_ref as R
    x = torch.from_numpy(np.stack([R.smooth_pair(s, H, W)[0] for s in range(n)]))
    return (x - torch.tensor(MEAN)[None, :, None, None]) / torch.tensor(STD)[None, :, None, None]


def mixed_pairs(n, H, W, noise=0.1):
    """-> (images, recons), (n, 3, H, W) fp32 in [0, 1]: smooth_pair(s, H, W, noise)'s image and its noisy version; for odd j the reconstruction is
    clip(0.5 own noisy + 0.5 next noisy, 0, 1) (the next of the last is the first), so some reconstructions sit between two images"""
    import recon_metrics_ref as R
    pairs = [R.smooth_pair(s, H, W, noise=noise) for s in range(n)]
    a = np.stack([p[0] for p in pairs])
    b = np.stack([p[1] for p in pairs])
    r = b.copy()
    for j in range(1, n, 2):
        r[j] = np.clip(0.5 * b[j] + 0.5 * b[(j + 1) % n], 0.0, 1.0)
    return torch.from_numpy(a), torch.from_numpy(r)
