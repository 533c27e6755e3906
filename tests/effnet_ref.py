"""fp64 restatement of torchvision's EfficientNet (B0 / B1 widths) up to `avgpool`, from torch.nn.functional.conv2d(groups=), eval-mode BatchNorm written out,
x sigmoid(x), mean((2, 3)) and the squeeze-and-excitation formula on the CPU (torchvision/models/efficientnet.py; torchvision itself is not a dependency): the
oracle of tests/test_kernels_mbconv.py, tests/test_effnet_emu.py and tests/test_metric_effnet_gpu.py.

  features(x, sd, layers)           ((N, 1280) fp64 `avgpool`, the largest |activation| of any launch's output) from a state dict in torchvision's keys
  yardstick(x, sd, layers, dtype)   the same chain in fp32 with the input, the convolution weights and EVERY launch's output -- stem, expansion, depthwise, gate
                                    multiply, projection (+ residual), head -- rounded to `dtype`; scale and shift, the pooled mean and the gate stay fp32, the
                                    squeeze's 16-bit weights and biases are rounded, and `avgpool` is not: what any 16-bit implementation of the net pays
  block_keys(sd, prefix)            the sub-keys of one MBConv block (with or without an expansion)
  dw_pre / dw_abs / se_gate / conv_bn_act       one launch in fp64, for the kernel tests; dw_weight / stem_frame: the layouts of include/eegclip.h
"""
import numpy as np
import torch
import torch.nn.functional as F

import metric_nets_ref as MR
from resnet_ref import correlation  # noqa: F401  (scipy's correlation distance per pair of rows, fp64: the two "distance" rows share it)

# (expand ratio, kernel, stride, input channels, output channels) of features.1 .. features.7
STAGES = ((1, 3, 1, 32, 16), (6, 3, 2, 16, 24), (6, 5, 2, 24, 40), (6, 3, 2, 40, 80), (6, 5, 1, 80, 112), (6, 5, 2, 112, 192), (6, 3, 1, 192, 320))
B1_LAYERS = (2, 3, 3, 4, 4, 5, 2)
EPS = 1e-5
UNIT = MR.UNIT


def silu(z):
    return z * torch.sigmoid(z)


def scale_shift(sd, bn, ftype):
    g, b, m, v = (sd[f"{bn}.{k}"].to(ftype) for k in ("weight", "bias", "running_mean", "running_var"))
    scale = g / torch.sqrt(v + EPS)
    return scale, b - m * scale


def block_keys(sd, prefix):
    """-> (expansion or None, depthwise, squeeze-and-excitation, projection) key prefixes of the block `prefix`"""
    if f"{prefix}.block.3.0.weight" in sd:
        return tuple(f"{prefix}.block.{j}" for j in range(4))
    return (None,) + tuple(f"{prefix}.block.{j}" for j in range(3))


def _chain(x, sd, layers, rnd, ftype):
    peak = [0.0]

    def launch(x, key, stride, act, residual=None):
        w = rnd(sd[f"{key}.0.weight"].to(ftype))
        z = F.conv2d(x, w, None, stride=stride, padding=w.shape[2] // 2, groups=x.shape[1] // w.shape[1])
        scale, shift = scale_shift(sd, f"{key}.1", ftype)
        z = z * scale[None, :, None, None] + shift[None, :, None, None]
        if act:
            z = silu(z)
        if residual is not None:
            z = z + residual
        z = rnd(z)
        peak[0] = max(peak[0], float(z.abs().max()))
        return z

    x = launch(rnd(x), "features.0", 2, True)
    for s, ((expand, k, stride, cin, cout), n) in enumerate(zip(STAGES, layers)):
        for i in range(n):
            ex, dw, se, pr = block_keys(sd, f"features.{s + 1}.{i}")
            assert (ex is None) == (expand == 1)
            y = launch(x, ex, 1, True) if ex else x
            y = launch(y, dw, stride if i == 0 else 1, True)
            gate = se_gate(y.mean((2, 3)), *(rnd(sd[f"{se}.{p}"].to(ftype)) for p in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")))
            y = rnd(y * gate[:, :, None, None])
            peak[0] = max(peak[0], float(y.abs().max()))
            x = launch(y, pr, 1, False, residual=x if (i > 0 or (stride == 1 and cin == cout)) else None)
    x = launch(x, "features.8", 1, True)
    return x.mean((2, 3)), peak[0]


def _cpu(sd, ftype):
    return {k: v.detach().cpu().to(ftype) for k, v in sd.items() if v.is_floating_point()}


def features(x, sd, layers=B1_LAYERS):
    return _chain(x.detach().cpu().double(), _cpu(sd, torch.float64), layers, lambda t: t, torch.float64)


def yardstick(x, sd, layers, dtype):
    return _chain(x.detach().cpu().float(), _cpu(sd, torch.float32), layers, lambda t: t.to(dtype).float(), torch.float32)[0]


# ---- one launch, for the kernel tests ----
def se_gate(mean, w1, b1, w2, b2):
    """mean (N, C), fc1 (sq, C[, 1, 1]), fc2 (C, sq[, 1, 1]) -> sigmoid(W2 silu(W1 mean + b1) + b2), in the operands' dtype"""
    w1, w2 = w1.reshape(w1.shape[0], -1), w2.reshape(w2.shape[0], -1)
    return torch.sigmoid(silu(mean @ w1.t() + b1) @ w2.t() + b2)


def dw_pre(x, w, scale, shift, stride):
    """the depthwise convolution and BatchNorm in fp64, before SiLU: x (N, C, H, W), w (C, 1, k, k)"""
    z = F.conv2d(x.double(), w.double(), None, stride=stride, padding=w.shape[2] // 2, groups=x.shape[1])
    return z * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]


def dw_abs(x, w, stride):
    return F.conv2d(x.double().abs(), w.double().abs(), None, stride=stride, padding=w.shape[2] // 2, groups=x.shape[1])


def conv_bn_act(x, w, scale, shift, stride, pad, act, residual=None):
    """act(scale conv + shift) + residual in fp64; act: 0 none, 1 ReLU, 2 SiLU -> (result, the pre-activation)"""
    pre = F.conv2d(x.double(), w.double(), None, stride=stride, padding=pad) * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    z = silu(pre) if act == 2 else F.relu(pre) if act == 1 else pre
    return (z + residual.double() if residual is not None else z), pre


def dw_weight(w, dtype):
    """(C, 1, k, k) -> patterns [ky][kx][C]"""
    return MR.bits(w[:, 0].permute(1, 2, 0), dtype)


def stem_frame(x, width, dtype):
    """(N, 3, H, W) -> the stem's frame (N, H + 2, width, 4): pixel (y, x) at (y + 1, x + 1) as {c0, c1, c2, 0}"""
    N, _, H, W = x.shape
    f = np.zeros((N, H + 2, width, 4), np.uint16)
    f[:, 1:1 + H, 1:1 + W, :3] = MR.bits(x.permute(0, 2, 3, 1), dtype)
    return f
