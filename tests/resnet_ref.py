"""fp64 restatement of torchvision's ResNet with Bottleneck blocks (v1.5: the stride on conv2) up to `avgpool`, from torch.nn.functional.conv2d, eval-mode
BatchNorm written out, max_pool2d(3, 2, 1), add, relu and mean((2, 3)) on the CPU (torchvision/models/resnet.py; torchvision itself is not a dependency): the
oracle of tests/test_kernels_resnet.py, tests/test_resnet_emu.py and tests/test_resnet_gpu.py.

  features(x, sd, layers)           ((N, 2048) fp64 `avgpool`, the largest |activation| of any launch's output) from a state dict in torchvision's keys
  yardstick(x, sd, layers, dtype)   the same chain in fp32 with the input, the convolution weights and EVERY launch's output -- conv -> BatchNorm (-> + residual)
                                    (-> ReLU) -- rounded to `dtype`; scale and shift stay fp32 and `avgpool` is not rounded: what any 16-bit
                                    implementation of the net pays against features()
  correlation(a, b)                 scipy.spatial.distance.correlation of every pair of rows, fp64
  conv_bn / conv_abs                one launch in fp64, and |x| (*) |w|; stem_frame / stem_weight: the stem's layouts of include/eegclip.h
"""
import numpy as np
import torch
import torch.nn.functional as F

import metric_nets_ref as MR

WIDTHS = (64, 128, 256, 512)
EPS = 1e-5
UNIT = MR.UNIT


def scale_shift(sd, bn, dtype):
    """eval-mode BatchNorm as y = scale z + shift, computed in `dtype` from the state dict's tensors"""
    g, b, m, v = (sd[f"{bn}.{k}"].to(dtype) for k in ("weight", "bias", "running_mean", "running_var"))
    scale = g / torch.sqrt(v + EPS)
    return scale, b - m * scale


def _chain(x, sd, layers, rnd, ftype):
    peak = [0.0]

    def launch(x, conv, bn, stride, pad, relu=True, residual=None):
        z = F.conv2d(x, rnd(sd[f"{conv}.weight"].to(ftype)), None, stride=stride, padding=pad)
        scale, shift = scale_shift(sd, bn, ftype)
        z = z * scale[None, :, None, None] + shift[None, :, None, None]
        if residual is not None:
            z = z + residual
        z = rnd(F.relu(z) if relu else z)
        peak[0] = max(peak[0], float(z.abs().max()))
        return z

    x = launch(rnd(x), "conv1", "bn1", 2, 3)
    x = F.max_pool2d(x, 3, 2, 1)
    for s, n in enumerate(layers):
        for i in range(n):
            p, stride = f"layer{s + 1}.{i}", 2 if s > 0 and i == 0 else 1
            y = launch(x, f"{p}.conv1", f"{p}.bn1", 1, 0)
            y = launch(y, f"{p}.conv2", f"{p}.bn2", stride, 1)
            res = launch(x, f"{p}.downsample.0", f"{p}.downsample.1", stride, 0, relu=False) if i == 0 else x
            x = launch(y, f"{p}.conv3", f"{p}.bn3", 1, 0, residual=res)
    return x.mean((2, 3)), peak[0]


def _cpu(sd, ftype):
    return {k: v.detach().cpu().to(ftype) for k, v in sd.items() if v.is_floating_point()}


def features(x, sd, layers=(3, 4, 6, 3)):
    return _chain(x.detach().cpu().double(), _cpu(sd, torch.float64), layers, lambda t: t, torch.float64)


def yardstick(x, sd, layers, dtype):
    return _chain(x.detach().cpu().float(), _cpu(sd, torch.float32), layers, lambda t: t.to(dtype).float(), torch.float32)[0]


def correlation(a, b):
    """scipy's correlation distance of row i of a and row i of b, in fp64 -> numpy (N,)"""
    from scipy.spatial.distance import correlation as dist
    a, b = (np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, np.float64) for t in (a, b))
    return np.array([dist(a[i], b[i]) for i in range(a.shape[0])])


# ---- one launch, for the kernel tests ----
def conv_bn(x, w, scale, shift, stride, pad, residual=None, relu=True):
    z = F.conv2d(x.double(), w.double(), None, stride=stride, padding=pad) * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    if residual is not None:
        z = z + residual.double()
    return F.relu(z) if relu else z


conv_abs = MR.conv_abs


def stem_frame(x, width, dtype):
    """(N, 3, H, W) -> the stem's frame (N, H + 6, width, 4): pixel (y, x) at (y + 3, x + 3) as {c0, c1, c2, 0}"""
    N, _, H, W = x.shape
    f = np.zeros((N, H + 6, width, 4), np.uint16)
    f[:, 3:3 + H, 3:3 + W, :3] = MR.bits(x.permute(0, 2, 3, 1), dtype)
    return f
