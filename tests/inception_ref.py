"""fp64 restatement of torchvision's Inception3 up to `avgpool` (torchvision/models/inception.py; torchvision itself is not a dependency, so the net is
written out from its layer table), from torch.nn.functional.conv2d, eval-mode BatchNorm(eps = 0.001) written out, relu, avg_pool2d(3, 1, 1), max_pool2d(3, 2)
and torch.cat on the CPU: the oracle of tests/test_kernels_inception.py, tests/test_inception_emu.py and tests/test_metric_inception_gpu.py.

  features(x, sd, blocks, transform_input)           ((N, 2048) fp64 `avgpool`, the largest |activation| of any launch's output) from a state dict in torchvision's keys
  yardstick(x, sd, blocks, dtype, transform_input)   the same chain in fp32 with the input, the convolution weights and EVERY launch's output -- the pack with its
                                                     affine, every BasicConv2d, every 3 x 3 average pool, every max-pool -- rounded to `dtype`; scale and shift stay
                                                     fp32 and `avgpool` is not rounded: what any 16-bit implementation of the net pays
  keys(blocks)                                       name -> shape of the state dict, in torchvision's order; PARAMS, CONVS: the counts at full depth
  conv_bn / conv_abs                                 one launch in fp64, for the kernel tests; stem_frame: the first layer's frame of include/eegclip.h
"""
import numpy as np
import torch
import torch.nn.functional as F

import metric_nets_ref as MR

EPS = 1e-3
UNIT = MR.UNIT
FULL = (3, 4, 2)
PARAMS, CONVS = 21785568, 94                    # torchvision's 27,161,264 less fc (2,049,000) and AuxLogits (3,326,696)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
A_NAMES, A_POOL = ("Mixed_5b", "Mixed_5c", "Mixed_5d"), (32, 64, 64)
C_NAMES, C_MID = ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"), (128, 160, 160, 192)
E_NAMES = ("Mixed_7b", "Mixed_7c")

# (name, in, out, (KH, KW), stride, (pad_h, pad_w))
STEM = (("Conv2d_1a_3x3", 3, 32, (3, 3), 2, (0, 0)), ("Conv2d_2a_3x3", 32, 32, (3, 3), 1, (0, 0)), ("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1)),
        ("Conv2d_3b_1x1", 64, 80, (1, 1), 1, (0, 0)), ("Conv2d_4a_3x3", 80, 192, (3, 3), 1, (0, 0)))


def block_a(cin, pf):
    return [("branch1x1", cin, 64, (1, 1), 1, (0, 0)), ("branch5x5_1", cin, 48, (1, 1), 1, (0, 0)), ("branch5x5_2", 48, 64, (5, 5), 1, (2, 2)),
            ("branch3x3dbl_1", cin, 64, (1, 1), 1, (0, 0)), ("branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)), ("branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1)),
            ("branch_pool", cin, pf, (1, 1), 1, (0, 0))]


def block_b(cin):
    return [("branch3x3", cin, 384, (3, 3), 2, (0, 0)), ("branch3x3dbl_1", cin, 64, (1, 1), 1, (0, 0)), ("branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)),
            ("branch3x3dbl_3", 96, 96, (3, 3), 2, (0, 0))]


def block_c(cin, c7):
    return [("branch1x1", cin, 192, (1, 1), 1, (0, 0)), ("branch7x7_1", cin, c7, (1, 1), 1, (0, 0)), ("branch7x7_2", c7, c7, (1, 7), 1, (0, 3)),
            ("branch7x7_3", c7, 192, (7, 1), 1, (3, 0)), ("branch7x7dbl_1", cin, c7, (1, 1), 1, (0, 0)), ("branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0)),
            ("branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3)), ("branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0)), ("branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3)),
            ("branch_pool", cin, 192, (1, 1), 1, (0, 0))]


def block_d(cin):
    return [("branch3x3_1", cin, 192, (1, 1), 1, (0, 0)), ("branch3x3_2", 192, 320, (3, 3), 2, (0, 0)), ("branch7x7x3_1", cin, 192, (1, 1), 1, (0, 0)),
            ("branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)), ("branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)), ("branch7x7x3_4", 192, 192, (3, 3), 2, (0, 0))]


def block_e(cin):
    return [("branch1x1", cin, 320, (1, 1), 1, (0, 0)), ("branch3x3_1", cin, 384, (1, 1), 1, (0, 0)), ("branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)),
            ("branch3x3_2b", 384, 384, (3, 1), 1, (1, 0)), ("branch3x3dbl_1", cin, 448, (1, 1), 1, (0, 0)), ("branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1)),
            ("branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)), ("branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0)), ("branch_pool", cin, 192, (1, 1), 1, (0, 0))]


def plan(blocks=FULL):
    """[(block name, kind, [layers], output channels)] behind the stem; a block's input width is its predecessor's output width"""
    out, c = [], 192
    for i in range(blocks[0]):
        out.append((A_NAMES[i], "A", block_a(c, A_POOL[i]), 224 + A_POOL[i]))
        c = out[-1][3]
    out.append(("Mixed_6a", "B", block_b(c), 480 + c))
    c = out[-1][3]
    for i in range(blocks[1]):
        out.append((C_NAMES[i], "C", block_c(c, C_MID[i]), 768))
        c = 768
    out.append(("Mixed_7a", "D", block_d(c), 512 + c))
    c = out[-1][3]
    for i in range(blocks[2]):
        out.append((E_NAMES[i], "E", block_e(c), 2048))
        c = 2048
    return out


def layers(blocks=FULL):
    """[(key prefix, in, out, (KH, KW), stride, (pad_h, pad_w))] of every BasicConv2d, in torchvision's registration order"""
    return list(STEM) + [(f"{name}.{l[0]}", *l[1:]) for name, _, ls, _ in plan(blocks) for l in ls]


def keys(blocks=FULL):
    out = {}
    for p, cin, cout, (kh, kw), _, _ in layers(blocks):
        out[f"{p}.conv.weight"] = (cout, cin, kh, kw)
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            out[f"{p}.bn.{leaf}"] = (cout,)
        out[f"{p}.bn.num_batches_tracked"] = ()
    return out


def param_count(blocks=FULL):
    return sum(cout * cin * kh * kw + 2 * cout for _, cin, cout, (kh, kw), _, _ in layers(blocks))


def launch_count(blocks=FULL):
    return 9 + 8 * blocks[0] + 5 + 11 * blocks[1] + 7 + 10 * blocks[2]


def affine(transform_input, ftype=torch.float32):
    """torchvision's transform_input as per-channel (a, b): x_c (std_c / 0.5) + (mean_c - 0.5) / 0.5"""
    if not transform_input:
        return torch.ones(3, dtype=ftype), torch.zeros(3, dtype=ftype)
    return (torch.tensor([s / 0.5 for s in STD], dtype=torch.float64).to(ftype), torch.tensor([(m - 0.5) / 0.5 for m in MEAN], dtype=torch.float64).to(ftype))


def scale_shift(sd, bn, ftype):
    g, b, m, v = (sd[f"{bn}.{k}"].to(ftype) for k in ("weight", "bias", "running_mean", "running_var"))
    scale = g / torch.sqrt(v + EPS)
    return scale, b - m * scale


def _chain(x, sd, blocks, rnd, ftype, transform_input):
    peak = [0.0]

    def seen(z):
        z = rnd(z)
        peak[0] = max(peak[0], float(z.abs().max()))
        return z

    def conv(x, key, spec):
        _, _, _, _, stride, pad = spec
        z = F.conv2d(x, rnd(sd[f"{key}.conv.weight"].to(ftype)), None, stride=stride, padding=pad)
        scale, shift = scale_shift(sd, f"{key}.bn", ftype)
        return seen(F.relu(z * scale[None, :, None, None] + shift[None, :, None, None]))

    a, b = affine(transform_input, torch.float32)                  # (the product holds them in fp32)
    x = seen(rnd(x) * a.to(ftype)[None, :, None, None] + b.to(ftype)[None, :, None, None])
    for spec in STEM:
        x = conv(x, spec[0], spec)
        if spec[0] in ("Conv2d_2b_3x3", "Conv2d_4a_3x3"):
            x = seen(F.max_pool2d(x, 3, 2))
    for name, kind, ls, cout in plan(blocks):
        L = {l[0]: l for l in ls}
        run = lambda t, *names: [t := conv(t, f"{name}.{n}", L[n]) for n in names][-1]   # noqa: E731
        avg = lambda t: seen(F.avg_pool2d(t, 3, 1, 1))   # noqa: E731
        if kind == "A":
            parts = [run(x, "branch1x1"), run(x, "branch5x5_1", "branch5x5_2"), run(x, "branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"),
                     run(avg(x), "branch_pool")]
        elif kind == "B":
            parts = [run(x, "branch3x3"), run(x, "branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"), seen(F.max_pool2d(x, 3, 2))]
        elif kind == "C":
            parts = [run(x, "branch1x1"), run(x, "branch7x7_1", "branch7x7_2", "branch7x7_3"),
                     run(x, "branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"), run(avg(x), "branch_pool")]
        elif kind == "D":
            parts = [run(x, "branch3x3_1", "branch3x3_2"), run(x, "branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"), seen(F.max_pool2d(x, 3, 2))]
        else:
            t, u = run(x, "branch3x3_1"), run(x, "branch3x3dbl_1", "branch3x3dbl_2")
            parts = [run(x, "branch1x1"), run(t, "branch3x3_2a"), run(t, "branch3x3_2b"), run(u, "branch3x3dbl_3a"), run(u, "branch3x3dbl_3b"),
                     run(avg(x), "branch_pool")]
        x = torch.cat(parts, 1)
        assert x.shape[1] == cout, (name, x.shape[1], cout)
    return x.mean((2, 3)), peak[0]


def _cpu(sd, ftype):
    return {k: v.detach().cpu().to(ftype) for k, v in sd.items() if v.is_floating_point()}


def features(x, sd, blocks=FULL, transform_input=True):
    return _chain(x.detach().cpu().double(), _cpu(sd, torch.float64), blocks, lambda t: t, torch.float64, transform_input)


def yardstick(x, sd, blocks, dtype, transform_input=True):
    return _chain(x.detach().cpu().float(), _cpu(sd, torch.float32), blocks, lambda t: t.to(dtype).float(), torch.float32, transform_input)[0]


# ---- one launch, for the kernel tests ----
def conv_bn(x, w, scale, shift, stride, pad, relu=True):
    """relu?(scale conv + shift) in fp64, pad = (pad_h, pad_w) -> (result, the pre-activation)"""
    pre = F.conv2d(x.double(), w.double(), None, stride=stride, padding=pad) * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    return (F.relu(pre) if relu else pre), pre


def conv_abs(x, w, stride, pad):
    return F.conv2d(x.double().abs(), w.double().abs(), None, stride=stride, padding=pad)


def pack_weight(w, cout_pad, cin_pad, dtype):
    """(Cout, Cin, KH, KW) -> patterns [cout_pad][KH][KW][cin_pad], zero in the padding; for Cin = 3, [cout_pad][KH][64] with element 4 kx + ci"""
    cout, cin, kh, kw = w.shape
    if cin == 3:
        q = torch.zeros(cout_pad, kh, 16, 4, dtype=w.dtype)
        q[:cout, :, :kw, :3] = w.permute(0, 2, 3, 1)
    else:
        q = torch.zeros(cout_pad, kh, kw, cin_pad, dtype=w.dtype)
        q[:cout, :, :, :cin] = w.permute(0, 2, 3, 1)
    return MR.bits(q.reshape(cout_pad, -1), dtype)


def stem_frame(x, width, dtype):
    """(N, 3, H, W) -> the first layer's frame (N, H, width, 4) without a border: pixel (y, x) as {c0, c1, c2, 0}"""
    N, _, H, W = x.shape
    f = np.zeros((N, H, width, 4), np.uint16)
    f[:, :, :W, :3] = MR.bits(x.permute(0, 2, 3, 1), dtype)
    return f
