"""The feature nets of the reference's metrics table that this package carries: torchvision's AlexNet up to `features.11`, a ResNet-50 trunk up to
`avgpool` (the SwAV row), EfficientNet-B1 up to `avgpool` (the EffNet-B row) and InceptionV3 up to `avgpool` (the Inception row), on HIP kernels
(csrc/metric_nets.hip, csrc/mbconv.hip).  The metrics notebooks under Generation/ (copies of MindEye's Reconstruction_Metrics) take
alexnet(weights=IMAGENET1K_V1) through create_feature_extractor at `features.4` (the AlexNet(2) row) and `features.11` (the AlexNet(5) row) and score both by
two-way identification.

Each net is the architecture in torchvision's key layout with seeded random weights, as every model of this package: load the real checkpoint with
load_state_dict.  What the four share is _FrameNet below: the input check, the chunk loop, the cache of zero-bordered frames, the weight packer, the BatchNorm
fold, the seeded initialisation and the prefix-dropping load_state_dict; a class adds its graph walk (_forward_chunk) and its launches.  There is no eager path.
`lib`, `require_cuda` and `raw_stream` are called as this module's globals (tests/emu_patch.py swaps them).

AlexNetFeatures: one forward of a chunk of images is 8 launches: the NCHW -> frame pack, five convolution + bias + ReLU launches and two max-pools; the third
pool (`features.12`) and the classifier are never run.

ResNetFeatures is torchvision's ResNet with Bottleneck blocks (v1.5: the stride sits on conv2) without its `fc`, in torchvision's key layout, which is also
that of facebookresearch/swav's resnet50 (its ConstantPad2d(1) + padding=2 stem equals padding=3): the notebooks take the SwAV checkpoint at `avgpool` and
score np.mean of scipy's correlation distance per pair.  swav_resnet50() is the (3, 4, 6, 3) net; load the real file with load_state_dict.  One forward of a
chunk is 56 launches at full depth: the pack, 53 convolutions whose epilogue carries eval-mode BatchNorm as fp32 scale / shift, the residual add and the
ReLU (the downsample is a launch of its own without ReLU), one padded max-pool and one average pool -- no elementwise launch and no torch arithmetic between.
"""
import contextlib
import math

import torch
from torch import nn

from . import _abi
from ._lib import EegclipError, check, lib, raw_stream, require_cuda
from .ops16 import PackedWeights, dtype_code, seeded_parameters


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def pool_out(n):
    return (n - 3) // 2 + 1


def pool_pad_out(n):
    return (n - 1) // 2 + 1


def pad64(c):
    """the channel count a frame carries for `c` channels: the implicit-GEMM kernel takes multiples of 64; the padded channels are zero everywhere"""
    return (c + 63) // 64 * 64


class _FrameNet(nn.Module):
    """What the four feature nets share.  A subclass builds its children inside `with self._seeded(...)`, sets `out_features`, and gives
    _forward_chunk(x, out): the launches of one chunk of images."""
    min_side = 1                                # the smallest image side that reaches the output
    dropped = ()                                # key prefixes of the full torchvision state dict that load_state_dict drops

    @contextlib.contextmanager
    def _seeded(self, dtype, device, seed, gain=(0.5, 1.25)):
        """Build the children inside the block (seeded on the host: one seed gives one set of weights on every device).  Then, under the same seed: He's draw
        for the convolutions and every BatchNorm tensor away from the identity of PyTorch's defaults, which would let a wrong fold pass, its weight drawn
        from `gain` (None keeps PyTorch's initialisation); _draw_more() for a class's own tensors.  Last, BatchNorm tensors become fp32 (the seeded values
        are exact in `dtype`; a checkpoint's keep their precision): the kernels take them as fp32 scale / shift."""
        with seeded_parameters(self, dtype, seed=seed):
            yield
            for m in self.modules() if gain else ():
                if isinstance(m, nn.Conv2d):
                    nn.init.normal_(m.weight, 0.0, math.sqrt(2.0 / (m.in_channels // m.groups * m.kernel_size[0] * m.kernel_size[1])))
                elif isinstance(m, nn.BatchNorm2d):
                    nn.init.uniform_(m.weight, *gain)
                    nn.init.uniform_(m.bias, -0.25, 0.25)
                    nn.init.uniform_(m.running_mean, -0.25, 0.25)
                    nn.init.uniform_(m.running_var, 0.5, 1.5)
            self._draw_more()
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.float()
        self.to(device)
        self._packed, self._frames = PackedWeights(), {}

    def _draw_more(self):
        pass

    # _first: a class's first parameter (its first convolution's 16-bit weight), reached by its attribute path: a forward asks for the dtype and the device
    # before its first launch, and next(self.parameters()) walks the module tree on every call
    @property
    def dtype(self):
        return self._first.dtype

    @property
    def device(self):
        return self._first.device

    def load_state_dict(self, state_dict, strict=True, **kw):
        """the net's own keys in torchvision's layout; the full torchvision state dict loads too: the keys under the class's `dropped` prefixes are dropped.
        Any other unknown or missing key is an error (strict)."""
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith(self.dropped)}, strict=strict, **kw)

    def _checked(self, x, chunk, min_side, subject=None):
        """x as a contiguous (B, 3, H, W) batch of this net's dtype on its device with sides >= min_side, and chunk >= 1; anything else raises.  Leaves the
        dtype's C-ABI code in self._dt for the launches of this forward."""
        name, first = type(self).__name__, self._first
        require_cuda(x, "x")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1 or x.dtype != first.dtype or x.device != first.device:
            raise EegclipError(f"{name} takes (B, 3, H, W) {self.dtype} on {self.device}; got {tuple(x.shape)} {x.dtype} on {x.device}")
        H, W = x.shape[2:]
        if min(H, W) < min_side or chunk < 1:
            raise EegclipError(f"{subject or name + ' needs'} images of at least {min_side} x {min_side} and chunk >= 1; got {H} x {W}, chunk {chunk}")
        self._dt = dtype_code(x.dtype)
        return x.contiguous()

    def forward(self, x, chunk=64):
        """x: (B, 3, H, W), normalised (the row's preprocess.*_preprocess), of this net's dtype and on its device -> (B, out_features) fp32: the `avgpool`
        node, flattened.  H, W >= min_side.  The batch runs `chunk` images at a time through frames that are reused, so only the result grows with B."""
        x = self._checked(x, chunk, self.min_side)
        out = torch.empty(x.shape[0], self.out_features, dtype=torch.float32, device=x.device)
        for b0 in range(0, x.shape[0], chunk):
            self._forward_chunk(x[b0:b0 + chunk], out[b0:b0 + chunk])
        return out

    def _frame(self, role, nb, shape, dtype=None):
        """a zero-initialised buffer for `nb` images, kept between calls under (role, shape, dtype) and grown when nb exceeds it.  No launch writes a frame's
        border or its pad channels, and a role always has the same border and writes the same channels (where they vary, they are part of the role), so the
        interior is simply overwritten.  Every image size a net has seen keeps its entries (a second size adds frames, it replaces none)."""
        first = self._first
        key = (role, shape, dtype or first.dtype)
        f = self._frames.get(key)
        if f is None or f.shape[0] < nb or f.device != first.device:
            f = self._frames[key] = torch.zeros((nb, *shape), dtype=key[2], device=first.device)
        return f[:nb]

    @staticmethod
    def _pack_weight(w, cout_pad=None, cin_pad=None):
        """a convolution's weight (Cout, Cin, KH, KW) in the kernel's k order: [cout_pad][KH][KW][cin_pad] as a matrix of cout_pad rows, zero in the padding
        (None: no padding); for a 3-channel layer [cout_pad][KH][16][4], element 4 kx + ci, the rest zero"""
        cout, cin, kh, kw = w.shape
        p = torch.zeros(cout_pad or cout, kh, 16 if cin == 3 else kw, 4 if cin == 3 else cin_pad or cin, dtype=w.dtype, device=w.device)
        p[:cout, :, :kw, :cin] = w.permute(0, 2, 3, 1)
        return p.reshape(p.shape[0], -1)

    @staticmethod
    def _fold_bn(bn, padded=None):
        """eval-mode BatchNorm as fp32 (scale, shift) vectors of `padded` elements, zero in the padding; NOT folded into the 16-bit weights"""
        scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        shift = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
        out = torch.zeros(2, padded or scale.numel(), dtype=torch.float32, device=scale.device)
        out[0, :scale.numel()], out[1, :scale.numel()] = scale, shift
        return out[0], out[1]

    def _packed_layer(self, tag, conv, bn, cout_pad=None, cin_pad=None):
        """(packed weight, scale, shift) of a convolution and the BatchNorm behind it, made once per state of their tensors"""
        return self._packed.get(tag, (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var),
                                lambda: (self._pack_weight(conv.weight.detach(), cout_pad, cin_pad), *self._fold_bn(bn, cout_pad)))


# torchvision/models/alexnet.py: features.{index}: (Cin, Cout, kernel, stride, padding); a ReLU follows each, MaxPool2d(3, 2) follows the ReLUs of 0 and 3
CONVS = {"0": (3, 64, 11, 4, 2), "3": (64, 192, 5, 1, 2), "6": (192, 384, 3, 1, 1), "8": (384, 256, 3, 1, 1), "10": (256, 256, 3, 1, 1)}
NODES = ("features.4", "features.11")           # the outputs of the ReLUs behind features.3 and features.10
_MIN_SIDE = {"features.4": 15, "features.11": 31}


class AlexNetFeatures(_FrameNet):
    dropped = ("classifier.",)                  # (the net's own keys are the ten features.{0,3,6,8,10}.{weight,bias})
    _first = property(lambda self: self.features["0"].weight)

    def __init__(self, dtype=torch.float16, device="cuda", seed=0):
        super().__init__()
        with self._seeded(dtype, device, seed, gain=None):
            self.features = nn.ModuleDict({i: nn.Conv2d(cin, cout, k, s, p) for i, (cin, cout, k, s, p) in CONVS.items()})

    def _weight(self, i):
        """features.i's weight in the kernel's k order: [Cout][ky][kx][ci]; for the 3-channel layer [Cout][ky][64], element 4 kx + ci, the rest zero"""
        conv = self.features[i]
        return self._packed.get(i, (conv.weight,), lambda: self._pack_weight(conv.weight.detach()))

    def _conv(self, i, src, out, nb, Hi, Wi, out_pad):
        cin, cout, k, s, p = CONVS[i]
        d = _abi.ConvRelu16Desc(in_=src.data_ptr(), W=self._weight(i).data_ptr(), bias=self.features[i].bias.data_ptr(), out=out.data_ptr(), N=nb, Hi=Hi, Wi=Wi,
                                Cin=cin, Cout=cout, KS=k, stride=s, pad=p, out_pad=out_pad, dtype=self._dt)
        check(lib().eegclip_convrelu16(d, raw_stream()), f"convrelu16 (features.{i}, {nb} x {Hi} x {Wi})")

    def _pool(self, src, out, nb, H, W, C, out_pad):
        check(lib().eegclip_maxpool16(src.data_ptr(), out.data_ptr(), nb, H, W, C, 0, out_pad, self._dt, raw_stream()), f"maxpool16 ({nb} x {H} x {W} x {C})")

    def forward(self, x, nodes=NODES, chunk=64):
        """x: (B, 3, H, W), normalised (preprocess.alexnet_preprocess), of this net's dtype and on its device -> {node: (B, C, h, w)} for the nodes asked
        for, what torchvision's create_feature_extractor(alexnet, nodes) returns: `features.4` (B, 192, h2, w2), `features.11` (B, 256, h3, w3) -- (31, 31)
        and (15, 15) at 256 x 256.  Each is a permuted view of the kernels' NHWC result.  The batch runs `chunk` images at a time through frames that are
        reused, so only the results grow with B."""
        nodes = (nodes,) if isinstance(nodes, str) else tuple(nodes)
        if not nodes or any(n not in NODES for n in nodes):
            raise EegclipError(f"AlexNetFeatures returns {NODES}; got {nodes}")
        need = max(_MIN_SIDE[n] for n in nodes)
        x = self._checked(x, chunk, need, f"{' and '.join(nodes)} need")
        B, _, H, W = x.shape
        h2, w2 = pool_out(conv_out(H, 11, 4, 2)), pool_out(conv_out(W, 11, 4, 2))
        out4 = torch.empty(B, h2, w2, 192, dtype=x.dtype, device=x.device) if "features.4" in nodes else None
        out11 = torch.empty(B, pool_out(h2), pool_out(w2), 256, dtype=x.dtype, device=x.device) if "features.11" in nodes else None
        for b0 in range(0, B, chunk):
            self._forward_chunk(x[b0:b0 + chunk], *(o[b0:b0 + chunk] if o is not None else None for o in (out4, out11)))
        return {node: o.permute(0, 3, 1, 2) for node, o in zip(NODES, (out4, out11)) if o is not None}

    def _forward_chunk(self, x, out4, out11):
        (nb, _, H, W), L, dt = x.shape, lib(), self._dt
        h1, w1 = conv_out(H, 11, 4, 2), conv_out(W, 11, 4, 2)
        h2, w2 = pool_out(h1), pool_out(w1)
        f0 = self._frame("in", nb, (H + 4, L.eegclip_convrelu16_in_width(W), 4))
        check(L.eegclip_pack_nchw16(x.data_ptr(), f0.data_ptr(), nb, H, W, dt, raw_stream()), f"pack_nchw16 ({nb} x {H} x {W})")
        a1 = self._frame("c0", nb, (h1, w1, 64))
        self._conv("0", f0, a1, nb, H, W, 0)
        p1 = self._frame("p1", nb, (h2 + 4, w2 + 4, 64))
        self._pool(a1, p1, nb, h1, w1, 64, 2)
        a2 = out4 if out4 is not None else self._frame("c3", nb, (h2, w2, 192))
        self._conv("3", p1, a2, nb, h2, w2, 0)
        if out11 is None:
            return
        h3, w3 = pool_out(h2), pool_out(w2)
        p2 = self._frame("p2", nb, (h3 + 2, w3 + 2, 192))
        self._pool(a2, p2, nb, h2, w2, 192, 1)
        a3 = self._frame("c6", nb, (h3 + 2, w3 + 2, 384))
        self._conv("6", p2, a3, nb, h3, w3, 1)
        a4 = self._frame("c8", nb, (h3 + 2, w3 + 2, 256))
        self._conv("8", a3, a4, nb, h3, w3, 1)
        self._conv("10", a4, out11, nb, h3, w3, 0)


# ---------------------------------------------------------------------------------------------------------------------- ResNet trunk (the SwAV row)
WIDTHS = (64, 128, 256, 512)                    # torchvision/models/resnet.py: the bottleneck width of layer1 .. layer4; a block's output is 4 x that
DROPPED = ("fc.", "projection_head.", "prototypes.")
MIN_SIDE = 1                                    # every layer pads by KS / 2 and the pools round up: a 1 x 1 image reaches `avgpool` (as 1 x 1 throughout)


class _Bottleneck(nn.Module):
    """torchvision's Bottleneck as a holder of parameters (never called): conv1 1 x 1, conv2 3 x 3 with the stride, conv3 1 x 1 to 4 x width, a BatchNorm
    behind each, and in a stage's first block `downsample` = Sequential(1 x 1 convolution with the stride, BatchNorm)"""

    def __init__(self, cin, width, stride, downsample):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(cin, width, 1, bias=False), nn.BatchNorm2d(width)
        self.conv2, self.bn2 = nn.Conv2d(width, width, 3, stride, 1, bias=False), nn.BatchNorm2d(width)
        self.conv3, self.bn3 = nn.Conv2d(width, 4 * width, 1, bias=False), nn.BatchNorm2d(4 * width)
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(cin, 4 * width, 1, stride, bias=False), nn.BatchNorm2d(4 * width))
        self.stride = stride


class ResNetFeatures(_FrameNet):
    min_side, dropped, out_features = MIN_SIDE, DROPPED, 4 * WIDTHS[3]
    _first = property(lambda self: self.conv1.weight)

    def __init__(self, layers=(3, 4, 6, 3), dtype=torch.float16, device="cuda", seed=0):
        super().__init__()
        if len(layers) != 4 or any(int(n) < 1 for n in layers):
            raise EegclipError(f"ResNetFeatures takes four stage depths >= 1; got {layers}")
        self.layers = tuple(int(n) for n in layers)
        with self._seeded(dtype, device, seed):
            self.conv1, self.bn1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64)
            cin = 64
            for s, (width, n) in enumerate(zip(WIDTHS, self.layers)):
                blocks = []
                for i in range(n):
                    blocks.append(_Bottleneck(cin, width, (2 if s > 0 and i == 0 else 1), i == 0))
                    cin = 4 * width
                setattr(self, f"layer{s + 1}", nn.Sequential(*blocks))

    def load_state_dict(self, state_dict, strict=True, **kw):
        """torchvision's ResNet keys without `fc`; a full torchvision state dict or a SwAV checkpoint loads too: a leading `module.` is stripped and the
        fc.* / projection_head.* / prototypes.* keys are dropped.  Any other unknown or missing key is an error (strict)."""
        return super().load_state_dict({k[len("module."):] if k.startswith("module.") else k: v for k, v in state_dict.items()}, strict=strict, **kw)

    def _layer(self, tag, conv, bn):
        """(packed weight, scale, shift) of a convolution and the BatchNorm behind it: the weight in the kernel's k order -- [Cout][ky][kx][ci]; for the stem
        [64][ky][64], element 4 kx + ci, the rest zero -- and eval-mode BatchNorm as fp32 vectors"""
        return self._packed_layer(tag, conv, bn)

    def _conv(self, tag, conv, bn, src, out, nb, Hi, Wi, out_pad, relu, residual=None):
        w, scale, shift = self._layer(tag, conv, bn)
        d = _abi.ConvBn16Desc(in_=src.data_ptr(), W=w.data_ptr(), scale=scale.data_ptr(), shift=shift.data_ptr(),
                              residual=residual.data_ptr() if residual is not None else None, out=out.data_ptr(), N=nb, Hi=Hi, Wi=Wi,
                              Cin=conv.in_channels, Cout=conv.out_channels, KS=conv.kernel_size[0], stride=conv.stride[0], pad=conv.padding[0],
                              out_pad=out_pad, relu=int(relu), dtype=self._dt)
        check(lib().eegclip_convbn16(d, raw_stream()), f"convbn16 ({tag}, {nb} x {Hi} x {Wi})")

    def _forward_chunk(self, x, out):
        """x: normalised by preprocess.swav_preprocess -> out (nb, 2048)"""
        (nb, _, H, W), L, dt = x.shape, lib(), self._dt
        h1, w1 = conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3)
        f0 = self._frame("in", nb, (H + 6, L.eegclip_convbn16_in_width(W), 4))
        check(L.eegclip_pack_nchw16_stem(x.data_ptr(), f0.data_ptr(), nb, H, W, dt, raw_stream()), f"pack_nchw16_stem ({nb} x {H} x {W})")
        a = self._frame("conv1", nb, (h1, w1, 64))
        self._conv("conv1", self.conv1, self.bn1, f0, a, nb, H, W, 0, True)
        h, w = pool_pad_out(h1), pool_pad_out(w1)
        cur = self._frame("pool", nb, (h, w, 64))
        check(L.eegclip_maxpool16_pad(a.data_ptr(), cur.data_ptr(), nb, h1, w1, 64, 0, 0, dt, raw_stream()), f"maxpool16_pad ({nb} x {h1} x {w1} x 64)")
        for s, width in enumerate(WIDTHS):
            for i, blk in enumerate(getattr(self, f"layer{s + 1}")):
                tag = f"layer{s + 1}.{i}"
                ho, wo = conv_out(h, 3, blk.stride, 1), conv_out(w, 3, blk.stride, 1)
                c1 = self._frame(f"layer{s + 1}.c1.{min(i, 1)}", nb, (h + 2, w + 2, width))        # (a border of 1: the 3 x 3 layer reads it)
                self._conv(tag + ".conv1", blk.conv1, blk.bn1, cur, c1, nb, h, w, 1, True)
                c2 = self._frame(f"layer{s + 1}.c2", nb, (ho, wo, width))
                self._conv(tag + ".conv2", blk.conv2, blk.bn2, c1, c2, nb, h, w, 0, True)
                res = cur
                if i == 0:
                    res = self._frame(f"layer{s + 1}.ds", nb, (ho, wo, 4 * width))
                    self._conv(tag + ".downsample", blk.downsample[0], blk.downsample[1], cur, res, nb, h, w, 0, False)
                nxt = self._frame(f"layer{s + 1}.out.{i & 1}", nb, (ho, wo, 4 * width))
                self._conv(tag + ".conv3", blk.conv3, blk.bn3, c2, nxt, nb, ho, wo, 0, True, residual=res)
                cur, h, w = nxt, ho, wo
        check(L.eegclip_avgpool16(cur.data_ptr(), out.data_ptr(), nb, h, w, 4 * WIDTHS[3], dt, raw_stream()), f"avgpool16 ({nb} x {h} x {w})")


def swav_resnet50(**kw):
    """the ResNet-50 trunk of the metrics table's SwAV row (facebookresearch/swav's resnet50 without its projection head and prototypes), seeded weights"""
    return ResNetFeatures(layers=(3, 4, 6, 3), **kw)


# ---------------------------------------------------------------------------------------------------------------------- EfficientNet trunk (the EffNet-B row)
# torchvision/models/efficientnet.py: (expand ratio, kernel, stride, input channels, output channels) of features.1 .. features.7; B0's depths are
# (1, 2, 2, 3, 3, 4, 1) and B1's ceil(1.1 x) of them
EFF_STAGES = ((1, 3, 1, 32, 16), (6, 3, 2, 16, 24), (6, 5, 2, 24, 40), (6, 3, 2, 40, 80), (6, 5, 1, 80, 112), (6, 5, 2, 112, 192), (6, 3, 1, 192, 320))
EFF_B1_LAYERS = (2, 3, 3, 4, 4, 5, 2)
EFF_STEM, EFF_HEAD = 32, 1280
ACT_NONE, ACT_RELU, ACT_SILU = 0, 1, 2


def _conv_bn(cin, cout, k, stride, groups=1):
    """torchvision's Conv2dNormActivation as a holder of parameters: `.0` the convolution without bias, `.1` the BatchNorm (the activation has no key)"""
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride, k // 2, groups=groups, bias=False), nn.BatchNorm2d(cout))


class _SqueezeExcitation(nn.Module):
    def __init__(self, channels, squeeze):
        super().__init__()
        self.fc1, self.fc2 = nn.Conv2d(channels, squeeze, 1), nn.Conv2d(squeeze, channels, 1)


class _MBConv(nn.Module):
    """torchvision's MBConv as a holder of parameters (never called): `block` = [1 x 1 expansion unless the ratio is 1,] depthwise k x k with the stride,
    squeeze-and-excitation with max(1, input channels // 4) hidden units, 1 x 1 projection (no activation); the input is added when the shapes allow"""

    def __init__(self, expand, k, stride, cin, cout):
        super().__init__()
        self.expand, self.k, self.stride, self.cin, self.cout, self.cexp = expand, k, stride, cin, cout, cin * expand
        self.residual = stride == 1 and cin == cout
        layers = [_conv_bn(cin, self.cexp, 1, 1)] if expand != 1 else []
        layers += [_conv_bn(self.cexp, self.cexp, k, stride, groups=self.cexp), _SqueezeExcitation(self.cexp, max(1, cin // 4)), _conv_bn(self.cexp, cout, 1, 1)]
        self.block = nn.Sequential(*layers)


class EfficientNetFeatures(_FrameNet):
    """torchvision's EfficientNet (B0 / B1 widths) without its classifier, in torchvision's key layout: the notebooks take efficientnet_b1(weights=DEFAULT) at
    `avgpool`, flatten to (N, 1280) and score np.mean of scipy's correlation distance per pair.  efficientnet_b1() is the (2, 3, 3, 4, 4, 5, 2) net; load the real
    checkpoint with load_state_dict(torchvision.models.efficientnet_b1(weights="DEFAULT").state_dict()).

    Channel counts here (16, 24, 40, 80, 112, 144, 240, 672 ..) are not multiples of the convolution kernel's 64: every frame carries pad64(C) channels, the
    packed weights have zero rows / columns there and scale = shift = 0, so a padded channel is exactly 0 through SiLU (0 sigmoid(0)), the gate multiply and the
    residual.  One forward of a chunk at full depth is 117 launches: the pack, the stem, per block [the expansion,] the depthwise convolution (BatchNorm, SiLU
    and the squeeze's pooled sums in its epilogue), the gate, the gate multiply and the projection (which carries the residual), the head and the average
    pool -- no torch arithmetic between.  There is no eager path."""

    min_side, dropped, out_features = MIN_SIDE, ("classifier.",), EFF_HEAD
    _first = property(lambda self: self.features[0][0].weight)

    def __init__(self, layers=EFF_B1_LAYERS, dtype=torch.float16, device="cuda", seed=0):
        super().__init__()
        if len(layers) != 7 or any(int(n) < 1 for n in layers):
            raise EegclipError(f"EfficientNetFeatures takes seven stage depths >= 1; got {layers}")
        self.layers = tuple(int(n) for n in layers)
        with self._seeded(dtype, device, seed):
            stages = [_conv_bn(3, EFF_STEM, 3, 2)]
            for (expand, k, stride, cin, cout), n in zip(EFF_STAGES, self.layers):
                stages.append(nn.Sequential(*[_MBConv(expand, k, stride if i == 0 else 1, cin if i == 0 else cout, cout) for i in range(n)]))
            stages.append(_conv_bn(EFF_STAGES[-1][4], EFF_HEAD, 1, 1))
            self.features = nn.Sequential(*stages)

    def _draw_more(self):
        # the gates are drawn mostly OPEN (fc2.bias around 2): with PyTorch's defaults every gate averages 0.5, the signal halves per block and `avgpool`
        # no longer depends on the input
        for m in self.modules():
            if isinstance(m, _SqueezeExcitation):
                nn.init.normal_(m.fc1.weight, 0.0, math.sqrt(1.0 / m.fc1.in_channels))
                nn.init.normal_(m.fc1.bias, 0.0, 0.5)
                nn.init.normal_(m.fc2.weight, 0.0, math.sqrt(4.0 / m.fc2.in_channels))
                nn.init.normal_(m.fc2.bias, 2.0, 0.5)

    def blocks(self):
        """[(key prefix, _MBConv)] in the order they run"""
        return [(f"features.{s}.{i}", blk) for s in range(1, 8) for i, blk in enumerate(self.features[s])]

    def _layer(self, tag, conv, bn):
        """(packed weight, scale, shift) of a dense convolution and the BatchNorm behind it, padded with zeros to pad64 channels: [pad64(Cout)][pad64(Cin)] for
        a 1 x 1 layer, [64][ky][64] with element 4 kx + ci for the stem (rows 32 .. 63 zero); eval-mode BatchNorm as fp32 vectors, zero in the padding"""
        return self._packed_layer(tag, conv, bn, pad64(conv.out_channels), pad64(conv.in_channels))

    def _depthwise(self, tag, conv, bn):
        """(weight [ky][kx][pad64(C)], scale, shift) of a depthwise convolution and its BatchNorm"""
        def make():
            w = conv.weight.detach()                              # (C, 1, k, k)
            p = torch.zeros(w.shape[2], w.shape[3], pad64(w.shape[0]), dtype=w.dtype, device=w.device)
            p[:, :, :w.shape[0]] = w[:, 0].permute(1, 2, 0)
            return (p, *self._fold_bn(bn, pad64(w.shape[0])))
        return self._packed.get(tag, (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var), make)

    def _se(self, tag, se):
        """(fc1 [sq][pad64(C)], b1 [sq], fc2 [pad64(C)][sq], b2 [pad64(C)]) in the net's dtype, zero in the padding (a padded channel's gate is 0.5, times 0)"""
        def make():
            sq, c = se.fc1.weight.shape[:2]
            w1 = torch.zeros(sq, pad64(c), dtype=self.dtype, device=self.device)
            w1[:, :c] = se.fc1.weight.detach()[:, :, 0, 0]
            w2 = torch.zeros(pad64(c), sq, dtype=self.dtype, device=self.device)
            w2[:c] = se.fc2.weight.detach()[:, :, 0, 0]
            b2 = torch.zeros(pad64(c), dtype=self.dtype, device=self.device)
            b2[:c] = se.fc2.bias.detach()
            return w1, se.fc1.bias.detach().contiguous(), w2, b2
        return self._packed.get(tag, (se.fc1.weight, se.fc1.bias, se.fc2.weight, se.fc2.bias), make)

    def _conv(self, tag, layer, src, out, nb, Hi, Wi, in_pad, out_pad, act, residual=None):
        conv, bn = layer[0], layer[1]
        w, scale, shift = self._layer(tag, conv, bn)
        stem = conv.in_channels == 3
        d = _abi.ConvBnAct16Desc(in_=src.data_ptr(), W=w.data_ptr(), scale=scale.data_ptr(), shift=shift.data_ptr(),
                                 residual=residual.data_ptr() if residual is not None else None, out=out.data_ptr(), N=nb, Hi=Hi, Wi=Wi,
                                 Cin=3 if stem else pad64(conv.in_channels), Cout=pad64(conv.out_channels), KS=conv.kernel_size[0], stride=conv.stride[0],
                                 pad=conv.padding[0], in_pad=in_pad, out_pad=out_pad, act=act, dtype=self._dt)
        check(lib().eegclip_convbnact16(d, raw_stream()), f"convbnact16 ({tag}, {nb} x {Hi} x {Wi})")

    def _forward_chunk(self, x, out):
        """x: normalised by preprocess.effnet_preprocess -> out (nb, 1280)"""
        (nb, _, H, W), L, dt = x.shape, lib(), self._dt
        h0, w0 = conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1)
        blocks = self.blocks()
        f0 = self._frame("in", nb, (H + 2, L.eegclip_convbnact16_in_width(W), 4))
        check(L.eegclip_pack_nchw16_pad1(x.data_ptr(), f0.data_ptr(), nb, H, W, dt, raw_stream()), f"pack_nchw16_pad1 ({nb} x {H} x {W})")
        # a frame's border is what its READER pads by: the first block has no expansion, so its depthwise layer reads the stem's output itself
        cur_pad = blocks[0][1].k // 2 if blocks[0][1].expand == 1 else 0
        cur = self._frame("stem", nb, (h0 + 2 * cur_pad, w0 + 2 * cur_pad, pad64(EFF_STEM)))
        self._conv("features.0", self.features[0], f0, cur, nb, H, W, 0, cur_pad, ACT_SILU)
        h, w = h0, w0
        for idx, (tag, blk) in enumerate(blocks):
            p, ce = blk.k // 2, pad64(blk.cexp)
            ho, wo = conv_out(h, blk.k, blk.stride, p), conv_out(w, blk.k, blk.stride, p)
            if blk.expand != 1:
                src = self._frame(f"expand.pad{p}", nb, (h + 2 * p, w + 2 * p, ce))
                self._conv(tag + ".block.0", blk.block[0], cur, src, nb, h, w, cur_pad, p, ACT_SILU)
            elif cur_pad == p:
                src = cur
            else:
                raise EegclipError(f"{tag}: a block without expansion reads its input frame's border ({p}); the frame has {cur_pad}")
            dwl, se = blk.block[-3], blk.block[-2]
            dw_w, dw_scale, dw_shift = self._depthwise(tag + ".depthwise", dwl[0], dwl[1])
            S = L.eegclip_dwconv16_slabs(h, w, blk.k, blk.stride)
            y = self._frame("depthwise", nb, (ho, wo, ce))
            slab, gate = self._frame("slab", nb, (S, ce), torch.float32), self._frame("gate", nb, (ce,), torch.float32)
            check(L.eegclip_dwconv16(src.data_ptr(), dw_w.data_ptr(), dw_scale.data_ptr(), dw_shift.data_ptr(), y.data_ptr(), slab.data_ptr(), nb, h, w, ce, blk.k,
                                     blk.stride, dt, raw_stream()), f"dwconv16 ({tag}, {nb} x {h} x {w} x {ce})")
            w1, b1, w2, b2 = self._se(tag + ".se", se)
            check(L.eegclip_se_gate16(slab.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), gate.data_ptr(), nb, S, ho * wo, ce,
                                      w1.shape[0], dt, raw_stream()), f"se_gate16 ({tag}, {nb} x {ce})")
            check(L.eegclip_gate_mul16(y.data_ptr(), gate.data_ptr(), nb, ho * wo, ce, dt, raw_stream()), f"gate_mul16 ({tag}, {nb} x {ho} x {wo} x {ce})")
            # the output frame: the residual is read in the output's own layout, so a block that adds its input keeps the input's border; otherwise the
            # border the next reader needs (a following block without expansion; a 1 x 1 layer skips whatever border it meets)
            nxt = blocks[idx + 1][1] if idx + 1 < len(blocks) else None
            out_pad = cur_pad if blk.residual else (nxt.k // 2 if nxt is not None and nxt.expand == 1 else 0)
            o = self._frame(f"out{idx & 1}.pad{out_pad}", nb, (ho + 2 * out_pad, wo + 2 * out_pad, pad64(blk.cout)))
            self._conv(tag + ".block.project", blk.block[-1], y, o, nb, ho, wo, 0, out_pad, ACT_NONE, residual=cur if blk.residual else None)
            cur, cur_pad, h, w = o, out_pad, ho, wo
        head = self._frame("head", nb, (h, w, EFF_HEAD))
        self._conv("features.8", self.features[8], cur, head, nb, h, w, cur_pad, 0, ACT_SILU)
        check(L.eegclip_avgpool16(head.data_ptr(), out.data_ptr(), nb, h, w, EFF_HEAD, dt, raw_stream()), f"avgpool16 ({nb} x {h} x {w})")


def efficientnet_b1(**kw):
    """the EfficientNet-B1 trunk of the metrics table's EffNet-B row (torchvision's efficientnet_b1 without its classifier), seeded weights"""
    return EfficientNetFeatures(layers=EFF_B1_LAYERS, **kw)


# ---------------------------------------------------------------------------------------------------------------------- InceptionV3 trunk (the Inception row)
# torchvision/models/inception.py.  A branch is a chain of BasicConv2d layers (name, Cout, (KH, KW), stride, (pad_h, pad_w)); the last layer(s) of a chain write
# their slice of the block's output frame.  "pool" stands for the block's pooling branch.
MIN_SIDE_INCEPTION = 75                         # 75 -> 37 -> 35 -> 35 -> 17 -> 17 -> 15 -> 7 (Mixed_5*) -> 3 (Mixed_6*) -> 1 (Mixed_7*); at 74 Mixed_7a meets 2 x 2
INC_A_POOL, INC_C_MID = (32, 64, 64), (128, 160, 160, 192)
INC_NAMES = {"A": ("Mixed_5b", "Mixed_5c", "Mixed_5d"), "B": ("Mixed_6a",), "C": ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"), "D": ("Mixed_7a",),
             "E": ("Mixed_7b", "Mixed_7c")}
INC_STEM = (("Conv2d_1a_3x3", 3, 32, 3, 2, 0), ("Conv2d_2a_3x3", 32, 32, 3, 1, 0), ("Conv2d_2b_3x3", 32, 64, 3, 1, 1), ("Conv2d_3b_1x1", 64, 80, 1, 1, 0),
            ("Conv2d_4a_3x3", 80, 192, 3, 1, 0))
INC_MEAN, INC_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def inception_block_layers(kind, cin, arg=None):
    """[(name, Cin, Cout, (KH, KW), stride, (pad_h, pad_w))] of a block in torchvision's registration order; arg: pool_features (A) or channels_7x7 (C)"""
    sq = lambda n, i, o, k, s=1, p=0: (n, i, o, (k, k), s, (p, p))   # noqa: E731
    if kind == "A":
        return [sq("branch1x1", cin, 64, 1), sq("branch5x5_1", cin, 48, 1), sq("branch5x5_2", 48, 64, 5, 1, 2), sq("branch3x3dbl_1", cin, 64, 1),
                sq("branch3x3dbl_2", 64, 96, 3, 1, 1), sq("branch3x3dbl_3", 96, 96, 3, 1, 1), sq("branch_pool", cin, arg, 1)]
    if kind == "B":
        return [sq("branch3x3", cin, 384, 3, 2), sq("branch3x3dbl_1", cin, 64, 1), sq("branch3x3dbl_2", 64, 96, 3, 1, 1), sq("branch3x3dbl_3", 96, 96, 3, 2)]
    row, col = lambda n, i, o, k: (n, i, o, (1, k), 1, (0, k // 2)), lambda n, i, o, k: (n, i, o, (k, 1), 1, (k // 2, 0))   # noqa: E731
    if kind == "C":
        c = arg
        return [sq("branch1x1", cin, 192, 1), sq("branch7x7_1", cin, c, 1), row("branch7x7_2", c, c, 7), col("branch7x7_3", c, 192, 7),
                sq("branch7x7dbl_1", cin, c, 1), col("branch7x7dbl_2", c, c, 7), row("branch7x7dbl_3", c, c, 7), col("branch7x7dbl_4", c, c, 7),
                row("branch7x7dbl_5", c, 192, 7), sq("branch_pool", cin, 192, 1)]
    if kind == "D":
        return [sq("branch3x3_1", cin, 192, 1), sq("branch3x3_2", 192, 320, 3, 2), sq("branch7x7x3_1", cin, 192, 1), row("branch7x7x3_2", 192, 192, 7),
                col("branch7x7x3_3", 192, 192, 7), sq("branch7x7x3_4", 192, 192, 3, 2)]
    return [sq("branch1x1", cin, 320, 1), sq("branch3x3_1", cin, 384, 1), row("branch3x3_2a", 384, 384, 3), col("branch3x3_2b", 384, 384, 3),
            sq("branch3x3dbl_1", cin, 448, 1), sq("branch3x3dbl_2", 448, 384, 3, 1, 1), row("branch3x3dbl_3a", 384, 384, 3), col("branch3x3dbl_3b", 384, 384, 3),
            sq("branch_pool", cin, 192, 1)]


# how a block runs: per launch (layer name | "pool", source, destination); sources / destinations are "in" (the block's input frame), "out" (a slice of its output
# frame, in the order of concatenation) or a temporary's name
INC_FLOW = {
    "A": (("branch1x1", "in", "out"), ("branch5x5_1", "in", "a"), ("branch5x5_2", "a", "out"), ("branch3x3dbl_1", "in", "a"), ("branch3x3dbl_2", "a", "b"),
          ("branch3x3dbl_3", "b", "out"), ("pool", "in", "p"), ("branch_pool", "p", "out")),
    "B": (("branch3x3", "in", "out"), ("branch3x3dbl_1", "in", "a"), ("branch3x3dbl_2", "a", "b"), ("branch3x3dbl_3", "b", "out"), ("pool", "in", "out")),
    "C": (("branch1x1", "in", "out"), ("branch7x7_1", "in", "a"), ("branch7x7_2", "a", "b"), ("branch7x7_3", "b", "out"), ("branch7x7dbl_1", "in", "a"),
          ("branch7x7dbl_2", "a", "b"), ("branch7x7dbl_3", "b", "a"), ("branch7x7dbl_4", "a", "b"), ("branch7x7dbl_5", "b", "out"), ("pool", "in", "p"),
          ("branch_pool", "p", "out")),
    "D": (("branch3x3_1", "in", "a"), ("branch3x3_2", "a", "out"), ("branch7x7x3_1", "in", "a"), ("branch7x7x3_2", "a", "b"), ("branch7x7x3_3", "b", "a"),
          ("branch7x7x3_4", "a", "out"), ("pool", "in", "out")),
    "E": (("branch1x1", "in", "out"), ("branch3x3_1", "in", "a"), ("branch3x3_2a", "a", "out"), ("branch3x3_2b", "a", "out"), ("branch3x3dbl_1", "in", "a"),
          ("branch3x3dbl_2", "a", "b"), ("branch3x3dbl_3a", "b", "out"), ("branch3x3dbl_3b", "b", "out"), ("pool", "in", "p"), ("branch_pool", "p", "out")),
}


class _BasicConv2d(nn.Module):
    """torchvision's BasicConv2d as a holder of parameters (never called): `conv` without bias, `bn` with eps = 0.001; a ReLU follows"""

    def __init__(self, cin, cout, kernel, stride, padding):
        super().__init__()
        self.conv, self.bn = nn.Conv2d(cin, cout, kernel, stride, padding, bias=False), nn.BatchNorm2d(cout, eps=0.001)


class _InceptionBlock(nn.Module):
    def __init__(self, kind, cin, arg=None):
        super().__init__()
        self.kind, self.cin = kind, cin
        layers = inception_block_layers(kind, cin, arg)
        for name, i, o, k, s, p in layers:
            setattr(self, name, _BasicConv2d(i, o, k, s, p))
        sliced = [getattr(self, n).conv.out_channels for n, _, dst in INC_FLOW[kind] if dst == "out" and n != "pool"]
        self.cout = sum(sliced) + (cin if kind in "BD" else 0)     # (B and D concatenate the max-pooled input)


class InceptionFeatures(_FrameNet):
    """torchvision's Inception3 up to `avgpool` (no AuxLogits, no fc), in torchvision's key layout: the notebooks take inception_v3(weights=DEFAULT) -- so
    transform_input=True -- at `avgpool`, flatten to (N, 2048) and score two-way identification.  inception_v3() is the (3, 4, 2) net; load the real checkpoint
    with load_state_dict(torchvision.models.inception_v3(weights="DEFAULT").state_dict()).  blocks = (InceptionA, InceptionC, InceptionE blocks kept, from the
    front of each group); a block's input width is its predecessor's output width.

    A block's output is ONE frame of pad64(total) channels per pixel: every branch's last convolution (and the max-pool branch of Mixed_6a / Mixed_7a) writes its
    own channel slice through eegclip_convbncat16 / eegclip_maxpool16_cat, so nothing is concatenated or copied; pad channels (288 -> 320, 736 -> 768) stay the
    zeros the frame was allocated with and meet zero weight columns.  One forward of a chunk at full depth is 109 launches: the pack (with transform_input's
    affine), 94 convolutions, the two stem max-pools, 9 average pools 3 x 3, 2 max-pool branches and the global average pool -- no torch arithmetic between.
    There is no eager path."""

    min_side, dropped = MIN_SIDE_INCEPTION, ("AuxLogits.", "fc.")
    _first = property(lambda self: self.Conv2d_1a_3x3.conv.weight)

    def __init__(self, blocks=(3, 4, 2), transform_input=True, dtype=torch.float16, device="cuda", seed=0):
        super().__init__()
        if len(blocks) != 3 or any(int(n) < 1 for n in blocks) or blocks[0] > 3 or blocks[1] > 4 or blocks[2] > 2:
            raise EegclipError(f"InceptionFeatures takes (1..3, 1..4, 1..2) InceptionA / C / E blocks; got {blocks}")
        self.blocks, self.transform_input = tuple(int(n) for n in blocks), bool(transform_input)
        # The BatchNorm gain is drawn from (0.7, 1.4): with the other nets' (0.5, 1.25) the 3 x 3 average pools and 1 / sqrt(var) shrink the signal at every
        # block until `avgpool` is the BatchNorm shifts' alone (its spread over images falls below fp16's rounding); with (0.75, 1.5) it grows to hundreds at
        # 342 x 342.  Here the fp64 chain peaks below 100.
        with self._seeded(dtype, device, seed, gain=(0.7, 1.4)):
            for name, cin, cout, k, s, p in INC_STEM:
                setattr(self, name, _BasicConv2d(cin, cout, k, s, p))
            c, self.order = 192, []
            for kind, n, args in (("A", self.blocks[0], INC_A_POOL), ("B", 1, (None,)), ("C", self.blocks[1], INC_C_MID), ("D", 1, (None,)),
                                  ("E", self.blocks[2], (None, None))):
                for i in range(n):
                    blk = _InceptionBlock(kind, c, args[i])
                    setattr(self, INC_NAMES[kind][i], blk)
                    self.order.append(INC_NAMES[kind][i])
                    c = blk.cout
            self.out_features = c

    def _layer(self, tag, layer, cin_pad):
        """(packed weight, scale, shift) of a BasicConv2d: [pad64(Cout)][KH][KW][cin_pad] with zero rows / columns in the padding -- for the first layer
        [64][ky][64] with element 4 kx + ci -- and eval-mode BatchNorm as fp32 [pad64(Cout)] vectors, zero in the padding"""
        return self._packed_layer((tag, cin_pad), layer.conv, layer.bn, pad64(layer.conv.out_channels), cin_pad)

    def _affine(self):
        """transform_input as fp32 (a, b) [3] on the device: torchvision's x_c (std_c / 0.5) + (mean_c - 0.5) / 0.5; the identity without it"""
        key = ("affine", self.transform_input, self.device)
        if key not in self._frames:
            a = [s / 0.5 for s in INC_STD] if self.transform_input else [1.0] * 3
            b = [(m - 0.5) / 0.5 for m in INC_MEAN] if self.transform_input else [0.0] * 3
            self._frames[key] = torch.tensor([a, b], dtype=torch.float32, device=self.device)
        return self._frames[key]

    def _bordered(self, role, nb, h, w, c, pad):
        """(frame [nb][h + 2 pad][w + 2 pad][pad64(c)], pad): the channel count and the border are part of the role, so a role always writes the same channels"""
        return self._frame((role, c, pad), nb, (h + 2 * pad, w + 2 * pad, pad64(c))), pad

    def _conv(self, tag, layer, src, dst, c0, nb, h, w):
        """one BasicConv2d launch from frame `src` = (tensor, border) at h x w into channels c0 .. of frame `dst`"""
        (s, in_pad), (d, out_pad), conv = src, dst, layer.conv
        first = conv.in_channels == 3
        wt, scale, shift = self._layer(tag, layer, 4 if first else s.shape[3])
        desc = _abi.ConvBnCat16Desc(in_=s.data_ptr(), W=wt.data_ptr(), scale=scale.data_ptr(), shift=shift.data_ptr(), out=d.data_ptr(), N=nb, Hi=h, Wi=w,
                                    Cin=3 if first else s.shape[3], Cout=conv.out_channels, KH=conv.kernel_size[0], KW=conv.kernel_size[1],
                                    stride=conv.stride[0], pad_h=conv.padding[0], pad_w=conv.padding[1], in_pad=in_pad, out_pad=out_pad, out_stride=d.shape[3],
                                    out_c0=c0, relu=1, dtype=self._dt)
        check(lib().eegclip_convbncat16(desc, raw_stream()), f"convbncat16 ({tag}, {nb} x {h} x {w})")

    def _block(self, name, blk, cur, nb, h, w, out_pad, parity):
        """one Inception block from frame `cur` -> (its output frame, ho, wo)"""
        kind, L, dt = blk.kind, lib(), self._dt
        ho, wo = (pool_out(h), pool_out(w)) if kind in "BD" else (h, w)
        out = self._bordered(f"mixed.{parity}", nb, ho, wo, blk.cout, out_pad)
        flow = INC_FLOW[kind]
        c0, tmp = 0, {"in": cur}
        for j, (lname, src, dst) in enumerate(flow):
            if lname == "pool" and kind in "BD":                  # MaxPool2d(3, 2) of the input, a branch of the concatenation
                check(L.eegclip_maxpool16_cat(cur[0].data_ptr(), out[0].data_ptr(), nb, h, w, blk.cin, cur[0].shape[3], cur[1], out[0].shape[3], c0, out_pad, dt,
                                              raw_stream()), f"maxpool16_cat ({name}, {nb} x {h} x {w} x {blk.cin})")
                c0 += blk.cin
                continue
            if lname == "pool":                                   # avg_pool2d(3, 1, 1) of the input, pad channels included (they are zero)
                tmp["p"] = self._bordered("avg", nb, h, w, cur[0].shape[3], 0)
                check(L.eegclip_avgpool3x3_16(cur[0].data_ptr(), tmp["p"][0].data_ptr(), nb, h, w, cur[0].shape[3], cur[1], dt, raw_stream()),
                      f"avgpool3x3_16 ({name}, {nb} x {h} x {w} x {cur[0].shape[3]})")
                continue
            layer = getattr(blk, lname)
            if dst == "out":
                self._conv(f"{name}.{lname}", layer, tmp[src], out, c0, nb, h, w)
                c0 += layer.conv.out_channels
                continue
            # a temporary carries the border its reader pads by (readers of one temporary agree: the two halves of InceptionE's split read 1 x 3 and 3 x 1)
            rewritten = next((i for i in range(j + 1, len(flow)) if flow[i][2] == dst), len(flow) - 1)
            pad = max(max(getattr(blk, n).conv.padding) for n, s2, _ in flow[j + 1:rewritten + 1] if s2 == dst)
            tmp[dst] = self._bordered(f"tmp.{dst}", nb, h, w, layer.conv.out_channels, pad)
            self._conv(f"{name}.{lname}", layer, tmp[src], tmp[dst], 0, nb, h, w)
        assert c0 == blk.cout
        return out, ho, wo

    def _forward_chunk(self, x, out):
        """x: normalised by preprocess.inception_preprocess -> out (nb, 2048)"""
        (nb, _, H, W), L, dt = x.shape, lib(), self._dt
        ab = self._affine()
        blocks = [(n, getattr(self, n)) for n in self.order]
        f0 = self._frame("in", nb, (H, L.eegclip_convbncat16_in_width(W), 4))
        check(L.eegclip_pack_nchw16_affine(x.data_ptr(), f0.data_ptr(), ab[0].data_ptr(), ab[1].data_ptr(), nb, H, W, dt, raw_stream()),
              f"pack_nchw16_affine ({nb} x {H} x {W})")
        cur, h, w = (f0, 0), H, W
        # the stem: a frame's border is what its reader pads by (Conv2d_2b_3x3 pads by 1; the first Inception block's average pool reads a border of 1)
        for i, (name, _, cout, k, s, p) in enumerate(INC_STEM):
            ho, wo = conv_out(h, k, s, p), conv_out(w, k, s, p)
            nxt = self._bordered(f"stem.{i}", nb, ho, wo, cout, INC_STEM[i + 1][5] if i + 1 < len(INC_STEM) else 0)
            self._conv(name, getattr(self, name), cur, nxt, 0, nb, h, w)
            cur, h, w = nxt, ho, wo
            if name in ("Conv2d_2b_3x3", "Conv2d_4a_3x3"):    # maxpool1, maxpool2
                ho, wo = pool_out(h), pool_out(w)
                last = name == "Conv2d_4a_3x3"
                nxt = self._bordered(f"pool.{i}", nb, ho, wo, cout, 1 if last else 0)
                check(L.eegclip_maxpool16(cur[0].data_ptr(), nxt[0].data_ptr(), nb, h, w, cur[0].shape[3], 0, nxt[1], dt, raw_stream()),
                      f"maxpool16 ({nb} x {h} x {w} x {cur[0].shape[3]})")
                cur, h, w = nxt, ho, wo
        for idx, (name, blk) in enumerate(blocks):
            nxt_kind = blocks[idx + 1][1].kind if idx + 1 < len(blocks) else None
            cur, h, w = self._block(name, blk, cur, nb, h, w, 1 if nxt_kind in ("A", "C", "E") else 0, idx & 1)
        check(L.eegclip_avgpool16(cur[0].data_ptr(), out.data_ptr(), nb, h, w, self.out_features, dt, raw_stream()), f"avgpool16 ({nb} x {h} x {w})")


def inception_v3(**kw):
    """the InceptionV3 trunk of the metrics table's Inception row (torchvision's inception_v3 without AuxLogits and fc, transform_input=True), seeded weights"""
    return InceptionFeatures(blocks=(3, 4, 2), **kw)
