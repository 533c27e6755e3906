"""The feature nets of the reference's metrics table that this package carries: torchvision's AlexNet up to `features.11`, on HIP kernels
(csrc/metric_nets.hip).  The metrics notebooks under Generation/ (copies of MindEye's Reconstruction_Metrics) take alexnet(weights=IMAGENET1K_V1)
through create_feature_extractor at `features.4` (the AlexNet(2) row) and `features.11` (the AlexNet(5) row) and score both by two-way identification.

AlexNetFeatures is the architecture in torchvision's key layout with seeded random weights, as every model of this package: load the real checkpoint
with load_state_dict(torchvision.models.alexnet(weights="IMAGENET1K_V1").state_dict()).  One forward of a chunk of images is 8 launches: the NCHW ->
frame pack, five convolution + bias + ReLU launches and two max-pools; the third pool (`features.12`) and the classifier are never run.  There is no
eager path.  `lib`, `require_cuda` and `raw_stream` are called as this module's globals (tests/emu_patch.py swaps them).
"""
import torch
from torch import nn

from . import _abi
from ._lib import EegclipError, check, lib, raw_stream, require_cuda
from .ops16 import PackedWeights, dtype_code, seeded_parameters

# torchvision/models/alexnet.py: features.{index}: (Cin, Cout, kernel, stride, padding); a ReLU follows each, MaxPool2d(3, 2) follows the ReLUs of 0 and 3
CONVS = {"0": (3, 64, 11, 4, 2), "3": (64, 192, 5, 1, 2), "6": (192, 384, 3, 1, 1), "8": (384, 256, 3, 1, 1), "10": (256, 256, 3, 1, 1)}
NODES = ("features.4", "features.11")           # the outputs of the ReLUs behind features.3 and features.10
_MIN_SIDE = {"features.4": 15, "features.11": 31}


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def pool_out(n):
    return (n - 3) // 2 + 1


class AlexNetFeatures(nn.Module):
    def __init__(self, dtype=torch.float16, device="cuda", seed=0):
        super().__init__()
        with seeded_parameters(self, dtype, seed=seed):           # (initialised on the host: one seed gives one set of weights on every device)
            self.features = nn.ModuleDict({i: nn.Conv2d(cin, cout, k, s, p) for i, (cin, cout, k, s, p) in CONVS.items()})
        self.to(device)
        self._packed, self._frames = PackedWeights(), {}

    @property
    def dtype(self):
        return self.features["0"].weight.dtype

    @property
    def device(self):
        return self.features["0"].weight.device

    def load_state_dict(self, state_dict, strict=True, **kw):
        """the ten keys features.{0,3,6,8,10}.{weight,bias}; a full torchvision AlexNet state dict loads too: its classifier.* keys are dropped"""
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("classifier.")}, strict=strict, **kw)

    def _weight(self, i):
        """features.i's weight in the kernel's k order: [Cout][ky][kx][ci]; for the 3-channel layer [Cout][ky][64], element 4 kx + ci, the rest zero"""
        conv = self.features[i]

        def make():
            w = conv.weight.detach().permute(0, 2, 3, 1)          # (Cout, ky, kx, ci)
            if w.shape[3] != 3:
                return w.reshape(w.shape[0], -1).contiguous()
            p = torch.zeros(w.shape[0], w.shape[1], 16, 4, dtype=w.dtype, device=w.device)
            p[:, :, :w.shape[2], :3] = w
            return p.reshape(w.shape[0], -1)
        return self._packed.get(i, (conv.weight,), make)

    def _frame(self, tag, nb, shape):
        """a zero-bordered frame for `nb` images, kept between calls: no launch writes a border, so the interior is simply overwritten"""
        f = self._frames.get(tag)
        if f is None or f.shape[0] < nb or tuple(f.shape[1:]) != shape or f.dtype != self.dtype or f.device != self.device:
            f = self._frames[tag] = torch.zeros((nb, *shape), dtype=self.dtype, device=self.device)
        return f[:nb]

    def _conv(self, i, src, out, nb, Hi, Wi, out_pad):
        cin, cout, k, s, p = CONVS[i]
        d = _abi.ConvRelu16Desc(in_=src.data_ptr(), W=self._weight(i).data_ptr(), bias=self.features[i].bias.data_ptr(), out=out.data_ptr(), N=nb, Hi=Hi, Wi=Wi,
                                Cin=cin, Cout=cout, KS=k, stride=s, pad=p, out_pad=out_pad, dtype=dtype_code(self.dtype))
        check(lib().eegclip_convrelu16(d, raw_stream()), f"convrelu16 (features.{i}, {nb} x {Hi} x {Wi})")

    def _pool(self, src, out, nb, H, W, C, out_pad):
        check(lib().eegclip_maxpool16(src.data_ptr(), out.data_ptr(), nb, H, W, C, 0, out_pad, dtype_code(self.dtype), raw_stream()), f"maxpool16 ({nb} x {H} x {W} x {C})")

    def forward(self, x, nodes=NODES, chunk=64):
        """x: (B, 3, H, W), normalised (preprocess.alexnet_preprocess), of this net's dtype and on its device -> {node: (B, C, h, w)} for the nodes asked
        for, what torchvision's create_feature_extractor(alexnet, nodes) returns: `features.4` (B, 192, h2, w2), `features.11` (B, 256, h3, w3) -- (31, 31)
        and (15, 15) at 256 x 256.  Each is a permuted view of the kernels' NHWC result.  The batch runs `chunk` images at a time through frames that are
        reused, so only the results grow with B."""
        nodes = (nodes,) if isinstance(nodes, str) else tuple(nodes)
        if not nodes or any(n not in NODES for n in nodes):
            raise EegclipError(f"AlexNetFeatures returns {NODES}; got {nodes}")
        require_cuda(x, "x")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1 or x.dtype != self.dtype or x.device != self.device:
            raise EegclipError(f"AlexNetFeatures takes (B, 3, H, W) {self.dtype} on {self.device}; got {tuple(x.shape)} {x.dtype} on {x.device}")
        B, _, H, W = x.shape
        need = max(_MIN_SIDE[n] for n in nodes)
        if min(H, W) < need or chunk < 1:
            raise EegclipError(f"{' and '.join(nodes)} need images of at least {need} x {need} and chunk >= 1; got {H} x {W}, chunk {chunk}")
        x = x.contiguous()
        L, dt = lib(), dtype_code(self.dtype)
        h1, w1 = conv_out(H, 11, 4, 2), conv_out(W, 11, 4, 2)
        h2, w2 = pool_out(h1), pool_out(w1)
        deep = "features.11" in nodes
        out4 = torch.empty(B, h2, w2, 192, dtype=self.dtype, device=self.device) if "features.4" in nodes else None
        if deep:
            h3, w3 = pool_out(h2), pool_out(w2)
            out11 = torch.empty(B, h3, w3, 256, dtype=self.dtype, device=self.device)
        wf = L.eegclip_convrelu16_in_width(W)
        for b0 in range(0, B, chunk):
            nb = min(chunk, B - b0)
            f0 = self._frame("in", nb, (H + 4, wf, 4))
            check(L.eegclip_pack_nchw16(x[b0:b0 + nb].data_ptr(), f0.data_ptr(), nb, H, W, dt, raw_stream()), f"pack_nchw16 ({nb} x {H} x {W})")
            a1 = self._frame("c0", nb, (h1, w1, 64))
            self._conv("0", f0, a1, nb, H, W, 0)
            p1 = self._frame("p1", nb, (h2 + 4, w2 + 4, 64))
            self._pool(a1, p1, nb, h1, w1, 64, 2)
            a2 = out4[b0:b0 + nb] if out4 is not None else self._frame("c3", nb, (h2, w2, 192))
            self._conv("3", p1, a2, nb, h2, w2, 0)
            if not deep:
                continue
            p2 = self._frame("p2", nb, (h3 + 2, w3 + 2, 192))
            self._pool(a2, p2, nb, h2, w2, 192, 1)
            a3 = self._frame("c6", nb, (h3 + 2, w3 + 2, 384))
            self._conv("6", p2, a3, nb, h3, w3, 1)
            a4 = self._frame("c8", nb, (h3 + 2, w3 + 2, 256))
            self._conv("8", a3, a4, nb, h3, w3, 1)
            self._conv("10", a4, out11[b0:b0 + nb], nb, h3, w3, 0)
        out = {}
        if out4 is not None:
            out["features.4"] = out4.permute(0, 3, 1, 2)
        if deep:
            out["features.11"] = out11.permute(0, 3, 1, 2)
        return out
