"""CPU-only checks of metric_nets.EfficientNetFeatures: torchvision's key layout and shapes, the parameter count, the seeded tensors, the packed weights' order
and zero padding, the host's size arithmetic and the reference's own consistency (tests/effnet_ref.py) -- nothing here launches a kernel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import effnet_ref as R
import metric_nets_ref as MR
from eeg_image_decode_amd import _abi, metric_nets


def expected_keys(layers):
    """torchvision.models.efficientnet_b1().state_dict() without classifier.* (for B1's depths): name -> shape, written out from the stage table --
    (expand ratio, kernel, stride, input channels, output channels) = (1,3,1,32,16), (6,3,2,16,24), (6,5,2,24,40), (6,3,2,40,80), (6,5,1,80,112), (6,5,2,112,192),
    (6,3,1,192,320); Conv2dNormActivation is `.0` convolution without bias, `.1` BatchNorm; the squeeze has max(1, block input channels // 4) units"""
    def conv_bn(p, cout, cin, k):
        return {f"{p}.0.weight": (cout, cin, k, k), f"{p}.1.weight": (cout,), f"{p}.1.bias": (cout,), f"{p}.1.running_mean": (cout,), f"{p}.1.running_var": (cout,),
                f"{p}.1.num_batches_tracked": ()}

    def se(p, c, sq):
        return {f"{p}.fc1.weight": (sq, c, 1, 1), f"{p}.fc1.bias": (sq,), f"{p}.fc2.weight": (c, sq, 1, 1), f"{p}.fc2.bias": (c,)}
    table = ((1, 3, 1, 32, 16), (6, 3, 2, 16, 24), (6, 5, 2, 24, 40), (6, 3, 2, 40, 80), (6, 5, 1, 80, 112), (6, 5, 2, 112, 192), (6, 3, 1, 192, 320))
    keys = conv_bn("features.0", 32, 3, 3)
    for s, ((expand, k, _, cin, cout), n) in enumerate(zip(table, layers)):
        for i in range(n):
            p, c = f"features.{s + 1}.{i}.block", (cin if i == 0 else cout)
            ce, j = c * expand, 0
            if expand != 1:
                keys.update(conv_bn(f"{p}.0", ce, c, 1))
                j = 1
            keys.update(conv_bn(f"{p}.{j}", ce, 1, k))
            keys.update(se(f"{p}.{j + 1}", ce, max(1, c // 4)))
            keys.update(conv_bn(f"{p}.{j + 2}", cout, ce, 1))
    keys.update(conv_bn("features.8", 1280, 320, 1))
    return keys


@pytest.fixture(scope="module")
def net():
    return metric_nets.efficientnet_b1(dtype=torch.float16, device="cpu", seed=0)


def test_state_dict_is_torchvisions_efficientnet_b1_without_classifier(net):
    sd, want = net.state_dict(), expected_keys((2, 3, 3, 4, 4, 5, 2))
    assert list(sd) == list(want) and {k: tuple(v.shape) for k, v in sd.items()} == want
    assert net.layers == (2, 3, 3, 4, 4, 5, 2) and len(net.blocks()) == 23
    assert sum(p.numel() for p in net.parameters()) == 6513184 and not any(p.requires_grad for p in net.parameters())   # torchvision's 7794184 less the classifier's 1281000
    assert sorted({v.shape[0] for k, v in sd.items() if k.endswith("fc1.bias")}) == [4, 6, 8, 10, 20, 28, 48, 80]
    bn = [k for k, v in sd.items() if v.dim() == 1 and ".fc" not in k]
    assert len(bn) == 4 * (2 + 2 * 2 + 3 * 21) and all(sd[k].dtype == torch.float32 for k in bn)
    assert all(v.dtype == torch.float16 for k, v in sd.items() if v.dim() == 4 or ".fc" in k)
    assert all(m.eps == 1e-5 for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    assert _abi.ABI_VERSION >= 25
    for layers in ((1,) * 7, (1, 2, 2, 3, 3, 4, 1)):
        small = metric_nets.EfficientNetFeatures(layers=layers, device="cpu").state_dict()
        assert {k: tuple(v.shape) for k, v in small.items()} == expected_keys(layers)
    for bad in ((2, 3, 3, 4, 4, 5), (2, 3, 3, 4, 4, 5, 0), (1,) * 8):
        with pytest.raises(metric_nets.EegclipError):
            metric_nets.EfficientNetFeatures(layers=bad, device="cpu")


def normal(t, mean, var):
    """a sample of n values of N(mean, var), each within 4 standard errors (sigma / sqrt(n) for the mean, sigma / sqrt(2 n) for the standard deviation) plus
    fp16's rounding: the draws are seeded, so this is a fixed statement about them, loose enough to hold for any seed"""
    n, sigma = t.numel(), var ** 0.5
    return abs(float(t.mean()) - mean) <= 4 * sigma / n ** 0.5 + 2.0 ** -10 * max(abs(mean), sigma) and abs(float(t.std()) / sigma - 1) <= 4 / (2 * n) ** 0.5 + 2.0 ** -10


def test_seeded_weights(net):
    """BatchNorm away from the identity, in ResNetFeatures' ranges and exact in the net's dtype; convolution weights N(0, 2 / fan_in) with fan_in =
    (Cin / groups) k^2; fc1.weight N(0, 1 / C), fc1.bias N(0, 0.25), fc2.weight N(0, 4 / sq), fc2.bias 2 + N(0, 0.25): the gates are mostly open; one seed
    gives one net"""
    sd = net.state_dict()
    pooled = {"fc1.bias": [], "fc2.bias": []}
    for k, v in sd.items():
        leaf = k.rsplit(".", 1)[1]
        if ".fc" in k:
            f = v.float()
            if leaf == "weight":
                var = 1.0 / v.shape[1] if "fc1" in k else 4.0 / v.shape[1]
                assert normal(f, 0.0, var), k
            else:
                pooled[k.rsplit(".", 2)[1] + ".bias"].append(f)
        elif v.dim() == 1:
            lo, hi = {"weight": (0.5, 1.25), "bias": (-0.25, 0.25), "running_mean": (-0.25, 0.25), "running_var": (0.5, 1.5)}[leaf]
            assert float(v.min()) >= lo and float(v.max()) <= hi and float(v.max() - v.min()) > 0.5 * (hi - lo), k
            assert torch.equal(v, v.half().float()), k
        elif v.dim() == 4:
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]          # (the state dict's second dimension is already Cin / groups)
            assert normal(v.float(), 0.0, 2.0 / fan_in), k
    b1, b2 = torch.cat(pooled["fc1.bias"]), torch.cat(pooled["fc2.bias"])
    assert normal(b1, 0.0, 0.25) and normal(b2, 2.0, 0.25) and float((b2 > 0.5).float().mean()) > 0.99
    again = metric_nets.efficientnet_b1(dtype=torch.float16, device="cpu", seed=0).state_dict()
    other = metric_nets.efficientnet_b1(dtype=torch.float16, device="cpu", seed=1).state_dict()
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    assert not torch.equal(sd["features.3.1.block.1.0.weight"], other["features.3.1.block.1.0.weight"])
    assert not torch.equal(sd["features.6.2.block.2.fc2.bias"], other["features.6.2.block.2.fc2.bias"])


def test_packed_weights_and_zero_padding(net):
    """the stem [64][ky][64] with element 4 kx + ci, rows 32 .. 63 zero; a 1 x 1 layer [pad64(Cout)][pad64(Cin)]; the depthwise weight [ky][kx][pad64(C)]; the
    squeeze's matrices with zero padded columns / rows; padded scale and shift are zero, the others the BatchNorm formula in fp32; all follow a load"""
    conv, bn = net.features[0]
    w, scale, shift = net._layer("features.0", conv, bn)
    assert tuple(w.shape) == (64, 192) and w.is_contiguous()
    assert np.array_equal(MR.bits(w[:32], torch.float16), MR.pack_weight(conv.weight.detach(), torch.float16)) and not w[32:].any()
    p0 = w.reshape(64, 3, 16, 4)
    assert not p0[:, :, 3:].any() and not p0[:, :, :, 3].any() and torch.equal(p0[5, 2, 1, :3], conv.weight[5, :, 2, 1])
    want = bn.weight / torch.sqrt(bn.running_var + 1e-5)
    assert scale.dtype == shift.dtype == torch.float32 and tuple(scale.shape) == tuple(shift.shape) == (64,)
    assert torch.equal(scale[:32], want) and torch.equal(shift[:32], bn.bias - bn.running_mean * want) and not scale[32:].any() and not shift[32:].any()
    blk = net.features[3][0]                                   # 24 -> 144 -> (5 x 5, stride 2) -> 40, squeeze 6
    assert (blk.cin, blk.cexp, blk.cout, blk.k, blk.stride, blk.residual) == (24, 144, 40, 5, 2, False) and net.features[3][1].residual
    w, scale, shift = net._layer("e", blk.block[0][0], blk.block[0][1])
    assert tuple(w.shape) == (192, 64) and torch.equal(w[:144, :24], blk.block[0][0].weight[:, :, 0, 0]) and not w[144:].any() and not w[:, 24:].any()
    assert tuple(scale.shape) == (192,) and not scale[144:].any() and not shift[144:].any() and bool((scale[:144] != 0).all())
    assert net._layer("e", blk.block[0][0], blk.block[0][1])[0] is w
    dw, dscale, dshift = net._depthwise("d", blk.block[1][0], blk.block[1][1])
    assert tuple(dw.shape) == (5, 5, 192) and dw.is_contiguous() and not dw[:, :, 144:].any() and not dscale[144:].any() and not dshift[144:].any()
    assert np.array_equal(MR.bits(dw[:, :, :144], torch.float16), R.dw_weight(blk.block[1][0].weight.detach(), torch.float16))
    assert torch.equal(dw[3, 1, 77], blk.block[1][0].weight[77, 0, 3, 1])
    se = blk.block[2]
    w1, b1, w2, b2 = net._se("s", se)
    assert tuple(w1.shape) == (6, 192) and tuple(b1.shape) == (6,) and tuple(w2.shape) == (192, 6) and tuple(b2.shape) == (192,)
    assert torch.equal(w1[:, :144], se.fc1.weight[:, :, 0, 0]) and not w1[:, 144:].any() and torch.equal(w2[:144], se.fc2.weight[:, :, 0, 0]) and not w2[144:].any()
    assert torch.equal(b2[:144], se.fc2.bias) and not b2[144:].any() and torch.equal(b1, se.fc1.bias)
    w, scale, _ = net._layer("p", blk.block[3][0], blk.block[3][1])
    assert tuple(w.shape) == (64, 192) and not w[40:].any() and not w[:, 144:].any() and not scale[40:].any()
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict(dict(sd, **{"features.3.0.block.1.1.running_var": torch.full_like(sd["features.3.0.block.1.1.running_var"], 4.0 - 1e-5)}))
    assert torch.allclose(net._depthwise("d", blk.block[1][0], blk.block[1][1])[1][:144], blk.block[1][1].weight / 2.0, rtol=1e-6)
    net.load_state_dict(sd)
    assert [metric_nets.pad64(c) for c in (1, 16, 64, 65, 144, 1920)] == [64, 64, 64, 128, 192, 1920]


def test_load_state_dict_drops_the_classifier_and_is_strict(net):
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    res = net.load_state_dict(dict(sd, **{"classifier.1.weight": torch.zeros(2, 2), "classifier.1.bias": torch.zeros(2)}))
    assert not res.missing_keys and not res.unexpected_keys
    for bad in (dict(sd, extra=torch.zeros(1)), {k: v for k, v in sd.items() if k != "features.0.1.running_mean"},
                dict(sd, **{"features.1.2.block.0.0.weight": torch.zeros(1)}), {k: v for k, v in sd.items() if k != "features.7.1.block.2.fc1.weight"}):
        with pytest.raises(RuntimeError):
            net.load_state_dict(bad)
    res = net.load_state_dict({k: v for k, v in sd.items() if k != "features.8.1.bias"}, strict=False)
    assert res.missing_keys == ["features.8.1.bias"]


def test_no_eager_path(net):
    with pytest.raises(metric_nets.EegclipError):
        net(torch.zeros(1, 3, 32, 32, dtype=torch.float16))


def test_size_arithmetic_and_reference_conditions():
    """the host's output sizes are F.conv2d's for k in {3, 5}, stride in {1, 2}; the restatement on a tiny image: (N, 1280), the conditions the network tests
    assert, a yardstick that differs from fp64 by rounding only; the one-launch references agree with the chain's formulas"""
    for n in (1, 2, 7, 33, 47, 255):
        t = torch.zeros(1, 1, n, n)
        for k in (3, 5):
            for s in (1, 2):
                assert metric_nets.conv_out(n, k, s, k // 2) == F.conv2d(t, torch.zeros(1, 1, k, k), stride=s, padding=k // 2).shape[2], (n, k, s)
    small = metric_nets.EfficientNetFeatures(layers=(1,) * 7, dtype=torch.float16, device="cpu", seed=0)
    x = MR.normalised_images(2, 17, 23).half()
    ref, peak = R.features(x, small.state_dict(), (1,) * 7)
    yard = R.yardstick(x, small.state_dict(), (1,) * 7, torch.float16)
    assert tuple(ref.shape) == (2, 1280) and peak < 2.0 ** 12 and float((ref > 0).double().mean()) > 0.05
    assert 0 < MR.rel_l2(yard, ref) < 5e-3
    g = torch.Generator().manual_seed(0)
    mean, w1, b1, w2, b2 = (torch.randn(s, generator=g).double() for s in ((2, 8), (3, 8, 1, 1), (3,), (8, 3, 1, 1), (8,)))
    h = mean @ w1[:, :, 0, 0].t() + b1
    want = torch.sigmoid((h * torch.sigmoid(h)) @ w2[:, :, 0, 0].t() + b2)
    assert torch.allclose(R.se_gate(mean, w1, b1, w2, b2), want, rtol=1e-12)
    assert R.block_keys(small.state_dict(), "features.1.0")[0] is None and R.block_keys(small.state_dict(), "features.2.0")[0] == "features.2.0.block.0"
