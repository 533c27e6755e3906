"""CPU-only checks of metric_nets.InceptionFeatures: torchvision's key layout and shapes, the parameter count, the seeded tensors, the packed weights' order and
zero padding, the host's tables against the reference's and the reference's own conditions (tests/inception_ref.py) -- nothing here launches a kernel."""
import numpy as np
import pytest
import torch

import inception_ref as R
import metric_nets_ref as MR
from eeg_image_decode_amd import _abi, metric_nets


@pytest.fixture(scope="module")
def net():
    return metric_nets.inception_v3(dtype=torch.float16, device="cpu", seed=0)


def test_state_dict_is_torchvisions_inception3_without_auxlogits_and_fc(net):
    sd, want = net.state_dict(), R.keys(R.FULL)
    assert list(sd) == list(want) and {k: tuple(v.shape) for k, v in sd.items()} == want
    assert net.blocks == (3, 4, 2) and net.transform_input and net.out_features == 2048
    convs = [m for m in net.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == R.CONVS == 94 and all(c.bias is None for c in convs)
    assert sum(p.numel() for p in net.parameters()) == R.PARAMS == R.param_count() == 21785568 == 27161264 - 2049000 - 3326696
    assert not any(p.requires_grad for p in net.parameters())
    assert "Conv2d_1a_3x3.conv.weight" in sd and tuple(sd["Mixed_6b.branch7x7dbl_3.bn.running_var"].shape) == (128,)
    assert tuple(sd["Mixed_6b.branch7x7_2.conv.weight"].shape) == (128, 128, 1, 7) and tuple(sd["Mixed_7c.branch3x3dbl_3b.conv.weight"].shape) == (384, 384, 3, 1)
    assert net.Mixed_6c.branch7x7dbl_2.conv.padding == (3, 0) and net.Mixed_7b.branch3x3_2a.conv.padding == (0, 1)
    bn = [k for k, v in sd.items() if v.dim() == 1]
    assert len(bn) == 4 * 94 and all(sd[k].dtype == torch.float32 for k in bn) and all(v.dtype == torch.float16 for v in sd.values() if v.dim() == 4)
    assert all(m.eps == 1e-3 for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    assert _abi.ABI_VERSION >= 26 and R.launch_count() == 109
    for blocks in ((1, 1, 1), (2, 1, 1), (1, 3, 2)):
        small = metric_nets.InceptionFeatures(blocks=blocks, device="cpu")
        assert {k: tuple(v.shape) for k, v in small.state_dict().items()} == R.keys(blocks) and small.out_features == 2048
    one = metric_nets.InceptionFeatures(blocks=(1, 1, 1), device="cpu")
    assert (one.Mixed_6a.cin, one.Mixed_6a.cout, one.Mixed_6b.cin, one.Mixed_7a.cout) == (256, 736, 736, 1280)
    assert (net.Mixed_5c.cout, net.Mixed_6a.cin, net.Mixed_6a.cout, net.Mixed_7a.cout) == (288, 288, 768, 1280)
    for bad in ((3, 4), (0, 4, 2), (4, 4, 2), (3, 5, 2), (3, 4, 3)):
        with pytest.raises(metric_nets.EegclipError):
            metric_nets.InceptionFeatures(blocks=bad, device="cpu")


def test_host_tables_equal_the_references(net):
    """the product's layer table and launch flow, written independently of tests/inception_ref.py's, describe the same net: every layer's shape, and every
    block's slices in the order of concatenation"""
    for blocks in (R.FULL, (1, 1, 1)):
        n = metric_nets.InceptionFeatures(blocks=blocks, device="cpu")
        assert n.order == [name for name, *_ in R.plan(blocks)]
        for name, kind, layers, cout in R.plan(blocks):
            blk = getattr(n, name)
            assert blk.kind == kind and blk.cout == cout
            for lname, cin, co, k, s, p in layers:
                c = getattr(blk, lname).conv
                assert (c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding) == (cin, co, k, (s, s), p), (name, lname)
            flow = metric_nets.INC_FLOW[kind]
            assert sorted(l for l, _, _ in flow if l != "pool") == sorted(l[0] for l in layers) and sum(1 for l, _, _ in flow if l == "pool") == 1
    assert metric_nets.MIN_SIDE_INCEPTION == 75


def test_seeded_weights(net):
    """BatchNorm away from the identity and exact in the net's dtype; convolution weights N(0, 2 / fan_in); one seed gives one net"""
    sd = net.state_dict()
    for k, v in sd.items():
        leaf = k.rsplit(".", 1)[1]
        if v.dim() == 1:
            lo, hi = {"weight": (0.7, 1.4), "bias": (-0.25, 0.25), "running_mean": (-0.25, 0.25), "running_var": (0.5, 1.5)}[leaf]
            assert float(v.min()) >= lo - 1e-3 and float(v.max()) <= hi + 1e-3 and float(v.max() - v.min()) > 0.5 * (hi - lo), k
            assert torch.equal(v, v.half().float()), k
        elif v.dim() == 4:
            fan_in, n = v.shape[1] * v.shape[2] * v.shape[3], v.numel()
            assert abs(float(v.float().std()) / (2.0 / fan_in) ** 0.5 - 1) <= 4 / (2 * n) ** 0.5 + 2.0 ** -10, k
    again = metric_nets.inception_v3(dtype=torch.float16, device="cpu", seed=0).state_dict()
    other = metric_nets.inception_v3(dtype=torch.float16, device="cpu", seed=1).state_dict()
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    assert not torch.equal(sd["Mixed_6d.branch7x7_2.conv.weight"], other["Mixed_6d.branch7x7_2.conv.weight"])


def test_packed_weights_and_zero_padding(net):
    """the first layer [64][ky][64] with element 4 kx + ci, rows 32 .. 63 zero; any other layer [pad64(Cout)][KH][KW][input frame's channels], zero in the
    padding; scale and shift the BatchNorm formula with eps = 0.001 in fp32, zero in the padding; all follow a load"""
    w, scale, shift = net._layer("s", net.Conv2d_1a_3x3, 4)
    conv, bn = net.Conv2d_1a_3x3.conv, net.Conv2d_1a_3x3.bn
    assert tuple(w.shape) == (64, 192) and w.is_contiguous() and not w[32:].any()
    assert np.array_equal(MR.bits(w, torch.float16), R.pack_weight(conv.weight.detach(), 64, 3, torch.float16))
    p0 = w.reshape(64, 3, 16, 4)
    assert not p0[:, :, 3:].any() and not p0[:, :, :, 3].any() and torch.equal(p0[5, 2, 1, :3], conv.weight[5, :, 2, 1])
    want = bn.weight / torch.sqrt(bn.running_var + 1e-3)
    assert scale.dtype == shift.dtype == torch.float32 and tuple(scale.shape) == tuple(shift.shape) == (64,)
    assert torch.equal(scale[:32], want) and torch.equal(shift[:32], bn.bias - bn.running_mean * want) and not scale[32:].any() and not shift[32:].any()
    layer = net.Mixed_6c.branch7x7_2                              # 160 -> 160, 1 x 7, reading a 192-channel frame
    w, scale, _ = net._layer("c", layer, 192)
    assert tuple(w.shape) == (192, 7 * 192) and not w[160:].any() and not scale[160:].any() and bool((scale[:160] != 0).all())
    p = w.reshape(192, 1, 7, 192)
    assert not p[..., 160:].any() and torch.equal(p[33, 0, 5, :160], layer.conv.weight[33, :, 0, 5])
    assert np.array_equal(MR.bits(w, torch.float16), R.pack_weight(layer.conv.weight.detach(), 192, 192, torch.float16))
    layer = net.Mixed_6a.branch3x3                                # reads Mixed_5d's 288 channels in a 320-channel frame
    w, _, _ = net._layer("b", layer, 320)
    assert tuple(w.shape) == (384, 9 * 320) and not w.reshape(384, 3, 3, 320)[..., 288:].any()
    assert net._layer("b", layer, 320)[0] is w
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict(dict(sd, **{"Mixed_6a.branch3x3.bn.running_var": torch.full_like(sd["Mixed_6a.branch3x3.bn.running_var"], 4.0 - 1e-3)}))
    assert torch.allclose(net._layer("b", layer, 320)[1], layer.bn.weight / 2.0, rtol=1e-6)
    net.load_state_dict(sd)
    ab = net._affine()
    assert torch.equal(ab[0], R.affine(True)[0]) and torch.equal(ab[1], R.affine(True)[1])
    off = metric_nets.InceptionFeatures(blocks=(1, 1, 1), transform_input=False, device="cpu")._affine()
    assert off.tolist() == [[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]]


def test_load_state_dict_drops_auxlogits_and_fc_and_is_strict(net):
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    assert any(k.endswith("num_batches_tracked") for k in sd)
    res = net.load_state_dict(dict(sd, **{"fc.weight": torch.zeros(2, 2), "fc.bias": torch.zeros(2), "AuxLogits.conv0.conv.weight": torch.zeros(1),
                                          "AuxLogits.conv1.bn.num_batches_tracked": torch.tensor(0), "AuxLogits.fc.weight": torch.zeros(3)}))
    assert not res.missing_keys and not res.unexpected_keys
    for bad in (dict(sd, extra=torch.zeros(1)), {k: v for k, v in sd.items() if k != "Conv2d_2a_3x3.bn.running_mean"}, {"module." + k: v for k, v in sd.items()},
                dict(sd, **{"Mixed_5b.branch5x5_2.conv.weight": torch.zeros(1)}), {k: v for k, v in sd.items() if k != "Mixed_7c.branch_pool.conv.weight"}):
        with pytest.raises(RuntimeError):
            net.load_state_dict(bad)
    res = net.load_state_dict({k: v for k, v in sd.items() if k != "Mixed_7c.branch_pool.bn.bias"}, strict=False)
    assert res.missing_keys == ["Mixed_7c.branch_pool.bn.bias"]


def test_no_eager_path_and_exports(net):
    import eeg_image_decode_amd as pkg
    from eeg_image_decode_amd import metrics, preprocess
    with pytest.raises(metric_nets.EegclipError):
        net(torch.zeros(1, 3, 75, 75, dtype=torch.float16))
    for name, mod in (("InceptionFeatures", metric_nets), ("inception_v3", metric_nets), ("inception_two_way", metrics), ("inception_preprocess", preprocess)):
        assert getattr(pkg, name) is getattr(mod, name) and name in pkg.__all__
    for fn in ("eegclip_convbncat16", "eegclip_convbncat16_in_width", "eegclip_avgpool3x3_16", "eegclip_maxpool16_cat", "eegclip_pack_nchw16_affine"):
        assert fn in _abi.PROTOTYPES
    assert _abi.PARAMS["eegclip_maxpool16_cat"] == ("in_", "out", "N", "H", "W", "C", "in_stride", "in_pad", "out_stride", "out_c0", "out_pad", "dtype", "stream")


def test_reference_conditions_on_a_small_net():
    """the restatement on the smallest image: (N, 2048), the conditions the network tests assert, a yardstick that differs from fp64 by rounding only, and
    transform_input as torchvision writes it"""
    small = metric_nets.InceptionFeatures(blocks=(1, 1, 1), dtype=torch.float16, device="cpu", seed=0)
    x = MR.normalised_images(2, 75, 75).half()
    ref, peak = R.features(x, small.state_dict(), (1, 1, 1))
    yard = R.yardstick(x, small.state_dict(), (1, 1, 1), torch.float16)
    assert tuple(ref.shape) == (2, 2048) and peak < 2.0 ** 12 and float((ref > 0).double().mean()) > 0.05
    assert 0 < MR.rel_l2(yard, ref) < 5e-3
    off, _ = R.features(x, small.state_dict(), (1, 1, 1), transform_input=False)
    assert not torch.equal(off, ref)
    a, b = R.affine(True, torch.float64)
    t = torch.stack([x[:, c].double() * (R.STD[c] / 0.5) + (R.MEAN[c] - 0.5) / 0.5 for c in range(3)], 1)       # torchvision's _transform_input
    assert torch.allclose(x.double() * a[None, :, None, None] + b[None, :, None, None], t, atol=1e-6)
    for n in (75, 83, 107, 342):
        sizes = [n]
        for k, s, p in ((3, 2, 0), (3, 1, 0), (3, 1, 1), (3, 2, 0), (1, 1, 0), (3, 1, 0), (3, 2, 0), (3, 2, 0), (3, 2, 0)):
            sizes.append(metric_nets.conv_out(sizes[-1], k, s, p))
        assert sizes[-1] >= 1, sizes
    assert [metric_nets.conv_out(s, 3, 2, 0) for s in (74, 36)] == [36, 17] and metric_nets.pool_out(2) == 0
