"""CPU-only checks of metric_nets.ResNetFeatures: torchvision's key layout and shapes, the seeded BatchNorm tensors, the packed weights' k order, the exports,
and the reference's own consistency (tests/resnet_ref.py) -- nothing here launches a kernel."""
import numpy as np
import pytest
import torch

import metric_nets_ref as MR
import resnet_ref as R
from eeg_image_decode_amd import _abi, metric_nets


def expected_keys(layers):
    """torchvision.models.resnet.ResNet(Bottleneck, layers).state_dict() without fc.*: name -> shape"""
    def bn(p, c):
        return {f"{p}.weight": (c,), f"{p}.bias": (c,), f"{p}.running_mean": (c,), f"{p}.running_var": (c,), f"{p}.num_batches_tracked": ()}
    keys = {"conv1.weight": (64, 3, 7, 7), **bn("bn1", 64)}
    cin = 64
    for s, (width, n) in enumerate(zip(R.WIDTHS, layers)):
        for i in range(n):
            p = f"layer{s + 1}.{i}"
            keys[f"{p}.conv1.weight"] = (width, cin, 1, 1)
            keys.update(bn(f"{p}.bn1", width))
            keys[f"{p}.conv2.weight"] = (width, width, 3, 3)
            keys.update(bn(f"{p}.bn2", width))
            keys[f"{p}.conv3.weight"] = (4 * width, width, 1, 1)
            keys.update(bn(f"{p}.bn3", 4 * width))
            if i == 0:
                keys[f"{p}.downsample.0.weight"] = (4 * width, cin, 1, 1)
                keys.update(bn(f"{p}.downsample.1", 4 * width))
            cin = 4 * width
    return keys


@pytest.fixture(scope="module")
def net():
    return metric_nets.swav_resnet50(dtype=torch.float16, device="cpu", seed=0)


def test_state_dict_is_torchvisions_resnet50_without_fc(net):
    sd, want = net.state_dict(), expected_keys((3, 4, 6, 3))
    assert list(sd) == list(want) and {k: tuple(v.shape) for k, v in sd.items()} == want
    convs = [k for k in sd if k.endswith("conv1.weight") or k.endswith("conv2.weight") or k.endswith("conv3.weight") or k.endswith("downsample.0.weight")]
    assert len(convs) == 53 and all(sd[k].dtype == torch.float16 for k in convs)
    assert sum(p.numel() for p in net.parameters()) == 23508032 and not any(p.requires_grad for p in net.parameters())      # ResNet-50's 25557032 less fc's 2049000
    assert all(v.dtype == torch.float32 for k, v in sd.items() if ".bn" in k or k.startswith("bn1.") or ".downsample.1." in k if v.is_floating_point())
    assert _abi.ABI_VERSION >= 24


def test_seeded_weights_exercise_batchnorm(net):
    """no BatchNorm is the identity: gamma in [0.5, 1.25], beta and the running mean in [-0.25, 0.25], the running variance in [0.5, 1.5], all spread out and
    exact in the net's dtype; convolution weights N(0, 2 / fan_in); one seed gives one net"""
    sd = net.state_dict()
    for k, v in sd.items():
        lo, hi = {"weight": (0.5, 1.25), "bias": (-0.25, 0.25), "running_mean": (-0.25, 0.25), "running_var": (0.5, 1.5)}.get(k.rsplit(".", 1)[1], (None, None))
        if v.dim() == 1 and lo is not None:
            assert float(v.min()) >= lo and float(v.max()) <= hi and float(v.max() - v.min()) > 0.5 * (hi - lo), k
            assert torch.equal(v, v.half().float()), k
        elif v.dim() == 4:
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]
            assert abs(float(v.float().std()) / (2.0 / fan_in) ** 0.5 - 1) < 0.05 and abs(float(v.float().mean())) < 0.1 * (2.0 / fan_in) ** 0.5, k
    again = metric_nets.swav_resnet50(dtype=torch.float16, device="cpu", seed=0).state_dict()
    other = metric_nets.swav_resnet50(dtype=torch.float16, device="cpu", seed=1).state_dict()
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    assert not torch.equal(sd["layer2.1.conv2.weight"], other["layer2.1.conv2.weight"]) and not torch.equal(sd["layer4.2.bn3.weight"], other["layer4.2.bn3.weight"])


def test_packed_weights_scale_and_shift(net):
    """[Cout][ky][kx][ci]; for the stem [64][ky][64] with element 4 kx + ci and zeros elsewhere (tests/metric_nets_ref.pack_weight); scale and shift are the
    BatchNorm formula in fp32; all three follow a load"""
    blk = net.layer2[0]
    for tag, conv, bn in (("conv1", net.conv1, net.bn1), ("a", blk.conv2, blk.bn2), ("b", blk.downsample[0], blk.downsample[1])):
        w, scale, shift = net._layer(tag, conv, bn)
        assert w.is_contiguous() and np.array_equal(MR.bits(w, torch.float16), MR.pack_weight(conv.weight.detach(), torch.float16))
        assert scale.dtype == shift.dtype == torch.float32
        want = bn.weight / torch.sqrt(bn.running_var + 1e-5)
        assert torch.equal(scale, want) and torch.equal(shift, bn.bias - bn.running_mean * want)
        assert net._layer(tag, conv, bn)[0] is w
    p0 = net._layer("conv1", net.conv1, net.bn1)[0].reshape(64, 7, 16, 4)
    assert not p0[:, :, 7:].any() and not p0[:, :, :, 3].any() and torch.equal(p0[5, 2, 6, :3], net.conv1.weight[5, :, 2, 6])
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict(dict(sd, **{"layer2.0.bn2.running_var": torch.full_like(sd["layer2.0.bn2.running_var"], 4.0 - 1e-5)}))
    assert torch.allclose(net._layer("a", blk.conv2, blk.bn2)[1], blk.bn2.weight / 2.0, rtol=1e-6)
    net.load_state_dict(sd)


def test_load_state_dict_prefixes_and_strictness(net):
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    full = {"module." + k: v for k, v in sd.items()}
    full.update({"module.projection_head.0.weight": torch.zeros(2, 2), "module.prototypes.weight": torch.zeros(2, 2), "fc.weight": torch.zeros(2, 2), "fc.bias": torch.zeros(2)})
    res = net.load_state_dict(full)
    assert not res.missing_keys and not res.unexpected_keys
    for bad in (dict(sd, extra=torch.zeros(1)), {k: v for k, v in sd.items() if k != "bn1.running_mean"}, dict(sd, **{"layer1.3.conv1.weight": torch.zeros(1)})):
        with pytest.raises(RuntimeError):
            net.load_state_dict(bad)
    res = net.load_state_dict({k: v for k, v in sd.items() if k != "bn1.bias"}, strict=False)
    assert res.missing_keys == ["bn1.bias"]
    with pytest.raises(metric_nets.EegclipError):
        metric_nets.ResNetFeatures(layers=(3, 4, 6), device="cpu")


def test_no_eager_path(net):
    with pytest.raises(metric_nets.EegclipError):
        net(torch.zeros(1, 3, 32, 32, dtype=torch.float16))


def test_reference_shapes_and_conditions():
    """the restatement at full depth on a tiny image: (N, 2048), the conditions the network tests assert (no activation near fp16's range, a live node), and
    the yardstick differs from fp64 by rounding only; the host's size arithmetic agrees with torch's"""
    small = metric_nets.ResNetFeatures(layers=(1, 1, 1, 1), dtype=torch.float16, device="cpu", seed=0)
    x = MR.normalised_images(2, 32, 40).half()
    ref, peak = R.features(x, small.state_dict(), (1, 1, 1, 1))
    yard = R.yardstick(x, small.state_dict(), (1, 1, 1, 1), torch.float16)
    assert tuple(ref.shape) == (2, 2048) and peak < 2.0 ** 12 and float((ref > 0).double().mean()) > 0.05
    assert 0 < MR.rel_l2(yard, ref) < 5e-3
    for n in (1, 2, 7, 33, 47, 224):
        t = torch.zeros(1, 1, n, n)
        assert metric_nets.conv_out(n, 7, 2, 3) == torch.nn.functional.conv2d(t, torch.zeros(1, 1, 7, 7), stride=2, padding=3).shape[2]
        assert metric_nets.pool_pad_out(n) == torch.nn.functional.max_pool2d(t, 3, 2, 1).shape[2]
    a, b = np.arange(6.0).reshape(2, 3) ** 2, np.array([[1.0, 0.0, 2.0], [3.0, 5.0, 4.0]])
    want = [1 - np.corrcoef(a[i], b[i])[0, 1] for i in range(2)]
    assert np.allclose(R.correlation(a, b), want, rtol=1e-12)
