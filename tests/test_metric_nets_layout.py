"""CPU-only checks of eeg_image_decode_amd/metric_nets.py: torchvision's key layout, the packed weights' k order, state-dict strictness, the sizes the host
computes, and the reference's own consistency (tests/metric_nets_ref.py) -- nothing here launches a kernel."""
import numpy as np
import pytest
import torch

import metric_nets_ref as R
from eeg_image_decode_amd import _abi, metric_nets, preprocess


@pytest.fixture(scope="module")
def net():
    return metric_nets.AlexNetFeatures(dtype=torch.float16, device="cpu", seed=0)


def test_state_dict_is_torchvisions_feature_keys(net):
    sd = net.state_dict()
    assert list(sd) == [f"features.{i}.{p}" for i, *_ in R.LAYERS for p in ("weight", "bias")]
    for i, cin, cout, k, s, p in R.LAYERS:
        assert tuple(sd[f"features.{i}.weight"].shape) == (cout, cin, k, k) and tuple(sd[f"features.{i}.bias"].shape) == (cout,)
        assert metric_nets.CONVS[i] == (cin, cout, k, s, p)
    assert all(v.dtype == torch.float16 and not v.requires_grad for v in sd.values())
    again = metric_nets.AlexNetFeatures(dtype=torch.float16, device="cpu", seed=0).state_dict()
    other = metric_nets.AlexNetFeatures(dtype=torch.float16, device="cpu", seed=1).state_dict()
    assert all(torch.equal(sd[k], again[k]) for k in sd) and not torch.equal(sd["features.3.weight"], other["features.3.weight"])
    assert _abi.ABI_VERSION >= 22


def test_packed_weights_are_the_kernels_k_order(net):
    """[Cout][ky][kx][ci]; for the 3-channel layer [Cout][ky][64] with element 4 kx + ci and zeros elsewhere -- the layout tests/metric_nets_ref.pack_weight
    hands the kernel tests; repacked after a load"""
    for i, cin, cout, k, _, _ in R.LAYERS:
        w = net.features[i].weight
        packed = net._weight(i)
        assert packed.is_contiguous() and np.array_equal(R.bits(packed, torch.float16), R.pack_weight(w.detach(), torch.float16))
        assert tuple(packed.shape) == (cout, 11 * 64 if cin == 3 else k * k * cin)
        assert net._weight(i) is packed
    p0 = net._weight("0").reshape(64, 11, 16, 4)
    assert not p0[:, :, 11:].any() and not p0[:, :, :, 3].any() and torch.equal(p0[5, 7, 9, :3], net.features["0"].weight[5, :, 7, 9])
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict(dict(sd, **{"features.6.weight": torch.ones_like(sd["features.6.weight"])}))
    assert bool((net._weight("6") == 1).all())
    net.load_state_dict(sd)


def test_load_state_dict_takes_torchvisions_full_dict_and_nothing_else(net):
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    full = dict(sd, **{f"classifier.{i}.{p}": torch.zeros(2) for i in (1, 4, 6) for p in ("weight", "bias")})
    res = net.load_state_dict(full)
    assert not res.missing_keys and not res.unexpected_keys
    for bad in (dict(sd, extra=torch.zeros(1)), {k: v for k, v in sd.items() if k != "features.0.bias"}, dict(sd, **{"features.1.weight": torch.zeros(1)})):
        with pytest.raises(RuntimeError):
            net.load_state_dict(bad)
    res = net.load_state_dict({k: v for k, v in sd.items() if k != "features.0.bias"}, strict=False)
    assert res.missing_keys == ["features.0.bias"]


def test_no_eager_path_and_argument_errors(net):
    from eeg_image_decode_amd._lib import EegclipError
    x = torch.zeros(2, 3, 40, 40, dtype=torch.float16)
    for bad in (lambda: net(x), lambda: net(x, nodes=("features.12",)), lambda: net(x, nodes=()),
                lambda: preprocess.alexnet_preprocess(x.float(), device="cpu")):          # (a float batch needs in_range)
        with pytest.raises(EegclipError):
            bad()


def test_reference_shapes_and_yardstick():
    """the restatement gives torchvision's node shapes -- (192, 31, 31) and (256, 15, 15) at 256 x 256 -- and the host's size arithmetic agrees with it; the
    yardstick differs from fp64 by rounding only"""
    sd = metric_nets.AlexNetFeatures(dtype=torch.float16, device="cpu", seed=0).state_dict()
    f = R.features(torch.zeros(1, 3, 256, 256), sd)
    assert tuple(f["features.4"].shape) == (1, 192, 31, 31) and tuple(f["features.11"].shape) == (1, 256, 15, 15)
    for n, want in ((256, (63, 31, 15)), (67, (16, 7, 3)), (83, (20, 9, 4)), (31, (7, 3, 1))):
        a = metric_nets.conv_out(n, 11, 4, 2)
        assert (a, metric_nets.pool_out(a), metric_nets.pool_out(metric_nets.pool_out(a))) == want
    x = R.normalised_images(2, 31, 37)
    ref, yard = R.features(x.half(), sd), R.yardstick(x.half(), sd, torch.float16)
    assert tuple(ref["features.4"].shape) == (2, 192, 3, 3) and tuple(ref["features.11"].shape) == (2, 256, 1, 1)
    assert all(0 < R.rel_l2(yard[n], ref[n]) < 2e-3 for n in ref)
