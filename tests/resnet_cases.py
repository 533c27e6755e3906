"""What tests/test_resnet_emu.py (product host code on the lane emulator, device "cpu") and tests/test_resnet_gpu.py (the MI355X, device "cuda") share:
metric_nets.ResNetFeatures, metrics.correlation_distance / swav_distance against tests/resnet_ref.py.

The network bound is tests/metric_nets_cases.py's: the relative L2 distance of `avgpool` to the fp64 restatement is at most 2 x the yardstick's own -- the same
chain in fp32 with the input, the weights and every launch's output rounded to the dtype, on the same inputs and weights.  That is what any 16-bit
implementation pays; the factor 2 covers a different accumulation order and that two sets of random roundings do not coincide."""
import torch

import metric_nets_ref as MR
import net_cases as C
import resnet_ref as R
from net_cases import MARGIN

FULL, SHALLOW = (3, 4, 6, 3), (1, 1, 1, 1)
_refs = {}


def net_and_refs(device, H, W, N, dtype, layers):
    """(net, x on the device, fp64 avgpool, its largest activation, yardstick avgpool); the references of a shape are computed once and shared"""
    from eeg_image_decode_amd import metric_nets
    net = metric_nets.ResNetFeatures(layers=layers, dtype=dtype, device=device, seed=0)
    x = MR.normalised_images(N, H, W).to(dtype)
    key = (H, W, N, dtype, layers)
    if key not in _refs:
        sd = net.state_dict()
        _refs[key] = (*R.features(x, sd, layers), R.yardstick(x, sd, layers, dtype))
    return (net, x.to(device)) + _refs[key]


def launches(net, x, **kw):
    """-> (the C-ABI launches of one forward, in order; for eegclip_convbn16 also (KS, stride, relu, has a residual); the forward's result)"""
    seen, rec, out = C.launches(lambda: net(x, **kw), ("eegclip_convbn16_in_width",),
                                {"eegclip_convbn16": lambda d, stream: (d.KS, d.stride, d.relu, d.residual is not None)})
    return seen, [v for _, v in rec], out


def check_features(device, H, W, N, dtype, layers=FULL, extras=True):
    """`avgpool` against the fp64 restatement within 2 x the yardstick; from the reference alone: no activation near fp16's range and a live node; run-to-run bit
    identity, the launch list, a batch split into chunks, state-dict loading, the bad inputs, the smallest image.  Returns product error / yardstick error."""
    net, x, ref, peak, yard = net_and_refs(device, H, W, N, dtype, layers)
    pos = float((ref > 0).double().mean())
    print(f"\n[resnet] {layers} {H}x{W} N={N} {dtype}: largest activation of the fp64 chain {peak:.1f}, {100 * pos:.1f} % of avgpool positive", end=" ")
    assert peak < 2.0 ** 12 and pos > 0.05
    got = net(x)
    assert tuple(got.shape) == tuple(ref.shape) == (N, 2048) and got.dtype == torch.float32 and got.device.type == torch.device(device).type
    e, ey = MR.rel_l2(got, ref), MR.rel_l2(yard, ref)
    print(f"\n[resnet] {layers} {H}x{W} N={N} {dtype} avgpool: rel L2 {e:.2e}, yardstick {ey:.2e}, ratio {e / ey:.2f}", end=" ")
    assert ey > 0 and e <= MARGIN * ey, (e, ey)
    assert torch.equal(net(x), got)
    if not extras:
        return e / ey
    n_conv = 3 * sum(layers) + 5
    seen, convs, again = launches(net, x)
    assert torch.equal(again, got)
    assert seen == ["eegclip_pack_nchw16_stem", "eegclip_convbn16", "eegclip_maxpool16_pad"] + ["eegclip_convbn16"] * (n_conv - 1) + ["eegclip_avgpool16"]
    assert convs[0] == (7, 2, 1, False)
    assert sum(1 for c in convs if c[2] == 0) == 4 and all(c[0] == 1 and not c[3] for c in convs if c[2] == 0)           # the four downsamples: no ReLU
    assert sum(1 for c in convs if c[3]) == sum(layers) and all(c[:3] == (1, 1, 1) for c in convs if c[3])               # one residual add per block, in conv3
    assert sum(1 for c in convs if c[0] == 3) == sum(layers) and sum(1 for c in convs if c[1] == 2) == 1 + 2 * 3
    if N > 1:
        seen2, _, split = launches(net, x, chunk=N - 1)
        assert seen2 == 2 * seen and torch.equal(split, got)                # two chunks, the second smaller, through the same frames
    # state dict: BatchNorm reaches the result and follows a load; the dropped prefixes load; a wrong key raises
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict(dict(sd, **{"layer3.0.bn3.weight": torch.zeros_like(sd["layer3.0.bn3.weight"])}))
    assert not torch.equal(net(x), got)
    full = {"module." + k: v for k, v in sd.items()}
    full.update({"module.fc.weight": torch.zeros(4, 8), "module.fc.bias": torch.zeros(4), "module.projection_head.0.weight": torch.zeros(4, 8),
                 "module.prototypes.weight": torch.zeros(4, 8)})
    res = net.load_state_dict(full)
    assert not res.missing_keys and not res.unexpected_keys
    C.wrong_keys_raise(net, (dict(sd, **{"layer1.0.conv4.weight": torch.zeros(1)}), {k: v for k, v in sd.items() if k != "layer2.0.downsample.1.running_var"},
                             dict(sd, **{"avgpool.weight": torch.zeros(1)}), {"backbone." + k: v for k, v in sd.items()}))
    net.load_state_dict(sd)
    assert torch.equal(net(x), got)
    C.bad_inputs_raise(net, x, dtype, (x[:, :, :0],))
    return e / ey


def check_smallest(device, dtype, layers=SHALLOW):
    C.check_smallest("resnet", net_and_refs, device, dtype, layers, 2048)


def check_swav_row(device, H, W, N, layers=FULL, dtype=torch.float16):
    """C.check_distance_row for metrics.swav_distance.  Returns (images, recons, net)."""
    from eeg_image_decode_amd import metric_nets, metrics as M, preprocess as P
    return C.check_distance_row("resnet", "SwAV", R, metric_nets.ResNetFeatures, P.swav_preprocess, M.swav_distance, device, H, W, N, layers, dtype)


def check_table(device, images, recons, net, size, alexnet=None):
    """metrics.reconstruction_metrics(..., swav=net): the key "SwAV" is swav_distance's at its default size, the other rows are those of the call without it"""
    from eeg_image_decode_amd import metrics as M
    return C.check_table("SwAV", "swav", M.swav_distance, device, images, recons, net, size, alexnet=alexnet)[1]
