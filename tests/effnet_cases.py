"""What tests/test_effnet_emu.py (product host code on the lane emulator, device "cpu") and tests/test_metric_effnet_gpu.py (the MI355X, device "cuda") share:
metric_nets.EfficientNetFeatures, metrics.effnet_distance and the table against tests/effnet_ref.py.

The network bound is tests/metric_nets_cases.py's and tests/resnet_cases.py's: the relative L2 distance of `avgpool` to the fp64 restatement is at most 2 x the
yardstick's own -- the same chain in fp32 with the input, the weights and every launch's output rounded to the dtype, on the same inputs and weights.  That is
what any 16-bit implementation pays; the factor 2 covers a different accumulation order and that two sets of random roundings do not coincide."""
import torch

import effnet_ref as R
import metric_nets_ref as MR
import net_cases as C
from net_cases import MARGIN

FULL, SHALLOW = R.B1_LAYERS, (1,) * 7
_refs = {}


def net_and_refs(device, H, W, N, dtype, layers):
    """(net, x on the device, fp64 avgpool, its largest activation, yardstick avgpool); the references of a shape are computed once and shared"""
    from eeg_image_decode_amd import metric_nets
    net = metric_nets.EfficientNetFeatures(layers=layers, dtype=dtype, device=device, seed=0)
    x = MR.normalised_images(N, H, W).to(dtype)
    key = (H, W, N, dtype, layers)
    if key not in _refs:
        sd = net.state_dict()
        _refs[key] = (*R.features(x, sd, layers), R.yardstick(x, sd, layers, dtype))
    return (net, x.to(device)) + _refs[key]


def launches(net, x, **kw):
    """-> (the C-ABI launches of one forward, in order; for eegclip_convbnact16 also (KS, stride, act, has a residual, in_pad, out_pad) and for
    eegclip_dwconv16 (k, stride); the forward's result)"""
    seen, rec, out = C.launches(lambda: net(x, **kw), ("eegclip_convbnact16_in_width", "eegclip_dwconv16_slabs"),
                                {"eegclip_convbnact16": lambda d, stream: (d.KS, d.stride, d.act, d.residual is not None, d.in_pad, d.out_pad),
                                 "eegclip_dwconv16": lambda *a: (a[10], a[11])})
    return seen, [v for n, v in rec if n == "eegclip_convbnact16"], [v for n, v in rec if n == "eegclip_dwconv16"], out


def expected_launches(layers):
    block = ["eegclip_dwconv16", "eegclip_se_gate16", "eegclip_gate_mul16", "eegclip_convbnact16"]
    seen = ["eegclip_pack_nchw16_pad1", "eegclip_convbnact16"]
    for s, n in enumerate(layers):
        seen += (block if s == 0 else ["eegclip_convbnact16"] + block) * n
    return seen + ["eegclip_convbnact16", "eegclip_avgpool16"]


def check_features(device, H, W, N, dtype, layers=FULL, extras=True):
    """`avgpool` against the fp64 restatement within 2 x the yardstick; from the reference alone, first: no activation near fp16's range, a live node and a
    yardstick that differs; run-to-run bit identity, the launch list, a batch split into chunks, state-dict loading, the bad inputs.  Returns product error /
    yardstick error."""
    net, x, ref, peak, yard = net_and_refs(device, H, W, N, dtype, layers)
    pos, ey = float((ref > 0).double().mean()), MR.rel_l2(yard, ref)
    print(f"\n[effnet] {layers} {H}x{W} N={N} {dtype}: largest activation of the fp64 chain {peak:.1f}, {100 * pos:.1f} % of avgpool positive, yardstick {ey:.2e}", end=" ")
    assert peak < 2.0 ** 12 and pos > 0.05 and ey > 0
    got = net(x)
    assert tuple(got.shape) == tuple(ref.shape) == (N, 1280) and got.dtype == torch.float32 and got.device.type == torch.device(device).type
    e = MR.rel_l2(got, ref)
    print(f"\n[effnet] {layers} {H}x{W} N={N} {dtype} avgpool: rel L2 {e:.2e}, yardstick {ey:.2e}, ratio {e / ey:.2f}", end=" ")
    assert e <= MARGIN * ey, (e, ey)
    assert torch.equal(net(x), got)
    if not extras:
        return e / ey
    nblocks = sum(layers)
    seen, convs, dws, again = launches(net, x)
    assert torch.equal(again, got)
    assert seen == expected_launches(layers) and len(seen) == 5 * nblocks - layers[0] + 4
    if layers == FULL:
        assert len(seen) == 117
    assert convs[0] == (3, 2, 2, False, 0, 1) and convs[-1][:4] == (1, 1, 2, False) and all(c[:2] == (1, 1) for c in convs[1:])
    assert sum(1 for c in convs if c[2] == 0) == nblocks and sum(1 for c in convs if c[2] == 2) == nblocks - layers[0] + 2        # projections: no activation
    assert sum(1 for c in convs if c[3]) == nblocks - 7 and all(c[2] == 0 for c in convs if c[3])                                # one residual per repeated block
    assert dws == [(k, stride if i == 0 else 1) for (_, k, stride, _, _), n in zip(R.STAGES, layers) for i in range(n)]
    if N > 1:
        seen2, _, _, split = launches(net, x, chunk=N - 1)
        assert seen2 == 2 * seen and torch.equal(split, got)                # two chunks, the second smaller, through the same frames
    # state dict: BatchNorm and the gate's bias reach the result and follow a load; classifier.* loads; a wrong or missing key raises
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    for key in ("features.3.0.block.1.1.weight", "features.4.0.block.2.fc2.bias"):
        net.load_state_dict(dict(sd, **{key: torch.zeros_like(sd[key])}))
        assert not torch.equal(net(x), got), key
    res = net.load_state_dict(dict(sd, **{"classifier.1.weight": torch.zeros(4, 8), "classifier.1.bias": torch.zeros(4)}))
    assert not res.missing_keys and not res.unexpected_keys
    C.wrong_keys_raise(net, (dict(sd, **{"features.1.0.block.3.0.weight": torch.zeros(1)}), {k: v for k, v in sd.items() if k != "features.2.0.block.1.1.running_var"},
                             dict(sd, **{"avgpool.weight": torch.zeros(1)}), {"module." + k: v for k, v in sd.items()},
                             {k: v for k, v in sd.items() if k != "features.5.0.block.2.fc1.bias"}))
    net.load_state_dict(sd)
    assert torch.equal(net(x), got)
    C.bad_inputs_raise(net, x, dtype, (x[:, :, :0],))
    return e / ey


def check_smallest(device, dtype, layers=SHALLOW):
    C.check_smallest("effnet", net_and_refs, device, dtype, layers, 1280)


def check_effnet_row(device, H, W, N, layers=FULL, dtype=torch.float16):
    """C.check_distance_row for metrics.effnet_distance.  Returns (images, recons, net)."""
    from eeg_image_decode_amd import metric_nets, metrics as M, preprocess as P
    return C.check_distance_row("effnet", "EffNet-B", R, metric_nets.EfficientNetFeatures, P.effnet_preprocess, M.effnet_distance, device, H, W, N, layers, dtype)


def check_table(device, images, recons, net, size, **rows):
    """metrics.reconstruction_metrics(..., effnet=net) adds exactly the key "EffNet-B" -- effnet_distance's at its default size -- and leaves the rows of the
    call without it equal; a feature net may not take that name"""
    from eeg_image_decode_amd import metrics as M
    return C.check_table("EffNet-B", "effnet", M.effnet_distance, device, images, recons, net, size, **rows)[1]
