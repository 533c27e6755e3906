"""What tests/test_effnet_emu.py (product host code on the lane emulator, device "cpu") and tests/test_metric_effnet_gpu.py (the MI355X, device "cuda") share:
metric_nets.EfficientNetFeatures, metrics.effnet_distance and the table against tests/effnet_ref.py.

The network bound is tests/metric_nets_cases.py's and tests/resnet_cases.py's: the relative L2 distance of `avgpool` to the fp64 restatement is at most 2 x the
yardstick's own -- the same chain in fp32 with the input, the weights and every launch's output rounded to the dtype, on the same inputs and weights.  That is
what any 16-bit implementation pays; the factor 2 covers a different accumulation order and that two sets of random roundings do not coincide."""
import numpy as np
import torch

import effnet_ref as R
import metric_nets_ref as MR

MARGIN = 2.0
CORR_BOUND = 64 * 2.0 ** -24                    # tests/test_kernels_resnet.py: eegclip_corr_distance against scipy
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
    """-> (the C-ABI launches of one forward, in order, seen through a proxy in front of the library (metric_nets fetches it per call); for
    eegclip_convbnact16 also (KS, stride, act, has a residual, in_pad, out_pad) and for eegclip_dwconv16 (k, stride); the forward's result)"""
    import eeg_image_decode_amd.metric_nets as MN
    real, seen, convs, dws = MN.lib, [], [], []

    class Recording:
        def __getattr__(self, name):
            fn = getattr(real(), name)
            if name in ("eegclip_convbnact16_in_width", "eegclip_dwconv16_slabs"):             # (host arithmetic, no launch)
                return fn
            seen.append(name)
            if name == "eegclip_convbnact16":
                def conv(d, stream):
                    convs.append((d.KS, d.stride, d.act, d.residual is not None, d.in_pad, d.out_pad))
                    return fn(d, stream)
                return conv
            if name == "eegclip_dwconv16":
                def dw(*a):
                    dws.append((a[10], a[11]))
                    return fn(*a)
                return dw
            return fn
    MN.lib = lambda: Recording()
    try:
        out = net(x, **kw)
    finally:
        MN.lib = real
    return seen, convs, dws, out


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
    from eeg_image_decode_amd._lib import EegclipError
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
    for bad in (dict(sd, **{"features.1.0.block.3.0.weight": torch.zeros(1)}), {k: v for k, v in sd.items() if k != "features.2.0.block.1.1.running_var"},
                dict(sd, **{"avgpool.weight": torch.zeros(1)}), {"module." + k: v for k, v in sd.items()},
                {k: v for k, v in sd.items() if k != "features.5.0.block.2.fc1.bias"}):
        try:
            net.load_state_dict(bad)
        except RuntimeError:
            continue
        raise AssertionError("a wrong key loaded")
    net.load_state_dict(sd)
    assert torch.equal(net(x), got)
    for bad in (lambda: net(x.to(torch.float32)), lambda: net(x[:, :2]), lambda: net(x[0]), lambda: net(x, chunk=0), lambda: net(x[:0]), lambda: net(x[:, :, :0]),
                lambda: net(x.to(torch.bfloat16 if dtype == torch.float16 else torch.float16))):
        try:
            bad()
        except EegclipError:
            continue
        raise AssertionError("no EegclipError")
    return e / ey


def check_smallest(device, dtype, layers=SHALLOW):
    """MIN_SIDE = 1: a 1 x 1 and a 1 x 2 image reach `avgpool` and meet the same bound"""
    from eeg_image_decode_amd import metric_nets
    assert metric_nets.MIN_SIDE == 1
    for H, W in ((1, 1), (1, 2)):
        net, x, ref, peak, yard = net_and_refs(device, H, W, 2, dtype, layers)
        got = net(x)
        e, ey = MR.rel_l2(got, ref), MR.rel_l2(yard, ref)
        print(f"\n[effnet] {layers} {H}x{W} {dtype}: rel L2 {e:.2e}, yardstick {ey:.2e}", end=" ")
        assert tuple(got.shape) == (2, 1280) and ey > 0 and e <= MARGIN * ey


def check_effnet_row(device, H, W, N, layers=FULL, dtype=torch.float16):
    """metrics.effnet_distance at H x W (size=H: no resize) on MR.mixed_pairs: bit for bit correlation_distance of the net's features of both sides, its mean
    their mean, and each distance within the corr_distance bound of scipy's on the product's own features.  From the reference alone, first: every reference
    distance is at least 10 x what the yardstick's rounding moves it by.  Returns (images, recons, net)."""
    from eeg_image_decode_amd import metric_nets, metrics as M, preprocess as P
    images, recons = (t.to(device) for t in MR.mixed_pairs(N, H, W))
    net = metric_nets.EfficientNetFeatures(layers=layers, dtype=dtype, device=device, seed=0)
    pre = lambda t: P.effnet_preprocess(t, size=H, dtype=dtype, device=device, in_range=(0.0, 1.0))   # noqa: E731
    xa, xb = pre(images), pre(recons)
    assert tuple(xa.shape) == (N, 3, H, W)
    sd = net.state_dict()
    (fa, _), (fb, _) = R.features(xa, sd, layers), R.features(xb, sd, layers)
    d_ref, d_yard = R.correlation(fa, fb), R.correlation(R.yardstick(xa, sd, layers, dtype), R.yardstick(xb, sd, layers, dtype))
    moved = float(np.abs(d_yard - d_ref).max())
    print(f"\n[effnet] EffNet-B row {layers} {H}x{W} N={N}: reference distances {d_ref.min():.2e} .. {d_ref.max():.2e}, {dtype} rounding moves them by {moved:.1e}", end=" ")
    assert (d_ref >= 10 * moved).all(), (d_ref, moved)
    mean, d = M.effnet_distance(images, recons, net, size=H, return_distances=True)
    ga, gb = net(xa), net(xb)
    assert d.dtype == torch.float32 and tuple(d.shape) == (N,) and d.device.type == torch.device(device).type
    assert torch.equal(d, M.correlation_distance(ga, gb)) and mean == float(d.mean()) and isinstance(mean, float)
    assert M.effnet_distance(images, recons, net, size=H) == mean
    own = R.correlation(ga, gb)
    err = float(np.abs(d.cpu().double().numpy() - own).max())
    print(f"\n[effnet] EffNet-B row: max |d - scipy on the same features| {err:.2e} = {err * 2 ** 24:.1f} x 2^-24", end=" ")
    assert err <= CORR_BOUND
    return images, recons, net


def check_table(device, images, recons, net, size, **rows):
    """metrics.reconstruction_metrics(..., effnet=net) adds exactly the key "EffNet-B" -- effnet_distance's at its default size -- and leaves the rows of the
    call without it equal; a feature net may not take that name"""
    from eeg_image_decode_amd import metrics as M
    from eeg_image_decode_amd._lib import EegclipError
    base = M.reconstruction_metrics(images, recons, size=size, device=device, **rows)
    out = M.reconstruction_metrics(images, recons, size=size, device=device, effnet=net, **rows)
    assert sorted(out) == sorted(list(base) + ["EffNet-B"]) and all(out[k] == base[k] for k in base)
    assert isinstance(out["EffNet-B"], float) and out["EffNet-B"] == M.effnet_distance(images, recons, net)
    try:
        M.reconstruction_metrics(images, recons, size=size, device=device, effnet=net, feature_nets={"EffNet-B": lambda t: t})
    except EegclipError:
        return out
    raise AssertionError("a feature net took the EffNet-B row's name")
