"""What the four case modules of the metric nets (metric_nets_cases, resnet_cases, effnet_cases, inception_cases) share: the recording proxy in front of the
library, the loops over inputs that must raise, the smallest-image check, the distance-row check and the table check."""
import numpy as np
import torch

import metric_nets_ref as MR

MARGIN = 2.0                                    # the network bound: at most 2 x the yardstick's own error (tests/metric_nets_cases.py)
CORR_BOUND = 64 * 2.0 ** -24                    # tests/test_kernels_resnet.py: eegclip_corr_distance against scipy


def launches(call, host_only, fields=None):
    """-> (the C-ABI launches of call(), in order, seen through a proxy in front of the library (metric_nets fetches it per call); [(name, fields[name](*args))]
    of the entry points in `fields`, in launch order; call's result).  The names in `host_only` are host arithmetic, no launch."""
    import eeg_image_decode_amd.metric_nets as MN
    real, seen, recorded, fields = MN.lib, [], [], fields or {}

    class Recording:
        def __getattr__(self, name):
            fn = getattr(real(), name)
            if name in host_only:
                return fn
            seen.append(name)
            if name not in fields:
                return fn

            def wrapped(*a):
                recorded.append((name, fields[name](*a)))
                return fn(*a)
            return wrapped
    MN.lib = lambda: Recording()
    try:
        out = call()
    finally:
        MN.lib = real
    return seen, recorded, out


def all_raise(exc, calls, otherwise):
    for bad in calls:
        try:
            bad()
        except exc:
            continue
        raise AssertionError(otherwise)


def wrong_keys_raise(net, dicts):
    all_raise(RuntimeError, [lambda bad=bad: net.load_state_dict(bad) for bad in dicts], "a wrong key loaded")


def bad_inputs_raise(net, x, dtype, too_small):
    """fp32, two channels, three dimensions, chunk 0, an empty batch, the images of `too_small`, the other 16-bit dtype"""
    from eeg_image_decode_amd._lib import EegclipError
    all_raise(EegclipError, [lambda: net(x.to(torch.float32)), lambda: net(x[:, :2]), lambda: net(x[0]), lambda: net(x, chunk=0), lambda: net(x[:0]),
                             *[lambda t=t: net(t) for t in too_small], lambda: net(x.to(torch.bfloat16 if dtype == torch.float16 else torch.float16))],
              "no EegclipError")


def check_smallest(label, net_and_refs, device, dtype, layers, width):
    """MIN_SIDE = 1: a 1 x 1 and a 1 x 2 image reach `avgpool` and meet the same bound"""
    from eeg_image_decode_amd import metric_nets
    assert metric_nets.MIN_SIDE == 1
    for H, W in ((1, 1), (1, 2)):
        net, x, ref, peak, yard = net_and_refs(device, H, W, 2, dtype, layers)
        got = net(x)
        e, ey = MR.rel_l2(got, ref), MR.rel_l2(yard, ref)
        print(f"\n[{label}] {layers} {H}x{W} {dtype}: rel L2 {e:.2e}, yardstick {ey:.2e}", end=" ")
        assert tuple(got.shape) == (2, width) and ey > 0 and e <= MARGIN * ey


def check_distance_row(label, row, R, make_net, pre, metric, device, H, W, N, layers, dtype):
    """metric (metrics.swav_distance / effnet_distance) at H x W (size=H: no resize) on MR.mixed_pairs: bit for bit correlation_distance of the net's features of
    both sides, its mean their mean, and each distance within the corr_distance bound of scipy's on the product's own features.  From the reference alone, first:
    every reference distance is at least 10 x what the yardstick's rounding moves it by.  Returns (images, recons, net)."""
    from eeg_image_decode_amd import metrics as M
    images, recons = (t.to(device) for t in MR.mixed_pairs(N, H, W))
    net = make_net(layers=layers, dtype=dtype, device=device, seed=0)
    xa, xb = (pre(t, size=H, dtype=dtype, device=device, in_range=(0.0, 1.0)) for t in (images, recons))
    assert tuple(xa.shape) == (N, 3, H, W)
    sd = net.state_dict()
    (fa, _), (fb, _) = R.features(xa, sd, layers), R.features(xb, sd, layers)
    d_ref, d_yard = R.correlation(fa, fb), R.correlation(R.yardstick(xa, sd, layers, dtype), R.yardstick(xb, sd, layers, dtype))
    moved = float(np.abs(d_yard - d_ref).max())
    print(f"\n[{label}] {row} row {layers} {H}x{W} N={N}: reference distances {d_ref.min():.2e} .. {d_ref.max():.2e}, {dtype} rounding moves them by {moved:.1e}", end=" ")
    assert (d_ref >= 10 * moved).all(), (d_ref, moved)
    mean, d = metric(images, recons, net, size=H, return_distances=True)
    ga, gb = net(xa), net(xb)
    assert d.dtype == torch.float32 and tuple(d.shape) == (N,) and d.device.type == torch.device(device).type
    assert torch.equal(d, M.correlation_distance(ga, gb)) and mean == float(d.mean()) and isinstance(mean, float)
    assert metric(images, recons, net, size=H) == mean
    own = R.correlation(ga, gb)
    err = float(np.abs(d.cpu().double().numpy() - own).max())
    print(f"\n[{label}] {row} row: max |d - scipy on the same features| {err:.2e} = {err * 2 ** 24:.1f} x 2^-24", end=" ")
    assert err <= CORR_BOUND
    return images, recons, net


def check_table(row, keyword, metric, device, images, recons, net, size, **rows):
    """metrics.reconstruction_metrics(..., keyword=net) adds exactly `row` -- metric's value at its default size; row=None: the rows of the dict
    that metric returns -- and leaves the rows of the call without it equal; a feature net may not take `row` as its name.  Returns (the table without, the table with)."""
    from eeg_image_decode_amd import metrics as M
    from eeg_image_decode_amd._lib import EegclipError
    base = M.reconstruction_metrics(images, recons, size=size, device=device, **rows)
    out = M.reconstruction_metrics(images, recons, size=size, device=device, **{keyword: net}, **rows)
    own = metric(images, recons, net) if row is None else {row: metric(images, recons, net)}
    assert sorted(out) == sorted(list(base) + list(own)) and all(out[k] == base[k] for k in base)
    assert all(isinstance(out[k], float) and out[k] == own[k] for k in own)
    if row is None:
        return base, out
    all_raise(EegclipError, [lambda: M.reconstruction_metrics(images, recons, size=size, device=device, **{keyword: net}, feature_nets={row: lambda t: t})],
              f"a feature net took the {row} row's name")
    return base, out
