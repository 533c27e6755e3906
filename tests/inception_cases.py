"""What tests/test_inception_emu.py (product host code on the lane emulator, device "cpu") and tests/test_metric_inception_gpu.py (the MI355X, device "cuda")
share: metric_nets.InceptionFeatures, metrics.inception_two_way and the table against tests/inception_ref.py.

The network bound is tests/metric_nets_cases.py's, tests/resnet_cases.py's and tests/effnet_cases.py's: the relative L2 distance of `avgpool` to the fp64
restatement is at most 2 x the yardstick's own -- the same chain in fp32 with the input, the weights and every launch's output (the pack and both pool kinds
included) rounded to the dtype, on the same inputs and weights.  That is what any 16-bit implementation pays; the factor 2 covers a different accumulation order
and that two sets of random roundings do not coincide."""
import numpy as np
import torch

import inception_ref as R
import metric_nets_ref as MR
import net_cases as C
import recon_metrics_ref as RM
from net_cases import MARGIN

FULL, SHALLOW = R.FULL, (1, 1, 1)
CAT, AVG3, MAXCAT = "eegclip_convbncat16", "eegclip_avgpool3x3_16", "eegclip_maxpool16_cat"
ROW_NOISE = 0.3                                # MR.mixed_pairs' noise for the row (two_way_inputs)
_refs = {}


def net_and_refs(device, H, W, N, dtype, blocks):
    """(net, x on the device, fp64 avgpool, its largest activation, yardstick avgpool); the references of a shape are computed once and shared"""
    from eeg_image_decode_amd import metric_nets
    net = metric_nets.InceptionFeatures(blocks=blocks, dtype=dtype, device=device, seed=0)
    x = MR.normalised_images(N, H, W).to(dtype)
    key = (H, W, N, dtype, blocks)
    if key not in _refs:
        sd = net.state_dict()
        _refs[key] = (*R.features(x, sd, blocks), R.yardstick(x, sd, blocks, dtype))
    return (net, x.to(device)) + _refs[key]


def launches(net, x, **kw):
    """-> (the C-ABI launches of one forward, in order; per eegclip_convbncat16 its descriptor's (KH, KW, stride, pad_h, pad_w, Cout); per eegclip_convbncat16
    (out, out_c0, Cout, out_stride) and per eegclip_maxpool16_cat (out, out_c0, C, out_stride), in launch order; the result)"""
    seen, rec, out = C.launches(lambda: net(x, **kw), ("eegclip_convbncat16_in_width",),
                                {CAT: lambda d, stream: ((d.KH, d.KW, d.stride, d.pad_h, d.pad_w, d.Cout), (d.out, d.out_c0, d.Cout, d.out_stride)),
                                 MAXCAT: lambda *a: (None, (a[1], a[9], a[5], a[8]))})
    return seen, [conv for n, (conv, _) in rec if n == CAT], [part for _, (_, part) in rec], out


def expected_launches(blocks):
    per = {"A": [CAT] * 6 + [AVG3, CAT], "B": [CAT] * 4 + [MAXCAT], "C": [CAT] * 9 + [AVG3, CAT], "D": [CAT] * 6 + [MAXCAT], "E": [CAT] * 8 + [AVG3, CAT]}
    seen = ["eegclip_pack_nchw16_affine"] + [CAT] * 3 + ["eegclip_maxpool16"] + [CAT] * 2 + ["eegclip_maxpool16"]
    for _, kind, _, _ in R.plan(blocks):
        seen += per[kind]
    return seen + ["eegclip_avgpool16"]


def check_slices(slices, blocks):
    """every output frame that more than one launch writes is a block's: its slices tile [0, total) in the order of concatenation, without a gap or an overlap, and
    the frame's pixel stride is total rounded up to 64"""
    frames = {}
    for out, c0, c, stride in slices:
        frames.setdefault((out, stride), []).append((c0, c))
    totals = sorted(t for _, _, _, t in R.plan(blocks))
    tiled = []
    for (_, stride), parts in frames.items():
        if len({c0 for c0, _ in parts}) == 1:
            continue                                             # a temporary or a stem frame: channel 0 on, one writer at a time
        end = None                                               # (a frame serves a block per chunk, and blocks of one output shape in turn: Mixed_6a and 6c)
        for c0, c in parts + [(0, 0)]:                           # launch order: a block's slices are written in the order of concatenation, from channel 0
            if c0 == 0 and end is not None:
                assert stride == (end + 63) // 64 * 64
                tiled.append(end)
            assert c0 == (0 if c0 == 0 else end), (parts, "a gap or an overlap")
            end = c0 + c
    assert sorted(set(tiled)) == sorted(set(totals)), (tiled, totals)


def check_features(device, H, W, N, dtype, blocks=FULL, extras=True):
    """`avgpool` against the fp64 restatement within 2 x the yardstick; from the reference alone, first: no activation near fp16's range, a live node and a
    yardstick that differs; run-to-run bit identity, the launch list, the slices, a batch split into chunks, state-dict loading, transform_input, the bad inputs.
    Returns product error / yardstick error."""
    from eeg_image_decode_amd import metric_nets
    net, x, ref, peak, yard = net_and_refs(device, H, W, N, dtype, blocks)
    pos, ey = float((ref > 0).double().mean()), MR.rel_l2(yard, ref)
    print(f"\n[inception] {blocks} {H}x{W} N={N} {dtype}: largest activation of the fp64 chain {peak:.1f}, {100 * pos:.1f} % of avgpool positive, yardstick {ey:.2e}", end=" ")
    assert peak < 2.0 ** 12 and pos > 0.05 and ey > 0
    got = net(x)
    assert tuple(got.shape) == tuple(ref.shape) == (N, 2048) and got.dtype == torch.float32 and got.device.type == torch.device(device).type
    e = MR.rel_l2(got, ref)
    print(f"\n[inception] {blocks} {H}x{W} N={N} {dtype} avgpool: rel L2 {e:.2e}, yardstick {ey:.2e}, ratio {e / ey:.2f}", end=" ")
    assert e <= MARGIN * ey, (e, ey)
    assert torch.equal(net(x), got)
    if not extras:
        return e / ey
    seen, convs, slices, again = launches(net, x)
    assert torch.equal(again, got)
    assert seen == expected_launches(blocks) and len(seen) == R.launch_count(blocks)
    if blocks == FULL:
        assert len(seen) == 109 and seen.count(CAT) == 94 and seen.count(AVG3) == 9 and seen.count(MAXCAT) == 2 and seen.count("eegclip_maxpool16") == 2
    assert sorted(convs) == sorted((kh, kw, s, ph, pw, cout) for _, _, cout, (kh, kw), s, (ph, pw) in R.layers(blocks))
    check_slices(slices, blocks)
    if N > 1:
        seen2, _, _, split = launches(net, x, chunk=N - 1)
        assert seen2 == 2 * seen and torch.equal(split, got)                # two chunks, the second smaller, through the same frames
    # state dict: BatchNorm keys reach the result and follow a load; AuxLogits.* / fc.* / num_batches_tracked load; a wrong or missing key raises
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    for key in ("Mixed_5b.branch_pool.bn.weight", "Mixed_7b.branch3x3dbl_3b.bn.bias", "Mixed_6a.branch3x3dbl_2.bn.running_mean"):
        net.load_state_dict(dict(sd, **{key: torch.full_like(sd[key], 0.5)}))
        assert not torch.equal(net(x), got), key
    res = net.load_state_dict(dict(sd, **{"fc.weight": torch.zeros(4, 8), "fc.bias": torch.zeros(4), "AuxLogits.conv0.conv.weight": torch.zeros(2, 2, 1, 1),
                                          "AuxLogits.fc.bias": torch.zeros(3)}))
    assert not res.missing_keys and not res.unexpected_keys and "Conv2d_1a_3x3.bn.num_batches_tracked" in sd
    C.wrong_keys_raise(net, (dict(sd, **{"Mixed_5b.branch1x1.conv.weight": torch.zeros(1)}), {k: v for k, v in sd.items() if k != "Mixed_6a.branch3x3.bn.running_var"},
                             dict(sd, **{"avgpool.weight": torch.zeros(1)}), {"module." + k: v for k, v in sd.items()},
                             {k: v for k, v in sd.items() if k != "Mixed_7a.branch7x7x3_4.conv.weight"}))
    net.load_state_dict(sd)
    assert torch.equal(net(x), got)
    # transform_input: without it the result differs; on input transformed beforehand (the product's fp32 a x + b, one rounding) it is the same bit for bit
    plain = metric_nets.InceptionFeatures(blocks=blocks, transform_input=False, dtype=dtype, device=device, seed=0)
    assert all(torch.equal(v, plain.state_dict()[k]) for k, v in sd.items())
    a, b = (t.to(device) for t in R.affine(True))
    pre = (x.float() * a[None, :, None, None] + b[None, :, None, None]).to(dtype)
    assert not torch.equal(plain(x), got) and torch.equal(plain(pre), got)
    C.bad_inputs_raise(net, x, dtype, (x[:, :, :74], x[:, :, :, :74]))
    return e / ey


def two_way_inputs(device, H, W, N, dtype, blocks):
    """-> (images, recons, reference counts).  images / recons: MR.mixed_pairs as (N, 3, H, W) fp32 in [0, 1] on the device.  The reference is the fp64 restatement
    applied to preprocess.inception_preprocess's OWN output at size H.  From the reference alone, on the CPU (tests/metric_nets_cases.py's conditions): every
    comparison is away from a tie by 10 x what 16-bit rounding moves r (the yardstick against fp64), and the counts are not all N - 1.  The pairs carry
    noise 0.3: at mixed_pairs' default 0.1 the seeded net's 2048 correlations of N = 6 pairs at 83 x 107 come within 8e-5 of a tie, 3.4 x the rounding's 2.3e-5;
    at 0.3 the smallest margin is 1.5e-3 (48 x) at full depth and 1.9e-3 at (1, 1, 1), N = 3."""
    from eeg_image_decode_amd import metric_nets, preprocess as P
    images, recons = (t.to(device) for t in MR.mixed_pairs(N, H, W, noise=ROW_NOISE))
    sd = metric_nets.InceptionFeatures(blocks=blocks, dtype=dtype, device="cpu", seed=0).state_dict()
    xa, xb = (P.inception_preprocess(t, size=H, dtype=dtype, device=device, in_range=(0.0, 1.0)).cpu() for t in (images, recons))
    assert tuple(xa.shape) == (N, 3, H, W)
    fa, fb = R.features(xa, sd, blocks)[0], R.features(xb, sd, blocks)[0]
    ya, yb = R.yardstick(xa, sd, blocks, dtype), R.yardstick(xb, sd, blocks, dtype)
    r, count, _ = RM.two_way(fa.numpy(), fb.numpy())
    ry, _, _ = RM.two_way(ya.double().numpy(), yb.double().numpy())
    gap, moved = RM.two_way_gap(r), float(np.abs(ry - r).max())
    print(f"\n[inception] Inception row {blocks} {H}x{W} N={N}: reference counts {count.tolist()}, smallest margin {gap:.1e}, {dtype} rounding moves r by {moved:.1e}", end=" ")
    assert gap >= 10 * moved, (gap, moved)
    assert not (count == N - 1).all(), count
    return images, recons, count


def check_inception_row(device, H, W, N, blocks=FULL, dtype=torch.float16):
    """metrics.inception_two_way at H x W (size=H: no resize): the counts are the reference's, every comparison included.  Returns (images, recons, net)."""
    from eeg_image_decode_amd import metric_nets, metrics as M
    images, recons, counts = two_way_inputs(device, H, W, N, dtype, blocks)
    net = metric_nets.InceptionFeatures(blocks=blocks, dtype=dtype, device=device, seed=0)
    score, count = M.inception_two_way(images, recons, net, size=H, return_counts=True)
    assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), counts), (count.tolist(), counts.tolist())
    assert isinstance(score, float) and abs(score - counts.mean() / (N - 1)) < 1e-12
    assert M.inception_two_way(images, recons, net, size=H) == score
    return images, recons, net


def check_table(device, images, recons, net, size, **rows):
    """metrics.reconstruction_metrics(..., inception=net) adds exactly the key "Inception" -- inception_two_way's at its default size -- and leaves the rows of
    the call without it equal; a feature net may not take that name"""
    from eeg_image_decode_amd import metrics as M
    return C.check_table("Inception", "inception", M.inception_two_way, device, images, recons, net, size, **rows)[1]
