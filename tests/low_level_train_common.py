"""What tests/test_low_level_train_emu.py and tests/test_low_level_train_gpu.py share: the fp32 reference of a training step of the low-level encoder
(tests/low_level_ref.py in train mode, fp32 autograd on the CPU, torch.optim.AdamW) and its YARDSTICK, the same reference with the weights rounded to the 16-bit
dtype in every forward and the activations (and, through autograd, their gradients) rounded at the layer boundaries (`round_to=`): the format's own error.  The
product is allowed 3 x the yardstick's deviation from the fp32 reference, as the forward tests allow: its summation orders differ, and ReLU masks flip where a
pre-activation rounds across 0.  Nothing here looks at the product."""
import functools

import torch
import torch.nn as nn

from low_level_ref import EncoderLowLevelRef

LR, WD, STEPS = 2e-3, 1e-2, 30
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def make_ref(num_channels, hidden, channels, dtype, seed=0):
    """train-mode restatement with a BatchNorm affine part that is not the identity (as low_level_ref.calibrated), every parameter representable in `dtype`"""
    g = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        ref = EncoderLowLevelRef(num_channels=num_channels, hidden=hidden, channels=channels)
    for m in ref.upsampler:
        if isinstance(m, nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
    ref.to(dtype).float()
    return ref.train()


def batch(num_channels, channels, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    S = 2 ** (len(channels) - 1)
    return torch.randn(B, num_channels, 250, generator=g), torch.randn(B, channels[-1], S, S, generator=g)


def run_reference(ref0, x, t, steps, round_to=None):
    """`steps` AdamW steps on the fixed batch from ref0's state (ref0 is left alone) -> per step: loss, gradients, running statistics; the final module.
    round_to: the yardstick (weights rounded in every forward, activations and their gradients at the layer boundaries)."""
    import copy
    ref = copy.deepcopy(ref0).train()
    params = dict(ref.named_parameters())
    opt = torch.optim.AdamW(params.values(), lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=WD)
    out, dz_abs = [], {}
    for name, m in ref.upsampler.named_children():                    # sum |dz| per output channel of every convolution: the bound of a bias gradient below
        if isinstance(m, nn.ConvTranspose2d):
            m.register_full_backward_hook(lambda mod, gi, go, name=name: dz_abs.__setitem__(name, go[0].detach().abs().sum((0, 2, 3))))
    for _ in range(steps):
        opt.zero_grad()
        if round_to is None:
            pred = ref(x)
        else:
            pred = torch.func.functional_call(ref, {k: v.to(round_to).float() for k, v in params.items()}, (x,), {"round_to": round_to})
        loss = ((pred - t) ** 2).mean()
        loss.backward()
        out.append(dict(loss=float(loss.detach()), dz_abs=dict(dz_abs), grads={k: v.grad.detach().clone() for k, v in params.items()},
                        stats={k: v.detach().clone() for k, v in ref.named_buffers() if "num_batches" not in k}, pred=pred.detach().clone()))
        opt.step()
    return out, ref


@functools.lru_cache(maxsize=None)
def references(num_channels, hidden, channels, B, dtype, steps):
    """(initial reference, batch, fp32 run, yardstick run): computed once per configuration and shared, never modified"""
    ref0 = make_ref(num_channels, hidden, channels, dtype)
    x, t = batch(num_channels, channels, B)
    return ref0, (x, t), run_reference(ref0, x, t, steps), run_reference(ref0, x, t, steps, round_to=dtype)


def check_one_step(grads, stats, loss, fp32, yard, dtype, label=""):
    """the one-step assertions; returns the worst product / allowance ratio"""
    worst = 0.0
    allow = 3 * abs(yard["loss"] - fp32["loss"])
    print(f"{label} loss {loss:.6f} reference {fp32['loss']:.6f} yardstick {yard['loss']:.6f} allowance {allow:.2e}")
    assert abs(loss - fp32["loss"]) <= allow
    for k, gref in fp32["grads"].items():
        got = grads[k].cpu().float()
        idx = k.split(".")
        zero_bias = idx[0] == "upsampler" and idx[2] == "bias" and f"upsampler.{int(idx[1]) + 1}.weight" in fp32["grads"]
        if zero_bias:
            # mathematically 0 (BatchNorm removes the mean), so no relative measure: by absolute size, reported against the weight gradient's norm.  The
            # yardstick rounds nothing between BatchNorm's backward and this sum and says nothing here; the product holds dz in 16 bits, each element off by
            # at most u |dz|, which adds coherently in the worst case: |db[co]| <= u sum|dz[.., co]| (the reference's own dz), times 3 as everywhere.
            # The criterion is that derived bound, || db - db_ref || <= 3 u || sum|dz| ||; both sides are divided by the weight gradient's norm `wn` ONLY
            # so that the printed figures read as a size against |dW| (the norm cancels in the assertion)
            wn = float(fp32["grads"][f"upsampler.{idx[1]}.weight"].norm())
            e_y, e_p = U[dtype] * float(fp32["dz_abs"][idx[1]].norm()) / wn, float((got - gref).norm()) / wn
        else:
            e_y, e_p = rel_l2(yard["grads"][k], gref), rel_l2(got, gref)
        print(f"{label} grad {k}: product {e_p:.3e} yardstick {e_y:.3e} ratio {e_p / e_y:.2f}" + (" (|.| / |dW|)" if zero_bias else ""))
        worst = max(worst, e_p / (3 * e_y))
        assert e_p <= 3 * e_y, k
    for k, sref in fp32["stats"].items():
        e_y, e_p = rel_l2(yard["stats"][k], sref), rel_l2(stats[k].cpu().float(), sref)
        print(f"{label} {k}: product {e_p:.3e} yardstick {e_y:.3e} ratio {e_p / e_y:.2f}")
        worst = max(worst, e_p / (3 * e_y))
        assert e_p <= 3 * e_y, k
    print(f"{label} worst product / allowance {worst:.3f}")
    return worst
