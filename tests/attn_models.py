"""CPU models of the 16-bit attention kernels' STATED arithmetic, and the structured inputs their kernel tests share (TEST ONLY).

The models are references: numpy on the host, never the code under test.  They exist to say how far a CORRECT kernel of that arithmetic lies from the
fp64 oracle on a test's inputs, so that a tolerance is the arithmetic's own error times a stated margin and not a rule of thumb:

  cross_attn_model   csrc/cross_attn.hip: fp32 scores, single pass, NORMALISED probabilities (times ip_scale in the image branch) rounded to the I/O type,
                     fp32 accumulation of both branches, one output rounding.
  flash_model        csrc/self_attn.hip (head dims 64 and 80): fp32 scores, UN-normalised base-2 probabilities rounded to the I/O type, fp32 accumulation and
                     an fp32 row sum of the unrounded probabilities, one division, one output rounding.  (The model takes the row maximum of the whole row; the
                     kernel's running maximum rescales by exact powers' worth of fp32 and is what the tests' 3x margin is for.)

`python tests/attn_models.py` prints, per test file and dtype, the models' worst max and worst mean error against fp64 over the exact shapes and seeds of
that file's parity tests (each file lists them in MODEL_CASES), and the figures of the stress cases; the files' docstrings quote these numbers."""
import numpy as np
import torch

LOG2E = 1.44269504088896340736


def round16(a, f16):
    """values rounded to fp16 / bf16 (round to nearest even, as the kernels' pack2), as float64"""
    return torch.tensor(np.asarray(a, np.float32)).to(torch.float16 if f16 else torch.bfloat16).double().numpy()


def _heads(t, heads):
    B, T, C = t.shape
    return np.asarray(t, np.float64).reshape(B, T, heads, C // heads).transpose(0, 2, 1, 3)


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def cross_attn_model(qf, kf, vf, heads, kif=None, vif=None, ip_scale=1.0, f16=True):
    """q (B,HW,C), k / v (B,S,C), k_ip / v_ip (B,S_ip,C): values already on the 16-bit grid -> (B,HW,C) float64 on the 16-bit grid"""
    B, HW, C = qf.shape
    qh = _heads(qf, heads)
    scale2 = float(np.float32(0.125 * LOG2E))

    def branch(kk, vv, pscale):
        s = _f32(qh @ _heads(kk, heads).transpose(0, 1, 3, 2))                     # fp32 raw scores
        mxs = _f32(s.max(-1, keepdims=True) * scale2)
        e = _f32(np.exp2(_f32(s * scale2 - mxs)))                                  # one FMA, then v_exp_f32
        nrm = _f32(pscale / _f32(e.sum(-1, keepdims=True)))
        return round16(_f32(e * nrm), f16) @ _heads(vv, heads)

    o = branch(kf, vf, 1.0)
    if kif is not None:
        o = o + branch(kif, vif, float(np.float32(ip_scale)))
    return round16(_f32(o), f16).transpose(0, 2, 1, 3).reshape(B, HW, C)


def flash_model(qf, kf, vf, heads, scale, f16):
    """q (B,Tq,C), k / v (B,Tk,C): values already on the 16-bit grid -> (B,Tq,C) float64 on the 16-bit grid; head dim C / heads"""
    B, Tq, C = qf.shape
    scale2 = float(np.float32(np.float32(scale) * np.float32(LOG2E)))
    s = _f32(_heads(qf, heads) @ _heads(kf, heads).transpose(0, 1, 3, 2))
    e = _f32(np.exp2(_f32(_f32(s - s.max(-1, keepdims=True)) * scale2)))           # (s - m) * scale2: never positive, 0 at the maximum
    inv = _f32(1.0 / _f32(e.sum(-1, keepdims=True)))
    o = _f32(_f32(round16(e, f16) @ _heads(vf, heads)) * inv)
    return round16(o, f16).transpose(0, 2, 1, 3).reshape(B, Tq, C)


# ---- structured inputs: a wrong, dropped or doubled key moves the output by an integer, not by a few 1e-3 --------------------------------------------

def count_values(B, T, heads, D, shift=0):
    """v[b, j, h] = T * onehot((j + h + shift) mod D), and what uniform attention (q = 0) makes of it: the number of keys per column, (heads * D,)"""
    v = np.zeros((B, T, heads, D), np.float32)
    count = np.zeros((heads, D), np.float64)
    j = np.arange(T)
    for h in range(heads):
        v[:, j, h, (j + h + shift) % D] = float(T)
        count[h] = np.bincount((j + h + shift) % D, minlength=D)
    return v.reshape(B, T, heads * D), count.reshape(heads * D)


def onehot_keys(B, T, heads, D, col0=0, ncols=None):
    """k[b, j, h] = +-16 e_(col0 + (j + h) mod ncols), + for j < ncols and - behind: T <= 2 ncols distinct codes whose mutual products are 0 or -256"""
    ncols = D if ncols is None else ncols
    assert T <= 2 * ncols and col0 + ncols <= D
    k = np.zeros((B, T, heads, D), np.float32)
    j = np.arange(T)
    for h in range(heads):
        k[:, j, h, col0 + (j + h) % ncols] = np.where(j < ncols, 16.0, -16.0)
    return k.reshape(B, T, heads * D)


def twohot_keys(B, T, heads, D):
    """k[b, j, h] = 16 (e_((j + h) mod D/2) + e_(D/2 + j div D/2)): T <= D^2 / 4 codes; a key scores 512 against itself and 256 or 0 against another"""
    assert T <= (D // 2) ** 2
    k = np.zeros((B, T, heads, D), np.float32)
    j = np.arange(T)
    for h in range(heads):
        k[:, j, h, (j + h) % (D // 2)] = 16.0
        k[:, j, h, D // 2 + j // (D // 2)] = 16.0
    return k.reshape(B, T, heads * D)


def targets(Tq, T, heads, mul=5):
    """target(i, h) = (mul i + h) mod T, (heads, Tq)"""
    return (mul * np.arange(Tq)[None, :] + np.arange(heads)[:, None]) % T


def gather_rows(x, tgt, heads):
    """x (B,T,C), tgt (heads,Tq) -> (B,Tq,C): row tgt[h, i] of x in head h's columns"""
    B, T, C = x.shape
    D = C // heads
    xh = x.reshape(B, T, heads, D)
    return np.stack([xh[:, tgt[h], h] for h in range(heads)], axis=2).reshape(B, tgt.shape[1], C)


def int_values(B, T, heads, D, lo=-50, mul=1):
    """small integers that differ by key, column, head and sample: mul * (lo .. lo + 100)"""
    b, j, h, c = np.ix_(np.arange(B), np.arange(T), np.arange(heads), np.arange(D))
    return (mul * ((7 * j + 3 * c + 11 * h + 13 * b) % 101 + lo)).astype(np.float32).reshape(B, T, heads * D)


def _measure():
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import importlib
    for name in ("test_kernels_cross_attn", "test_kernels_self_attn", "test_kernels_attn80"):
        mod = importlib.import_module(name)
        for group, cases in mod.MODEL_CASES.items():
            worst = {True: [0.0, 0.0, 0.0], False: [0.0, 0.0, 0.0]}
            for label, f16, make in cases:
                model, ref = make()
                err = np.abs(model - ref)
                w = worst[f16]
                w[0], w[1], w[2] = max(w[0], err.max()), max(w[1], err.mean()), max(w[2], np.abs(ref).max())
                print(f"  {name} {group} {label} {'f16' if f16 else 'bf16'}: max {err.max():.2e} mean {err.mean():.2e} max|ref| {np.abs(ref).max():.2f}", flush=True)
            for f16 in (True, False):
                w = worst[f16]
                print(f"{name} {group} {'f16' if f16 else 'bf16'}: worst max {w[0]:.2e}, worst mean {w[1]:.2e}, max|ref| {w[2]:.2f}  ->  3x = {3 * w[0]:.2e} / {3 * w[1]:.2e}",
                      flush=True)


if __name__ == "__main__":
    _measure()
