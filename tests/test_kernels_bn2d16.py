"""csrc/bn2d16.hip (train-mode BatchNorm2d + ReLU on padded 16-bit NHWC frames, forward and backward) through the C ABI on both backends, against numpy fp64 on
the 16-bit-rounded inputs.

Bounds, from the arithmetic (u = half an ulp of the 16-bit format relative to 1; e = 2^-24; `pix` = the pixels of one partial row, whose sum is fp32 in some order;
the partial rows are added in fp64, which adds nothing visible):
  mean        |error| <= pix e mean|z| + e |mean|  (the cast)                                                                             =: E_m
  variance    sum z^2 carries one more rounding per term: E_q = (pix + 1) e mean(z^2);  var = q / M - mean^2  ->  E_v = E_q + 2 |mean| E_m + E_m^2
  rstd        1 / sqrt(var + eps): |relative error| <= E_v / (2 (var + eps)) (first order; 1 % slack for the rest) + e
  running     new = (1 - m) old + m stat: three fp32 roundings -> m E_stat + 3 e (|old| + |stat|); the variance enters as var M / (M - 1)
  apply       against fp64 on the kernel's OWN saved fp32 mean / rstd (they are checked above): xhat = (z - mean) rstd (two roundings), xhat gamma + beta (two),
              one rounding to 16 bit: 4 e (|xhat gamma| + |beta|) + u |a| + the smallest subnormal.  ReLU is 1-Lipschitz and applied to the reference too.
  dbeta       sum g: pix e sum|g| + e |sum g|;   dgamma  sum g xhat: (pix + 3) e sum|g xhat| + e |sum|     (both exact in the power-of-two loss scale)
  dz          gamma rstd (g - S_g / M - xhat S_gx / M): the two sums' errors enter as |gamma rstd| (E_g + |xhat| E_gx) / M; the fp32 expression itself has
              at most 8 roundings on terms bounded by T = |gamma rstd| (|g| + |S_g| / M + |xhat S_gx| / M); one rounding to 16 bit: ... + 8 e T + u |dz| + subnormal.
Worst |error| / bound over the cases below (printed per case with `pytest -s`), emulator and MI355X alike, fp16 / bf16: mean 0.031 / 0.039, rstd 0.124 / 0.103,
running_mean 0.181 / 0.177, running_var 0.174 / 0.161, apply 0.998 / 0.995, dbeta 0.002 / 0.001, dgamma 0.126 / 0.088, dz 0.996 / 0.996 (apply and dz: the half-ulp
term of the final rounding).
"""
import numpy as np
import pytest

from backends import be, byref, ok  # noqa: F401
from eeg_image_decode_amd import _abi
from test_kernels_convt16 import SENT, TINY, U
from test_kernels_gemm16 import DT, from16, to16

EINVAL, EALIGN = -1, -2
E = 2.0 ** -24
EPS, MOM = 1e-5, 0.1

# (N, H, W, C): fewer pixels than one group pass; odd sides; several slabs; more than 256 x 32 pixels (the slab count is capped: 33 pixels per slab)
CASES = [(4, 2, 2, 128), (3, 3, 5, 64), (2, 16, 16, 64), (1, 91, 92, 64)]


def slabs(M):
    n = min((M + 31) // 32, 256)
    pix = -(-M // n)
    return -(-M // pix), pix


def frame_of(bits):
    N, H, W, C = bits.shape
    fr = np.zeros((N, H + 2, W + 2, C), np.uint16)
    fr[:, 1:-1, 1:-1] = bits
    return fr


def out_frame(be, N, H, W, C, extra=3):
    fr = np.zeros((N, H + 2, W + 2, C), np.uint16)
    fr[:, 1:-1, 1:-1] = SENT
    return be.dev(np.concatenate([fr.ravel(), np.full(extra * (W + 2) * C, SENT, np.uint16)])), fr.size


def interior(be, buf, nframe, N, H, W, C):
    raw = be.host(buf)
    assert (raw[nframe:] == SENT).all(), "rows behind the frame were written"
    fr = raw[:nframe].reshape(N, H + 2, W + 2, C)
    assert not fr[:, 0].any() and not fr[:, -1].any() and not fr[:, :, 0].any() and not fr[:, :, -1].any(), "the frame's border was written"
    got = fr[:, 1:-1, 1:-1]
    assert (got != SENT).all(), "an interior element was left unwritten"
    return np.ascontiguousarray(got)


def inputs(N, H, W, C, dt):
    rng = np.random.default_rng(100 * N + 10 * H + W + C)
    z16, z = to16((rng.standard_normal((N, H, W, C)) * rng.uniform(0.5, 2.0, C) + rng.standard_normal(C)).astype(np.float32), dt)
    gamma = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(C)).astype(np.float32)
    return rng, z16, z.astype(np.float64), gamma, beta


def forward(be, z16, gamma, beta, rm0, rv0, dt):
    N, H, W, C = z16.shape
    nws = be.lib.eegclip_bn2d16_workspace_floats(N, H, W, C)
    assert nws == slabs(N * H * W)[0] * 2 * C + 2 * C
    out, nframe = out_frame(be, N, H, W, C)
    bufs = dict(Z=be.dev(frame_of(z16)), G=be.dev(gamma), B=be.dev(beta), mean=be.zeros(C), rstd=be.zeros(C), rm=be.dev(rm0), rv=be.dev(rv0),
                ws=be.dev(np.full(nws + 8, -7.5, np.float32)))
    d = _abi.Bn2d16FwdDesc(z=be.ptr(bufs["Z"]), a=be.ptr(out), gamma=be.ptr(bufs["G"]), beta=be.ptr(bufs["B"]), mean=be.ptr(bufs["mean"]), rstd=be.ptr(bufs["rstd"]),
                           running_mean=be.ptr(bufs["rm"]), running_var=be.ptr(bufs["rv"]), workspace=be.ptr(bufs["ws"]), workspace_floats=nws, N=N, H=H, W=W, C=C, eps=EPS, momentum=MOM,
                           dtype=DT[dt])
    ok(be.lib.eegclip_bn2d16_fwd(byref(d), be.stream))
    be.sync()
    assert (be.host(bufs["ws"])[nws:] == -7.5).all(), "memory behind the workspace was written"
    return interior(be, out, nframe, N, H, W, C), be.host(bufs["mean"]), be.host(bufs["rstd"]), be.host(bufs["rm"]), be.host(bufs["rv"])


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("N,H,W,C", CASES)
def test_bn2d16_fwd(be, N, H, W, C, dt):
    rng, z16, z, gamma, beta = inputs(N, H, W, C, dt)
    rm0, rv0 = rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2.0, C).astype(np.float32)
    a16, mean, rstd, rm, rv = forward(be, z16, gamma, beta, rm0, rv0, dt)
    M = N * H * W
    pix = slabs(M)[1]
    zf = z.reshape(M, C)
    m_ref, v_ref = zf.mean(0), zf.var(0)
    E_m = pix * E * np.abs(zf).mean(0) + E * np.abs(m_ref)
    E_v = (pix + 1) * E * (zf ** 2).mean(0) + 2 * np.abs(m_ref) * E_m + E_m ** 2
    r_ref = 1.0 / np.sqrt(v_ref + EPS)
    E_r = r_ref * (1.01 * E_v / (2 * (v_ref + EPS)) + E)
    rm_ref, rv_ref = (1 - MOM) * rm0 + MOM * m_ref, (1 - MOM) * rv0 + MOM * v_ref * M / (M - 1)
    E_rm = MOM * E_m + 3 * E * (np.abs(rm0) + np.abs(m_ref))
    E_rv = MOM * (E_v + E * v_ref) * M / (M - 1) + 3 * E * (np.abs(rv0) + v_ref * M / (M - 1))
    ratios = {"mean": np.abs(mean - m_ref) / E_m, "rstd": np.abs(rstd - r_ref) / E_r, "running_mean": np.abs(rm - rm_ref) / E_rm, "running_var": np.abs(rv - rv_ref) / E_rv}
    xh = (z - mean.astype(np.float64)) * rstd.astype(np.float64)
    pre = xh * gamma + beta
    ref = np.maximum(pre, 0.0)
    got = from16(a16, dt).astype(np.float64)
    assert np.isfinite(got).all() and (got >= 0).all() and (got == 0).any() and (got > 0).any()
    ratios["apply"] = np.abs(got - ref) / (4 * E * (np.abs(xh * gamma) + np.abs(beta)) + U[dt] * np.abs(ref) + TINY[dt])
    worst = {k: float(v.max()) for k, v in ratios.items()}
    print(f"bn2d16_fwd {be.name} {N}x{H}x{W}x{C} {dt}: worst |error| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    again = forward(be, z16, gamma, beta, rm0, rv0, dt)
    for x, y in zip((a16, mean, rstd, rm, rv), again):
        assert np.array_equal(x.view(np.uint16 if x.dtype == np.uint16 else np.uint32), y.view(np.uint16 if y.dtype == np.uint16 else np.uint32)), "two runs differ"


def backward(be, z16, a16, da16, gamma, mean, rstd, scale, dt):
    N, H, W, C = z16.shape
    nws = be.lib.eegclip_bn2d16_workspace_floats(N, H, W, C)
    out, nframe = out_frame(be, N, H, W, C)
    bufs = dict(Z=be.dev(frame_of(z16)), A=be.dev(frame_of(a16)), D=be.dev(frame_of(da16)), G=be.dev(gamma), mean=be.dev(mean), rstd=be.dev(rstd), dg=be.zeros(C),
                db=be.zeros(C), ws=be.dev(np.full(nws + 8, -7.5, np.float32)))
    d = _abi.Bn2d16BwdDesc(da=be.ptr(bufs["D"]), a=be.ptr(bufs["A"]), z=be.ptr(bufs["Z"]), gamma=be.ptr(bufs["G"]), mean=be.ptr(bufs["mean"]), rstd=be.ptr(bufs["rstd"]),
                           dgamma=be.ptr(bufs["dg"]), dbeta=be.ptr(bufs["db"]), dz=be.ptr(out), workspace=be.ptr(bufs["ws"]), workspace_floats=nws, N=N, H=H, W=W, C=C, loss_scale=scale,
                           dtype=DT[dt])
    ok(be.lib.eegclip_bn2d16_bwd(byref(d), be.stream))
    be.sync()
    assert (be.host(bufs["ws"])[nws:] == -7.5).all(), "memory behind the workspace was written"
    return interior(be, out, nframe, N, H, W, C), be.host(bufs["dg"]), be.host(bufs["db"])


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("N,H,W,C", CASES)
def test_bn2d16_bwd(be, N, H, W, C, dt):
    rng, z16, z, gamma, beta = inputs(N, H, W, C, dt)
    M = N * H * W
    pix = slabs(M)[1]
    zf = z.reshape(M, C)
    mean, rstd = zf.mean(0).astype(np.float32), (1.0 / np.sqrt(zf.var(0) + EPS)).astype(np.float32)
    xh = (z - mean.astype(np.float64)) * rstd.astype(np.float64)
    a16, a = to16(np.maximum(xh * gamma + beta, 0.0).astype(np.float32), dt)
    scale = 256.0
    da16, da = to16((scale * rng.standard_normal((N, H, W, C))).astype(np.float32), dt)
    g = np.where(a > 0, da.astype(np.float64), 0.0)
    assert (a > 0).any() and (a == 0).any()
    S_g, S_gx = g.reshape(M, C).sum(0), (g * xh).reshape(M, C).sum(0)
    E_g = pix * E * np.abs(g).reshape(M, C).sum(0) + E * np.abs(S_g)
    E_gx = (pix + 3) * E * np.abs(g * xh).reshape(M, C).sum(0) + E * np.abs(S_gx)
    k = gamma.astype(np.float64) * rstd
    ref = k * (g - S_g / M - xh * S_gx / M)
    T = np.abs(k) * (np.abs(g) + np.abs(S_g) / M + np.abs(xh * S_gx) / M)
    dz16, dg, db = backward(be, z16, a16, da16, gamma, mean, rstd, scale, dt)
    got = from16(dz16, dt).astype(np.float64)
    assert np.isfinite(got).all()
    worst = {"dbeta": float((np.abs(db - S_g / scale) / (E_g / scale)).max()), "dgamma": float((np.abs(dg - S_gx / scale) / (E_gx / scale)).max()),
             "dz": float((np.abs(got - ref) / (np.abs(k) * (E_g + np.abs(xh) * E_gx) / M + 8 * E * T + U[dt] * np.abs(ref) + TINY[dt])).max())}
    print(f"bn2d16_bwd {be.name} {N}x{H}x{W}x{C} {dt}: worst |error| / bound " + ", ".join(f"{k_} {v:.3f}" for k_, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    dz2, dg2, db2 = backward(be, z16, a16, da16, gamma, mean, rstd, scale, dt)
    assert np.array_equal(dz2, dz16) and np.array_equal(dg2.view(np.uint32), dg.view(np.uint32)) and np.array_equal(db2.view(np.uint32), db.view(np.uint32))


def test_bn2d16_rejections(be):
    N, H, W, C = 2, 2, 2, 64
    fr = lambda: be.zeros((N, H + 2, W + 2, C + 8), np.uint16)   # noqa: E731
    Z, A, D, O = fr(), fr(), fr(), fr()
    v = [be.zeros(C + 4) for _ in range(8)]
    nws = be.lib.eegclip_bn2d16_workspace_floats(N, H, W, C)
    ws = be.zeros(nws + 4)
    assert be.lib.eegclip_bn2d16_workspace_floats(N, H, W, 96) == 0 and be.lib.eegclip_bn2d16_workspace_floats(1, 1, 1, C) == 0

    def f(**over):
        kw = dict(z=be.ptr(Z), a=be.ptr(A), gamma=be.ptr(v[0]), beta=be.ptr(v[1]), mean=be.ptr(v[2]), rstd=be.ptr(v[3]), running_mean=be.ptr(v[4]), running_var=be.ptr(v[5]),
                  workspace=be.ptr(ws), workspace_floats=nws, N=N, H=H, W=W, C=C, eps=EPS, momentum=MOM, dtype=0)
        kw.update(over)
        return be.lib.eegclip_bn2d16_fwd(byref(_abi.Bn2d16FwdDesc(**kw)), be.stream)

    def b(**over):
        kw = dict(da=be.ptr(D), a=be.ptr(A), z=be.ptr(Z), gamma=be.ptr(v[0]), mean=be.ptr(v[2]), rstd=be.ptr(v[3]), dgamma=be.ptr(v[6]), dbeta=be.ptr(v[7]), dz=be.ptr(O),
                  workspace=be.ptr(ws), workspace_floats=nws, N=N, H=H, W=W, C=C, loss_scale=1.0, dtype=1)
        kw.update(over)
        return be.lib.eegclip_bn2d16_bwd(byref(_abi.Bn2d16BwdDesc(**kw)), be.stream)

    assert f() == 0 and f(running_mean=None, running_var=None) == 0 and b() == 0
    assert f(C=96) == EINVAL and f(C=32) == EINVAL and f(N=0) == EINVAL and f(N=1, H=1, W=1) == EINVAL and f(dtype=2) == EINVAL
    assert f(workspace_floats=nws - 1) == EINVAL and b(workspace_floats=nws - 1) == EINVAL and f(workspace_floats=0) == EINVAL
    assert f(eps=0.0) == EINVAL and f(momentum=1.5) == EINVAL and f(z=None) == EINVAL and f(mean=None) == EINVAL and f(workspace=None) == EINVAL
    assert f(z=be.ptr(Z) + 2) == EALIGN and f(a=be.ptr(A) + 8) == EALIGN and f(gamma=be.ptr(v[0]) + 2) == EALIGN and f(running_var=be.ptr(v[5]) + 1) == EALIGN
    assert b(C=96) == EINVAL and b(N=1, H=1, W=1) == EINVAL and b(dtype=7) == EINVAL and b(loss_scale=0.0) == EINVAL and b(da=None) == EINVAL and b(dz=None) == EINVAL
    assert b(da=be.ptr(D) + 2) == EALIGN and b(dz=be.ptr(O) + 8) == EALIGN and b(dgamma=be.ptr(v[6]) + 2) == EALIGN
    assert be.lib.eegclip_bn2d16_fwd(None, be.stream) == EINVAL and be.lib.eegclip_bn2d16_bwd(None, be.stream) == EINVAL
    be.sync()
