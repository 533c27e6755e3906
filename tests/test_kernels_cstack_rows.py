"""csrc/cstack_bwd.hip, cstack_bwd_rows_kernel: the BatchNorm1-backward sums and the spatial-conv weight-gradient slabs from ONE recompute of the tiles
(eegclip_cstack_bwd_stats_w2 + eegclip_cstack_w2_reduce), against autograd of the fp64 torch reference of
Conv2d(1,40,(1,25)) -> AvgPool2d((1,51),(1,5)) -> BatchNorm2d -> ELU -> Conv2d(40,40,(H,1)) (the construction of tests/test_kernels_cstack.py) and against
the entry points it replaces in the training plans, on both backends (CPU lane emulator here, MI355X with -m gpu)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from backends import be, ok  # noqa: F401
from eeg_image_decode_amd import _abi

C, WD = 40, 36


def rnd(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _problem(B, H, seed):
    rng = np.random.default_rng(seed)
    return dict(x=rnd(rng, B, 64, 250), w25=rnd(rng, C, 25, scale=0.2), bias1=rnd(rng, C, scale=0.1), g1=(1 + 0.1 * rnd(rng, C)).astype(np.float32),
                b1=(0.1 * rnd(rng, C)).astype(np.float32), Ws=(rnd(rng, C, C, H) / np.sqrt(C * H)).astype(np.float32), bias2=(0.1 * rnd(rng, C)).astype(np.float32),
                dy2=rnd(rng, B, C, WD))


def _reference(p, B, H):
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=k in ("x", "w25", "g1", "b1", "Ws")) for k, v in p.items()}
    y1 = F.avg_pool2d(F.conv2d(t["x"][:, :H].unsqueeze(1), t["w25"].view(C, 1, 1, 25), t["bias1"]), (1, 51), (1, 5))
    z1 = F.elu(F.batch_norm(y1, None, None, t["g1"], t["b1"], True, 0.1, 1e-5))
    y2 = F.conv2d(z1, t["Ws"].view(C, C, H, 1), t["bias2"]).squeeze(2)
    return t, y1, y2


# (B, H): the real row count (last row block short, sub-groups 2 and 3 idle) | odd H, B no multiple of 4 | full row blocks | several sample groups |
# B > 32 = 4 x 8 groups: a wave walks two samples, so the prefetch and the cross-sample accumulation run
@pytest.mark.parametrize("B,H", [(2, 63), (3, 5), (2, 64), (18, 7), (37, 3)])
def test_cstack_rows_sums_and_weight_gradient(be, B, H):
    p = _problem(B, H, 2000 + 11 * B + H)
    t, y1t, y2t = _reference(p, B, H)
    y2t.backward(t["dy2"])
    y1 = y1t.detach().numpy()
    mean_ref, var_ref = y1.mean((0, 2, 3)), y1.var((0, 2, 3))
    X, W25, BIAS1, G1, B1, DY2, WS = (be.dev(p[k]) for k in ("x", "w25", "bias1", "g1", "b1", "dy2", "Ws"))
    MU, RS = be.dev(mean_ref.astype(np.float32)), be.dev((1 / np.sqrt(var_ref + 1e-5)).astype(np.float32))
    PT = be.dev(np.full(int(be.lib.eegclip_cstack_packed_t_bytes(H)) // 2, 0x7FC0, np.uint16))
    ok(be.lib.eegclip_cstack_pack_t(be.ptr(WS), be.ptr(PT), H, be.stream))
    nrows = int(be.lib.eegclip_cstack_bwd_rows_count(B, H))
    assert nrows == ((H + 1) // 2) * min((B + 3) // 4, 8)
    assert int(be.lib.eegclip_cstack_bwd_rows_count(0, H)) == 0 and int(be.lib.eegclip_cstack_bwd_rows_count(B, 65)) == 0
    nws = int(be.lib.eegclip_cstack_bwd_w2_workspace_floats(B, H))
    PAD = 3                                                             # rows past rows_count: must stay untouched
    DG, DB = be.dev(np.full(C, 0.25, np.float32)), be.dev(np.full(C, -0.25, np.float32))
    DX = be.dev(np.full((B, 64, 250), 7.0, np.float32))
    DWP = be.dev(np.full(int(be.lib.eegclip_cstack_bwd_workspace_floats(B)), np.nan, np.float32))
    DW25 = be.dev(np.ones((C, 25), np.float32))

    def desc(rows):
        return _abi.CstackBwdDesc(B=B, H=H, x=be.ptr(X), xs_b=64 * 250, xs_h=250, w25=be.ptr(W25), bias1=be.ptr(BIAS1), mean1=be.ptr(MU), rstd1=be.ptr(RS),
                                  gamma1=be.ptr(G1), beta1=be.ptr(B1), packed_t=be.ptr(PT), dy2=be.ptr(DY2), rows_out=be.ptr(rows), stat=be.ptr(rows),
                                  nstat=nrows, count=float(B * H * WD), stat_local=None, nstat_local=0, dgamma=be.ptr(DG), dbeta=be.ptr(DB), dx=be.ptr(DX),
                                  dw_partials=be.ptr(DWP), dw25=be.ptr(DW25))

    runs = []
    for _ in range(2):
        ROWS = be.dev(np.full((nrows + PAD, 80), np.nan, np.float64))
        SLABS = be.dev(np.full(nws + 5, np.nan, np.float32))
        d = desc(ROWS)
        ok(be.lib.eegclip_cstack_bwd_stats_w2(ctypes.byref(d), be.ptr(SLABS), be.stream))
        runs.append((ROWS, SLABS, d))
    (ROWS, SLABS, d), (ROWS2, SLABS2, _) = runs
    rows, slabs = be.host(ROWS), be.host(SLABS)
    # 1. rows_count finite rows, nothing past them (rows or slabs) is touched
    assert np.isfinite(rows[:nrows]).all() and np.isnan(rows[nrows:]).all()
    assert np.isfinite(slabs[:nws]).all() and np.isnan(slabs[nws:]).all()
    # 6. bit-reproducible from call to call
    assert np.array_equal(rows[:nrows], be.host(ROWS2)[:nrows]) and np.array_equal(slabs[:nws], be.host(SLABS2)[:nws])
    # 2. the column sums are autograd's dbeta / dgamma
    gb, gg = t["b1"].grad.numpy(), t["g1"].grad.numpy()
    print(f"B={B} H={H}: |sum rows - dbeta|max = {np.abs(rows[:nrows, :40].sum(0) - gb).max():.3e} (|g|max {np.abs(gb).max():.3e}), "
          f"|sum rows - dgamma|max = {np.abs(rows[:nrows, 40:].sum(0) - gg).max():.3e} (|g|max {np.abs(gg).max():.3e})")
    np.testing.assert_allclose(rows[:nrows, :40].sum(0), gb, atol=2e-4 * max(1.0, np.abs(gb).max()))
    np.testing.assert_allclose(rows[:nrows, 40:].sum(0), gg, atol=2e-4 * max(1.0, np.abs(gg).max()))
    # 3. the apply pass fed these rows
    ok(be.lib.eegclip_cstack_bwd_apply(ctypes.byref(d), be.stream))
    dx, gx = be.host(DX), t["x"].grad.numpy()
    np.testing.assert_array_equal(dx[:, H:], 7.0)
    np.testing.assert_allclose(dx[:, :H], gx[:, :H], atol=3e-5 * max(1.0, float(np.abs(gx).max())))
    gw = t["w25"].grad.numpy()
    np.testing.assert_allclose(be.host(DW25) - 1.0, gw, atol=2e-4 * max(1.0, np.abs(gw).max()))
    np.testing.assert_allclose(be.host(DB) + 0.25, gb, atol=2e-4 * max(1.0, np.abs(gb).max()))
    np.testing.assert_allclose(be.host(DG) - 0.25, gg, atol=2e-4 * max(1.0, np.abs(gg).max()))
    # 4. the slabs, reduced: autograd's dWs (an increment onto the sentinel 1.0)
    DWS = be.dev(np.ones((C, C, H), np.float32))
    ok(be.lib.eegclip_cstack_w2_reduce(be.ptr(SLABS), B, H, be.ptr(DWS), be.stream))
    gws = t["Ws"].grad.numpy()
    print(f"B={B} H={H}: |dWs - autograd|max = {np.abs(be.host(DWS) - 1.0 - gws).max():.3e} (|g|max {np.abs(gws).max():.3e})")
    np.testing.assert_allclose(be.host(DWS) - 1.0, gws, atol=1e-4 * max(1.0, np.abs(gws).max()))
    # 5. ... bit-identical to eegclip_cstack_bwd_w2: the same DWS code path
    DWS_B = be.dev(np.ones((C, C, H), np.float32))
    WSP = be.dev(np.full(nws, np.nan, np.float32))
    ok(be.lib.eegclip_cstack_bwd_w2(be.ptr(X), 64 * 250, 250, be.ptr(W25), be.ptr(BIAS1), be.ptr(MU), be.ptr(RS), be.ptr(G1), be.ptr(B1), be.ptr(DY2),
                                    be.ptr(DWS_B), be.ptr(WSP), B, H, be.stream))
    assert np.array_equal(be.host(DWS), be.host(DWS_B))
    assert np.array_equal(be.host(WSP), slabs[:nws])
    # 7. argument checks
    for field in ("rows_out", "packed_t"):
        bad = desc(ROWS)
        setattr(bad, field, None)
        assert be.lib.eegclip_cstack_bwd_stats_w2(ctypes.byref(bad), be.ptr(SLABS), be.stream) < 0, field
    assert be.lib.eegclip_cstack_bwd_stats_w2(ctypes.byref(d), None, be.stream) < 0
    bad = desc(ROWS)
    bad.H = 65
    assert be.lib.eegclip_cstack_bwd_stats_w2(ctypes.byref(bad), be.ptr(SLABS), be.stream) < 0
    bad = desc(ROWS)
    bad.rows_out = be.ptr(ROWS) + 4
    assert be.lib.eegclip_cstack_bwd_stats_w2(ctypes.byref(bad), be.ptr(SLABS), be.stream) < 0
    assert be.lib.eegclip_cstack_w2_reduce(None, B, H, be.ptr(DWS), be.stream) < 0 and be.lib.eegclip_cstack_w2_reduce(be.ptr(SLABS), B, 65, be.ptr(DWS), be.stream) < 0
    assert np.array_equal(be.host(ROWS)[:nrows], rows[:nrows])          # (the rejected calls wrote nothing)
