"""Race screen for the token-block kernels' counted waits (csrc/token_block.hip: the weight ring, the fragments carried across phase boundaries,
the residual rows requested ahead of a barrier that no longer drains vmcnt).  A wrong count does not show as a tolerance failure but as a rare
wrong tile: a register read before its load has landed.  Nothing in these kernels may vary from run to run -- there are no atomics in them -- so
the same seed and inputs, run 8 times, must give every tensor they write bit for bit: the fp32 activations, the LayerNorm statistics, the five
forward and the four backward token planes, dctx, dr1 and the parameter partial rows."""
import numpy as np
import pytest
import torch

from conftest import SEED
from eeg_image_decode_amd import synthetic as syn
from test_token_block import _model

RUNS = 8
FWD = ["h", "qkv", "r1", "mu1", "rs1", "f1", "r2", "mu2", "rs2", "n3", "mu3", "rs3", "xp", "hp", "ctxp", "n1p", "g1p"]
BWD_IN = ["dn3", "dqkvp"]                                        # what the layers above / the attention backward hand to the two backward parts
BWD = ["df2p", "dg1p", "da1p", "dr1p", "dctx", "dr1", "tb_part"]


def _bits(t):
    return t.detach().contiguous().view(torch.uint8).cpu().numpy().copy()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("train,subject", [(True, 1), (False, 10), (True, None)])
def test_every_output_of_the_block_kernels_is_bitwise_reproducible(B, train, subject, monkeypatch):
    monkeypatch.setenv("EEGCLIP_TOKEN_BLOCK", "1")
    m = _model("cuda")
    m.train(train)
    x = torch.from_numpy(syn.eeg_batch(SEED + 41, B)).cuda()
    tgt = torch.from_numpy(syn.unit_features(SEED + 41, B, tag="img")).cuda()
    first = None
    for run in range(RUNS):
        m.zero_grad(set_to_none=True)
        torch.manual_seed(2468)                                  # the engine draws the step's Philox seed from torch's generator
        z = m(x, subject)
        (z * tgt).sum().backward()
        torch.cuda.synchronize()
        eng = m._engine()
        assert "eegclip_token_block_fwd" in eng.plans[next(k for k in eng.plans if k[0] == "f")].op_names()
        assert "eegclip_token_block_bwd" in eng.plans[next(k for k in eng.plans if k[0] == "b")].op_names()
        bufs = eng.bufs[B]
        got = {k: _bits(bufs[k]) for k in FWD + BWD_IN + BWD if k in bufs}
        assert set(FWD[:12] + FWD[13:] + BWD[:3] + BWD[4:]) <= set(got)      # (xp and dr1p exist only where the value embedding's gradient wants them)
        if first is None:
            first = got
            continue
        for k in FWD:
            if k in got:
                assert np.array_equal(got[k], first[k]), f"{k} differs between run 0 and run {run}"
        # the backward parts are functions of the forward's tensors and of dn3 / the dq | dk | dv planes: where those arrived bit-identical
        # (they do unless a kernel above accumulates with atomics), so must everything the parts write
        if all(np.array_equal(got[k], first[k]) for k in BWD_IN):
            for k in BWD:
                if k in got:
                    assert np.array_equal(got[k], first[k]), f"{k} differs between run 0 and run {run}"
        else:
            pytest.fail("the backward parts' inputs (dn3, dqkvp) differ between runs: " + ", ".join(k for k in BWD_IN if not np.array_equal(got[k], first[k])))
