"""GITCaptioner on the GPU against the fp32 restatement (tests/git_ref.py; tests/git_cases.py builds the seeded cases): the reduced config of
tests/test_git_layout.py with vision 192, B = 3, fp16 and bf16, P in {1, 5, 70} image tokens (P = 1: all but one row causal; P = 70: the prefix and the cache
cross a 64-key tile).

Measured on an MI355X (relative L2 of forward's logits, T = 12: HIP against the restatement / the format's own error = the restatement with activations
rounded at every layer boundary against itself; the bound is 3 x the latter, computed by the test, which prints both for every case):
    fp16  P = 1: 1.32e-3 / 1.52e-3    P = 5: 1.62e-3 / 1.47e-3    P = 70: 1.59e-3 / 1.54e-3
    bf16  P = 1: 7.92e-3 / 7.61e-3    P = 5: 7.70e-3 / 8.64e-3    P = 70: 9.39e-3 / 1.01e-2
generate: the ids equal the reference's greedy ids in all six cases, no step within eps of the reference's maximum (eps 0.29 / 0.26 / 0.59 against gaps of
1.33 / 1.35 / 2.93 in fp16; 33 / 64 / 67 against 195 / 433 / 307 in bf16, whose LM head is scaled wider: tests/git_cases.py).
"""
import copy

import pytest
import torch

import git_cases as G
from eeg_image_decode_amd._lib import EegclipError

pytestmark = pytest.mark.gpu

SEEDS = {("f16", 1): 0, ("f16", 5): 1, ("f16", 70): 5, ("bf16", 1): 87, ("bf16", 5): 76, ("bf16", 70): 185}      # chosen on the CPU: tests/git_cases.py
CASES = [pytest.param(dt, P, id=f"{dt}-P{P}") for dt in ("f16", "bf16") for P in (1, 5, 70)]
MAX_LENGTH, B, VISION = 8, 3, 192
_models = {}


def _case(dt, P):
    c = G.case(dt, P, B, VISION, SEEDS[dt, P], MAX_LENGTH)
    if dt not in _models:
        _models[dt] = copy.deepcopy(c.model).to("cuda")
    return c, _models[dt], c.vis.cuda()


@pytest.mark.parametrize("dt,P", CASES)
def test_forward_logits_against_the_restatement(dt, P):
    """T = 12 random ids; HIP relative L2 < 3 x the format's own error (computed here, not fixed in advance); both printed"""
    c, m, vis = _case(dt, P)
    ids = torch.randint(0, G.TINY["vocab_size"], (B, 12), generator=torch.Generator().manual_seed(P))
    want = c.ref(ids, c.vis.float())
    e_fmt = G.rel_l2(c.rounded(ids, c.vis.float()), want)
    got = m(ids, vis)
    err = G.rel_l2(got.cpu(), want)
    print(f"forward {dt} P={P}: HIP relative L2 {err:.3e}, format error {e_fmt:.3e}, bound {3 * e_fmt:.3e}")
    assert got.dtype == torch.float32 and got.shape == (B, 12, G.TINY["vocab_size"]) and got.is_cuda
    assert torch.equal(got, m(ids.cuda(), vis))                             # device ids are copied back and checked; bit-reproducible
    assert err < 3 * e_fmt


@pytest.mark.parametrize("dt,P", CASES)
def test_generate_equals_the_reference_and_the_uncached_path(dt, P):
    c, m, vis = _case(dt, P)
    c.check()                                                                # the reference's own margin, before the HIP output is looked at
    ids = m.generate(vis, max_length=MAX_LENGTH)
    uses = G.eps_uses(c, ids)
    print(f"generate {dt} P={P}: eps {c.eps:.3g}, reference gap {c.gap:.3g}, steps within eps of the maximum: {uses}")
    assert uses == 0
    assert ids.dtype == torch.long and torch.equal(ids, c.ids)
    logits = m(ids, vis).cpu()                                               # cached == uncached on the HIP path
    assert torch.equal(logits[:, :-1].argmax(-1), ids[:, 1:])
    assert torch.equal(m.generate(vis, max_length=MAX_LENGTH, prompt_ids=c.ids[:, :4]), c.ids)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_eos_ends_a_sample_and_pads_it(dt):
    """eos := the token the reference emits at step 3 of sample 0: that sample ends at its first eos (step 3 at the latest) and is pad from then on;
    the others run to their own eos or max_length; the whole loop equals the reference's loop under the same rule"""
    c, m, vis = _case(dt, 5)
    m = copy.deepcopy(m)
    eos = int(c.ids[0, 3])
    m.config.eos_token_id = eos
    want, _ = c.ref.greedy(c.vis.float(), MAX_LENGTH, eos=eos)
    ids = m.generate(vis, max_length=MAX_LENGTH)
    assert torch.equal(ids, want)
    first = c.ids[0].tolist().index(eos)
    assert first <= 3 and int(ids[0, first]) == eos and bool((ids[0, first + 1:] == 0).all())
    for b in range(1, B):
        row = c.ids[b].tolist()
        n = min(row.index(eos) + 1 if eos in row[1:] else len(row), ids.shape[1])
        assert ids[b, :n].tolist() == row[:n] and bool((ids[b, n:] == 0).all())


def test_errors():
    c, m, vis = _case("f16", 5)
    ids = c.ids
    with pytest.raises(EegclipError):
        m(ids, c.vis)                                                        # a CPU tensor
    with pytest.raises(EegclipError):
        m(torch.zeros(B, 65, dtype=torch.long), vis)                         # T beyond max_position_embeddings
    with pytest.raises(EegclipError):
        m(torch.full((B, 4), 515), vis)                                      # an id >= vocab
    with pytest.raises(EegclipError):
        m(ids, vis[:, :0])                                                   # P = 0
    with pytest.raises(EegclipError):
        m.generate(vis, max_length=65)
    with pytest.raises(EegclipError):
        type(m)(hidden_size=96, num_attention_heads=2)
