"""The product's GITCaptioner host code with its kernels under the lane emulator (tests/emu_patch.py), against the fp32 restatement: the CPU-side cover of
git_caption.py's forward (packed q | k | v, the prefix mask, the LM head in 16-row launches) and of generate (prefill into the cache, the decode step's
strides, greedy choice, stopping) beside tests/test_kernels_caption.py.  The reduced config of tests/test_git_layout.py, fp16, P = 5, B = 2."""
import pytest
import torch

import git_cases as G
from eeg_image_decode_amd import git_caption          # noqa: F401  (before product_on_emulator(): it patches the modules already loaded)
from emu_patch import product_on_emulator

pytestmark = pytest.mark.emu


@pytest.fixture(scope="module")
def c():
    c = G.case("f16", 5, 2, 128, 7, 6)
    c.check()
    return c


def test_forward_on_emulator(c):
    """logits (B, T, vocab) of the reference's own caption ids: within 3 x the format's error of the restatement, bit-reproducible"""
    with product_on_emulator():
        got = c.model(c.ids, c.vis)
        again = c.model(c.ids, c.vis)
    want = c.ref(c.ids, c.vis.float())
    err = G.rel_l2(got, want)
    print(f"emulator forward: relative L2 {err:.3e}, format error {c.e_fmt:.3e}")
    assert got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got, again)
    assert err < 3 * c.e_fmt


def test_generate_on_emulator(c):
    """a 6-token greedy caption through the cache equals the reference's recomputed greedy loop, and the uncached forward chooses the same tokens"""
    with product_on_emulator():
        ids = c.model.generate(c.vis, max_length=6)
        logits = c.model(ids, c.vis)
        prompted = c.model.generate(c.vis, max_length=6, prompt_ids=c.ids[:, :3])
    assert ids.dtype == torch.long and G.eps_uses(c, ids) == 0
    assert torch.equal(ids, c.ids)
    assert torch.equal(logits[:, :-1].argmax(-1), ids[:, 1:])
    assert torch.equal(prompted, c.ids)                                      # a 3-token prompt: prefill over P + 3 rows, then the same continuation
