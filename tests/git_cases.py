"""The seeded test cases of the GIT caption decoder shared by tests/test_git_caption_emu.py and tests/test_git_caption_gpu.py: a reduced GITCaptioner whose
greedy captions are decided by a margin the 16-bit formats cannot close, and everything the reference (tests/git_ref.py) says about it, computed once on the CPU.

  * weights: seeded_parameters (PyTorch's default init under seed 0, built on the CPU so that every machine gets the same numbers), every matrix times 3 so that
    the samples do not all decode alike, and the LM head's rows times exp(head_sigma g_v), g_v ~ N(0, 1): a vocabulary with a few likely tokens, as a trained
    head has.  With 515 equally likely tokens (head_sigma = 0) the reference's own top-1 / top-2 gap is ~0.1 of max|logit| at a typical step and no seed
    keeps it above 4 eps for 21 steps in bf16, whose format error is 7 x fp16's; head_sigma is 1 for fp16 and 2 for bf16.
  * e_fmt: relative L2 between the restatement and the restatement with its activations rounded to the I/O dtype at every layer boundary (both on the
    module's own 16-bit weights): the error the format alone causes.  The HIP path is held to 3 x e_fmt (the margin tests/test_clip_text_gpu.py uses
    between the path and its rounded restatement), and eps = 3 e_fmt max|logit| is what that bound can move a logit by.
  * the visual features' seed is chosen (on the CPU, with the restatement alone) so that at every step of every sample the reference's top-1 / top-2 gap
    is >= 4 eps and at least two of the samples decode differently; `Case.check()` asserts both before a test looks at the HIP output.
"""
import functools
from types import SimpleNamespace

import torch

from eeg_image_decode_amd.git_caption import GITCaptioner
from git_ref import GitRef

TINY = dict(vocab_size=515, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, max_position_embeddings=64)
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
HEAD_SIGMA = {"f16": 1.0, "bf16": 2.0}
INIT_SCALE = 3.0


@functools.lru_cache(maxsize=None)
def captioner(dt, vision):
    """the reduced model on the CPU (its weights are the test's data; a GPU test moves it with .to("cuda"))"""
    m = GITCaptioner(dtype=DTYPES[dt], seed=0, vision_hidden_size=vision, **TINY)
    g = torch.randn(TINY["vocab_size"], generator=torch.Generator().manual_seed(99))
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(INIT_SCALE)
        m.output.weight.mul_(torch.exp(HEAD_SIGMA[dt] * g)[:, None].to(DTYPES[dt]))
    return m


def rel_l2(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


@functools.lru_cache(maxsize=None)
def case(dt, P, B, vision, feat_seed, max_length):
    m = captioner(dt, vision)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    ref, rounded = GitRef(sd, TINY["num_attention_heads"]), GitRef(sd, TINY["num_attention_heads"], round_to=DTYPES[dt])
    vis = torch.randn(B, P, vision, generator=torch.Generator().manual_seed(feat_seed)).to(DTYPES[dt])
    ids, steps = ref.greedy(vis.float(), max_length)
    full = ref(ids, vis.float())
    e_fmt = rel_l2(rounded(ids, vis.float()), full)
    eps = 3 * e_fmt * float(full.abs().max())
    top2 = torch.stack(steps, 1).topk(2, -1).values
    c = SimpleNamespace(dt=dt, P=P, B=B, model=m, ref=ref, rounded=rounded, vis=vis, ids=ids, steps=steps, e_fmt=e_fmt, eps=eps,
                        gap=float((top2[..., 0] - top2[..., 1]).min()), max_length=max_length)

    def check():
        assert len({tuple(r) for r in ids.tolist()}) >= 2, "the samples all decode alike: raise the init scale"
        assert c.gap >= 4 * c.eps, f"the reference's own top-1 / top-2 gap {c.gap:.3g} is below 4 eps = {4 * c.eps:.3g}: choose another seed"
    c.check = check
    return c


def eps_uses(c, hip_ids):
    """the restatement teacher-forced on the HIP ids: the number of steps at which the HIP token is not the reference's arg-max (each must then be
    within eps of the maximum)"""
    logits = c.ref(hip_ids, c.vis.float())
    uses = 0
    pad, eos = c.model.config.pad_token_id, c.model.config.eos_token_id
    for b in range(hip_ids.shape[0]):
        done = False
        for t in range(1, hip_ids.shape[1]):
            tok, row = int(hip_ids[b, t]), logits[b, t - 1]
            if done:
                assert tok == pad
                continue
            if tok != int(row.argmax()):
                assert float(row.max() - row[tok]) <= c.eps, f"sample {b}, step {t}: token {tok} is {float(row.max() - row[tok]):.3g} below the maximum"
                uses += 1
            done = tok == eos
    return uses
