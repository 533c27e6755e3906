"""CLIPTextEncoder on the MI355X against the fp32 restatement of transformers' CLIP text models (tests/clip_text_ref.py, pinned to transformers by
tests/test_clip_text_layout.py), run on the module's own 16-bit weights.  Error measure: relative L2, |hip - ref| / |ref|, of every entry of hidden_states,
of last_hidden_state, pooler_output and text_embeds; prompts of 0 / 9 / 40 / 75 tokens with both pad ids; default module initialisation.

Bounds: 3 x the largest value measured over all outputs, both pad ids, per model and dtype (the path is deterministic from run to run: the margin covers
other seeds and prompt lengths, not noise), under caps that come from the reference alone:
  (i)  fp16, hidden_states[-2]: <= 4e-3, and <= a third of what swapping quick_gelu <-> gelu in the RESTATEMENT moves hidden_states[-2] of the very model
       under test (computed in the test, on the model's weights: with PyTorch's default initialisation, N(0, 1) embeddings, it is 2.2e-3 for the reduced
       model, 5.0e-3 for the first encoder, 8.0e-3 for the second; 1.2e-2 - 1.4e-2 is what transformers' own initialisation gives) -- so the test tells the
       two encoders' activations apart.  bf16 cannot resolve the activation at model level; tests/test_kernels_clip_text.py does at kernel level.
  (ii) <= 1e-2 (fp16) / 4e-2 (bf16), the whole-UNet bounds of tests/test_sdxl_unet_gpu.py.
Measured (largest over all outputs | hidden_states[-2]):   reduced  fp16 6.3e-4 | 4.8e-4   bf16 5.9e-3 | 3.9e-3
                                                            encoder 1 fp16 1.06e-3 | 1.00e-3  bf16 8.8e-3 | 8.0e-3
                                                            encoder 2 fp16 1.68e-3 | 1.59e-3  bf16 1.34e-2 | 1.28e-2
so 3 x measured is 1.9e-3 / 1.8e-2, 3.2e-3 / 2.6e-2 and 5.0e-3 / 4.0e-2; the second encoder's pair is cut to 4e-3 / 4e-2 by (i) and (ii).  The error grows
with depth (the 16-bit residual stream is rounded after every layer): 2.3e-4 at the embeddings, 1.6e-3 after 32 layers in fp16."""
import pytest
import torch

from clip_text_ref import Ref, prompt_batch
from eeg_image_decode_amd import clip_text
from eeg_image_decode_amd._lib import EegclipError

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
BOUNDS = {"reduced": {F16: 1.9e-3, BF16: 1.8e-2}, "text_encoder": {F16: 3.2e-3, BF16: 2.6e-2}, "text_encoder_2": {F16: 4e-3, BF16: 4e-2}}
PIPELINE_BOUND = {F16: 1.8e-3, BF16: 1.4e-2}       # tests/test_sdxl_text_prompt_gpu.py: 2-layer encoders of SDXL's widths, measured 6.0e-4 / 4.7e-3
REDUCED = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2)


def rel(a, b, what=""):
    a, b = a.float(), b.float()
    r = float((a - b).norm() / b.norm())
    print(f"\n[rel-l2] {what} {r:.3e}", end=" ")
    return r


def ref_of(m):
    return Ref(m.state_dict(), m.config.num_attention_heads, m.config.hidden_act, eps=m.config.layer_norm_eps, device="cuda")


def compare(m, ref, ids, tag=""):
    """every output of one forward against the restatement -> (the largest relative L2, that of hidden_states[-2]); each one printed"""
    out = m(ids, output_hidden_states=True)
    want = ref(ids)
    torch.cuda.synchronize()
    L = m.config.num_hidden_layers
    assert len(out.hidden_states) == L + 1 and all(h.shape == (ids.shape[0], ids.shape[1], m.config.hidden_size) for h in out.hidden_states)
    errs = []
    for i, (a, b) in enumerate(zip(out.hidden_states, want["hidden_states"])):
        assert torch.isfinite(a.float()).all()
        errs.append(rel(a, b, f"{tag} hidden_states[{i}]"))
    hs2 = errs[-2]
    errs.append(rel(out.last_hidden_state, want["last_hidden_state"], f"{tag} last_hidden_state"))
    errs.append(rel(out.pooler_output, want["pooler_output"], f"{tag} pooler_output"))
    if m.config.projection_dim is not None:
        assert out[0] is out.text_embeds and out.text_embeds.shape == (ids.shape[0], m.config.projection_dim)
        errs.append(rel(out.text_embeds, want["text_embeds"], f"{tag} text_embeds"))
    else:
        assert out[0] is out.last_hidden_state and out.text_embeds is None
    return max(errs), hs2


def check_model(m, name, tag):
    """both pad ids against BOUNDS[name]; fp16: hidden_states[-2] also under cap (i) of the module docstring, from the restatement alone"""
    dtype, bound = m.dtype, BOUNDS[name][m.dtype]
    ref = ref_of(m)
    other = Ref(m.state_dict(), m.config.num_attention_heads, "gelu" if m.config.hidden_act == "quick_gelu" else "quick_gelu", device="cuda")
    for pad in (49407, 0):
        ids = prompt_batch(pad)
        worst, hs2 = compare(m, ref, ids, f"{tag} {str(dtype).split('.')[-1]} pad{pad}")
        assert worst < bound, (worst, bound)
        if dtype == F16:
            swap = rel(other(ids)["hidden_states"][-2], ref(ids)["hidden_states"][-2], f"{tag} restatement, activations swapped, hidden_states[-2]")
            assert hs2 < min(4e-3, swap / 3), (hs2, swap)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_reduced_encoder(act, dtype):
    """128 wide, 2 heads, 3 layers, projection 128.  Bound 1.9e-3 (fp16) / 1.8e-2 (bf16); measured 6.2e-4 - 6.3e-4 / 5.5e-3 - 5.9e-3; hidden_states[-2] in
    fp16 4.8e-4 against a swap distance of 2.2e-3."""
    m = clip_text.CLIPTextEncoder(hidden_act=act, projection_dim=128, dtype=dtype, device="cuda", **REDUCED)
    check_model(m, "reduced", f"reduced {act}")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_sdxl_text_encoder(dtype):
    """the full first encoder (CLIP ViT-L/14 text tower, quick_gelu).  Bound 3.2e-3 (fp16) / 2.6e-2 (bf16); measured 1.06e-3 / 8.8e-3; hidden_states[-2] in
    fp16 1.00e-3 against a swap distance of 5.0e-3."""
    check_model(clip_text.sdxl_text_encoder(dtype=dtype, device="cuda"), "text_encoder", "text_encoder")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_sdxl_text_encoder_2(dtype):
    """the full second encoder (OpenCLIP bigG text tower, gelu, text_projection).  Bound 4e-3 (fp16) / 4e-2 (bf16), both caps; measured 1.68e-3 / 1.34e-2;
    hidden_states[-2] in fp16 1.59e-3 against a swap distance of 8.0e-3."""
    check_model(clip_text.sdxl_text_encoder_2(dtype=dtype, device="cuda"), "text_encoder_2", "text_encoder_2")
    torch.cuda.empty_cache()


def _small(dtype=F16, **kw):
    return clip_text.CLIPTextEncoder(hidden_act="gelu", projection_dim=128, dtype=dtype, device="cuda", **REDUCED, **kw)


def test_causality_end_to_end():
    """ids at positions >= 60 changed: hidden_states[-2][:, :60] bit-identical, later positions different"""
    m = _small()
    ids = prompt_batch(49407, lengths=(75, 70))
    ids2 = ids.clone()
    ids2[:, 60:] = torch.randint(1, 40000, ids2[:, 60:].shape, generator=torch.Generator().manual_seed(3))
    a = m(ids, output_hidden_states=True).hidden_states[-2]
    b = m(ids2, output_hidden_states=True).hidden_states[-2]
    assert torch.equal(a[:, :60], b[:, :60])
    assert not torch.equal(a[:, 60:], b[:, 60:])


def test_two_forwards_are_bit_identical_and_partial_runs_agree():
    m = _small()
    ids = prompt_batch(0)
    a, b = m(ids, output_hidden_states=True), m(ids, output_hidden_states=True)
    for x, y in zip(a.hidden_states + (a.last_hidden_state, a.pooler_output, a.text_embeds), b.hidden_states + (b.last_hidden_state, b.pooler_output, b.text_embeds)):
        assert torch.equal(x, y)
    part = m(ids, output_hidden_states=True, num_layers=2)                # the first two layers only: the same hidden states, no pooled outputs
    assert len(part.hidden_states) == 3 and all(torch.equal(x, y) for x, y in zip(part.hidden_states, a.hidden_states))
    assert part.last_hidden_state is None and part.pooler_output is None and part.text_embeds is None
    assert m(ids).hidden_states is None
    one = m(ids[1].tolist())                                              # a plain list of ids: one prompt
    assert torch.equal(one.text_embeds[0], a.text_embeds[1])


def test_load_state_dict_takes_effect_on_the_next_forward():
    """the packed q | k | v weights are rebuilt after load_state_dict (cache keyed on the parameters' version)"""
    m, other = _small(seed=0), _small(seed=1)
    ids = prompt_batch(49407)
    before = m(ids, output_hidden_states=True)
    m.load_state_dict(other.state_dict())
    after = m(ids, output_hidden_states=True)
    want = other(ids, output_hidden_states=True)
    assert not torch.equal(before.hidden_states[1], after.hidden_states[1])
    for x, y in zip(after.hidden_states + (after.text_embeds,), want.hidden_states + (want.text_embeds,)):
        assert torch.equal(x, y)


def test_rejections():
    m = _small()
    ids = prompt_batch(49407)
    for bad in (49408, -1):
        ids2 = ids.clone()
        ids2[1, 5] = bad
        with pytest.raises(EegclipError):
            m(ids2)
    with pytest.raises(EegclipError):
        m(torch.zeros(1, 78, dtype=torch.long))
    with pytest.raises(EegclipError):
        m(ids, attention_mask=torch.ones_like(ids))
    with pytest.raises(EegclipError):
        m(ids.float())
    with pytest.raises(EegclipError):
        m(ids, num_layers=4)


def test_no_library_gemm_on_the_path(monkeypatch):
    """tests/test_sdxl_gpu.py's rule for this module: no nn.Linear / F.linear / F.layer_norm / F.embedding / matmul call during a forward"""
    m = _small()
    ids = prompt_batch(49407)
    want = m(ids, output_hidden_states=True)

    def forbidden(*a, **k):
        raise AssertionError("library op on the text encoder's path")
    for mod, name in ((torch.nn.functional, "linear"), (torch.nn.Linear, "forward"), (torch.nn.functional, "layer_norm"), (torch.nn.LayerNorm, "forward"),
                      (torch.nn.functional, "embedding"), (torch.nn.Embedding, "forward"), (torch, "matmul"), (torch, "bmm"), (torch.nn.functional, "gelu"),
                      (torch.nn.functional, "softmax"), (torch.nn.functional, "scaled_dot_product_attention")):
        monkeypatch.setattr(mod, name, forbidden)
    got = m(ids, output_hidden_states=True)
    assert torch.equal(got.text_embeds, want.text_embeds)
