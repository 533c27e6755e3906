"""StandInSDXLPipeline with CLIP text encoders on the MI355X: encode_prompt against the restatement's cat(hidden_states_1[-2], hidden_states_2[-2]) /
text_embeds_2 (what StableDiffusionXLPipeline.encode_prompt of diffusers 0.30.0 returns), the sampling loop and Generator4Embeds with a text prompt, and
the unchanged behaviour of a pipeline without encoders.  Encoders of SDXL's widths (768 and 1280) at 2 layers each: (B, 77, 2048) / (B, 1280) come out.
Bounds: 3 x the largest value measured here per dtype (tests/test_clip_text_gpu.py PIPELINE_BOUND, under the caps stated there): 1.8e-3 fp16 (measured
<= 6.0e-4), 1.4e-2 bf16 (measured <= 4.7e-3)."""
import pytest
import torch

from clip_text_ref import Ref
from eeg_image_decode_amd import clip_text
from eeg_image_decode_amd._lib import EegclipError
from eeg_image_decode_amd.sdxl import DDIMScheduler, Generator4Embeds, SDXLShapedUNet, StandInSDXLPipeline
from test_clip_text_gpu import PIPELINE_BOUND as BOUND, rel
from test_clip_text_layout import _synthetic_vocab

pytestmark = pytest.mark.gpu

_state = {}


def encoders(dtype=torch.float16):
    if dtype not in _state:
        e1 = clip_text.CLIPTextEncoder(768, 3072, 2, 12, "quick_gelu", None, dtype=dtype, device="cuda", seed=1)
        e2 = clip_text.CLIPTextEncoder(1280, 5120, 2, 20, "gelu", 1280, dtype=dtype, device="cuda", seed=2)
        r1 = Ref(e1.state_dict(), 12, "quick_gelu", device="cuda")
        r2 = Ref(e2.state_dict(), 20, "gelu", device="cuda")
        _state[dtype] = (e1, e2, r1, r2)
    return _state[dtype]


def tokenizers():
    vocab, merges = _synthetic_vocab()
    return clip_text.BPETokenizer(vocab, merges), clip_text.BPETokenizer(vocab, merges, pad_token="!")


def pipeline(dtype=torch.float16, with_tokenizers=False, **kw):
    e1, e2, _, _ = encoders(dtype)
    t1, t2 = tokenizers() if with_tokenizers else (None, None)
    return StandInSDXLPipeline(SDXLShapedUNet(stage_layers=(1, 1, 1, 1, 1), dtype=dtype, seed=5), DDIMScheduler(), device="cuda", dtype=dtype,
                               default_sample_size=16, text_encoder=e1, text_encoder_2=e2, tokenizer=t1, tokenizer_2=t2, **kw)


def expected(dtype, ids1, ids2, index=-2):
    _, _, r1, r2 = encoders(dtype)
    a, b = r1(torch.tensor(ids1)), r2(torch.tensor(ids2))
    return torch.cat([a["hidden_states"][index], b["hidden_states"][index]], dim=-1), b["text_embeds"]


def check(dtype, got, want, tag):
    pe, _, pooled, _ = got
    assert pe.shape == want[0].shape and pe.shape[1:] == (77, 2048) and pooled.shape == want[1].shape and pooled.shape[1] == 1280 and pe.dtype == dtype
    assert rel(pe, want[0], f"{tag} prompt_embeds") < BOUND[dtype]
    assert rel(pooled, want[1], f"{tag} pooled") < BOUND[dtype]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_empty_prompt_without_tokenizers(dtype):
    """'' through empty_prompt_ids (pad 49407 for the first encoder, 0 for the second).  Measured: 3.7e-4 / 5.7e-4 (prompt_embeds / pooled) fp16, 3.0e-3 / 4.7e-3 bf16."""
    pipe = pipeline(dtype)
    got = pipe.encode_prompt("", 2)
    assert got[1] is None and got[3] is None
    want = expected(dtype, [clip_text.empty_prompt_ids(49407)] * 2, [clip_text.empty_prompt_ids(0)] * 2)
    check(dtype, got, want, "empty")
    with pytest.raises(EegclipError, match="vocab.json"):
        pipe.encode_prompt("a cat", 1)


def test_prompt_list_through_the_tokenizers():
    """a list of prompts through a synthetic-vocabulary BPETokenizer pair; prompt_2 defaults to prompt, and may differ.  Measured: 3.7e-4 / 5.6e-4."""
    dtype = torch.float16
    pipe = pipeline(dtype, with_tokenizers=True)
    prompts = ["The cat and the hat!", "hello, hello: an thing on the mat " * 4, ""]
    t1, t2 = tokenizers()
    ids1, ids2 = t1(prompts), t2(prompts)
    assert ids1 != ids2                                                  # (the pad ids differ, and tokenizer_2 cuts "!" out)
    check(dtype, pipe.encode_prompt(prompts, 3), expected(dtype, ids1, ids2), "list")
    other = ["in the cat", "on", "the the the"]
    check(dtype, pipe.encode_prompt(prompts, 3, prompt_2=other), expected(dtype, ids1, t2(other)), "prompt_2")
    one = pipe.encode_prompt("the cat", 2)                               # one string for a batch of two image embeddings
    assert one[0].shape[0] == 2 and torch.equal(one[0][0], one[0][1])


def test_prompt_ids_and_clip_skip():
    """ids tokenised elsewhere; clip_skip = 1 reads hidden_states[-3] (of these 2-layer encoders: the embeddings).  Measured: 3.7e-4 / 5.7e-4; clip_skip = 1: 2.3e-4 / 5.7e-4."""
    dtype = torch.float16
    pipe = pipeline(dtype)
    g = torch.Generator().manual_seed(0)
    ids = [[49406] + torch.randint(1, 49406, (n,), generator=g).tolist() + [49407] + [pad] * (75 - n) for n, pad in ((5, 49407), (60, 49407))]
    ids2 = [[i if k <= n + 1 else 0 for k, i in enumerate(row)] for row, n in zip(ids, (5, 60))]
    check(dtype, pipe.encode_prompt(None, 2, prompt_ids=(ids, ids2)), expected(dtype, ids, ids2), "prompt_ids")
    got = pipe.encode_prompt(None, 2, prompt_ids=(ids, ids2), clip_skip=1)
    check(dtype, got, expected(dtype, ids, ids2, index=-3), "clip_skip=1")
    with pytest.raises(EegclipError):
        pipe.encode_prompt(None, 2, prompt_ids=(ids, ids2), clip_skip=2)


def test_negative_prompt_under_guidance():
    """no negative prompt under guidance: zeros, as before; a given one is encoded like the prompt.  Measured: 3.7e-4 / 6.0e-4."""
    dtype = torch.float16
    pipe = pipeline(dtype, with_tokenizers=True)
    t1, t2 = tokenizers()
    pe, npe, pooled, npooled = pipe.encode_prompt(["the cat"], 1, do_classifier_free_guidance=True)
    assert not npe.any() and not npooled.any() and npe.shape == pe.shape                 # no negative prompt: zeros, as before
    got = pipe.encode_prompt(["the cat"], 1, do_classifier_free_guidance=True, negative_prompt=["an hat"])
    check(dtype, (got[1], None, got[3], None), expected(dtype, t1(["an hat"]), t2(["an hat"])), "negative")
    check(dtype, got, expected(dtype, t1(["the cat"]), t2(["the cat"])), "positive")


def test_sampling_loop_and_generator_take_a_text_prompt():
    pipe = pipeline(with_tokenizers=True)
    emb = torch.randn(1, 1024, generator=torch.Generator().manual_seed(0)).cuda().half()

    def run(prompt, **kw):
        gen = torch.Generator(device="cuda").manual_seed(0)
        return pipe.generate_ip_adapter_embeds(prompt=prompt, ip_adapter_embeds=emb, num_inference_steps=2, guidance_scale=kw.pop("guidance_scale", 0.0),
                                               generator=gen, **kw).images
    a, b, a2 = run("the cat"), run("hello on the mat"), run("the cat")
    assert a.shape == (1, 4, 16, 16) and torch.isfinite(a.float()).all()
    assert torch.equal(a, a2) and not torch.equal(a, b)
    c = run("the cat", guidance_scale=5.0, negative_prompt="an hat")
    d = run("the cat", guidance_scale=5.0)
    assert torch.isfinite(c.float()).all() and not torch.equal(c, d)
    assert not torch.equal(run("the cat", clip_skip=1), a)
    g4 = Generator4Embeds(num_inference_steps=2, device="cuda", pipe=pipe)
    x = g4.generate(emb[0], text_prompt="the cat", generator=torch.Generator(device="cuda").manual_seed(0))
    y = g4.generate(emb[0], text_prompt="hello", generator=torch.Generator(device="cuda").manual_seed(0))
    assert torch.equal(x, a[0]) and not torch.equal(x, y)


def test_pipeline_without_encoders_is_unchanged():
    pipe = StandInSDXLPipeline(SDXLShapedUNet(stage_layers=(1, 1, 1, 1, 1), seed=5), DDIMScheduler(), device="cuda", default_sample_size=16)
    g = torch.Generator().manual_seed(1234)
    pe = (torch.randn(1, 77, 2048, generator=g) * 0.5).to(device="cuda", dtype=torch.float16)
    pooled = (torch.randn(1, 1280, generator=g) * 0.5).to(device="cuda", dtype=torch.float16)
    got = pipe.encode_prompt("", 2)
    assert torch.equal(got[0], pe.expand(2, -1, -1)) and torch.equal(got[2], pooled.expand(2, -1)) and got[1] is None
    with pytest.raises(EegclipError, match="no text encoder"):
        pipe.encode_prompt("a cat", 1)
    with pytest.raises(EegclipError, match="no text encoder"):
        Generator4Embeds(num_inference_steps=1, device="cuda", pipe=pipe).generate(torch.zeros(1024), text_prompt="a cat")
    with pytest.raises(EegclipError):
        StandInSDXLPipeline(SDXLShapedUNet(stage_layers=(1, 1, 1, 1, 1)), text_encoder=encoders()[0])
