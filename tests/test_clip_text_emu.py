"""The product's CLIPTextEncoder host code with its kernels under the lane emulator (tests/emu_patch.py), against the fp32 restatement: the CPU-side
cover of clip_text.py's forward (layer order, packed q | k | v, strides of the fused buffer, pooling index) beside tests/test_kernels_clip_text.py."""
import pytest
import torch

from clip_text_ref import Ref, prompt_ids
from eeg_image_decode_amd import clip_text          # (before product_on_emulator(): it patches the modules already loaded)
from emu_patch import product_on_emulator

pytestmark = pytest.mark.emu


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_reduced_encoder_on_emulator(act):
    """1 prompt, 128 wide, 2 heads, 2 layers, fp16.  Bound: the fp16 bound of tests/test_clip_text_gpu.py (4e-3 on every output)."""
    m = clip_text.CLIPTextEncoder(128, 512, 2, 2, act, projection_dim=128, dtype=torch.float16)
    ids = torch.tensor([prompt_ids(9, 0)])
    with product_on_emulator():
        out = m(ids, output_hidden_states=True)
        again = m(ids, output_hidden_states=True)
    want = Ref(m.state_dict(), 2, act)(ids)
    pairs = list(zip(out.hidden_states, want["hidden_states"])) + [(out.last_hidden_state, want["last_hidden_state"]),
                                                                   (out.pooler_output, want["pooler_output"]), (out.text_embeds, want["text_embeds"])]
    for a, b in pairs:
        assert float((a.float() - b).norm() / b.norm()) < 4e-3
    assert torch.equal(out.text_embeds, again.text_embeds) and out[0] is out.text_embeds
    assert torch.equal(out.pooler_output[0], out.last_hidden_state[0, 10])          # BOS + 9 tokens: <|endoftext|> at position 10


def test_pipeline_encode_prompt_on_emulator():
    """StandInSDXLPipeline.encode_prompt with two reduced encoders (128 and 256 wide, 2 layers) and a synthetic-vocabulary tokenizer pair: the first
    encoder stops one layer early, hidden_states[-2] of both are concatenated, pooled = the second encoder's text_embeds; clip_skip and prompt_ids"""
    from eeg_image_decode_amd.sdxl import DDIMScheduler, SDXLShapedUNet, StandInSDXLPipeline
    from test_clip_text_layout import _synthetic_vocab
    vocab, merges = _synthetic_vocab()
    t1, t2 = clip_text.BPETokenizer(vocab, merges), clip_text.BPETokenizer(vocab, merges, pad_token="!")
    e1 = clip_text.CLIPTextEncoder(128, 512, 2, 2, "quick_gelu", None, vocab_size=len(vocab), seed=1)
    e2 = clip_text.CLIPTextEncoder(256, 512, 2, 4, "gelu", 128, vocab_size=len(vocab), seed=2)
    pipe = StandInSDXLPipeline(SDXLShapedUNet(stage_layers=(1, 0, 0, 0, 0)), DDIMScheduler(), device="cpu", text_encoder=e1, text_encoder_2=e2, tokenizer=t1,
                               tokenizer_2=t2)
    prompts = ["the cat!", ""]
    r1, r2 = Ref(e1.state_dict(), 2, "quick_gelu"), Ref(e2.state_dict(), 4, "gelu")
    a, b = r1(torch.tensor(t1(prompts))), r2(torch.tensor(t2(prompts)))
    with product_on_emulator():
        pe, npe, pooled, npooled = pipe.encode_prompt(prompts, 2, do_classifier_free_guidance=True)
        skip = pipe.encode_prompt(prompts, 2, clip_skip=1)
        by_ids = pipe.encode_prompt(None, 2, prompt_ids=(t1(prompts), t2(prompts)))
        neg = pipe.encode_prompt(prompts[:1], 1, do_classifier_free_guidance=True, negative_prompt="hello")
    err = lambda x, y: float((x.float() - y).norm() / y.norm())
    assert pe.shape == (2, 77, 384) and pooled.shape == (2, 128) and not npe.any() and not npooled.any()
    assert err(pe, torch.cat([a["hidden_states"][-2], b["hidden_states"][-2]], -1)) < 4e-3 and err(pooled, b["text_embeds"]) < 4e-3
    assert err(skip[0], torch.cat([a["hidden_states"][-3], b["hidden_states"][-3]], -1)) < 4e-3
    assert torch.equal(by_ids[0], pe) and torch.equal(by_ids[2], pooled)
    assert neg[1].any() and not torch.equal(neg[1], neg[0])
    with pytest.raises(Exception, match="vocab.json"):
        StandInSDXLPipeline(pipe.unet, DDIMScheduler(), device="cpu", text_encoder=e1, text_encoder_2=e2).encode_prompt("a cat", 1)
