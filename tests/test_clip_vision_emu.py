"""The product's CLIPVisionEncoder host code with its kernels under the lane emulator (tests/emu_patch.py), against the fp32 restatement
(tests/clip_vision_ref.py): the CPU-side cover of clip_vision.py's forward (patch rows -> GEMM -> position + pre_layrnorm, the shared layer loop at head dim
64 and 80, the pooled row read in place, the projection) and of the places it plugs into (StandInSDXLPipeline.encode_image / ip_adapter_image=,
git_caption.caption_images), beside tests/test_kernels_clip_vision.py and tests/test_kernels_attn80.py."""
import pytest
import torch

from clip_vision_ref import Ref, pixel_batch
from eeg_image_decode_amd import clip_vision, datasets, git_caption, sdxl          # noqa: F401  (before product_on_emulator(): it patches the loaded modules)
from emu_patch import product_on_emulator

pytestmark = pytest.mark.emu

CASES = {
    # 128 wide / 2 heads of 64 / 2 layers, post_layernorm on every token: GIT's tower, reduced
    "dim64_git": dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, hidden_act="quick_gelu", projection_dim=None,
                      post_layernorm_all=True),
    # 640 wide / 8 heads of 80 / 2 layers / projection 128: 640 is the smallest width that is a multiple of 80 and of gemm16's 128
    "dim80_projection": dict(hidden_size=640, intermediate_size=1280, num_hidden_layers=2, num_attention_heads=8, hidden_act="gelu", projection_dim=128),
}


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


@pytest.mark.parametrize("name", list(CASES))
def test_reduced_tower_on_emulator(name):
    """image 28 x 28 (5 tokens), batch 2 with one all-zero sample, fp16.  Bound on every output: tests/test_clip_text_emu.py's fp16 bound (relative L2 < 4e-3;
    the same layers at the same depth); two runs bit-identical."""
    kw = CASES[name]
    m = clip_vision.CLIPVisionEncoder(image_size=28, dtype=torch.float16, seed=3, **kw)
    with torch.no_grad():                                                    # LayerNorm parameters away from 1 / 0, so that their order matters
        g = torch.Generator().manual_seed(4)
        for n, p in m.named_parameters():
            if "norm" in n:
                p.copy_((torch.randn(p.shape, generator=g) * 0.2 + (1.0 if n.endswith("weight") else 0.0)).to(p.dtype))
    px = pixel_batch(2, 28, seed=5)
    with product_on_emulator():
        out = m(px, output_hidden_states=True)
        again = m(px.half(), output_hidden_states=True)                      # (fp16 pixels: the copy path of patch_rows16; the same rounded values)
    want = Ref(m.state_dict(), kw["num_attention_heads"], kw["hidden_act"], post_layernorm_all=kw.get("post_layernorm_all", False))(px.half().float())
    assert len(out.hidden_states) == 3 and out.last_hidden_state.shape == (2, 5, kw["hidden_size"])
    pairs = [(f"hidden_states[{i}]", a, b) for i, (a, b) in enumerate(zip(out.hidden_states, want["hidden_states"]))]
    pairs += [("last_hidden_state", out.last_hidden_state, want["last_hidden_state"]), ("pooler_output", out.pooler_output, want["pooler_output"])]
    if kw["projection_dim"] is not None:
        pairs.append(("image_embeds", out.image_embeds, want["image_embeds"]))
        assert out[0] is out.image_embeds
    else:
        assert out.image_embeds is None and out[0] is out.last_hidden_state
    for what, a, b in pairs:
        e = _rel(a, b)
        print(f"\n[rel-l2] {name} {what}: {e:.2e}", end=" ")
        assert a.shape == b.shape and torch.isfinite(a).all() and e < 4e-3, (what, e)
    for a, b in zip(out.hidden_states + (out.last_hidden_state, out.pooler_output), again.hidden_states + (again.last_hidden_state, again.pooler_output)):
        assert torch.equal(a, b)
    assert not torch.equal(out.last_hidden_state[0], out.last_hidden_state[1])              # (the all-zero sample and the random one)


def test_normalisation_folded_into_the_first_kernel():
    """forward(raw 0..255 pixels, mean, std, rescale = 1 / 255) against forward(the normalised pixels): hidden_states[0] within fp16 rounding of the input"""
    m = clip_vision.CLIPVisionEncoder(128, 256, 1, 2, "gelu", None, image_size=28, seed=1)
    raw = torch.rand(2, 3, 28, 28, generator=torch.Generator().manual_seed(2)) * 255
    mean, std = torch.tensor(clip_vision.CLIP_MEAN), torch.tensor(clip_vision.CLIP_STD)
    norm = (raw / 255 - mean[None, :, None, None]) / std[None, :, None, None]
    with product_on_emulator():
        a = m(raw, output_hidden_states=True, mean=clip_vision.CLIP_MEAN, std=clip_vision.CLIP_STD, rescale=1 / 255).hidden_states[0]
        b = m(norm, output_hidden_states=True).hidden_states[0]
    assert _rel(a, b) < 2e-3


def test_three_launches_from_pixels_to_hidden_states_0():
    """a tower without layers: the C ABI calls of one forward are patch_rows16, gemm16, embed_ln16 (hidden_states[0] is complete) and post_layernorm"""
    from eeg_image_decode_amd import ops16
    m = clip_vision.CLIPVisionEncoder(128, 256, 0, 2, "gelu", None, image_size=28, seed=1)
    calls = []

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            return lambda *a: (calls.append(name), fn(*a))[1]

    with product_on_emulator() as elib:
        saved, ops16.lib = ops16.lib, (lambda: Counting(elib))
        try:
            out = m(pixel_batch(2, 28), output_hidden_states=True)
        finally:
            ops16.lib = saved
    assert calls == ["eegclip_patch_rows16", "eegclip_gemm16", "eegclip_embed_ln16", "eegclip_layernorm16"]
    assert len(out.hidden_states) == 1 and torch.equal(out.last_hidden_state, out.hidden_states[0])


def test_embed_ln16_wrapper_checks_its_operands():
    """ops16.embed_ln16 sees what the C entry point cannot: ranks, dtypes and lengths"""
    from eeg_image_decode_amd._lib import EegclipError
    from eeg_image_decode_amd.ops16 import embed_ln16
    x, pos, w, b = torch.zeros(10, 128).half(), torch.zeros(5, 128).half(), torch.ones(128).half(), torch.zeros(128).half()
    with product_on_emulator():
        assert embed_ln16(x, pos, w, b, 1e-5).shape == (10, 128)
        assert embed_ln16(torch.zeros(10, 256).half()[:, ::2], pos, w, b, 1e-5).shape == (10, 128)         # (strided columns: made contiguous)
        for bad in ((x.float(), pos, w, b), (x[0], pos, w, b), (x, pos.bfloat16(), w, b), (x, pos[:, :64], w, b), (x, pos, w.float(), b), (x, pos, w, b[:64]),
                    (x[:0], pos, w, b)):
            with pytest.raises(EegclipError):
                embed_ln16(*bad, 1e-5)


def _reduced_pipe(enc):
    unet = sdxl.SDXLShapedUNet(stage_layers=(1, 0, 0, 0, 0), seed=5)          # (one attention slot: the image tokens reach it, the emulator stays quick)
    return sdxl.StandInSDXLPipeline(unet, sdxl.DDIMScheduler(), device="cpu", default_sample_size=4, image_encoder=enc)


def test_pipeline_encode_image_and_ip_adapter_image_on_emulator():
    """StandInSDXLPipeline(image_encoder=) with a reduced encoder (128 wide, 1 layer, projection 1024 = the image projection's input): encode_image returns
    (image_embeds, zeros); generate_ip_adapter_embeds(ip_adapter_image=) is generate_ip_adapter_embeds(ip_adapter_embeds=encode_image(..)[0]) bit for bit;
    without an encoder it raises as before"""
    enc = clip_vision.CLIPVisionEncoder(128, 256, 1, 2, "gelu", 1024, image_size=28, seed=7)
    px = pixel_batch(1, 28, seed=8, zero_sample=False)
    pipe = _reduced_pipe(enc)
    want = Ref(enc.state_dict(), 2, "gelu")(px.half().float())["image_embeds"]
    gen = lambda: torch.Generator().manual_seed(11)
    with product_on_emulator():
        emb, neg = pipe.encode_image(px)
        two = pipe.encode_image(px, num_images_per_prompt=2)[0]
        by_image = pipe.generate_ip_adapter_embeds(prompt="", ip_adapter_image=px, num_inference_steps=1, guidance_scale=0.0, generator=gen()).images
        by_embeds = pipe.generate_ip_adapter_embeds(prompt="", ip_adapter_embeds=emb, num_inference_steps=1, guidance_scale=0.0, generator=gen()).images
        with pytest.raises(Exception, match="not both"):
            pipe.generate_ip_adapter_embeds(prompt="", ip_adapter_image=px, ip_adapter_embeds=emb, num_inference_steps=1)
    assert emb.shape == (1, 1024) and emb.dtype == torch.float16 and neg.shape == emb.shape and not neg.any()
    assert _rel(emb, want) < 4e-3 and two.shape == (2, 1024) and torch.equal(two[0], emb[0]) and torch.equal(two[1], emb[0])
    assert torch.equal(by_image, by_embeds) and torch.isfinite(by_image).all()
    bare = sdxl.StandInSDXLPipeline(pipe.unet, pipe.scheduler, device="cpu", default_sample_size=4)
    with pytest.raises(Exception, match="needs the CLIP image encoder"):
        bare.generate_ip_adapter_embeds(prompt="", ip_adapter_image=px, num_inference_steps=1)
    with pytest.raises(Exception, match="needs the CLIP image encoder"):
        bare.encode_image(px)


class _Words:
    """a decoder stand-in: ids -> the ids as text"""

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(int(i)) for i in ids)


def test_caption_images_is_caption_of_the_towers_tokens():
    import git_cases as G
    model = G.captioner("f16", 128)
    tower = clip_vision.CLIPVisionEncoder(128, 256, 1, 2, "quick_gelu", None, image_size=28, post_layernorm_all=True, seed=9)
    px = pixel_batch(2, 28, seed=10)
    with product_on_emulator():
        tokens = tower(px).last_hidden_state
        direct = git_caption.caption(tokens, _Words(), model, max_length=4)
        through = git_caption.caption_images(px, _Words(), model, tower, max_length=4)
    assert tokens.shape == (2, 5, 128) and through == direct and len(through) == 2 and all(isinstance(s, str) and s for s in through)


def test_image_features_rows_on_emulator():
    """datasets.image_features: the encoder's image_embeds in batches, fp32, each row divided by its norm (or not)"""
    enc = clip_vision.CLIPVisionEncoder(128, 256, 1, 2, "gelu", 128, image_size=28, seed=12)
    px = pixel_batch(3, 28, seed=13, zero_sample=False)
    with product_on_emulator():
        feats = datasets.image_features(px, enc, batch_size=2)
        raw = datasets.image_features(px, enc, normalize=False, batch_size=2)
        whole = enc(px).image_embeds
    assert feats.shape == (3, 128) and feats.dtype == torch.float32
    assert torch.allclose(feats.norm(dim=-1), torch.ones(3), atol=1e-5)
    assert torch.equal(raw, whole.float())                                   # (rows do not depend on the batch they are computed in)
    assert torch.allclose(feats, raw / raw.norm(dim=-1, keepdim=True))
    with pytest.raises(Exception, match="visual_projection"):
        datasets.image_features(px, clip_vision.CLIPVisionEncoder(128, 256, 1, 2, "gelu", None, image_size=28))
