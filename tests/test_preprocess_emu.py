"""The product's preprocessing host code (eeg_image_decode_amd/preprocess.py and the consumers it is wired to) with its kernels under the lane emulator
(tests/emu_patch.py), against PIL (tests/preprocess_ref.py): the checks are tests/preprocess_cases.py's, shared with tests/test_preprocess_gpu.py."""
import numpy as np
import pytest
import torch

import preprocess_cases as cases
import preprocess_ref as R
from clip_vision_ref import pixel_batch
from eeg_image_decode_amd import clip_text, clip_vision, datasets, git_caption, low_level, preprocess, sdxl   # noqa: F401  (before product_on_emulator(): it patches the loaded modules)
from emu_patch import product_on_emulator

pytestmark = pytest.mark.emu


def test_presets_on_emulator():
    with product_on_emulator():
        cases.check_presets("cpu")


def test_feature_cache_on_emulator(tmp_path):
    with product_on_emulator():
        cases.check_feature_cache(str(tmp_path), "cpu")


def test_open_clip_vit_h_text_encoder_is_the_text_side_of_vit_h_14():
    """the constructor's configuration (no weights are built: a 24-layer tower on the meta device), and head dim 64"""
    with torch.device("meta"):
        m = clip_text.open_clip_vit_h_text_encoder()
    c = m.config
    assert (c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads, c.hidden_act, c.projection_dim) == (1024, 4096, 24, 16, "gelu", 1024)
    assert c.hidden_size // c.num_attention_heads == 64 and m.text_projection.weight.shape == (1024, 1024)


def test_encode_image_takes_what_the_feature_extractor_takes():
    """StandInSDXLPipeline.encode_image: a PIL list (and a uint8 array) gives what the tensor from clip_image_processor gives, bit for bit; a tensor behaves
    as before (tests/test_clip_vision_emu.py pins that path)"""
    enc = clip_vision.CLIPVisionEncoder(128, 256, 1, 2, "gelu", 1024, image_size=28, seed=7)
    unet = sdxl.SDXLShapedUNet(stage_layers=(1, 0, 0, 0, 0), seed=5)
    pipe = sdxl.StandInSDXLPipeline(unet, sdxl.DDIMScheduler(), device="cpu", default_sample_size=4, image_encoder=enc)
    ims = cases.pil_images()
    with product_on_emulator():
        px = preprocess.clip_image_processor(ims, size=28, device="cpu")
        by_tensor, neg = pipe.encode_image(px)
        by_pil, neg2 = pipe.encode_image(ims)
        one = pipe.encode_image(np.asarray(ims[0]))[0]
        plain = pipe.encode_image(pixel_batch(1, 28, seed=8, zero_sample=False))[0]
    assert px.shape == (3, 3, 28, 28) and by_tensor.shape == (3, 1024) and torch.equal(by_pil, by_tensor) and torch.equal(neg, neg2) and not neg.any()
    assert torch.equal(one[0], by_tensor[0]) and plain.shape == (1, 1024) and torch.isfinite(by_pil).all()


class _Words:
    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(int(i)) for i in ids)


def test_caption_images_takes_pil_and_decoded_images():
    """git_caption.caption_images: a PIL list == the tensor from clip_image_processor; a float (B, 3, H, W) batch with in_range=(-1, 1) (a VAE decode) is
    quantised as diffusers' postprocess(output_type="pil") does and gets the pixels PIL gives on those bytes; without in_range such a tensor raises as before"""
    import git_cases as G
    model = G.captioner("f16", 128)
    tower = clip_vision.CLIPVisionEncoder(128, 256, 1, 2, "quick_gelu", None, image_size=28, post_layernorm_all=True, seed=9)
    ims = cases.pil_images()
    decoded = torch.rand(2, 3, 40, 52, generator=torch.Generator().manual_seed(3)) * 2.4 - 1.2
    as_bytes = np.ascontiguousarray(((decoded / 2 + 0.5).clamp(0, 1).numpy() * 255).round().astype(np.uint8).transpose(0, 2, 3, 1))
    with product_on_emulator():
        px = preprocess.clip_image_processor(ims, size=28, device="cpu")
        by_tensor = git_caption.caption_images(px, _Words(), model, tower, max_length=4)
        by_pil = git_caption.caption_images(ims, _Words(), model, tower, max_length=4)
        px_dec = preprocess.clip_image_processor(decoded, size=28, device="cpu", in_range=(-1, 1))
        px_bytes = preprocess.clip_image_processor(as_bytes, size=28, device="cpu")
        by_decoded = git_caption.caption_images(decoded, _Words(), model, tower, max_length=4, in_range=(-1, 1))
        by_bytes = git_caption.caption_images(px_bytes, _Words(), model, tower, max_length=4)
        with pytest.raises(Exception, match="resized and cropped by the caller"):
            git_caption.caption_images(decoded, _Words(), model, tower, max_length=4)
    assert by_pil == by_tensor and len(by_pil) == 3 and all(isinstance(s, str) and s for s in by_pil)
    assert torch.equal(px_dec, px_bytes) and by_decoded == by_bytes and len(by_decoded) == 2
    for i in range(2):
        R.assert_normalized(px_dec[i], *R.clip_image_processor_ref(as_bytes[i], size=28))


def test_train_low_level_takes_image_batches_with_image_size():
    """train_low_level(vae=, image_size=): a uint8 (B, H, W, 3) batch from the loader is vae_preprocess(size=image_size) in the VAE's dtype -- the same losses as
    the float batch made by hand; float batches and image_size=None are untouched"""
    seen = []

    class _VAE:
        dtype, scaling_factor = torch.float16, 0.5

        def encode(self, x):
            seen.append(x)
            return torch.zeros(x.shape[0], 4, 2, 2)

    class _Trainer:
        def __init__(self, model, **kw):
            pass

        def step(self, eeg, target, subject_id):
            return target.float().sum() + eeg.sum()

        def sync_model(self):
            pass

    class _Model:
        device = torch.device("cpu")

    u8 = np.random.default_rng(2).integers(0, 256, (2, 20, 26, 3), dtype=np.uint8)
    saved, low_level.LowLevelTrainer = low_level.LowLevelTrainer, _Trainer
    try:
        with product_on_emulator():
            want = preprocess.vae_preprocess(u8, size=16, dtype=torch.float16, device="cpu")
            low_level.train_low_level(_Model(), [(torch.zeros(2, 3), u8)], 1, vae=_VAE(), image_size=16)
            low_level.train_low_level(_Model(), [(torch.zeros(2, 3), want)], 1, vae=_VAE(), image_size=16)
            low_level.train_low_level(_Model(), [(torch.zeros(2, 3), want)], 1, vae=_VAE())
    finally:
        low_level.LowLevelTrainer = saved
    assert len(seen) == 3 and all(torch.equal(s, want) for s in seen) and want.shape == (2, 3, 16, 16) and want.dtype == torch.float16
    for i in range(2):
        R.assert_normalized(want[i], *R.vae_ref(u8[i], size=16))
