"""CPU checks of the CLIP vision towers' host side: state_dict layout against transformers' own models, the fp32 restatement (tests/clip_vision_ref.py)
against transformers' forward at both head dims, the constructor's and the forward's rejections.  The tests that need transformers use importorskip; they
run wherever it is installed."""
import pytest
import torch

from clip_vision_ref import Ref, normalise_keys, pixel_batch
from eeg_image_decode_amd import clip_vision
from eeg_image_decode_amd._lib import EegclipError

VIT_H = dict(hidden_size=1280, intermediate_size=5120, num_attention_heads=16, hidden_act="gelu", projection_dim=1024)          # the IP-Adapter's image_encoder
VIT_L = dict(hidden_size=1024, intermediate_size=4096, num_attention_heads=16, hidden_act="quick_gelu")                          # GIT-large's git.image_encoder
SMALL_80 = dict(hidden_size=160, intermediate_size=256, num_attention_heads=2, hidden_act="gelu", projection_dim=96)
SMALL_64 = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, hidden_act="quick_gelu")


def _shapes(sd):
    return {k: tuple(v.shape) for k, v in sd.items()}


@pytest.mark.parametrize("which", ["ip_adapter_image_encoder", "git_vision_tower"])
def test_state_dict_layout_equals_transformers(which):
    """names and shapes at the real widths, depth reduced to 2 on both sides (on the meta device: nothing is allocated)"""
    transformers = pytest.importorskip("transformers")
    with torch.device("meta"):
        if which == "ip_adapter_image_encoder":
            hf = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(num_hidden_layers=2, image_size=224, patch_size=14, **VIT_H))
            ours = clip_vision.CLIPVisionEncoder(1280, 5120, 2, 16, "gelu", 1024, device="meta")
        else:
            hf = transformers.GitVisionModel(transformers.GitVisionConfig(num_hidden_layers=2, image_size=224, patch_size=14, **VIT_L))
            ours = clip_vision.CLIPVisionEncoder(1024, 4096, 2, 16, "quick_gelu", None, post_layernorm_all=True, device="meta")
    want, got = _shapes(hf.state_dict()), _shapes(ours.state_dict())
    assert set(got) == set(want), set(got) ^ set(want)
    assert got == want
    assert all(v.dtype == torch.float16 and v.device.type == "meta" for v in ours.state_dict().values())


def test_factories_and_key_names():
    """the factories' configurations and key names hold without transformers too"""
    h, g = clip_vision.ip_adapter_image_encoder(device="meta"), clip_vision.git_vision_tower(device="meta")
    ch, cg = h.config, g.config
    assert (ch.hidden_size, ch.intermediate_size, ch.num_hidden_layers, ch.num_attention_heads, ch.hidden_act, ch.projection_dim) == (1280, 5120, 32, 16, "gelu", 1024)
    assert (cg.hidden_size, cg.intermediate_size, cg.num_hidden_layers, cg.num_attention_heads, cg.hidden_act, cg.projection_dim) == (1024, 4096, 24, 16, "quick_gelu", None)
    assert cg.post_layernorm_all and not ch.post_layernorm_all
    kh, kg = _shapes(h.state_dict()), _shapes(g.state_dict())
    assert kh["vision_model.embeddings.class_embedding"] == (1280,) and kh["vision_model.embeddings.patch_embedding.weight"] == (1280, 3, 14, 14)
    assert kh["vision_model.embeddings.position_embedding.weight"] == (257, 1280) and kh["visual_projection.weight"] == (1024, 1280)
    assert {"vision_model.pre_layrnorm.weight", "vision_model.post_layernorm.bias", "vision_model.encoder.layers.23.self_attn.out_proj.bias",
            "vision_model.encoder.layers.0.mlp.fc1.weight", "vision_model.encoder.layers.5.layer_norm2.weight"} <= set(kg) and "visual_projection.weight" not in kg
    assert len(kh) == 3 + 2 + 32 * 16 + 2 + 1 and len(kg) == 3 + 2 + 24 * 16 + 2


def test_git_prefixed_state_dict_loads():
    """a full GIT state dict: the tower's keys under git.image_encoder., everything else dropped"""
    a = clip_vision.CLIPVisionEncoder(128, 256, 1, 2, "quick_gelu", None, image_size=28, post_layernorm_all=True, seed=1)
    b = clip_vision.CLIPVisionEncoder(128, 256, 1, 2, "quick_gelu", None, image_size=28, post_layernorm_all=True, seed=2)
    sd = {"git.image_encoder." + k: v for k, v in a.state_dict().items()}
    sd["git.embeddings.word_embeddings.weight"] = torch.zeros(3, 3)
    sd["output.weight"] = torch.zeros(3, 3)
    b.load_state_dict(sd)
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    assert set(normalise_keys(sd)) >= set(a.state_dict())
    b.load_state_dict(a.state_dict())                                       # and without the prefix


def test_rejections_and_no_cpu_forward():
    E = clip_vision.CLIPVisionEncoder
    with pytest.raises(EegclipError):
        E(128, 512, 1, 4, "gelu", device="meta")                            # head dim 32
    with pytest.raises(EegclipError):
        E(384, 512, 1, 4, "gelu", device="meta")                            # head dim 96
    with pytest.raises(EegclipError):
        E(160, 512, 1, 2, "gelu", device="meta")                            # head dim 80, but 160 is no multiple of 128
    with pytest.raises(EegclipError):
        E(128, 512, 1, 2, "relu", device="meta")
    with pytest.raises(EegclipError):
        E(128, 512, 1, 2, "gelu", image_size=30, device="meta")
    with pytest.raises(EegclipError):
        E(128, 512, 1, 2, "gelu", dtype=torch.float32, device="meta")
    m = E(128, 512, 1, 2, "gelu", image_size=28)
    with pytest.raises(EegclipError):                                       # weights on the CPU: an error, not an eager forward
        m(torch.zeros(1, 3, 28, 28))
    with pytest.raises(EegclipError):                                       # another size: resizing is the caller's
        m(torch.zeros(1, 3, 42, 42))
    with pytest.raises(EegclipError):
        m(torch.zeros(1, 3, 28, 28), interpolate_pos_encoding=True)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("name", ["clip_projection_dim80", "git_dim64"])
def test_restatement_equals_transformers_fp32(name):
    """tests/clip_vision_ref.py against transformers' forward in fp32 at both head dims (160 wide / 2 heads of 80 with a projection: CLIPVisionModelWithProjection;
    128 wide / 2 heads of 64: GitVisionModel), image 28, patch 14, 2 layers: relative L2 of every hidden state and every output.  Bound 1e-5."""
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    px = pixel_batch(3, 28, seed=1)
    if name == "git_dim64":
        hf = transformers.GitVisionModel(transformers.GitVisionConfig(num_hidden_layers=2, image_size=28, patch_size=14, **SMALL_64)).eval()
        act, post_all = "quick_gelu", True
    else:
        hf = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(num_hidden_layers=2, image_size=28, patch_size=14, **SMALL_80)).eval()
        act, post_all = "gelu", False
    with torch.no_grad():                                                   # (random LayerNorm / class parameters: the default initialisation is 1 / 0)
        for n, p in hf.named_parameters():
            if "norm" in n:                                                 # every LayerNorm: weights around 1, biases around 0
                p.copy_(torch.randn_like(p) * 0.3 + (1.0 if n.endswith(".weight") else 0.0))
            elif "class_embedding" in n:
                p.copy_(torch.randn_like(p) * 0.3)
        ref = Ref(hf.state_dict(), 2, act, post_layernorm_all=post_all)
        o = hf(pixel_values=px, output_hidden_states=True)
        r = ref(px)
    assert ref.L == 2 and len(o.hidden_states) == len(r["hidden_states"]) == 3
    assert _rel(o.hidden_states[1], o.hidden_states[0]) > 1e-2 and _rel(o.hidden_states[2], o.hidden_states[1]) > 1e-2      # (the layers do something)
    pairs = [(f"hidden_states[{i}]", a, b) for i, (a, b) in enumerate(zip(r["hidden_states"], o.hidden_states))]
    pairs.append(("last_hidden_state", r["last_hidden_state"], o.last_hidden_state))
    if name == "git_dim64":
        assert o[0] is o.last_hidden_state
    else:
        pairs.append(("image_embeds", r["image_embeds"], o.image_embeds))
        pairs.append(("pooler_output", r["pooler_output"], hf.vision_model(pixel_values=px).pooler_output))
        assert o[0] is o.image_embeds
    for what, a, b in pairs:
        e = _rel(a, b)
        print(f"\n[rel-l2] {name} {what}: {e:.2e}", end=" ")
        assert a.shape == b.shape and e < 1e-5, (what, e)
