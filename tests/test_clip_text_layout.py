"""CPU checks of the CLIP text encoders' host side: state_dict layout against transformers' own models, the fp32 restatement (tests/clip_text_ref.py)
against transformers' forward, BPETokenizer against transformers' CLIPTokenizer.  The tests that need transformers use importorskip; they run wherever it
is installed."""
import pytest
import torch

from clip_text_ref import Ref, normalise_keys, prompt_batch
from eeg_image_decode_amd import clip_text
from eeg_image_decode_amd._lib import EegclipError

SDXL_1 = dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, hidden_act="quick_gelu", projection_dim=768)
SDXL_2 = dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20, hidden_act="gelu", projection_dim=1280)
SMALL = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2, hidden_act="gelu", projection_dim=128)


def _hf_config(kw):
    from transformers import CLIPTextConfig
    return CLIPTextConfig(vocab_size=49408, max_position_embeddings=77, layer_norm_eps=1e-5, eos_token_id=2, bos_token_id=0, pad_token_id=1, **kw)


def _shapes(sd):
    return {k: tuple(v.shape) for k, v in sd.items()}


@pytest.mark.parametrize("which", ["text_encoder", "text_encoder_2"])
def test_state_dict_layout_equals_transformers(which):
    transformers = pytest.importorskip("transformers")
    with torch.device("meta"):
        hf = transformers.CLIPTextModel(_hf_config(SDXL_1)) if which == "text_encoder" else transformers.CLIPTextModelWithProjection(_hf_config(SDXL_2))
    ours = clip_text.sdxl_text_encoder(device="meta") if which == "text_encoder" else clip_text.sdxl_text_encoder_2(device="meta")
    want, got = _shapes(normalise_keys(hf.state_dict())), _shapes(ours.state_dict())
    assert set(got) == set(want), set(got) ^ set(want)
    assert got == want
    n_tensors, n_params = (196, 123_060_480) if which == "text_encoder" else (517, 694_659_840)
    assert len(got) == n_tensors and sum(p.numel() for p in ours.parameters()) == n_params
    assert all(v.dtype == torch.float16 and v.device.type == "meta" for v in ours.state_dict().values())
    assert ours.config.projection_dim == (None if which == "text_encoder" else 1280)


def test_layout_counts_without_transformers():
    """the counts of the published checkpoints, and their key names, hold without transformers too"""
    e1, e2 = clip_text.sdxl_text_encoder(device="meta"), clip_text.sdxl_text_encoder_2(device="meta")
    assert (len(e1.state_dict()), sum(p.numel() for p in e1.parameters())) == (196, 123_060_480)
    assert (len(e2.state_dict()), sum(p.numel() for p in e2.parameters())) == (517, 694_659_840)
    k1 = set(e1.state_dict())
    assert {"text_model.embeddings.token_embedding.weight", "text_model.embeddings.position_embedding.weight", "text_model.final_layer_norm.bias",
            "text_model.encoder.layers.11.self_attn.out_proj.bias", "text_model.encoder.layers.0.mlp.fc1.weight",
            "text_model.encoder.layers.5.layer_norm2.weight"} <= k1 and "text_projection.weight" not in k1
    assert tuple(e2.state_dict()["text_projection.weight"].shape) == (1280, 1280)


def test_constructor_rejections_and_no_cpu_forward():
    with pytest.raises(EegclipError):
        clip_text.CLIPTextEncoder(128, 512, 1, 3, "gelu", device="meta")                 # head dim != 64
    with pytest.raises(EegclipError):
        clip_text.CLIPTextEncoder(128, 512, 1, 2, "relu", device="meta")
    with pytest.raises(EegclipError):
        clip_text.CLIPTextEncoder(128, 500, 1, 2, "gelu", device="meta")
    with pytest.raises(EegclipError):
        clip_text.CLIPTextEncoder(128, 512, 1, 2, "gelu", dtype=torch.float32, device="meta")
    m = clip_text.CLIPTextEncoder(128, 512, 1, 2, "gelu")
    with pytest.raises(EegclipError):                                                    # weights on the CPU: an error, not an eager forward
        m(clip_text.empty_prompt_ids())
    with pytest.raises(EegclipError):
        m([clip_text.empty_prompt_ids()], attention_mask=torch.ones(1, 77))


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("name", ["small_gelu_projection", "clip_l"])
def test_restatement_equals_transformers_fp32(name):
    """tests/clip_text_ref.py against transformers' forward in fp32, relative L2 of hidden_states[-2], last_hidden_state, pooled, text_embeds over prompts
    of 0 / 9 / 40 / 75 tokens with both pad ids.  Bound 1e-5 (fp32 round-off headroom; measured <= 7e-7)."""
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    if name == "clip_l":
        hf = transformers.CLIPTextModel(_hf_config(SDXL_1)).eval()
    else:
        hf = transformers.CLIPTextModelWithProjection(_hf_config(SMALL)).eval()
    kw = SDXL_1 if name == "clip_l" else SMALL
    ref = Ref(hf.state_dict(), kw["num_attention_heads"], kw["hidden_act"])
    assert ref.L == kw["num_hidden_layers"]
    for pad in (49407, 0):
        ids = prompt_batch(pad)
        with torch.no_grad():
            o = hf(input_ids=ids, output_hidden_states=True)
            r = ref(ids)
        assert len(o.hidden_states) == len(r["hidden_states"]) == kw["num_hidden_layers"] + 1
        pairs = [("hidden_states[-2]", r["hidden_states"][-2], o.hidden_states[-2]), ("last_hidden_state", r["last_hidden_state"], o.last_hidden_state)]
        if name == "clip_l":
            pairs.append(("pooler_output", r["pooler_output"], o.pooler_output))
            assert o[0] is o.last_hidden_state
        else:
            pairs.append(("text_embeds", r["text_embeds"], o.text_embeds))
            assert o[0] is o.text_embeds
        for what, a, b in pairs:
            e = _rel(a, b)
            print(f"\n[rel-l2] {name} pad {pad} {what}: {e:.2e}", end=" ")
            assert e < 1e-5, (what, e)


# ------------------------------------------------------------------------------------------------------------------------------- tokenizer
def _synthetic_vocab():
    """the 256 byte symbols, their `</w>` forms, a dozen merges, the two specials"""
    byte = clip_text._bytes_to_unicode()
    syms = list(byte.values())                                      # (table order: the printable bytes first)
    vocab = {s: i for i, s in enumerate(syms)}                      # "!" = byte 33 is the first printable: id 0, as in CLIP's vocabulary
    assert vocab["!"] == 0
    for s in syms:
        vocab[s + "</w>"] = len(vocab)
    merges = ["t h", "th e</w>", "i n", "a n", "e r", "o n</w>", "an d</w>", "in g</w>", "c a", "ca t</w>", "! !</w>", "' s</w>",
              "h e", "l l", "he ll", "hell o</w>"]
    for m in merges:
        a, b = m.split()
        vocab[a + b] = len(vocab)
    vocab["<|startoftext|>"] = len(vocab)
    vocab["<|endoftext|>"] = len(vocab)
    return vocab, merges


TEXTS = ["", "The cat and THE Hat", "it's John's, don't they've I'm we'll he'd", "route 66 in 1984 x2", "wow!!! ... ?!?! --", "une fiancée dorée à l'été",
         "two  spaces\tand\n newlines ", "hello " * 90, "a photo of a cat, the thing on the mat: hello!! " * 6, "<|endoftext|> in the text", "naïve café №5 ½"]


@pytest.mark.parametrize("pad_token", ["<|endoftext|>", "!"])
def test_bpe_tokenizer_equals_transformers(pad_token):
    transformers = pytest.importorskip("transformers")
    vocab, merges = _synthetic_vocab()
    hf = transformers.CLIPTokenizer(vocab=vocab, merges=[tuple(m.split()) for m in merges], pad_token=pad_token)
    ours = clip_text.BPETokenizer(vocab, merges, pad_token=pad_token)
    want = hf(TEXTS, padding="max_length", max_length=77, truncation=True)["input_ids"]
    got = ours(TEXTS)
    for t, g, w in zip(TEXTS, got, want):
        assert len(g) == 77 and g == list(w), (t, g, list(w))
    assert got[0] == [vocab["<|startoftext|>"], vocab["<|endoftext|>"]] + [vocab[pad_token]] * 75
    assert got[7][-1] == vocab["<|endoftext|>"] and got[7][0] == vocab["<|startoftext|>"]       # truncated: EOS stays last
    assert ours("The cat") == [got_row for got_row in ours(["The cat"])]


def test_bpe_tokenizer_from_files(tmp_path):
    import json
    vocab, merges = _synthetic_vocab()
    (tmp_path / "vocab.json").write_text(json.dumps(vocab), encoding="utf-8")
    (tmp_path / "merges.txt").write_text("#version: 0.2\n" + "\n".join(merges) + "\n", encoding="utf-8")
    a = clip_text.BPETokenizer(str(tmp_path / "vocab.json"), str(tmp_path / "merges.txt"))
    b = clip_text.BPETokenizer(vocab, merges)
    assert a(TEXTS) == b(TEXTS)
    assert b.encode("the cat") == [vocab["the</w>"], vocab["cat</w>"]]
    with pytest.raises(EegclipError):
        clip_text.BPETokenizer({"a": 0}, [])


@pytest.mark.parametrize("pad_token", ["<|endoftext|>", "!"])
def test_empty_prompt_ids(pad_token):
    """[49406, 49407, pad x 75]: what the tokenizers give for '' once BOS / EOS are mapped to CLIP's ids (tokenizer_2's pad "!" is id 0 there as here)"""
    vocab, merges = _synthetic_vocab()
    tok = clip_text.BPETokenizer(vocab, merges, pad_token=pad_token)
    remap = {tok.bos_token_id: 49406, tok.eos_token_id: 49407}
    pad_id = 49407 if pad_token == "<|endoftext|>" else 0
    assert [remap.get(i, i) for i in tok("")[0]] == clip_text.empty_prompt_ids(pad_id)
    transformers = pytest.importorskip("transformers")
    hf = transformers.CLIPTokenizer(vocab=vocab, merges=[tuple(m.split()) for m in merges], pad_token=pad_token)
    assert [remap.get(i, i) for i in hf("", padding="max_length", max_length=77, truncation=True)["input_ids"]] == clip_text.empty_prompt_ids(pad_id)
    assert clip_text.empty_prompt_ids() == [49406, 49407] + [49407] * 75
