"""CPU-side pins of the GIT caption decoder: tests/git_ref.py against transformers' GitForCausalLM itself (use_cache=False, the image encoder replaced by
a stub that returns the visual tokens), GITCaptioner's state_dict layout against that model's, and WordPieceDecoder against BertTokenizer.decode."""
import types

import pytest
import torch

from eeg_image_decode_amd._lib import EegclipError
from eeg_image_decode_amd.git_caption import GITCaptioner, WordPieceDecoder
from git_ref import GitRef

transformers = pytest.importorskip("transformers")

TINY = dict(vocab_size=515, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, max_position_embeddings=64)
VISION, P, B = 128, 5, 2


class _Stub(torch.nn.Module):
    """stands where GitVisionModel stood: returns the visual tokens it was given (pixel_values is a rank-4 dummy)"""

    def __init__(self, feats):
        super().__init__()
        self.feats = feats

    def forward(self, pixel_values, **kw):
        return types.SimpleNamespace(last_hidden_state=self.feats.clone())


def _hf_model(seed=0):
    from transformers import GitConfig, GitForCausalLM
    cfg = GitConfig(vision_config=dict(hidden_size=VISION, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2, image_size=32, patch_size=16),
                    bos_token_id=101, eos_token_id=102, pad_token_id=0, **TINY)
    torch.manual_seed(seed)
    m = GitForCausalLM(cfg).eval()
    with torch.no_grad():                                  # wider than the default init (std 0.02): logits that tell tokens apart
        for n, p in m.named_parameters():
            if not n.startswith("git.image_encoder.") and p.dim() == 2:
                p.mul_(4.0)
    return m


@pytest.fixture(scope="module")
def hf():
    m = _hf_model()
    feats = torch.randn(B, P, VISION, generator=torch.Generator().manual_seed(1))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m.git.image_encoder = _Stub(feats)
    return m, sd, feats


def test_restatement_equals_transformers_uncached_forward(hf):
    m, sd, feats = hf
    ids = torch.randint(1, TINY["vocab_size"], (B, 9), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = m(input_ids=ids, pixel_values=torch.zeros(B, 3, 32, 32), use_cache=False).logits[:, P:]
    got = GitRef(sd, TINY["num_attention_heads"])(ids, feats)
    err = float((got - want).norm() / want.norm())
    print(f"restatement vs GitForCausalLM: relative L2 {err:.3e}")
    assert want.shape == got.shape == (B, 9, TINY["vocab_size"]) and err <= 1e-6


def test_restatement_greedy_equals_transformers_generate_uncached(hf):
    m, sd, feats = hf
    with torch.no_grad():
        want = m.generate(pixel_values=torch.zeros(B, 3, 32, 32), max_length=10, do_sample=False, use_cache=False, num_beams=1)
    got, steps = GitRef(sd, TINY["num_attention_heads"]).greedy(feats, 10)
    assert got.shape[1] == want.shape[1] and torch.equal(got, want), (got, want)
    assert len(steps) == got.shape[1] - 1


def test_state_dict_layout_is_gitforcausallm_without_the_image_encoder(hf):
    m, sd, _ = hf
    ours = GITCaptioner(vision_hidden_size=VISION, **TINY)
    want = {k: tuple(v.shape) for k, v in sd.items() if not k.startswith("git.image_encoder.")}
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == want
    ours.load_state_dict(sd)                                                   # the full state dict, image encoder included
    assert torch.equal(ours.output.weight, sd["output.weight"].half())
    assert torch.equal(ours.git.encoder.layer[1].attention.self.key.bias, sd["git.encoder.layer.1.attention.self.key.bias"].half())
    with pytest.raises(RuntimeError, match="nonsense"):
        ours.load_state_dict({**sd, "git.nonsense.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="output.bias"):
        ours.load_state_dict({k: v for k, v in sd.items() if k != "output.bias"})


def test_git_large_defaults_have_the_published_shapes():
    """microsoft/git-large's text side, on the meta device (no memory): 6 layers, 768 wide, 12 heads, vocabulary 30522, 1024 positions, visual tokens of 1024"""
    m = GITCaptioner(device="meta")
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes["git.embeddings.word_embeddings.weight"] == (30522, 768) and shapes["git.embeddings.position_embeddings.weight"] == (1024, 768)
    assert shapes["git.visual_projection.visual_projection.0.weight"] == (768, 1024) and shapes["output.weight"] == (30522, 768)
    assert shapes["git.encoder.layer.5.intermediate.dense.weight"] == (3072, 768) and "git.encoder.layer.6.output.dense.weight" not in shapes
    assert len(shapes) == 4 + 4 + 2 + 6 * 16 and m.dtype == torch.float16
    assert sum(v.numel() for v in m.state_dict().values()) == 2 * 30522 * 768 + 30522 + 1024 * 768 + 2 * 768 + 1024 * 768 + 768 + 2 * 768 + 6 * (
        4 * (768 * 768 + 768) + 2 * 768 + 2 * 768 * 3072 + 3072 + 768 + 2 * 768)


def test_constructor_rejects_shapes_the_kernels_do_not_take():
    for kw in ({"hidden_size": 96}, {"hidden_size": 128, "num_attention_heads": 4}, {"intermediate_size": 200}, {"vision_hidden_size": 100}, {"eos_token_id": 515}):
        with pytest.raises(EegclipError):
            GITCaptioner(**{**TINY, "vision_hidden_size": VISION, **kw})
    with pytest.raises(EegclipError):                                          # no CPU path
        GITCaptioner(vision_hidden_size=VISION, **TINY)(torch.tensor([[101, 5]]), torch.zeros(1, P, VISION, dtype=torch.float16))


# ------------------------------------------------------------------------------------------------------------------------------- ids -> text
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "a", "cat", "sit", "##ting", "##s", "on", "the", "mat", ".", ",", "'", "s", "it", "don", "t", "!", "?",
         "dog", "play", "##ing", "##ful", "we", "re", "ve", "m", "i", "n", "do", "not", "-", "red"]
CASES = [
    ([2, 5, 6, 7, 8, 10, 11, 12, 13, 3], "a cat sitting on the mat."),
    ([2, 11, 22, 15, 16, 23, 25, 6, 9, 14, 17, 23, 9, 20, 3, 0, 0], "the dog's playful cats, it plays!"),
    ([2, 30, 18, 15, 19, 23, 21, 26, 15, 27, 12, 3], "i don't play? we're mat"),
    ([2, 30, 15, 28, 6, 14, 30, 15, 29, 35, 34, 22, 13, 13, 3], "i've cat, i'm red - dog.."),
    ([2, 32, 33, 7, 1, 4, 13, 3], "do not sit."),
    ([2, 3, 0, 0], ""),
]


@pytest.fixture(scope="module")
def vocab_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("git_vocab") / "vocab.txt"
    path.write_text("\n".join(VOCAB) + "\n", encoding="utf-8")
    return str(path)


@pytest.mark.parametrize("ids,text", CASES)
def test_wordpiece_decoder_rules(vocab_file, ids, text):
    """the rules by explicit strings: specials dropped, `##` pieces merged, then the punctuation clean-up"""
    assert WordPieceDecoder(vocab_file).decode(ids) == text
    assert WordPieceDecoder(VOCAB).decode(torch.tensor(ids)) == text


def test_wordpiece_decoder_equals_bert_tokenizer(vocab_file):
    # constructed offline from the synthetic vocabulary (transformers 5 takes it as `vocab`); clean_up_tokenization_spaces=True is what
    # BertTokenizer.decode did by default in the transformers 4 releases the reference ran on
    tok = transformers.BertTokenizer(vocab=vocab_file)
    assert tok.convert_ids_to_tokens([5, 8]) == ["a", "##ting"]
    dec = WordPieceDecoder(vocab_file)
    for ids, _ in CASES:
        assert dec.decode(ids) == tok.decode(ids, skip_special_tokens=True, clean_up_tokenization_spaces=True), ids
    with pytest.raises(EegclipError):
        dec.decode([len(VOCAB)])
