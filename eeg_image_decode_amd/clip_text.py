"""SDXL's two CLIP text encoders on HIP kernels, and CLIP's tokenizer -- what the reference's pipeline loads beside the UNet and the VAE
(Generation/custom_pipeline.py:456-492, `text_encoder` / `text_encoder_2` / `tokenizer` / `tokenizer_2` of stabilityai/sdxl-turbo) and calls in
encode_prompt (custom_pipeline.py:296-316).

The modules are transformers' CLIPTextModel (CLIP ViT-L/14's text tower) and CLIPTextModelWithProjection (OpenCLIP bigG's); tests/clip_text_ref.py restates
them in fp32 torch and tests/test_clip_text_layout.py pins that restatement to transformers itself:

    x = token_embedding[ids] + position_embedding[:T];  hidden_states = [x]
    per layer:  h = layer_norm1(x); q, k, v = {q,k,v}_proj(h) split into heads of 64
                x = x + out_proj(softmax(q k^T / 8 + causal mask) v)
                x = x + fc2(act(fc1(layer_norm2(x))));  hidden_states.append(x)            act: quick_gelu = x sigmoid(1.702 x), or erf gelu
    last_hidden_state = final_layer_norm(x);  pooler_output = last_hidden_state[b, argmax_t ids[b]];  text_embeds = text_projection(pooler_output)

Arithmetic (the wrappers of ops16.py; no library GEMM, no torch math op, no eager fallback; bit-reproducible): csrc/clip_text.hip gather_rows16 for the embedding and the pooling,
csrc/unet.hip layernorm16, ONE csrc/gemm16.hip launch for q | k | v over a packed weight, the causal form of csrc/self_attn.hip reading that (B T, 3C)
buffer in place, out_proj / fc2 with the residual in the GEMM epilogue, csrc/clip_text.hip act16 between fc1 and fc2.  The nn.Embedding / nn.Linear /
nn.LayerNorm children hold parameters only (the published checkpoints' state_dict keys); they are never called.
"""
import json
import unicodedata
from types import SimpleNamespace

import torch
import torch.nn as nn

from ._lib import EegclipError, require_cuda
from .ops16 import PackedWeights, act16, gather_rows16, layernorm16, linear16, seeded_parameters, self_attention

BOS_ID, EOS_ID = 49406, 49407                  # <|startoftext|>, <|endoftext|> in CLIP's vocabulary (the two highest ids)
ACT_KINDS = {"quick_gelu": 0, "gelu": 1}


# ---------------------------------------------------------------------------------------------------------------------- parameter holders
class _Embeddings(nn.Module):
    def __init__(self, vocab, positions, c):
        super().__init__()
        self.token_embedding, self.position_embedding = nn.Embedding(vocab, c), nn.Embedding(positions, c)


class _Attention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)


class _MLP(nn.Module):
    def __init__(self, c, inner):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(c, inner), nn.Linear(inner, c)


class _Layer(nn.Module):
    def __init__(self, c, inner, eps):
        super().__init__()
        self.self_attn = _Attention(c)
        self.layer_norm1 = nn.LayerNorm(c, eps=eps)
        self.mlp = _MLP(c, inner)
        self.layer_norm2 = nn.LayerNorm(c, eps=eps)


class _Encoder(nn.Module):
    def __init__(self, c, inner, n, eps):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(c, inner, eps) for _ in range(n)])


class _TextTransformer(nn.Module):
    def __init__(self, vocab, positions, c, inner, n, eps):
        super().__init__()
        self.embeddings = _Embeddings(vocab, positions, c)
        self.encoder = _Encoder(c, inner, n, eps)
        self.final_layer_norm = nn.LayerNorm(c, eps=eps)


def clip_layers(layers, cache, x, B, T, heads, act, causal, head_dim=64):
    """CLIP's encoder layers over x (B T, C), shared by the text towers (causal, head dim 64) and the vision towers (clip_vision.py: no mask, head dim 64 or
    80): packed q | k | v in one gemm16 launch (the packed weight in `cache`, a PackedWeights), attention reading that buffer in place, the residuals in the
    GEMM epilogues.  Returns every layer's output, in order."""
    C = heads * head_dim
    ln = lambda t, mod: layernorm16(t, mod.weight, mod.bias, mod.eps)
    hs = []
    for i, layer in enumerate(layers):
        a, mlp = layer.self_attn, layer.mlp
        ps = [a.q_proj.weight, a.k_proj.weight, a.v_proj.weight, a.q_proj.bias, a.k_proj.bias, a.v_proj.bias]
        w, b = cache.get(("qkv", i), ps, lambda: (torch.cat([p.detach() for p in ps[:3]], 0).contiguous(),
                                                  torch.cat([p.detach() for p in ps[3:]], 0).contiguous()))
        qkv = linear16(ln(x, layer.layer_norm1), w, b).reshape(B, T, 3 * C)
        o = self_attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads, causal=causal, head_dim=head_dim)
        x = linear16(o.reshape(B * T, C), a.out_proj.weight, a.out_proj.bias, x)
        f = act16(linear16(ln(x, layer.layer_norm2), mlp.fc1.weight, mlp.fc1.bias), act)
        x = linear16(f, mlp.fc2.weight, mlp.fc2.bias, x)
        hs.append(x)
    return hs


class CLIPTextOutput:
    """What diffusers' encode_prompt reads from a transformers output: out[0] (text_embeds with a projection, else last_hidden_state), .hidden_states,
    .last_hidden_state, .pooler_output, .text_embeds.  Indexing skips the fields that are None, as transformers' ModelOutput does."""

    def __init__(self, last_hidden_state, pooler_output, text_embeds, hidden_states, projected):
        self.last_hidden_state, self.pooler_output, self.text_embeds, self.hidden_states = last_hidden_state, pooler_output, text_embeds, hidden_states
        order = (text_embeds, last_hidden_state, hidden_states) if projected else (last_hidden_state, pooler_output, hidden_states)
        self._tuple = tuple(v for v in order if v is not None)

    def __getitem__(self, i):
        return self._tuple[i]

    def __len__(self):
        return len(self._tuple)


class CLIPTextEncoder(nn.Module):
    """transformers' CLIPTextModel (projection_dim=None) / CLIPTextModelWithProjection on HIP kernels; state_dict keys and shapes of the published
    text_encoder*/model.safetensors.  Head dim 64 (hidden_size = 64 * num_attention_heads); hidden_size and projection_dim multiples of 128,
    intermediate_size a multiple of 128 (the 16-bit GEMM's shapes).  Weights get PyTorch's default module initialisation under `seed`;
    load_state_dict takes a real checkpoint.  Only the causal mask is applied (diffusers passes no attention_mask)."""

    def __init__(self, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, hidden_act, projection_dim=None, vocab_size=49408,
                 max_position_embeddings=77, layer_norm_eps=1e-5, dtype=torch.float16, device=None, seed=0):
        super().__init__()
        if hidden_size != 64 * num_attention_heads:
            raise EegclipError(f"CLIPTextEncoder: head dim must be 64 (hidden_size {hidden_size}, {num_attention_heads} heads)")
        if hidden_size % 128 or intermediate_size % 128 or (projection_dim is not None and projection_dim % 128):
            raise EegclipError("CLIPTextEncoder: hidden_size, intermediate_size and projection_dim must be multiples of 128 (csrc/gemm16.hip)")
        if hidden_act not in ACT_KINDS:
            raise EegclipError(f"CLIPTextEncoder: hidden_act must be one of {sorted(ACT_KINDS)}; got {hidden_act!r}")
        cfg = self.config = SimpleNamespace()
        cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads = hidden_size, intermediate_size, num_hidden_layers, num_attention_heads
        cfg.hidden_act, cfg.projection_dim, cfg.vocab_size, cfg.max_position_embeddings = hidden_act, projection_dim, vocab_size, max_position_embeddings
        cfg.layer_norm_eps, cfg.eos_token_id, cfg.bos_token_id = layer_norm_eps, 2, 0            # (SDXL's configs: eos_token_id 2 -> argmax pooling)
        with seeded_parameters(self, dtype, device, seed):
            self.text_model = _TextTransformer(vocab_size, max_position_embeddings, hidden_size, intermediate_size, num_hidden_layers, layer_norm_eps)
            if projection_dim is not None:
                self.text_projection = nn.Linear(hidden_size, projection_dim, bias=False)
        self._cache = PackedWeights()

    @property
    def dtype(self):
        return self.text_model.final_layer_norm.weight.dtype

    @property
    def device(self):
        return self.text_model.final_layer_norm.weight.device

    # ---- layers -------------------------------------------------------------------------------------------------------------------------------------
    def _ids(self, input_ids):
        """ids arrive as host data (a tokenizer's output); a device tensor is copied back: every id is range-checked before a kernel indexes with it"""
        ids = torch.as_tensor(input_ids).detach().to("cpu")
        if ids.dim() == 1:
            ids = ids[None]
        if ids.dim() != 2 or ids.dtype.is_floating_point or ids.dtype == torch.bool or ids.numel() == 0:
            raise EegclipError(f"input_ids must be a (B, T) integer tensor; got {tuple(ids.shape)} {ids.dtype}")
        ids = ids.long()
        cfg = self.config
        if ids.shape[1] > cfg.max_position_embeddings:
            raise EegclipError(f"input_ids has {ids.shape[1]} positions; the encoder has {cfg.max_position_embeddings}")
        lo, hi = int(ids.min()), int(ids.max())
        if lo < 0 or hi >= cfg.vocab_size:
            raise EegclipError(f"input_ids outside the vocabulary [0, {cfg.vocab_size}): min {lo}, max {hi}")
        return ids

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None, position_ids=None, output_hidden_states=False, return_dict=True, num_layers=None, **kw):
        """input_ids (B, T <= 77) -> CLIPTextOutput.  num_layers (not in transformers): run the first num_layers layers only and return their
        hidden_states; last_hidden_state / pooler_output / text_embeds are then None (SDXL reads hidden_states[-2] of its first encoder and nothing
        else: the last layer need not run)."""
        if attention_mask is not None or position_ids is not None:
            raise EegclipError("CLIPTextEncoder applies the causal mask alone (diffusers' encode_prompt passes no attention_mask / position_ids)")
        emb = self.text_model.embeddings
        require_cuda(emb.token_embedding.weight, "CLIPTextEncoder's weights")
        cfg = self.config
        ids = self._ids(input_ids)
        B, T = ids.shape
        C, heads, L = cfg.hidden_size, cfg.num_attention_heads, cfg.num_hidden_layers
        n_run = L if num_layers is None else int(num_layers)
        if not 0 <= n_run <= L:
            raise EegclipError(f"num_layers must be in [0, {L}]; got {num_layers}")
        dev, act = self.device, ACT_KINDS[cfg.hidden_act]
        ln = lambda x, mod: layernorm16(x, mod.weight, mod.bias, mod.eps)
        x = gather_rows16(emb.token_embedding.weight, ids.reshape(-1).to(dev), B * T, emb.position_embedding.weight, T)
        hs = [x] + clip_layers(self.text_model.encoder.layers[:n_run], self._cache, x, B, T, heads, act, causal=True)
        x = hs[-1]
        last = pooled = text_embeds = None
        if n_run == L:
            last2 = ln(x, self.text_model.final_layer_norm)
            eos = (torch.arange(B) * T + ids.argmax(dim=-1)).to(dev)                    # first maximum: <|endoftext|> is the vocabulary's highest id
            pooled = gather_rows16(last2, eos, B)
            last = last2.reshape(B, T, C)
            if cfg.projection_dim is not None:
                text_embeds = linear16(pooled, self.text_projection.weight)
        hidden = tuple(h.reshape(B, T, C) for h in hs) if output_hidden_states else None
        return CLIPTextOutput(last, pooled, text_embeds, hidden, cfg.projection_dim is not None)


def sdxl_text_encoder(**kw):
    """stabilityai/sdxl-turbo text_encoder: CLIP ViT-L/14's text tower (196 tensors, 123,060,480 parameters)"""
    return CLIPTextEncoder(768, 3072, 12, 12, "quick_gelu", None, **kw)


def sdxl_text_encoder_2(**kw):
    """stabilityai/sdxl-turbo text_encoder_2: OpenCLIP ViT-bigG/14's text tower with its projection (517 tensors, 694,659,840 parameters)"""
    return CLIPTextEncoder(1280, 5120, 32, 20, "gelu", 1280, **kw)


def open_clip_vit_h_text_encoder(**kw):
    """laion/CLIP-ViT-H-14-laion2B-s32B-b79K's text tower with its projection, in transformers' keys (open_clip ViT-H-14's encode_text: the `text_features`
    of the data sets' feature cache, eegdatasets_leaveone.py:90-106): 1024 wide, 24 layers, 16 heads of 64, gelu, text_embeds (B, 1024)"""
    return CLIPTextEncoder(1024, 4096, 24, 16, "gelu", 1024, **kw)


# ------------------------------------------------------------------------------------------------------------------------------- tokenizer
def empty_prompt_ids(pad_id=EOS_ID, length=77):
    """what CLIP's tokenizer gives for the reference's constant prompt '': [<|startoftext|>, <|endoftext|>, pad ...] (tokenizer pads with
    <|endoftext|> = 49407, tokenizer_2 with "!" = 0) -- needs no vocabulary file"""
    return [BOS_ID, EOS_ID] + [int(pad_id)] * (length - 2)


def _bytes_to_unicode():
    """the byte -> printable character table of byte-level BPE (GPT-2 / CLIP)"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


_SPECIALS = ("<|startoftext|>", "<|endoftext|>")
try:
    import regex as _re
    _PATTERN = _re.compile(r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+")
    _SPACE = _re.compile(r"\s+")
except ImportError:                             # `re` has no \p{..}: letters = word characters that are neither digits nor "_"; digits = \d (Nd only,
    import re as _re                            # \p{N} also has No / Nl such as "²" or "Ⅷ": those fall to the last class here)
    _PATTERN = _re.compile(r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[^\W\d_]+|\d|(?:[^\s\w]|_)+")
    _SPACE = _re.compile(r"\s+")


class BPETokenizer:
    """CLIP's byte-level BPE tokenizer in plain Python (transformers' CLIPTokenizer without ftfy): NFC, whitespace collapsed, lower case, the split
    pattern above, bytes -> unicode table, `</w>` on a word's last symbol, merges by rank; <|startoftext|> ids <|endoftext|>, truncated to
    `model_max_length` keeping <|endoftext|> last, padded with `pad_token` (which, like the two specials, is matched in the raw text first).  vocab: dict token -> id, or a path to vocab.json; merges: list of "a b"
    strings / (a, b) pairs, or a path to merges.txt (its "#version" line is skipped)."""

    def __init__(self, vocab, merges, pad_token="<|endoftext|>", model_max_length=77):
        if isinstance(vocab, str):
            with open(vocab, encoding="utf-8") as f:
                vocab = json.load(f)
        if isinstance(merges, str):
            with open(merges, encoding="utf-8") as f:
                merges = [ln for ln in f.read().split("\n") if ln and not ln.startswith("#version")]
        self.encoder = dict(vocab)
        pairs = [tuple(m.split()) if isinstance(m, str) else tuple(m) for m in merges]
        self.ranks = {p: i for i, p in enumerate(pairs)}
        self.byte = _bytes_to_unicode()
        for t in _SPECIALS + (pad_token,):
            if t not in self.encoder:
                raise EegclipError(f"BPETokenizer: the vocabulary has no {t!r}")
        self.bos_token_id, self.eos_token_id = self.encoder[_SPECIALS[0]], self.encoder[_SPECIALS[1]]
        self.pad_token_id, self.unk_token_id = self.encoder[pad_token], self.encoder[_SPECIALS[1]]
        self.model_max_length = model_max_length
        self._words = {}
        # the special tokens are cut out of the raw text before anything else, the pad token among them, as transformers' tokenizers do: with
        # tokenizer_2's pad_token "!" every "!" of a prompt becomes id 0 on its own (never "!</w>", never merged)
        specials = sorted(set(_SPECIALS + (pad_token,)), key=len, reverse=True)
        self._special_split = _re.compile("(" + "|".join(_re.escape(t) for t in specials) + ")")

    def _bpe(self, word):
        hit = self._words.get(word)
        if hit is not None:
            return hit
        sym = list(word[:-1]) + [word[-1] + "</w>"]
        while len(sym) > 1:
            best = min(((self.ranks.get((a, b), None), i) for i, (a, b) in enumerate(zip(sym, sym[1:])) if (a, b) in self.ranks), default=None)
            if best is None:
                break
            a, b = sym[best[1]], sym[best[1] + 1]
            out, i = [], 0
            while i < len(sym):                                       # every occurrence of the best pair, left to right
                if i + 1 < len(sym) and sym[i] == a and sym[i + 1] == b:
                    out.append(a + b)
                    i += 2
                else:
                    out.append(sym[i])
                    i += 1
            sym = out
        ids = self._words[word] = [self.encoder.get(s, self.unk_token_id) for s in sym]
        return ids

    def encode(self, text):
        """text -> ids without <|startoftext|> / <|endoftext|>, padding or truncation"""
        ids = []
        for k, seg in enumerate(self._special_split.split(text)):
            if k % 2:                                                 # a special token, matched in the raw text
                ids.append(self.encoder[seg])
                continue
            seg = _SPACE.sub(" ", unicodedata.normalize("NFC", seg)).lower()
            for piece in _PATTERN.findall(seg):
                ids.extend([self.encoder[piece]] if piece in _SPECIALS else self._bpe("".join(self.byte[b] for b in piece.encode("utf-8"))))
        return ids

    def __call__(self, text, **kw):
        """str or list of str -> list of `model_max_length` ids per text (always padded to the full length and truncated, as encode_prompt asks)"""
        texts = [text] if isinstance(text, str) else list(text)
        n = self.model_max_length
        rows = []
        for t in texts:
            ids = [self.bos_token_id] + self.encode(t)[:n - 2] + [self.eos_token_id]
            rows.append(ids + [self.pad_token_id] * (n - len(ids)))
        return rows
