"""GIT's caption decoder on HIP kernels: EEG embedding -> text prompt.  In the reference the prompt of the SDXL stage is a caption decoded from the embedding
itself (Generation/modeling_git.py, GitForCausalLMClipEmb: Hugging Face's GitForCausalLM with the vision tower bypassed, the visual tokens handed in at
:1970-1973).  The vision tower (CLIP ViT-L/14) and the reference's image adapter stay outside: the input here is the visual token tensor.

The model (tests/git_ref.py restates it in fp32 torch and tests/test_git_layout.py pins that restatement to transformers' GitForCausalLM, use_cache=False):

    x = cat([LN_v(Linear_v(visual_features)), LN_e(word_embeddings[ids] + position_embeddings[0 .. T-1])], dim=1)        (B, P + T, C); text positions only
    per layer (post-LN BERT):  a = attention(q, k, v) in heads of 64, scale 1/8;  x = LN(dense(a) + x);  x = LN(dense(gelu(intermediate(x))) + x)
    mask:  key j reaches query i iff j <= i or (i < P and j < P), i.e. j < max(i + 1, P)
    logits = output(x[:, P:])

forward() is the uncached path: one csrc/gemm16.hip launch for q | k | v over a packed weight, the prefix-causal form of csrc/self_attn.hip reading that buffer in
place, dense / output.dense with the residual in the GEMM epilogue, csrc/unet.hip layernorm16, csrc/clip_text.hip act16 and gather_rows16; the LM head (30522 rows:
no multiple of the GEMM's tile, and no padded copy of a 47 MB weight) runs on csrc/caption.hip's skinny GEMM, 16 rows per launch.
generate() prefills a (layers, B, Tmax, 2C) cache of [k | v] rows once and then decodes one token per step on csrc/caption.hip: the skinny GEMM at M = B
(q; k | v written straight into the cache row; dense; intermediate; output.dense; LM head -> fp32 logits), decode attention over the cache, layernorm16, act16 and
topk_rows(k = 1) -- 9 launches per layer, 6 * 9 + 4 = 58 per token at GIT-large's depth, and one host read (the chosen ids, for the finished flags).
No library GEMM, no torch math op, no eager fallback; the nn children hold parameters only (the published checkpoint's state_dict keys) and are never called.
"""
from types import SimpleNamespace

import torch
import torch.nn as nn

from ._lib import EegclipError, check, lib, raw_stream, require_cuda
from .ops16 import PackedWeights, act16, decode_attention, gather_rows16, layernorm16, linear16, linear16_skinny, seeded_parameters, self_attention

GELU = 1                                        # act16's kind: the erf GELU (GitConfig.hidden_act = "gelu")
_IGNORED = ("git.image_encoder.", "git.img_temporal_embedding")


# ---------------------------------------------------------------------------------------------------------------------- parameter holders
class _Embeddings(nn.Module):
    def __init__(self, vocab, positions, c, eps):
        super().__init__()
        self.word_embeddings, self.position_embeddings = nn.Embedding(vocab, c), nn.Embedding(positions, c)
        self.LayerNorm = nn.LayerNorm(c, eps=eps)


class _Self(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.query, self.key, self.value = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)


class _Output(nn.Module):
    def __init__(self, cin, c, eps):
        super().__init__()
        self.dense = nn.Linear(cin, c)
        self.LayerNorm = nn.LayerNorm(c, eps=eps)


class _Attention(nn.Module):
    def __init__(self, c, eps):
        super().__init__()
        self.self = _Self(c)
        self.output = _Output(c, c, eps)


class _Intermediate(nn.Module):
    def __init__(self, c, inner):
        super().__init__()
        self.dense = nn.Linear(c, inner)


class _Layer(nn.Module):
    def __init__(self, c, inner, eps):
        super().__init__()
        self.attention = _Attention(c, eps)
        self.intermediate = _Intermediate(c, inner)
        self.output = _Output(inner, c, eps)


class _Encoder(nn.Module):
    def __init__(self, c, inner, n, eps):
        super().__init__()
        self.layer = nn.ModuleList([_Layer(c, inner, eps) for _ in range(n)])


class _Projection(nn.Module):
    def __init__(self, dv, c, eps):
        super().__init__()
        self.visual_projection = nn.Sequential(nn.Linear(dv, c), nn.LayerNorm(c, eps=eps))


class _Git(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = _Embeddings(cfg.vocab_size, cfg.max_position_embeddings, cfg.hidden_size, cfg.layer_norm_eps)
        self.encoder = _Encoder(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.layer_norm_eps)
        self.visual_projection = _Projection(cfg.vision_hidden_size, cfg.hidden_size, cfg.vision_layer_norm_eps)


class GITCaptioner(nn.Module):
    """transformers' GitForCausalLM without its image encoder, on HIP kernels; the defaults are microsoft/git-large's numbers and the state_dict keys and
    shapes are that model's (load_state_dict takes its full state dict: keys under git.image_encoder. and git.img_temporal_embedding are dropped, any
    other unexpected or missing key raises).  Head dim 64 (hidden_size = 64 * num_attention_heads); hidden_size and intermediate_size multiples of 128
    (csrc/gemm16.hip's N), vision_hidden_size a multiple of 64 (a K only).  Weights get PyTorch's default module initialisation under `seed`."""

    def __init__(self, vocab_size=30522, hidden_size=768, num_hidden_layers=6, num_attention_heads=12, intermediate_size=3072, max_position_embeddings=1024,
                 vision_hidden_size=1024, layer_norm_eps=1e-12, bos_token_id=101, eos_token_id=102, pad_token_id=0, dtype=torch.float16, device=None, seed=0,
                 vision_layer_norm_eps=1e-5):
        super().__init__()
        if hidden_size != 64 * num_attention_heads:
            raise EegclipError(f"GITCaptioner: head dim must be 64 (hidden_size {hidden_size}, {num_attention_heads} heads)")
        if hidden_size % 128 or intermediate_size % 128 or vision_hidden_size % 64 or min(hidden_size, intermediate_size, vision_hidden_size) < 1:
            raise EegclipError("GITCaptioner: hidden_size and intermediate_size must be multiples of 128 and vision_hidden_size a multiple of 64 "
                               "(csrc/gemm16.hip)")
        if num_hidden_layers < 1 or vocab_size < 1 or max_position_embeddings < 1:
            raise EegclipError("GITCaptioner: num_hidden_layers, vocab_size and max_position_embeddings must be positive")
        for name, tok in (("bos_token_id", bos_token_id), ("eos_token_id", eos_token_id), ("pad_token_id", pad_token_id)):
            if not 0 <= tok < vocab_size:
                raise EegclipError(f"GITCaptioner: {name} {tok} is outside the vocabulary [0, {vocab_size})")
        cfg = self.config = SimpleNamespace(
            vocab_size=vocab_size, hidden_size=hidden_size, num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads,
            intermediate_size=intermediate_size, max_position_embeddings=max_position_embeddings, vision_hidden_size=vision_hidden_size,
            layer_norm_eps=layer_norm_eps, vision_layer_norm_eps=vision_layer_norm_eps, bos_token_id=bos_token_id, eos_token_id=eos_token_id,
            pad_token_id=pad_token_id, hidden_act="gelu")
        with seeded_parameters(self, dtype, device, seed):
            self.git = _Git(cfg)
            self.output = nn.Linear(hidden_size, vocab_size)
        self._cache = PackedWeights()

    @property
    def dtype(self):
        return self.output.weight.dtype

    @property
    def device(self):
        return self.output.weight.device

    def load_state_dict(self, state_dict, strict=True, **kw):
        """a full GitForCausalLM state dict loads: the image encoder's keys are dropped before the strict check"""
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith(_IGNORED)}, strict=strict, **kw)

    # ---- packed weights -----------------------------------------------------------------------------------------------------------------------------
    def _packed(self, i, s):
        """(q | k | v weight, bias) for the prefill's one launch; the decode step reads its q and k | v parts as row slices of the same tensors"""
        ps = [s.query.weight, s.key.weight, s.value.weight, s.query.bias, s.key.bias, s.value.bias]
        return self._cache.get(("qkv", i), ps, lambda: (torch.cat([p.detach() for p in ps[:3]], 0).contiguous(),
                                                          torch.cat([p.detach() for p in ps[3:]], 0).contiguous()))

    # ---- inputs -------------------------------------------------------------------------------------------------------------------------------------
    def _ids(self, input_ids, B=None):
        """ids arrive as host data; a device tensor is copied back: every id is range-checked before a kernel indexes with it"""
        ids = torch.as_tensor(input_ids).detach().to("cpu")
        if ids.dim() == 1:
            ids = ids[None]
        if ids.dim() != 2 or ids.dtype.is_floating_point or ids.dtype == torch.bool or ids.numel() == 0:
            raise EegclipError(f"input_ids must be a (B, T) integer tensor; got {tuple(ids.shape)} {ids.dtype}")
        ids = ids.long()
        cfg = self.config
        if B is not None and ids.shape[0] != B:
            ids = ids.expand(B, -1) if ids.shape[0] == 1 else ids
            if ids.shape[0] != B:
                raise EegclipError(f"input_ids has {ids.shape[0]} rows; visual_features has {B}")
        if ids.shape[1] > cfg.max_position_embeddings:
            raise EegclipError(f"input_ids has {ids.shape[1]} positions; the decoder has {cfg.max_position_embeddings}")
        lo, hi = int(ids.min()), int(ids.max())
        if lo < 0 or hi >= cfg.vocab_size:
            raise EegclipError(f"input_ids outside the vocabulary [0, {cfg.vocab_size}): min {lo}, max {hi}")
        return ids.contiguous()

    def _visual(self, visual_features):
        require_cuda(self.output.weight, "GITCaptioner's weights")
        if not isinstance(visual_features, torch.Tensor) or visual_features.dim() != 3:
            raise EegclipError("visual_features must be a (B, P, vision_hidden_size) tensor")
        require_cuda(visual_features, "visual_features")
        B, P, Dv = visual_features.shape
        if B < 1 or P < 1 or Dv != self.config.vision_hidden_size:
            raise EegclipError(f"visual_features {tuple(visual_features.shape)}: need B >= 1, P >= 1 image tokens of {self.config.vision_hidden_size} features")
        return visual_features.to(device=self.device, dtype=self.dtype).contiguous()

    # ---- the uncached path --------------------------------------------------------------------------------------------------------------------------
    def _ln(self, x, mod):
        return layernorm16(x, mod.weight, mod.bias, mod.eps)

    def _prefill(self, ids, vis, cache=None):
        """hidden states (B, P + T, C) of the last layer; cache (layers, B, Tmax, 2C): rows [0, P + T) of every layer receive that layer's k | v"""
        cfg, g = self.config, self.git
        B, P, Dv = vis.shape
        T = ids.shape[1]
        S, C, heads = P + T, cfg.hidden_size, cfg.num_attention_heads
        vp = g.visual_projection.visual_projection
        x = torch.empty(B, S, C, dtype=self.dtype, device=self.device)
        x[:, :P] = self._ln(linear16(vis.reshape(B * P, Dv), vp[0].weight, vp[0].bias), vp[1]).reshape(B, P, C)
        emb = g.embeddings
        x[:, P:] = self._ln(gather_rows16(emb.word_embeddings.weight, ids.reshape(-1).to(self.device), B * T, emb.position_embeddings.weight, T),
                            emb.LayerNorm).reshape(B, T, C)
        x = x.reshape(B * S, C)
        for i, layer in enumerate(g.encoder.layer):
            att = layer.attention
            w, b = self._packed(i, att.self)
            qkv = linear16(x, w, b).reshape(B, S, 3 * C)
            if cache is not None:
                cache[i, :, :S] = qkv[..., C:]
            a = self_attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads, prefix=P)
            x = self._ln(linear16(a.reshape(B * S, C), att.output.dense.weight, att.output.dense.bias, x), att.output.LayerNorm)
            f = act16(linear16(x, layer.intermediate.dense.weight, layer.intermediate.dense.bias), GELU)
            x = self._ln(linear16(f, layer.output.dense.weight, layer.output.dense.bias, x), layer.output.LayerNorm)
        return x.reshape(B, S, C)

    @torch.no_grad()
    def forward(self, input_ids, visual_features):
        """input_ids (B, T), visual_features (B, P, vision_hidden_size) -> fp32 logits (B, T, vocab) of the text positions (the uncached path)"""
        vis = self._visual(visual_features)
        ids = self._ids(input_ids, vis.shape[0])
        B, T = ids.shape
        P = vis.shape[1]
        x = self._prefill(ids, vis)
        text = x[:, P:].reshape(B * T, self.config.hidden_size)
        return linear16_skinny(text, self.output.weight, self.output.bias, out_f32=True).reshape(B, T, self.config.vocab_size)

    # ---- the cached path ----------------------------------------------------------------------------------------------------------------------------
    def _greedy(self, logits):
        """fp32 logits (B, vocab) -> the arg-max id per row on the host (ties: the lowest id)"""
        B, V = logits.shape
        out = torch.empty(B, 1, dtype=torch.long, device=logits.device)
        check(lib().eegclip_topk_rows(logits.data_ptr(), B, V, logits.stride(0), 1, None, out.data_ptr(), raw_stream()), "topk_rows")
        return out.reshape(B).cpu()

    def _step(self, tok, t, P, cache):
        """one decoding step: the token ids `tok` (B,) at text position t -> fp32 logits (B, vocab) of the next token; writes cache row P + t"""
        cfg, g = self.config, self.git
        C, heads = cfg.hidden_size, cfg.num_attention_heads
        B = tok.shape[0]
        emb = g.embeddings
        x = self._ln(gather_rows16(emb.word_embeddings.weight, tok.to(self.device), B, emb.position_embeddings.weight[t:t + 1], 1), emb.LayerNorm)
        for i, layer in enumerate(g.encoder.layer):
            att = layer.attention
            w, b = self._packed(i, att.self)
            q = linear16_skinny(x, w[:C], b[:C])
            linear16_skinny(x, w[C:], b[C:], out=cache[i, :, P + t])
            a = decode_attention(q, cache[i], P + t + 1, heads)
            x = self._ln(linear16_skinny(a, att.output.dense.weight, att.output.dense.bias, x), att.output.LayerNorm)
            f = act16(linear16_skinny(x, layer.intermediate.dense.weight, layer.intermediate.dense.bias), GELU)
            x = self._ln(linear16_skinny(f, layer.output.dense.weight, layer.output.dense.bias, x), layer.output.LayerNorm)
        return linear16_skinny(x, self.output.weight, self.output.bias, out_f32=True)

    @torch.no_grad()
    def generate(self, visual_features, max_length=20, prompt_ids=None):
        """greedy decoding (transformers' generate(do_sample=False) on the uncached forward): int64 ids (B, <= max_length) on the host, starting with
        bos or with prompt_ids (B or 1 rows).  A sample that has emitted eos emits pad from then on; the loop ends when every sample has finished or
        at max_length."""
        cfg = self.config
        vis = self._visual(visual_features)
        B, P, _ = vis.shape
        ids = self._ids(torch.full((B, 1), cfg.bos_token_id) if prompt_ids is None else prompt_ids, B)
        max_length = int(max_length)
        if max_length > cfg.max_position_embeddings:
            raise EegclipError(f"max_length {max_length} exceeds the decoder's {cfg.max_position_embeddings} positions")
        if ids.shape[1] >= max_length:
            return ids.clone()
        C = cfg.hidden_size
        cache = torch.empty(cfg.num_hidden_layers, B, P + max_length, 2 * C, dtype=self.dtype, device=self.device)
        T0 = ids.shape[1]
        x = self._prefill(ids, vis, cache)
        logits = linear16_skinny(x[:, P + T0 - 1], self.output.weight, self.output.bias, out_f32=True)
        finished = torch.zeros(B, dtype=torch.bool)
        out = [ids]
        for t in range(T0, max_length):
            nxt = self._greedy(logits)                                     # the one host read of the step
            nxt = torch.where(finished, torch.full_like(nxt, cfg.pad_token_id), nxt)
            out.append(nxt[:, None])
            finished = finished | (nxt == cfg.eos_token_id)
            if bool(finished.all()) or t + 1 == max_length:
                break
            logits = self._step(nxt, t, P, cache)
        return torch.cat(out, dim=1)

    def caption(self, visual_features, decoder, max_length=20, prompt_ids=None):
        """visual tokens -> one caption string per sample (`decoder`: a WordPieceDecoder of the checkpoint's vocab.txt)"""
        return [decoder.decode(row) for row in self.generate(visual_features, max_length, prompt_ids).tolist()]


def caption(visual_features, decoder, model, max_length=20, prompt_ids=None):
    """EEG-side visual tokens -> list[str]: model.generate + decoder.decode; the strings are what Generator4Embeds.generate takes as text_prompt"""
    return model.caption(visual_features, decoder, max_length, prompt_ids)


def caption_images(pixel_values, decoder, model, tower, max_length=20, prompt_ids=None, in_range=None):
    """images -> list[str]: GIT's own vision tower (clip_vision.git_vision_tower(), loaded from the same checkpoint's git.image_encoder.* keys) in front of
    `caption`.  pixel_values (B, 3, 224, 224), preprocessed; or, as GIT's processor takes them, something that is not a torch.Tensor (a PIL image, a list
    of them, a uint8 array); or with in_range=(lo, hi) a float (B, 3, H, W) tensor of any size whose values run from lo (black) to hi (white) -- a decoded
    image straight from the VAE, in_range=(-1, 1).  The last two go through preprocess.clip_image_processor first."""
    if not isinstance(pixel_values, torch.Tensor) or in_range is not None:
        from .preprocess import clip_image_processor
        pixel_values = clip_image_processor(pixel_values, size=tower.config.image_size, device=tower.device, in_range=in_range)
    return caption(tower(pixel_values).last_hidden_state, decoder, model, max_length, prompt_ids)


# ---------------------------------------------------------------------------------------------------------------------- ids -> text
class WordPieceDecoder:
    """ids -> text as BERT's uncased tokenizer decodes them (transformers' BertTokenizer.decode(ids, skip_special_tokens=True)), in plain Python: drop
    the special tokens, join the pieces with spaces, merge `##` continuation pieces into the word before them, then the punctuation clean-up.  Only
    decoding: GIT's captions start from bos, nothing is ever encoded.  vocab_path: vocab.txt, one token per line, line number = id."""

    SPECIALS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")
    _CLEAN = ((" .", "."), (" ?", "?"), (" !", "!"), (" ,", ","), (" ' ", "'"), (" n't", "n't"), (" 'm", "'m"), (" 's", "'s"), (" 've", "'ve"), (" 're", "'re"))

    def __init__(self, vocab_path):
        if isinstance(vocab_path, (list, tuple)):
            self.tokens = [str(t) for t in vocab_path]
        else:
            with open(vocab_path, encoding="utf-8") as f:
                self.tokens = [ln.rstrip("\n") for ln in f]
            while self.tokens and self.tokens[-1] == "":
                self.tokens.pop()
        if not self.tokens:
            raise EegclipError("WordPieceDecoder: the vocabulary is empty")

    def decode(self, ids, skip_special_tokens=True):
        ids = ids.tolist() if hasattr(ids, "tolist") else list(ids)
        toks = []
        for i in ids:
            i = int(i)
            if not 0 <= i < len(self.tokens):
                raise EegclipError(f"WordPieceDecoder: id {i} is outside the vocabulary [0, {len(self.tokens)})")
            t = self.tokens[i]
            if not (skip_special_tokens and t in self.SPECIALS):
                toks.append(t)
        text = " ".join(toks).replace(" ##", "").strip()
        for a, b in self._CLEAN:
            text = text.replace(a, b)
        return text
