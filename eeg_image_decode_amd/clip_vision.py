"""CLIP's vision towers on HIP kernels: the encoder that produces what the rest of the pipeline is trained against and conditioned on.

* ip_adapter_image_encoder(): CLIP ViT-H/14 (h94/IP-Adapter models/image_encoder, transformers' CLIPVisionModelWithProjection) -- its `image_embeds` are the
  IP-Adapter's input (Generation/custom_pipeline.py:365-373 conditions the UNet on them) and the `img_features` the data sets cache.
* git_vision_tower(): GIT-large's git.image_encoder (a CLIP ViT-L/14, transformers' GitVisionModel) -- its tokens are what Generation/modeling_git.py:1970-1973
  takes as an input and what git_caption.GITCaptioner captions.

The module is clip_text.CLIPTextEncoder with another front end and no mask; tests/clip_vision_ref.py restates it in fp32 torch and
tests/test_clip_vision_layout.py pins that restatement to transformers itself:

    x = cat(class_embedding, patch_embedding(pixels) as tokens) + position_embedding;  x = pre_layrnorm(x);  hidden_states = [x]
    per layer:  clip_text.clip_layers (heads of 64 or 80, no mask);  hidden_states.append(x)
    last_hidden_state = x (post_layernorm(x) with post_layernorm_all: GitVisionTransformer);  pooler_output = post_layernorm(x[:, 0])
    image_embeds = visual_projection(pooler_output)

Arithmetic (the wrappers of ops16.py; no library GEMM, no torch math op, no eager fallback; bit-reproducible): three launches to hidden_states[0] --
csrc/clip_vision.hip patch_rows16 (pixels -> GEMM rows, the class slot a zero row, optional per-channel normalisation), ONE csrc/gemm16.hip launch against the
patch weight packed to (C, Kpad), csrc/clip_vision.hip embed_ln16 (+ position row, row 0 carrying the class embedding, then pre_layrnorm) -- then the layers
on gemm16 / layernorm16 / act16 and csrc/self_attn.hip (head dim 64 or 80).  Resizing and cropping are preprocess.py's; there is
no interpolate_pos_encoding: a pixel tensor of another size raises.
"""
from types import SimpleNamespace

import torch
import torch.nn as nn

from ._lib import EegclipError, require_cuda
from .clip_text import ACT_KINDS, _Encoder, clip_layers
from .ops16 import PackedWeights, embed_ln16, layernorm16, linear16, patch_rows16, seeded_parameters

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)     # OPENAI_CLIP_MEAN / _STD (both towers' preprocessor configs)


class _VisionEmbeddings(nn.Module):
    def __init__(self, c, image_size, patch):
        super().__init__()
        self.class_embedding = nn.Parameter(torch.randn(c))
        self.patch_embedding = nn.Conv2d(3, c, patch, patch, bias=False)
        self.position_embedding = nn.Embedding((image_size // patch) ** 2 + 1, c)


class _VisionTransformer(nn.Module):
    def __init__(self, c, inner, n, eps, image_size, patch):
        super().__init__()
        self.embeddings = _VisionEmbeddings(c, image_size, patch)
        self.pre_layrnorm = nn.LayerNorm(c, eps=eps)              # (sic: transformers' spelling, the checkpoints' key)
        self.encoder = _Encoder(c, inner, n, eps)
        self.post_layernorm = nn.LayerNorm(c, eps=eps)


class CLIPVisionOutput:
    """transformers' CLIPVisionModelOutput fields: image_embeds (None without a projection), last_hidden_state, pooler_output, hidden_states; out[0] is
    image_embeds with a projection, else last_hidden_state.  Indexing skips the fields that are None, as transformers' ModelOutput does."""

    def __init__(self, image_embeds, last_hidden_state, pooler_output, hidden_states):
        self.image_embeds, self.last_hidden_state, self.pooler_output, self.hidden_states = image_embeds, last_hidden_state, pooler_output, hidden_states
        order = (image_embeds, last_hidden_state, hidden_states) if image_embeds is not None else (last_hidden_state, pooler_output, hidden_states)
        self._tuple = tuple(v for v in order if v is not None)

    def __getitem__(self, i):
        return self._tuple[i]

    def __len__(self):
        return len(self._tuple)


class CLIPVisionEncoder(nn.Module):
    """transformers' CLIPVisionModelWithProjection (CLIPVisionModel's keys with projection_dim=None) on HIP kernels; state_dict keys and shapes of the
    published checkpoints.  Head dim 64 or 80; hidden_size, intermediate_size and projection_dim multiples of 128 (the 16-bit GEMM's shapes).
    post_layernorm_all: last_hidden_state = post_layernorm of every token (transformers' GitVisionTransformer).  Weights get PyTorch's default module
    initialisation under `seed`; load_state_dict takes a real checkpoint (with or without GIT's `git.image_encoder.` prefix; other keys of a full GIT
    state dict are dropped)."""

    def __init__(self, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, hidden_act, projection_dim=None, image_size=224, patch_size=14,
                 layer_norm_eps=1e-5, post_layernorm_all=False, dtype=torch.float16, device=None, seed=0):
        super().__init__()
        if hidden_size % num_attention_heads or hidden_size // num_attention_heads not in (64, 80):
            raise EegclipError(f"CLIPVisionEncoder: head dim must be 64 or 80 (hidden_size {hidden_size}, {num_attention_heads} heads)")
        if hidden_size % 128 or intermediate_size % 128 or (projection_dim is not None and projection_dim % 128):
            raise EegclipError("CLIPVisionEncoder: hidden_size, intermediate_size and projection_dim must be multiples of 128 (csrc/gemm16.hip)")
        if hidden_act not in ACT_KINDS:
            raise EegclipError(f"CLIPVisionEncoder: hidden_act must be one of {sorted(ACT_KINDS)}; got {hidden_act!r}")
        if patch_size < 1 or image_size < patch_size or image_size % patch_size:
            raise EegclipError(f"CLIPVisionEncoder: image_size {image_size} is not a whole number of patches of {patch_size}")
        cfg = self.config = SimpleNamespace()
        cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads = hidden_size, intermediate_size, num_hidden_layers, num_attention_heads
        cfg.hidden_act, cfg.projection_dim, cfg.image_size, cfg.patch_size, cfg.layer_norm_eps = hidden_act, projection_dim, image_size, patch_size, layer_norm_eps
        cfg.post_layernorm_all = bool(post_layernorm_all)
        with seeded_parameters(self, dtype, device, seed):
            self.vision_model = _VisionTransformer(hidden_size, intermediate_size, num_hidden_layers, layer_norm_eps, image_size, patch_size)
            if projection_dim is not None:
                self.visual_projection = nn.Linear(hidden_size, projection_dim, bias=False)
        self._cache = PackedWeights()

    @property
    def dtype(self):
        return self.vision_model.post_layernorm.weight.dtype

    @property
    def device(self):
        return self.vision_model.post_layernorm.weight.device

    def load_state_dict(self, state_dict, strict=True, **kw):
        pre = "git.image_encoder."
        if any(k.startswith(pre) for k in state_dict):
            state_dict = {k[len(pre):]: v for k, v in state_dict.items() if k.startswith(pre)}
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def _front(self):
        """(patch weight as (C, Kpad) GEMM rows, position rows with the class embedding added to row 0 in fp32 and rounded once)"""
        emb = self.vision_model.embeddings
        ps = [emb.patch_embedding.weight, emb.position_embedding.weight, emb.class_embedding]

        def make():
            w = emb.patch_embedding.weight.detach()
            k = w[0].numel()
            wp = torch.zeros(w.shape[0], (k + 63) // 64 * 64, dtype=w.dtype, device=w.device)
            wp[:, :k] = w.reshape(w.shape[0], k)
            pos = emb.position_embedding.weight.detach().float().clone()
            pos[0] += emb.class_embedding.detach().float()
            return wp, pos.to(w.dtype).contiguous()
        return self._cache.get("front", ps, make)

    @torch.no_grad()
    def forward(self, pixel_values, output_hidden_states=False, return_dict=True, interpolate_pos_encoding=False, mean=None, std=None, rescale=None, **kw):
        """pixel_values (B, 3, image_size, image_size) in fp32 / fp16 / bf16, resized and normalised as transformers takes them -> CLIPVisionOutput.
        mean / std / rescale (not in transformers): the pixels are raw instead and (pixel * rescale - mean[c]) / std[c] is folded into the first kernel
        (CLIP_MEAN, CLIP_STD and rescale = 1 / 255 for 0..255 pixels); each defaults to the identity when another is given."""
        if interpolate_pos_encoding:
            raise EegclipError("CLIPVisionEncoder has no interpolate_pos_encoding: resize the image to the tower's image_size")
        cfg = self.config
        emb = self.vision_model.embeddings
        require_cuda(emb.class_embedding, "CLIPVisionEncoder's weights")
        px = torch.as_tensor(pixel_values)
        S = cfg.image_size
        if px.dim() != 4 or tuple(px.shape[1:]) != (3, S, S) or px.shape[0] == 0:
            raise EegclipError(f"pixel_values must be (B, 3, {S}, {S}), resized and cropped by the caller; got {tuple(px.shape)}")
        if px.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise EegclipError(f"pixel_values must be fp32, fp16 or bf16; got {px.dtype}")
        dev = self.device
        px = px.to(dev)
        scale = shift = None
        if mean is not None or std is not None or rescale is not None:
            m = torch.tensor([0.0] * 3 if mean is None else [float(v) for v in mean], dtype=torch.float64)
            s = torch.tensor([1.0] * 3 if std is None else [float(v) for v in std], dtype=torch.float64)
            if m.numel() != 3 or s.numel() != 3 or bool((s == 0).any()):
                raise EegclipError("mean and std take three values, std non-zero")
            scale = ((1.0 if rescale is None else float(rescale)) / s).float().to(dev)
            shift = (-m / s).float().to(dev)
        B, C, heads = px.shape[0], cfg.hidden_size, cfg.num_attention_heads
        T = (S // cfg.patch_size) ** 2 + 1
        vm = self.vision_model
        wp, pos = self._front()
        patches = linear16(patch_rows16(px, cfg.patch_size, self.dtype, scale, shift), wp)             # (B T, C), zero in the class rows
        x = embed_ln16(patches, pos, vm.pre_layrnorm.weight, vm.pre_layrnorm.bias, vm.pre_layrnorm.eps)
        hs = [x] + clip_layers(vm.encoder.layers, self._cache, x, B, T, heads, ACT_KINDS[cfg.hidden_act], causal=False, head_dim=C // heads)
        post = vm.post_layernorm
        if cfg.post_layernorm_all:
            last = layernorm16(hs[-1], post.weight, post.bias, post.eps).reshape(B, T, C)
            pooled = last[:, 0]
        else:
            last = hs[-1].reshape(B, T, C)
            pooled = layernorm16(last[:, 0], post.weight, post.bias, post.eps)                         # (rows T C apart, read in place)
        embeds = linear16(pooled, self.visual_projection.weight) if cfg.projection_dim is not None else None
        hidden = tuple(h.reshape(B, T, C) for h in hs) if output_hidden_states else None
        return CLIPVisionOutput(embeds, last, pooled, hidden)


def ip_adapter_image_encoder(**kw):
    """h94/IP-Adapter models/image_encoder: CLIP ViT-H/14's image tower with its projection (laion/CLIP-ViT-H-14-laion2B-s32B-b79K; head dim 80,
    257 tokens at 224 x 224) -- image_embeds (B, 1024) is what `ip-adapter_sdxl_vit-h` takes"""
    return CLIPVisionEncoder(1280, 5120, 32, 16, "gelu", 1024, **kw)


def git_vision_tower(**kw):
    """microsoft/git-large-coco git.image_encoder: CLIP ViT-L/14's image tower, no projection, post_layernorm on every token (head dim 64, 257 tokens
    of 1024 at 224 x 224: GITCaptioner's visual_features)"""
    return CLIPVisionEncoder(1024, 4096, 24, 16, "quick_gelu", None, post_layernorm_all=True, **kw)
