"""SDXL's UNet (diffusers 0.30.0 UNet2DConditionModel with the stabilityai/sdxl-turbo / SDXL-base config) on HIP kernels -- the model the reference's
Generator4Embeds loads (Generation/custom_pipeline.py:456-492) and samples with generate_ip_adapter_embeds (custom_pipeline.py:365-373).

diffusers is not vendored by the reference and absent offline, so the architecture is restated here from diffusers 0.30.0 (unet_2d_condition.py,
unet_2d_blocks.py, resnet.py, transformer_2d.py, attention.py, embeddings.py); tests/sdxl_unet_ref.py restates the same rules in fp32 torch:

* time:   emb = time_embedding(Timesteps(C0, flip_sin_to_cos, shift 0)(t)) + add_embedding(cat(text_embeds, Timesteps(256)(time_ids).reshape(B, -1)));
          TimestepEmbedding = linear_1, SiLU, linear_2.  Every ResnetBlock2D adds time_emb_proj(silu(emb)) after conv1.
* ResnetBlock2D:  h = conv1(silu(norm1(x))) + time_emb_proj(silu(emb)); h = conv2(silu(norm2(h))); out = (conv_shortcut(x) if Cin != Cout else x) + h;
          GroupNorm(32, eps 1e-5).
* Downsample2D: 3 x 3 convolution, stride 2, padding 1.  Upsample2D: nearest 2x, 3 x 3 convolution.
* Transformer2DModel (use_linear_projection): GroupNorm(32, eps 1e-6), proj_in (Linear), BasicTransformerBlocks, proj_out (Linear), + x.
* BasicTransformerBlock: h += attn1(norm1(h)); h += attn2(norm2(h), text [, IP tokens]); h += ff(norm3(h)); LayerNorm(eps 1e-5); to_q / to_k / to_v
          without bias, to_out.0 with; scale 1/8 (head dim 64); attn2 with the IP-Adapter: attn(q, k, v) + scale * attn(q, k_ip, v_ip);
          ff = GEGLU: a, g = net.0.proj(x).chunk(2); net.2(a * gelu_erf(g)), inner width 4 C.
* UNet: skips = conv_in output, every down resnet / transformer output, every downsampler output, popped from the end by the up blocks; each up resnet
          takes cat([h, skip], channel); mid = resnet, transformer, resnet; then conv_norm_out (GroupNorm, eps 1e-5), SiLU, conv_out.
* IP-Adapter (ip-adapter_sdxl_vit-h): encoder_hid_proj.image_projection_layers.0 = Linear(1024 -> 4 x 2048) + LayerNorm(2048) -> 4 image tokens;
          to_k_ip.0 / to_v_ip.0 (no bias) in every attn2 processor.

Arithmetic (no library GEMM, no eager fallback): 16-bit padded NHWC frames between the convolutional layers (vae._FrameOps: csrc/vae.hip conv16 with the
time-embedding add in conv1's epilogue, groupnorm16), token rows inside the transformers (the wrappers of ops16.py: csrc/gemm16.hip linear16 with fused residuals, csrc/unet.hip
layernorm16 / geglu16, csrc/self_attn.hip, csrc/cross_attn.hip), skip concatenation by csrc/unet.hip concat16.  The 17 time_emb_proj layers run as ONE
GEMM over their stacked weights; text / IP keys and values of all attn2 layers are projected once per sampling run (precompute).  The nn.Conv2d /
nn.Linear / nn.GroupNorm / nn.LayerNorm children hold parameters only; they are never called.
"""
from types import SimpleNamespace

import torch
import torch.nn as nn

from ._lib import EegclipError, require_cuda
from .ops16 import (PackedWeights, TokenKV, concat16, cross_attention, geglu16, image_embeds_of, layernorm16, linear, linear16, seeded_parameters,
                    self_attention, text_time_embedding)
from .vae import _FrameOps

RES_EPS, TF_GN_EPS, LN_EPS = 1e-5, 1e-6, 1e-5


# ---------------------------------------------------------------------------------------------------------------------- parameter holders
class _TimestepEmbedding(nn.Module):
    def __init__(self, cin, dim):
        super().__init__()
        self.linear_1, self.linear_2 = nn.Linear(cin, dim), nn.Linear(dim, dim)


class _Resnet(nn.Module):
    def __init__(self, cin, cout, temb, groups, eps):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, cin, eps=eps)
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1)
        self.time_emb_proj = nn.Linear(temb, cout)
        self.norm2 = nn.GroupNorm(groups, cout, eps=eps)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        if cin != cout:
            self.conv_shortcut = nn.Conv2d(cin, cout, 1)


class _IPProcessor(nn.Module):
    """the parameters diffusers' IPAdapterAttnProcessor2_0 holds after load_ip_adapter(ip-adapter_sdxl_vit-h): to_k_ip.0 / to_v_ip.0"""

    def __init__(self, c, cross):
        super().__init__()
        self.to_k_ip = nn.ModuleList([nn.Linear(cross, c, bias=False)])
        self.to_v_ip = nn.ModuleList([nn.Linear(cross, c, bias=False)])


class _Attention(nn.Module):
    def __init__(self, c, kv_dim, heads, ip=False):
        super().__init__()
        self.heads = heads
        self.to_q = nn.Linear(c, c, bias=False)
        self.to_k = nn.Linear(kv_dim, c, bias=False)
        self.to_v = nn.Linear(kv_dim, c, bias=False)
        self.to_out = nn.ModuleList([nn.Linear(c, c), nn.Dropout(0.0)])
        if ip:
            self.processor = _IPProcessor(c, kv_dim)


class _GEGLU(nn.Module):
    def __init__(self, c, inner):
        super().__init__()
        self.proj = nn.Linear(c, 2 * inner)


class _FeedForward(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.net = nn.ModuleList([_GEGLU(c, 4 * c), nn.Dropout(0.0), nn.Linear(4 * c, c)])


class _BasicTransformerBlock(nn.Module):
    def __init__(self, c, heads, cross, ip):
        super().__init__()
        self.norm1 = nn.LayerNorm(c, eps=LN_EPS)
        self.attn1 = _Attention(c, c, heads)
        self.norm2 = nn.LayerNorm(c, eps=LN_EPS)
        self.attn2 = _Attention(c, cross, heads, ip=ip)
        self.norm3 = nn.LayerNorm(c, eps=LN_EPS)
        self.ff = _FeedForward(c)


class _Transformer2D(nn.Module):
    def __init__(self, c, heads, layers, cross, groups, ip):
        super().__init__()
        self.norm = nn.GroupNorm(groups, c, eps=TF_GN_EPS)
        self.proj_in = nn.Linear(c, c)
        self.transformer_blocks = nn.ModuleList([_BasicTransformerBlock(c, heads, cross, ip) for _ in range(layers)])
        self.proj_out = nn.Linear(c, c)


class _Sampler(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, padding=1)


class _Block(nn.Module):
    """DownBlock2D / CrossAttnDownBlock2D / CrossAttnUpBlock2D / UpBlock2D / UNetMidBlock2DCrossAttn: the attribute names they share"""


class _ImageProjection(nn.Module):
    def __init__(self, image_dim, cross, tokens):
        super().__init__()
        self.image_embeds = nn.Linear(image_dim, tokens * cross)
        self.norm = nn.LayerNorm(cross)


class _MultiIPAdapterImageProjection(nn.Module):
    def __init__(self, image_dim, cross, tokens):
        super().__init__()
        self.image_projection_layers = nn.ModuleList([_ImageProjection(image_dim, cross, tokens)])


class SDXLUNet(_FrameOps):
    """UNet2DConditionModel in SDXL's layout (see the module docstring), state_dict keys and shapes of diffusers 0.30.0.  The default arguments are SDXL's
    config (1,680 tensors, 2,567,463,684 parameters); ip_adapter=True adds the ip-adapter_sdxl_vit-h parameters (1,824 / 2,916,651,780).  Weights get
    PyTorch's default module initialisation under `seed` (a freshly built diffusers UNet); load_state_dict takes a real checkpoint.  Channels must be
    multiples of 64, heads = C / 64."""

    def __init__(self, block_out_channels=(320, 640, 1280), layers_per_block=2, transformer_layers_per_block=(1, 2, 10), in_channels=4, out_channels=4,
                 cross_attention_dim=2048, addition_time_embed_dim=256, projection_class_embeddings_input_dim=2816, norm_num_groups=32, norm_eps=1e-5,
                 down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
                 up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"), sample_size=128, ip_adapter=True, ip_tokens=4,
                 image_embed_dim=1024, ip_scale=1.0, dtype=torch.float16, device=None, seed=0):
        super().__init__()
        chans = tuple(int(c) for c in block_out_channels)
        if any(c % 64 for c in chans):
            raise EegclipError(f"SDXLUNet: block_out_channels must be multiples of 64 (head dim 64); got {chans}")
        n = len(chans)
        tl = tuple(transformer_layers_per_block) if isinstance(transformer_layers_per_block, (tuple, list)) else (int(transformer_layers_per_block),) * n
        if len(down_block_types) != n or len(up_block_types) != n or len(tl) != n:
            raise EegclipError("SDXLUNet: one down block, one up block and one transformer depth per entry of block_out_channels")
        cfg = self.config = SimpleNamespace()
        cfg.in_channels, cfg.out_channels, cfg.sample_size = in_channels, out_channels, sample_size
        cfg.time_cond_proj_dim, cfg.addition_time_embed_dim, cfg.cross_attention_dim = None, addition_time_embed_dim, cross_attention_dim
        cfg.block_out_channels, cfg.layers_per_block, cfg.transformer_layers_per_block = chans, layers_per_block, tl
        cfg.down_block_types, cfg.up_block_types = tuple(down_block_types), tuple(up_block_types)
        cfg.norm_num_groups, cfg.norm_eps, cfg.addition_embed_type = norm_num_groups, norm_eps, "text_time"
        cfg.projection_class_embeddings_input_dim = projection_class_embeddings_input_dim
        self.ip_adapter, self.ip_tokens, self.ip_scale = bool(ip_adapter), ip_tokens, float(ip_scale)
        temb = 4 * chans[0]
        G, eps, X = norm_num_groups, norm_eps, cross_attention_dim
        with seeded_parameters(self, dtype, device, seed):
            self.conv_in = nn.Conv2d(in_channels, chans[0], 3, padding=1)
            self.time_embedding = _TimestepEmbedding(chans[0], temb)
            self.add_embedding = _TimestepEmbedding(projection_class_embeddings_input_dim, temb)
            self.down_blocks = nn.ModuleList()
            cout = chans[0]
            for i, kind in enumerate(down_block_types):
                cin, cout = cout, chans[i]
                b = _Block()
                if kind == "CrossAttnDownBlock2D":
                    b.attentions = nn.ModuleList([_Transformer2D(cout, cout // 64, tl[i], X, G, self.ip_adapter) for _ in range(layers_per_block)])
                elif kind != "DownBlock2D":
                    raise EegclipError(f"SDXLUNet: unknown down block {kind}")
                b.resnets = nn.ModuleList([_Resnet(cin if j == 0 else cout, cout, temb, G, eps) for j in range(layers_per_block)])
                if i < n - 1:
                    b.downsamplers = nn.ModuleList([_Sampler(cout)])
                self.down_blocks.append(b)
            self.up_blocks = nn.ModuleList()
            rev, rtl = list(reversed(chans)), list(reversed(tl))
            prev = rev[0]
            for i, kind in enumerate(up_block_types):
                cout, cin = rev[i], rev[min(i + 1, n - 1)]
                b = _Block()
                if kind == "CrossAttnUpBlock2D":
                    b.attentions = nn.ModuleList([_Transformer2D(cout, cout // 64, rtl[i], X, G, self.ip_adapter) for _ in range(layers_per_block + 1)])
                elif kind != "UpBlock2D":
                    raise EegclipError(f"SDXLUNet: unknown up block {kind}")
                b.resnets = nn.ModuleList([_Resnet((prev if j == 0 else cout) + (cin if j == layers_per_block else cout), cout, temb, G, eps)
                                           for j in range(layers_per_block + 1)])
                if i < n - 1:
                    b.upsamplers = nn.ModuleList([_Sampler(cout)])
                prev = cout
                self.up_blocks.append(b)
            mid = self.mid_block = _Block()
            mid.attentions = nn.ModuleList([_Transformer2D(chans[-1], chans[-1] // 64, tl[-1], X, G, self.ip_adapter)])
            mid.resnets = nn.ModuleList([_Resnet(chans[-1], chans[-1], temb, G, eps) for _ in range(2)])
            self.conv_norm_out = nn.GroupNorm(G, chans[0], eps=eps)
            self.conv_out = nn.Conv2d(chans[0], out_channels, 3, padding=1)
            if self.ip_adapter:                          # (load_ip_adapter attaches it last)
                self.encoder_hid_proj = _MultiIPAdapterImageProjection(image_embed_dim, X, ip_tokens)
        self._init_frames()
        self._cache, self._kv = PackedWeights(), None

    def forward(self, sample, timestep, encoder_hidden_states=None, timestep_cond=None, cross_attention_kwargs=None, added_cond_kwargs=None,
                return_dict=False, **kw):
        return (self._run(sample, timestep, encoder_hidden_states, added_cond_kwargs),)

    @property
    def dtype(self):
        return self.conv_in.weight.dtype

    @property
    def device(self):
        return self.conv_in.weight.device

    # ---- packed weights: repacked when their parameters change (ops16.PackedWeights) ---------------------------------------------------------------
    def _resnets(self):
        return [r for b in self.down_blocks for r in b.resnets] + list(self.mid_block.resnets) + [r for b in self.up_blocks for r in b.resnets]

    def _temb_stack(self):
        """the 17 (SDXL) time_emb_proj layers as one (rows padded to 128, temb) weight + bias, packed once per parameter version"""
        rs = self._resnets()
        ps = [p for r in rs for p in (r.time_emb_proj.weight, r.time_emb_proj.bias)]

        def make():
            w = torch.cat([r.time_emb_proj.weight.detach() for r in rs], 0)
            b = torch.cat([r.time_emb_proj.bias.detach() for r in rs], 0)
            pad = -w.shape[0] % 128
            return torch.nn.functional.pad(w, (0, 0, 0, pad)).contiguous(), torch.nn.functional.pad(b, (0, pad)).contiguous()
        return self._cache.get("temb", ps, make)

    def _qkv(self, attn):
        ps = [attn.to_q.weight, attn.to_k.weight, attn.to_v.weight]
        return self._cache.get(("qkv", id(attn)), ps, lambda: torch.cat([p.detach() for p in ps], 0).contiguous())

    # ---- token-row layers -------------------------------------------------------------------------------------------------------------------------
    def _lin(self, x, mod, residual=None):
        return linear(x, mod.weight, mod.bias, residual)

    def _concat(self, a, b):
        N, Hp, Wp, Ca = a.shape
        return concat16(a, b, self._frame(N, Hp - 2, Wp - 2, Ca + b.shape[3], 1))

    # ---- once per sampling run: image tokens, keys / values of every attn2 ------------------------------------------------------------------------
    def _transformers(self):
        ts = [t for b in self.down_blocks for t in getattr(b, "attentions", [])] + list(self.mid_block.attentions)
        return ts + [t for b in self.up_blocks for t in getattr(b, "attentions", [])]

    def _attn2s(self):
        return [blk.attn2 for t in self._transformers() for blk in t.transformer_blocks]

    def image_tokens(self, image_embeds):
        """(B, 1024) -> (B, 4, 2048): encoder_hid_proj (ImageProjection: Linear, then LayerNorm over each token)"""
        if not self.ip_adapter:
            raise EegclipError("SDXLUNet(ip_adapter=False) takes no image_embeds")
        pr = self.encoder_hid_proj.image_projection_layers[0]
        x = linear16(image_embeds.to(self.dtype).reshape(-1, pr.image_embeds.weight.shape[1]).contiguous(), pr.image_embeds.weight, pr.image_embeds.bias)
        rows = x.reshape(-1, self.config.cross_attention_dim)
        return layernorm16(rows, pr.norm.weight, pr.norm.bias, pr.norm.eps).reshape(x.shape[0], self.ip_tokens, -1)

    def _kv_weights_key(self):
        ps = [p for a in self._attn2s() for p in (a.to_k.weight, a.to_v.weight)]
        if self.ip_adapter:
            ps += [p for a in self._attn2s() for p in (a.processor.to_k_ip[0].weight, a.processor.to_v_ip[0].weight)]
            pr = self.encoder_hid_proj.image_projection_layers[0]
            ps += [pr.image_embeds.weight, pr.image_embeds.bias, pr.norm.weight, pr.norm.bias]
        return PackedWeights.key(ps)

    def precompute(self, encoder_hidden_states, image_embeds=None):
        """K / V of the text tokens (and of the 4 IP tokens) for all attn2 layers, computed once and reused by every forward with the same tensors"""
        require_cuda(encoder_hidden_states, "encoder_hidden_states")
        text = encoder_hidden_states.to(self.dtype).contiguous()
        ip = self.image_tokens(image_embeds) if image_embeds is not None else None
        weights = [(a.to_k.weight, a.to_v.weight) + ((a.processor.to_k_ip[0].weight, a.processor.to_v_ip[0].weight) if ip is not None else (None, None))
                   for a in self._attn2s()]
        self._kv = TokenKV.project(encoder_hidden_states, image_embeds, self._kv_weights_key(), text, ip, weights)
        return self

    def _kv_for(self, ehs, image_embeds):
        if self._kv is None or not self._kv.hit(ehs, image_embeds, self._kv_weights_key()):
            self.precompute(ehs, image_embeds)
        return iter(self._kv.entries)

    # ---- blocks -----------------------------------------------------------------------------------------------------------------------------------
    def _transformer(self, x, t, kv):
        N, H, W, C = x.shape[0], x.shape[1] - 2, x.shape[2] - 2, x.shape[3]
        hn = self._gn(x, 1, t.norm, silu=False, out_pad=0)
        h = self._lin(hn.reshape(-1, C), t.proj_in)
        self._done(hn)
        T = H * W
        for blk in t.transformer_blocks:
            a1, a2 = blk.attn1, blk.attn2
            n1 = layernorm16(h, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)
            qkv = linear16(n1, self._qkv(a1)).reshape(N, T, 3 * C)
            o = self_attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], a1.heads)
            h = self._lin(o.reshape(-1, C), a1.to_out[0], h)
            n2 = layernorm16(h, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)
            k, v, kip, vip = next(kv)
            if k.shape[0] != N:
                raise EegclipError(f"encoder_hidden_states has batch {k.shape[0]}, sample has {N}")
            q = self._lin(n2, a2.to_q).reshape(N, T, C)
            o = cross_attention(q, k, v, a2.heads, kip, vip, self.ip_scale)
            h = self._lin(o.reshape(-1, C), a2.to_out[0], h)
            n3 = layernorm16(h, blk.norm3.weight, blk.norm3.bias, blk.norm3.eps)
            g = geglu16(self._lin(n3, blk.ff.net[0].proj))
            h = self._lin(g, blk.ff.net[2], h)
        # proj_out + the block's residual, straight back into a padded frame (a 1 x 1 conv16 with residual=)
        return self._conv(h.reshape(N, H, W, C), 0, t.proj_out, out_pad=1, residual=x, KS=1)

    def _embedding(self, timestep, B, added):
        te, ae = self.time_embedding, self.add_embedding
        return text_time_embedding(timestep, B, added, (te.linear_1.weight, te.linear_1.bias, te.linear_2.weight, te.linear_2.bias),
                                   (ae.linear_1.weight, ae.linear_1.bias, ae.linear_2.weight, ae.linear_2.bias), self.config.block_out_channels[0],
                                   self.config.addition_time_embed_dim, self.dtype, self.device)

    @torch.no_grad()
    def _run(self, sample, timestep, ehs, added):
        require_cuda(sample, "sample")
        B, Cc, Hl, Wl = sample.shape
        n = len(self.config.block_out_channels)
        if Cc != self.config.in_channels or Hl % 2 ** (n - 1) or Wl % 2 ** (n - 1):
            raise EegclipError(f"sample must be (B, {self.config.in_channels}, H, W) with H, W multiples of {2 ** (n - 1)}; got {tuple(sample.shape)}")
        if ehs is None:
            raise EegclipError("SDXLUNet needs encoder_hidden_states")
        image_embeds = image_embeds_of(added)
        if image_embeds is not None and not self.ip_adapter:
            raise EegclipError("image_embeds given to SDXLUNet(ip_adapter=False)")
        kv = self._kv_for(ehs, image_embeds)
        emb = self._embedding(timestep, B, added)
        w, b = self._temb_stack()
        tproj = linear16(emb, w, b)                                           # ONE GEMM for every ResnetBlock2D's time_emb_proj
        offs, o = [], 0
        for r in self._resnets():
            c = r.time_emb_proj.weight.shape[0]
            offs.append(tproj[:, o:o + c].contiguous())
            o += c
        tb = iter(offs)
        x0 = self._to_frame(sample.to(self.dtype))
        h = self._conv(x0, 1, self.conv_in)
        self._done(x0)
        skips = [h]
        for blk in self.down_blocks:
            atts = getattr(blk, "attentions", None)
            for j, r in enumerate(blk.resnets):
                h = self._resnet(h, r, next(tb))
                if atts is not None:
                    h2 = self._transformer(h, atts[j], kv)
                    self._done(h)
                    h = h2
                skips.append(h)
            if hasattr(blk, "downsamplers"):
                h = self._conv(h, 1, blk.downsamplers[0].conv, stride=2)
                skips.append(h)
        m = self.mid_block
        h2 = self._resnet(h, m.resnets[0], next(tb))
        h3 = self._transformer(h2, m.attentions[0], kv)
        self._done(h2)
        h = self._resnet(h3, m.resnets[1], next(tb))
        self._done(h3)
        for blk in self.up_blocks:
            atts = getattr(blk, "attentions", None)
            for j, r in enumerate(blk.resnets):
                skip = skips.pop()
                hc = self._concat(h, skip)
                self._done(h, skip)
                h = self._resnet(hc, r, next(tb))
                self._done(hc)
                if atts is not None:
                    h2 = self._transformer(h, atts[j], kv)
                    self._done(h)
                    h = h2
            if hasattr(blk, "upsamplers"):
                h2 = self._conv(h, 1, blk.upsamplers[0].conv, upsample=True)
                self._done(h)
                h = h2
        hn = self._gn(h, 1, self.conv_norm_out)
        self._done(h)
        out = self._conv(hn, 1, self.conv_out, out_pad=0)
        self._done(hn)
        res = out.permute(0, 3, 1, 2).contiguous()
        self._done(out)
        return res


def forward_flops(unet, B, H, W, text_tokens=77, ip=True):
    """algorithmic FLOPs of one forward (2 per multiply-add) by layer family: {"linear", "conv", "self_attention", "cross_attention"}"""
    cfg = unet.config
    chans, n = cfg.block_out_channels, len(cfg.block_out_channels)
    f = {"linear": 0.0, "conv": 0.0, "self_attention": 0.0, "cross_attention": 0.0}

    def conv(cin, cout, ks, pix):
        f["conv"] += 2.0 * B * pix * cin * cout * ks * ks

    def resnet(cin, cout, pix):
        conv(cin, cout, 3, pix)
        conv(cout, cout, 3, pix)
        if cin != cout:
            conv(cin, cout, 1, pix)

    def transformer(c, layers, T):
        f["linear"] += 2.0 * B * T * c * c * 2                                 # proj_in, proj_out
        for _ in range(layers):
            f["linear"] += 2.0 * B * T * c * c * (3 + 1 + 1 + 1) + 2.0 * B * T * c * 8 * c + 2.0 * B * T * 4 * c * c   # qkv, out1, q2, out2, ff
            f["self_attention"] += 4.0 * B * T * T * c
            f["cross_attention"] += 4.0 * B * T * (text_tokens + (unet.ip_tokens if ip else 0)) * c

    h, w = H, W
    conv(cfg.in_channels, chans[0], 3, h * w)
    skip_ch = [chans[0]]
    cout = chans[0]
    for i, blk in enumerate(unet.down_blocks):
        for j in range(len(blk.resnets)):
            cin, cout = (cout if j == 0 else chans[i]), chans[i]
            resnet(cin, cout, h * w)
            if hasattr(blk, "attentions"):
                transformer(cout, cfg.transformer_layers_per_block[i], h * w)
            skip_ch.append(cout)
        if hasattr(blk, "downsamplers"):
            h, w = h // 2, w // 2
            conv(cout, cout, 3, h * w)
            skip_ch.append(cout)
    resnet(chans[-1], chans[-1], h * w)
    transformer(chans[-1], cfg.transformer_layers_per_block[-1], h * w)
    resnet(chans[-1], chans[-1], h * w)
    hc, rtl = chans[-1], list(reversed(cfg.transformer_layers_per_block))
    for i, blk in enumerate(unet.up_blocks):
        c = list(reversed(chans))[i]
        for j in range(len(blk.resnets)):
            resnet(hc + skip_ch.pop(), c, h * w)
            hc = c
            if hasattr(blk, "attentions"):
                transformer(c, rtl[i], h * w)
        if hasattr(blk, "upsamplers"):
            h, w = 2 * h, 2 * w
            conv(c, c, 3, h * w)
    conv(chans[0], cfg.out_channels, 3, h * w)
    return f
