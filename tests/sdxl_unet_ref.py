"""fp32 restatement of diffusers 0.30.0 UNet2DConditionModel in SDXL's layout (+ the ip-adapter_sdxl_vit-h attn2 branch), torch.nn.functional over a
state_dict -- the yardstick of eeg_image_decode_amd/sdxl_unet.py.  diffusers itself is absent offline; the rules restated here (unet_2d_condition.py,
unet_2d_blocks.py, resnet.py, transformer_2d.py, attention.py, attention_processor.py, embeddings.py):

  emb   = time_embedding(Timesteps(C0, flip_sin_to_cos=True, shift 0)(t)) + add_embedding(cat(text_embeds, Timesteps(256)(time_ids.flatten()).reshape(B, -1)))
  resnet(x) = (conv_shortcut(x) | x) + conv2(silu(GN(conv1(silu(GN(x))) + time_emb_proj(silu(emb))[:, :, None, None])))       GN: 32 groups, eps 1e-5
  transformer(x) = x + proj_out(blocks(proj_in(GN_eps1e-6(x) as (B, HW, C) tokens)))
  block(h): h += attn1(LN1(h)); h += attn2(LN2(h), text) [+ ip_scale * attn(q, k_ip, v_ip)]; h += net.2(a * gelu_erf(g)), (a, g) = net.0.proj(LN3(h)).chunk(2)
  down: skips = [conv_in] + every resnet / transformer output + every downsampler (3 x 3, stride 2, pad 1); up resnets take cat([h, skips.pop()]);
  mid = resnet, transformer, resnet; out = conv_out(silu(GN(h))).
"""
import math

import torch
import torch.nn.functional as F


def sinusoid(t, dim):
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32, device=t.device) / half)
    arg = t.float()[..., None] * freqs
    return torch.cat([arg.cos(), arg.sin()], dim=-1)


class Ref:
    def __init__(self, state_dict, config, ip_scale=1.0, ip_tokens=4, device=None):
        self.p = {k: v.detach().to(device=device or v.device, dtype=torch.float32) for k, v in state_dict.items()}
        self.cfg, self.ip_scale, self.ip_tokens = config, ip_scale, ip_tokens

    def lin(self, x, name, bias=True):
        b = self.p.get(name + ".bias") if bias else None
        return F.linear(x, self.p[name + ".weight"], b)

    def gn(self, x, name, eps):
        return F.group_norm(x, self.cfg.norm_num_groups, self.p[name + ".weight"], self.p[name + ".bias"], eps)

    def conv(self, x, name, stride=1, padding=1):
        return F.conv2d(x, self.p[name + ".weight"], self.p[name + ".bias"], stride=stride, padding=padding)

    def embedding(self, timestep, B, text_embeds, time_ids):
        dev = self.p["conv_in.weight"].device
        t = torch.as_tensor(timestep, device=dev).reshape(-1).float().expand(B)
        e = self.lin(F.silu(self.lin(sinusoid(t, self.cfg.block_out_channels[0]), "time_embedding.linear_1")), "time_embedding.linear_2")
        aug = torch.cat([text_embeds.float(), sinusoid(time_ids.to(dev).flatten(), self.cfg.addition_time_embed_dim).reshape(B, -1)], -1)
        return e + self.lin(F.silu(self.lin(aug, "add_embedding.linear_1")), "add_embedding.linear_2")

    def resnet(self, x, name, emb):
        h = self.conv(F.silu(self.gn(x, name + ".norm1", 1e-5)), name + ".conv1")
        h = h + self.lin(F.silu(emb), name + ".time_emb_proj")[:, :, None, None]
        h = self.conv(F.silu(self.gn(h, name + ".norm2", 1e-5)), name + ".conv2")
        sc = self.conv(x, name + ".conv_shortcut", padding=0) if name + ".conv_shortcut.weight" in self.p else x
        return sc + h

    def attn(self, q, k, v, heads):
        B, T, C = q.shape
        sh = lambda t: t.reshape(B, t.shape[1], heads, C // heads).transpose(1, 2)
        s = sh(q) @ sh(k).transpose(-1, -2) / math.sqrt(C // heads)
        return (s.softmax(-1) @ sh(v)).transpose(1, 2).reshape(B, T, C)

    def ln(self, x, name):
        return F.layer_norm(x, (x.shape[-1],), self.p[name + ".weight"], self.p[name + ".bias"], 1e-5)

    def image_tokens(self, image_embeds):
        pre = "encoder_hid_proj.image_projection_layers.0"
        x = self.lin(image_embeds.float(), pre + ".image_embeds").reshape(image_embeds.shape[0], self.ip_tokens, -1)
        return self.ln(x, pre + ".norm")

    def transformer(self, x, name, text, ip_tok=None):
        B, C, H, W = x.shape
        heads = C // 64
        h = self.gn(x, name + ".norm", 1e-6).permute(0, 2, 3, 1).reshape(B, H * W, C)
        h = self.lin(h, name + ".proj_in")
        i = 0
        while f"{name}.transformer_blocks.{i}.norm1.weight" in self.p:
            b = f"{name}.transformer_blocks.{i}"
            n = self.ln(h, b + ".norm1")
            h = h + self.lin(self.attn(self.lin(n, b + ".attn1.to_q", False), self.lin(n, b + ".attn1.to_k", False), self.lin(n, b + ".attn1.to_v", False),
                                       heads), b + ".attn1.to_out.0")
            n = self.ln(h, b + ".norm2")
            q = self.lin(n, b + ".attn2.to_q", False)
            a = self.attn(q, self.lin(text, b + ".attn2.to_k", False), self.lin(text, b + ".attn2.to_v", False), heads)
            if ip_tok is not None:
                a = a + self.ip_scale * self.attn(q, self.lin(ip_tok, b + ".attn2.processor.to_k_ip.0", False),
                                                  self.lin(ip_tok, b + ".attn2.processor.to_v_ip.0", False), heads)
            h = h + self.lin(a, b + ".attn2.to_out.0")
            av, g = self.lin(self.ln(h, b + ".norm3"), b + ".ff.net.0.proj").chunk(2, -1)
            h = h + self.lin(av * F.gelu(g), b + ".ff.net.2")
            i += 1
        h = self.lin(h, name + ".proj_out")
        return h.reshape(B, H, W, C).permute(0, 3, 1, 2) + x

    def __call__(self, sample, timestep, encoder_hidden_states, text_embeds, time_ids, image_embeds=None):
        cfg = self.cfg
        B = sample.shape[0]
        text = encoder_hidden_states.float()
        ip_tok = self.image_tokens(image_embeds) if image_embeds is not None else None
        emb = self.embedding(timestep, B, text_embeds, time_ids)
        h = self.conv(sample.float(), "conv_in")
        skips = [h]
        n = len(cfg.block_out_channels)
        for i in range(n):
            for j in range(cfg.layers_per_block):
                h = self.resnet(h, f"down_blocks.{i}.resnets.{j}", emb)
                if f"down_blocks.{i}.attentions.{j}.proj_in.weight" in self.p:
                    h = self.transformer(h, f"down_blocks.{i}.attentions.{j}", text, ip_tok)
                skips.append(h)
            if f"down_blocks.{i}.downsamplers.0.conv.weight" in self.p:
                h = self.conv(h, f"down_blocks.{i}.downsamplers.0.conv", stride=2)
                skips.append(h)
        h = self.resnet(h, "mid_block.resnets.0", emb)
        h = self.transformer(h, "mid_block.attentions.0", text, ip_tok)
        h = self.resnet(h, "mid_block.resnets.1", emb)
        for i in range(n):
            for j in range(cfg.layers_per_block + 1):
                h = self.resnet(torch.cat([h, skips.pop()], 1), f"up_blocks.{i}.resnets.{j}", emb)
                if f"up_blocks.{i}.attentions.{j}.proj_in.weight" in self.p:
                    h = self.transformer(h, f"up_blocks.{i}.attentions.{j}", text, ip_tok)
            if f"up_blocks.{i}.upsamplers.0.conv.weight" in self.p:
                h = self.conv(F.interpolate(h, scale_factor=2.0, mode="nearest"), f"up_blocks.{i}.upsamplers.0.conv")
        return self.conv(F.silu(self.gn(h, "conv_norm_out", 1e-5)), "conv_out")
