"""fp32 / fp64 restatement of transformers' CLIPVisionModelWithProjection and GitVisionModel (modeling_clip.py: CLIPVisionEmbeddings, pre_layrnorm,
CLIPEncoderLayer with no mask, CLIPMLP, post_layernorm; modeling_git.py: GitVisionTransformer applies post_layernorm to every token), torch.nn.functional
over a state_dict -- the yardstick of eeg_image_decode_amd/clip_vision.py.  tests/test_clip_vision_layout.py pins it to transformers itself.

  x = cat(class_embedding, conv2d(pixels, patch_embedding.weight, stride = patch) as (B, P, C)) + position_embedding;  x = pre_layrnorm(x);  hidden_states = [x]
  layer:  h = LN1(x); q, k, v = {q,k,v}_proj(h) in heads of d;  x = x + out_proj(softmax(q k^T / sqrt(d)) v)
          h = fc1(LN2(x)); h = h * sigmoid(1.702 h) (quick_gelu) | gelu_erf(h);  x = x + fc2(h);  hidden_states.append(x)
  last_hidden_state = x (post_layernorm(x) with post_layernorm_all);  pooler_output = post_layernorm(x[:, 0]);  image_embeds = pooler_output @ visual_projection.T
"""
import torch
import torch.nn.functional as F

PREFIX = "vision_model."


def normalise_keys(sd):
    """GIT's full state dict carries the tower under `git.image_encoder.`: strip it; everything else is already transformers' CLIPVisionModelWithProjection's"""
    pre = "git.image_encoder."
    return {(k[len(pre):] if k.startswith(pre) else k): v for k, v in sd.items()}


class Ref:
    def __init__(self, state_dict, num_heads, hidden_act, eps=1e-5, post_layernorm_all=False, dtype=torch.float32, device=None):
        self.p = {k: v.detach().to(device=device or v.device, dtype=dtype) for k, v in normalise_keys(state_dict).items()}
        self.heads, self.act, self.eps, self.post_all = num_heads, hidden_act, eps, post_layernorm_all
        self.L = 1 + max(int(k.split(".")[3]) for k in self.p if k.startswith(PREFIX + "encoder.layers."))

    def lin(self, x, name):
        return F.linear(x, self.p[name + ".weight"], self.p.get(name + ".bias"))

    def ln(self, x, name):
        return F.layer_norm(x, (x.shape[-1],), self.p[name + ".weight"], self.p[name + ".bias"], self.eps)

    def __call__(self, pixels):
        """pixels (B, 3, S, S) -> dict(hidden_states tuple of L + 1, last_hidden_state, pooler_output, image_embeds or None)"""
        p = self.p
        w = p[PREFIX + "embeddings.patch_embedding.weight"]
        px = torch.as_tensor(pixels).to(device=w.device, dtype=w.dtype)
        B = px.shape[0]
        patches = F.conv2d(px, w, stride=w.shape[-1]).flatten(2).transpose(1, 2)
        x = torch.cat([p[PREFIX + "embeddings.class_embedding"].expand(B, 1, -1), patches], dim=1) + p[PREFIX + "embeddings.position_embedding.weight"]
        x = self.ln(x, PREFIX + "pre_layrnorm")
        T, C, H = x.shape[1], x.shape[2], self.heads
        d = C // H
        hs = [x]
        for i in range(self.L):
            base = f"{PREFIX}encoder.layers.{i}."
            h = self.ln(x, base + "layer_norm1")
            q, k, v = (self.lin(h, base + f"self_attn.{n}_proj").reshape(B, T, H, d).transpose(1, 2) for n in "qkv")
            a = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1) @ v
            x = x + self.lin(a.transpose(1, 2).reshape(B, T, C), base + "self_attn.out_proj")
            h = self.lin(self.ln(x, base + "layer_norm2"), base + "mlp.fc1")
            h = h * torch.sigmoid(1.702 * h) if self.act == "quick_gelu" else F.gelu(h)
            x = x + self.lin(h, base + "mlp.fc2")
            hs.append(x)
        pooled = self.ln(x[:, 0], PREFIX + "post_layernorm")
        last = self.ln(x, PREFIX + "post_layernorm") if self.post_all else x
        ie = pooled @ p["visual_projection.weight"].T if "visual_projection.weight" in p else None
        return {"hidden_states": tuple(hs), "last_hidden_state": last, "pooler_output": pooled, "image_embeds": ie}


def pixel_batch(B, size, seed=0, zero_sample=True):
    """(B, 3, size, size) fp32, roughly normalised-image statistics; sample 0 all zeros (a black image after normalisation to mean 0)"""
    g = torch.Generator().manual_seed(seed)
    px = torch.randn(B, 3, size, size, generator=g) * 1.2
    if zero_sample:
        px[0] = 0
    return px
