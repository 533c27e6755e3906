"""fp32 / fp64 restatement of transformers' CLIPTextModel / CLIPTextModelWithProjection (modeling_clip.py: CLIPTextEmbeddings, CLIPEncoderLayer,
CLIPAttention with the causal mask alone, CLIPMLP, the eos pooling of configs with eos_token_id == 2), torch.nn.functional over a state_dict -- the
yardstick of eeg_image_decode_amd/clip_text.py.  tests/test_clip_text_layout.py pins it to transformers itself where transformers is installed.

  x = token_embedding[ids] + position_embedding[:T];  hidden_states = [x]
  layer:  h = LN1(x); q, k, v = {q,k,v}_proj(h) in heads of 64;  x = x + out_proj(softmax(q k^T / sqrt(64) + triu(-inf, 1)) v)
          h = fc1(LN2(x)); h = h * sigmoid(1.702 h) (quick_gelu) | gelu_erf(h);  x = x + fc2(h);  hidden_states.append(x)
  last_hidden_state = final_layer_norm(x);  pooler_output = last[b, argmax_t ids[b]];  text_embeds = pooler_output @ text_projection.T
"""
import torch
import torch.nn.functional as F

PREFIX = "text_model."


def normalise_keys(sd):
    """transformers 5 CLIPTextModel.state_dict() has no `text_model.` prefix, CLIPTextModelWithProjection and the published files have it: add it
    where it is absent (text_projection.weight stays at the top level)"""
    return {(k if k.startswith(PREFIX) or k.startswith("text_projection.") else PREFIX + k): v for k, v in sd.items()}


class Ref:
    def __init__(self, state_dict, num_heads, hidden_act, eps=1e-5, dtype=torch.float32, device=None):
        self.p = {k: v.detach().to(device=device or v.device, dtype=dtype) for k, v in normalise_keys(state_dict).items()}
        self.heads, self.act, self.eps = num_heads, hidden_act, eps
        self.L = 1 + max(int(k.split(".")[3]) for k in self.p if k.startswith(PREFIX + "encoder.layers."))

    def lin(self, x, name):
        return F.linear(x, self.p[name + ".weight"], self.p.get(name + ".bias"))

    def ln(self, x, name):
        return F.layer_norm(x, (x.shape[-1],), self.p[name + ".weight"], self.p[name + ".bias"], self.eps)

    def __call__(self, ids):
        """ids (B, T) -> dict(hidden_states tuple of L + 1, last_hidden_state, pooler_output, text_embeds or None)"""
        p = self.p
        ids = torch.as_tensor(ids).long().to(p[PREFIX + "final_layer_norm.weight"].device)
        B, T = ids.shape
        x = p[PREFIX + "embeddings.token_embedding.weight"][ids] + p[PREFIX + "embeddings.position_embedding.weight"][:T]
        C, H = x.shape[-1], self.heads
        d = C // H
        mask = torch.full((T, T), float("-inf"), dtype=x.dtype, device=x.device).triu(1)
        hs = [x]
        for i in range(self.L):
            base = f"{PREFIX}encoder.layers.{i}."
            h = self.ln(x, base + "layer_norm1")
            q, k, v = (self.lin(h, base + f"self_attn.{n}_proj").reshape(B, T, H, d).transpose(1, 2) for n in "qkv")
            a = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + mask, dim=-1) @ v
            x = x + self.lin(a.transpose(1, 2).reshape(B, T, C), base + "self_attn.out_proj")
            h = self.lin(self.ln(x, base + "layer_norm2"), base + "mlp.fc1")
            h = h * torch.sigmoid(1.702 * h) if self.act == "quick_gelu" else F.gelu(h)
            x = x + self.lin(h, base + "mlp.fc2")
            hs.append(x)
        last = self.ln(x, PREFIX + "final_layer_norm")
        pooled = last[torch.arange(B, device=x.device), ids.argmax(-1)]
        te = pooled @ p["text_projection.weight"].T if "text_projection.weight" in p else None
        return {"hidden_states": tuple(hs), "last_hidden_state": last, "pooler_output": pooled, "text_embeds": te}


def prompt_ids(n_tokens, pad_id, seed=0, vocab=49408, length=77):
    """[BOS, n_tokens random word ids, EOS, pad ...]: what a tokenizer gives for a prompt of n_tokens tokens (ids < 49406, so EOS is the row's maximum)"""
    g = torch.Generator().manual_seed(seed * 1000 + n_tokens)
    body = torch.randint(1, min(vocab, 49406), (n_tokens,), generator=g).tolist()
    ids = [49406] + body + [49407]
    return ids + [pad_id] * (length - len(ids))


def prompt_batch(pad_id, lengths=(0, 9, 40, 75), seed=0):
    return torch.tensor([prompt_ids(n, pad_id, seed) for n in lengths])
