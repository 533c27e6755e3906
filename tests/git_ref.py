"""fp32 restatement of transformers' GitForCausalLM with the visual tokens handed in (modeling_git.py: GitEmbeddings, GitProjection, the post-LN BERT layers of
GitEncoder, GitModel's prefix-causal mask, the untied `output` head), torch.nn.functional over a state_dict -- the yardstick of
eeg_image_decode_amd/git_caption.py.  tests/test_git_layout.py pins it to transformers itself (use_cache=False) where transformers is installed.

  x = cat([LN_v(Linear_v(visual_features)), LN_e(word_embeddings[ids] + position_embeddings[:T])], 1)       positions count text tokens only
  layer:  q, k, v = query / key / value(x) in heads of 64;  a = softmax(q k^T / 8 + mask) v;  x = LN(attention.output.dense(a) + x)
          x = LN(output.dense(gelu_erf(intermediate.dense(x))) + x)
  mask:   key j reaches query i iff j < max(i + 1, P)
  logits = output(x[:, P:])

`round_to`: a 16-bit dtype to which the activations are rounded at every layer boundary the HIP path has (each GEMM's, LayerNorm's, activation's and
attention's output): the error the I/O format alone causes, the reference against itself.
"""
import torch
import torch.nn.functional as F


class GitRef:
    def __init__(self, state_dict, num_heads, eps=1e-12, vision_eps=1e-5, dtype=torch.float32, round_to=None):
        self.p = {k: v.detach().to(dtype) for k, v in state_dict.items() if not k.startswith(("git.image_encoder.", "git.img_temporal_embedding"))}
        self.heads, self.eps, self.vision_eps, self.round_to = num_heads, eps, vision_eps, round_to
        self.L = 1 + max(int(k.split(".")[3]) for k in self.p if k.startswith("git.encoder.layer."))

    def r(self, x):
        return x if self.round_to is None else x.to(self.round_to).to(x.dtype)

    def lin(self, x, name, residual=None):
        y = F.linear(x, self.p[name + ".weight"], self.p[name + ".bias"])
        return self.r(y if residual is None else y + residual)

    def ln(self, x, name, eps):
        return self.r(F.layer_norm(x, (x.shape[-1],), self.p[name + ".weight"], self.p[name + ".bias"], eps))

    def __call__(self, ids, visual_features):
        """ids (B, T), visual_features (B, P, Dv) -> logits (B, T, vocab) of the text positions"""
        p = self.p
        ids = torch.as_tensor(ids).long()
        vis = self.r(visual_features.to(p["output.weight"].dtype))
        B, T = ids.shape
        P = vis.shape[1]
        vp = "git.visual_projection.visual_projection."
        xv = self.ln(self.lin(vis, vp + "0"), vp + "1", self.vision_eps)
        xe = self.r(p["git.embeddings.word_embeddings.weight"][ids] + p["git.embeddings.position_embeddings.weight"][:T])
        x = torch.cat([xv, self.ln(xe, "git.embeddings.LayerNorm", self.eps)], dim=1)
        S, C, H = P + T, x.shape[-1], self.heads
        d = C // H
        i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
        mask = torch.zeros(S, S, dtype=x.dtype).masked_fill(j >= torch.maximum(i + 1, torch.tensor(P)), float("-inf"))
        for n in range(self.L):
            base = f"git.encoder.layer.{n}."
            q, k, v = (self.lin(x, base + f"attention.self.{w}").reshape(B, S, H, d).transpose(1, 2) for w in ("query", "key", "value"))
            a = self.r((torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + mask, dim=-1) @ v).transpose(1, 2).reshape(B, S, C))
            x = self.ln(self.lin(a, base + "attention.output.dense", x), base + "attention.output.LayerNorm", self.eps)
            h = self.r(F.gelu(self.lin(x, base + "intermediate.dense")))
            x = self.ln(self.lin(h, base + "output.dense", x), base + "output.LayerNorm", self.eps)
        return F.linear(x[:, P:], p["output.weight"], p["output.bias"])

    def greedy(self, visual_features, max_length, bos=101, eos=102, pad=0, prompt_ids=None):
        """greedy decoding by recomputing the forward (transformers' generate(do_sample=False, use_cache=False)): ids (B, <= max_length); ties -> lowest
        id; a sample that has emitted eos emits pad from then on; ends when all have finished or at max_length.  Also returns the logits (B, vocab) each
        token was chosen from, per step."""
        B = visual_features.shape[0]
        ids = torch.full((B, 1), bos, dtype=torch.long) if prompt_ids is None else torch.as_tensor(prompt_ids).long()
        finished = torch.zeros(B, dtype=torch.bool)
        steps = []
        while ids.shape[1] < max_length:
            logits = self(ids, visual_features)[:, -1]
            steps.append(logits)
            nxt = torch.where(finished, torch.full((B,), pad), logits.argmax(-1))
            ids = torch.cat([ids, nxt[:, None]], dim=1)
            finished = finished | (nxt == eos)
            if bool(finished.all()):
                break
        return ids, steps
