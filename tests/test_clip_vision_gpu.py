"""CLIPVisionEncoder on the MI355X against the fp32 restatement of transformers' CLIP vision models (tests/clip_vision_ref.py, pinned to transformers by
tests/test_clip_vision_layout.py), run on the module's own 16-bit weights on the same device.  Error measure: relative L2, |hip - ref| / |ref|, of every
entry of hidden_states, of last_hidden_state, pooler_output and image_embeds; default module initialisation; B images of standard-normal-ish pixels, sample 0
all zeros.

Bound: nothing fixed in advance.  Each output's bound is 3 x the error of THE SAME restatement run in the module's 16-bit dtype (torch ops, weights and
activations in fp16 / bf16, same device, weights and input) against the fp32 one -- computed in the test from the reference alone; 3 x the format's own
error is the margin of the low-level trainer's gradients (tests/low_level_train_common.py).

Measured (MI355X; largest ratio hip error / format error over all outputs, and the errors of the last output -- image_embeds, or last_hidden_state for the
GIT tower -- hip | 16-bit restatement):
  2 layers, 1280 / 16 heads of 80, B = 2    fp16  0.98   image_embeds       5.87e-4 | 6.02e-4        bf16  1.00   image_embeds       4.59e-3 | 4.60e-3
  2 layers, 1024 / 16 heads of 64, B = 2    fp16  0.95   last_hidden_state  5.27e-4 | 5.73e-4        bf16  0.98   last_hidden_state  4.20e-3 | 4.56e-3
  ip_adapter_image_encoder(), B = 1         fp16  1.03   image_embeds       1.72e-3 | 1.68e-3        (hidden_states[0] 2.4e-4 | 3.3e-4, [32] 1.63e-3 | 1.66e-3)
  git_vision_tower(), B = 1                 fp16  1.04   last_hidden_state  1.46e-3 | 1.50e-3        (hidden_states[0] 2.4e-4 | 3.3e-4, [24] 1.44e-3 | 1.48e-3)
The HIP path is as far from fp32 as torch's own 16-bit arithmetic is; the error grows with depth, as the text encoders' does (the 16-bit residual stream is
rounded after every layer).  The same figures are in profiles/clip_vision_bench.json under `model_errors`.
"""
import pytest
import torch

from clip_vision_ref import Ref, pixel_batch
from eeg_image_decode_amd import clip_vision

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
REAL = {     # the real widths and token count (image 224, T = 257), 2 layers
    "vit_h_dim80": dict(hidden_size=1280, intermediate_size=5120, num_attention_heads=16, hidden_act="gelu", projection_dim=1024),
    "vit_l_dim64": dict(hidden_size=1024, intermediate_size=4096, num_attention_heads=16, hidden_act="quick_gelu", projection_dim=None, post_layernorm_all=True),
}


def rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / b.norm())


def outputs(o, projected):
    """(name, tensor) of every output of a CLIPVisionOutput or of the restatement's dict"""
    get = (lambda k: o[k]) if isinstance(o, dict) else (lambda k: getattr(o, k))
    items = [(f"hidden_states[{i}]", h) for i, h in enumerate(get("hidden_states"))]
    items += [("last_hidden_state", get("last_hidden_state")), ("pooler_output", get("pooler_output"))]
    return items + ([("image_embeds", get("image_embeds"))] if projected else [])


def check_model(m, B, tag):
    """every output within 3 x the 16-bit restatement's own error; two runs bit-identical.  Prints every figure before it asserts."""
    c = m.config
    kw = dict(eps=c.layer_norm_eps, post_layernorm_all=c.post_layernorm_all, device="cuda")
    px = pixel_batch(B, c.image_size, seed=B, zero_sample=B > 1).to(m.dtype).cuda()
    want = outputs(Ref(m.state_dict(), c.num_attention_heads, c.hidden_act, dtype=torch.float32, **kw)(px.float()), c.projection_dim is not None)
    fmt = outputs(Ref(m.state_dict(), c.num_attention_heads, c.hidden_act, dtype=m.dtype, **kw)(px), c.projection_dim is not None)
    out = m(px, output_hidden_states=True)
    again = m(px, output_hidden_states=True)
    torch.cuda.synchronize()
    got = outputs(out, c.projection_dim is not None)
    assert len(got) == len(want) == c.num_hidden_layers + 3 + (c.projection_dim is not None)
    rows = []
    for (name, a), (_, w), (_, f) in zip(got, want, fmt):
        assert a.shape == w.shape and a.dtype == m.dtype and torch.isfinite(a.float()).all(), name
        rows.append((name, rel(a, w), rel(f, w)))
        print(f"\n[rel-l2] {tag} {str(m.dtype).split('.')[-1]} {name}: hip {rows[-1][1]:.3e}  16-bit restatement {rows[-1][2]:.3e}  ratio {rows[-1][1] / rows[-1][2]:.2f}", end=" ")
    for (name, a), (_, b) in zip(got, outputs(again, c.projection_dim is not None)):
        assert torch.equal(a, b), f"{name}: two runs differ"
    for name, e, f in rows:
        assert e < 3 * f, (name, e, f)
    return rows


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", list(REAL))
def test_real_shape_two_layer_tower(name, dtype):
    """2 layers at the real width, head count and image size (T = 257), B = 2, for each head dim"""
    m = clip_vision.CLIPVisionEncoder(num_hidden_layers=2, dtype=dtype, device="cuda", seed=1, **REAL[name])
    check_model(m, 2, name)


@pytest.mark.parametrize("factory", ["ip_adapter_image_encoder", "git_vision_tower"])
def test_full_size_tower(factory):
    """one full-size forward of each factory at B = 1 in fp16 (32 layers of 1280 / 24 layers of 1024)"""
    m = getattr(clip_vision, factory)(dtype=F16, device="cuda")
    check_model(m, 1, factory)
    del m
    torch.cuda.empty_cache()


def test_no_library_op_on_the_path(monkeypatch):
    """tests/test_clip_text_gpu.py's rule for this module: no nn.Linear / F.linear / F.layer_norm / conv / matmul call during a forward"""
    m = clip_vision.CLIPVisionEncoder(640, 1280, 1, 8, "gelu", 128, image_size=28, device="cuda")
    px = pixel_batch(2, 28).cuda()
    want = m(px, output_hidden_states=True)

    def forbidden(*a, **k):
        raise AssertionError("library op on the vision tower's path")
    for mod, name in ((torch.nn.functional, "linear"), (torch.nn.Linear, "forward"), (torch.nn.functional, "layer_norm"), (torch.nn.LayerNorm, "forward"),
                      (torch.nn.functional, "conv2d"), (torch.nn.Conv2d, "forward"), (torch.nn.functional, "embedding"), (torch.nn.Embedding, "forward"),
                      (torch, "matmul"), (torch, "bmm"), (torch.nn.functional, "gelu"), (torch.nn.functional, "softmax"), (torch.nn.functional, "unfold"),
                      (torch.nn.functional, "scaled_dot_product_attention")):
        monkeypatch.setattr(mod, name, forbidden)
    got = m(px, output_hidden_states=True)
    assert torch.equal(got.image_embeds, want.image_embeds)
