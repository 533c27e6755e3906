"""SDXL self-attention (attn1) on HIP: HIPAttnProcessor, install_self_attention_processors, the stand-in UNet with self_attention=True."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sdxl_common import FakeAttention

pytestmark = pytest.mark.gpu


class SelfAttention(FakeAttention):
    """FakeAttention as diffusers builds attn1 (cross_dim = dim), with the attributes AttnProcessor2_0 reads"""

    def __init__(self, dim, heads):
        super().__init__(dim, dim, heads)
        self.scale = 64 ** -0.5
        self.group_norm = None
        self.spatial_norm = None


def _torch_ref(attn, x, enc=None):
    """AttnProcessor2_0 in fp32 on the 16-bit projections the product stores (q / k / v and the attention output rounded to x.dtype)"""
    dt = x.dtype
    shape4 = x.shape if x.dim() == 4 else None
    if shape4 is not None:
        b, c, hh, ww = shape4
        x = x.view(b, c, hh * ww).transpose(1, 2)
    res = x
    src = x if enc is None else enc
    lin = lambda t, layer: F.linear(t.float(), layer.weight.float(), None if layer.bias is None else layer.bias.float())
    q, k, v = lin(x, attn.to_q).to(dt), lin(src, attn.to_k).to(dt), lin(src, attn.to_v).to(dt)
    B, T, C = q.shape
    sp = lambda t: t.float().view(B, t.shape[1], attn.heads, 64).transpose(1, 2)
    p = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) * attn.scale, -1)
    o = (p @ sp(v)).transpose(1, 2).reshape(B, T, C).to(dt)
    out = lin(o, attn.to_out[0])
    if attn.residual_connection:
        out = out + res.float()
    out = out.to(dt)
    if shape4 is not None:
        out = out.transpose(-1, -2).reshape(shape4)
    return out / attn.rescale_output_factor


class _Forbid:
    """F.linear, nn.Linear.forward and F.scaled_dot_product_attention raise while active; counts linear16 / self_attention calls of the module"""

    def __init__(self, monkeypatch):
        from eeg_image_decode_amd import sdxl
        self.calls = {"linear16": 0, "self_attention": 0}

        def boom(*a, **k):
            raise AssertionError("a library GEMM / attention was called")
        monkeypatch.setattr(F, "linear", boom)
        monkeypatch.setattr(torch.nn.Linear, "forward", boom)
        monkeypatch.setattr(F, "scaled_dot_product_attention", boom)
        for name in self.calls:
            real = getattr(sdxl, name)

            def wrap(*a, _real=real, _name=name, **k):
                self.calls[_name] += 1
                return _real(*a, **k)
            monkeypatch.setattr(sdxl, name, wrap)


def _close(got, ref, dt):
    tol = 1e-2 if dt == torch.float16 else 5e-2
    d = (got.float() - ref.float()).abs()
    assert torch.isfinite(got).all()
    assert d.max().item() < tol * max(1.0, ref.float().abs().max().item()), d.max().item()
    assert d.mean().item() < tol / 6, d.mean().item()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("dim,heads,T", [(640, 10, 4096), (1280, 20, 1024)])
def test_processor_runs_no_library_gemm_and_matches_torch(monkeypatch, dim, heads, T, dt):
    from eeg_image_decode_amd.sdxl import HIPAttnProcessor
    torch.manual_seed(dim + T)
    attn = SelfAttention(dim, heads).cuda().to(dt)
    x = torch.randn(2, T, dim, device="cuda", dtype=dt)
    with torch.no_grad():
        ref = _torch_ref(attn, x)
        proc = HIPAttnProcessor()
        fb = _Forbid(monkeypatch)
        got = proc(attn, x)
        torch.cuda.synchronize()
        assert fb.calls == {"linear16": 2, "self_attention": 1}
        got2 = proc(attn, x)                                           # cached fused weight: the same launches, the same result
        assert fb.calls == {"linear16": 4, "self_attention": 2}
        monkeypatch.undo()
    assert torch.equal(got, got2)
    _close(got, ref, dt)


def test_processor_4d_input_residual_and_rescale():
    from eeg_image_decode_amd.sdxl import HIPAttnProcessor
    torch.manual_seed(3)
    dim, heads = 256, 4
    attn = SelfAttention(dim, heads).cuda().half()
    attn.residual_connection, attn.rescale_output_factor = True, 2.0
    with torch.no_grad():
        x4 = torch.randn(2, dim, 12, 10, device="cuda", dtype=torch.float16)
        got = HIPAttnProcessor()(attn, x4)
        assert got.shape == x4.shape
        _close(got, _torch_ref(attn, x4), torch.float16)
        x3 = torch.randn(2, 100, dim, device="cuda", dtype=torch.float16)
        _close(HIPAttnProcessor()(attn, x3), _torch_ref(attn, x3), torch.float16)
        # encoder states given: K / V from them (separate GEMMs), Tq != Tk
        enc = torch.randn(2, 300, dim, device="cuda", dtype=torch.float16)
        _close(HIPAttnProcessor()(attn, x3, encoder_hidden_states=enc), _torch_ref(attn, x3, enc), torch.float16)


def test_in_place_weight_edit_rebuilds_the_fused_weight():
    from eeg_image_decode_amd.sdxl import HIPAttnProcessor
    torch.manual_seed(4)
    attn = SelfAttention(256, 4).cuda().half()
    x = torch.randn(1, 200, 256, device="cuda", dtype=torch.float16)
    proc = HIPAttnProcessor()
    with torch.no_grad():
        a = proc(attn, x).clone()
        attn.to_k.weight.mul_(-1.5)                                     # same object, same address: only _version changes
        b = proc(attn, x)
        _close(b, _torch_ref(attn, x), torch.float16)
        assert not torch.equal(a, b)
        attn.to_v.weight = torch.nn.Parameter(attn.to_v.weight.detach() * 0.5)     # replaced object
        _close(proc(attn, x), _torch_ref(attn, x), torch.float16)


def test_unsupported_inputs_raise():
    from eeg_image_decode_amd._lib import EegclipError
    from eeg_image_decode_amd.sdxl import HIPAttnProcessor, self_attention
    attn = SelfAttention(256, 4).cuda().half()
    x = torch.randn(1, 64, 256, device="cuda", dtype=torch.float16)
    proc = HIPAttnProcessor()
    with torch.no_grad():
        with pytest.raises(EegclipError):
            proc(attn, x, attention_mask=torch.zeros(1, 64, 64, device="cuda", dtype=torch.float16))
        attn.group_norm = torch.nn.GroupNorm(32, 256)
        with pytest.raises(EegclipError):
            proc(attn, x)
        attn.group_norm = None
        attn.heads = 2                                                  # head_dim 128
        with pytest.raises(EegclipError):
            proc(attn, x)
        with pytest.raises(EegclipError):
            self_attention(x.cpu(), x.cpu(), x.cpu(), 4)
        with pytest.raises(EegclipError):
            self_attention(x, x, x, 5)


def test_long_sequence_allocates_no_score_matrix():
    from eeg_image_decode_amd.sdxl import self_attention
    T = 16384
    q, k, v = (torch.randn(1, T, 64, device="cuda", dtype=torch.float16) for _ in range(3))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = self_attention(q, k, v, 1)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 64 * 2 ** 20          # a T x T fp16 buffer would be 512 MB
    rows = torch.arange(0, T, 997, device="cuda")
    s = q[0, rows].float() @ k[0].float().T / 8
    e = torch.exp(s - s.max(-1, keepdim=True).values)                # the kernel rounds the UNnormalised probabilities, divides once at the end
    ref = (e.half().float() @ v[0].float()) / e.sum(-1, keepdim=True)
    np.testing.assert_allclose(out[0, rows].float().cpu().numpy(), ref.cpu().numpy(), atol=6e-3)


def test_installer_replaces_exactly_the_attn1_processors():
    from eeg_image_decode_amd.sdxl import HIPAttnProcessor, install_self_attention_processors
    names = [f"down_blocks.{i}.attentions.0.transformer_blocks.{j}.attn{a}.processor" for i in range(2) for j in range(2) for a in (1, 2)]
    names.append("mid_block.attentions.0.transformer_blocks.0.attn1.processor")

    class FakeUNet:
        def __init__(self):
            self.procs = {n: object() for n in names}

        @property
        def attn_processors(self):
            return dict(self.procs)

        def set_attn_processor(self, procs):
            assert set(procs) == set(self.procs)
            self.procs = procs

        def get_submodule(self, name):
            raise AssertionError("not needed")

    u = FakeUNet()
    old = dict(u.procs)
    install_self_attention_processors(u)
    for n in names:
        if ".attn1." in n:
            assert isinstance(u.procs[n], HIPAttnProcessor)
        else:
            assert u.procs[n] is old[n]
    assert len({id(u.procs[n]) for n in names if ".attn1." in n}) == 5       # one processor (and weight cache) per layer


def test_stand_in_default_is_unchanged():
    from eeg_image_decode_amd.sdxl import SDXLShapedUNet
    a, b = SDXLShapedUNet(stage_layers=(1, 2, 1, 1, 1), seed=3), SDXLShapedUNet(stage_layers=(1, 2, 1, 1, 1), seed=3, self_attention=False)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    c = SDXLShapedUNet(stage_layers=(1, 2, 1, 1, 1), seed=3, self_attention=True).state_dict()
    assert all(torch.equal(sa[k], c[k]) for k in sa) and set(c) - set(sa) and all(k.startswith("self_slots.") for k in set(c) - set(sa))


def _unet_inputs(B, L, dev="cuda"):
    g = torch.Generator().manual_seed(9)
    sample = torch.randn(B, 4, L, L, generator=g).half().to(dev)
    text = (torch.randn(B, 77, 2048, generator=g) * 0.5).half().to(dev)
    added = {"text_embeds": (torch.randn(B, 1280, generator=g) * 0.5).half().to(dev),
             "time_ids": torch.tensor([[L * 8.0, L * 8.0, 0.0, 0.0, L * 8.0, L * 8.0]] * B).half().to(dev),
             "image_embeds": torch.randn(B, 1024, generator=g).half().to(dev)}
    return sample, text, added


def test_stand_in_with_zeroed_attn1_output_is_the_default_model():
    from eeg_image_decode_amd.sdxl import SDXLShapedUNet
    sample, text, added = _unet_inputs(2, 16)
    a = SDXLShapedUNet(stage_layers=(1, 1, 1, 1, 1), seed=5).cuda()
    b = SDXLShapedUNet(stage_layers=(1, 1, 1, 1, 1), seed=5, self_attention=True).cuda()
    with torch.no_grad():
        for s in b.self_slots:
            s.to_out.zero_()
            s.to_out_bias.zero_()
        ya = a(sample, 999, encoder_hidden_states=text, added_cond_kwargs=added)[0]
        yb = b(sample, 999, encoder_hidden_states=text, added_cond_kwargs=added)[0]
    assert torch.equal(ya, yb)


def _stand_in_ref(unet, sample, t, text, added):
    """SDXLShapedUNet.forward with self_attention=True restated in torch fp32, 16-bit rounding where the product stores a tensor
    (oracle/sdxl_pipeline.standin_unet plus h = h + attn1(h) before every cross-attention)"""
    W = {k: v.detach().float() for k, v in unet.state_dict().items()}
    rnd = lambda x: x.half().float()
    B, _, L, _ = sample.shape
    l1, l2 = L // 2, L // 4
    lin = lambda x, w, b=None: rnd(x @ W[w].T + (W[b] if b else 0.0))
    silu = F.silu

    def sinus(tt, dim):
        half = dim // 2
        f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32, device=tt.device) / half)
        arg = tt.float()[..., None] * f
        return torch.cat([arg.cos(), arg.sin()], -1)

    def attend(q, k, v, heads):
        Bq, Tq, C = q.shape
        sp = lambda z: z.view(Bq, z.shape[1], heads, 64).transpose(1, 2)
        p = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / 8, -1)
        return (p @ sp(v)).transpose(1, 2).reshape(Bq, Tq, C)

    text, img = text.float(), added["image_embeds"].float()
    temb = rnd(sinus(torch.full((B,), float(t), device=sample.device), 320))
    e = lin(rnd(silu(lin(temb, "time_w1"))), "time_w2")
    aug = torch.cat([added["text_embeds"].float(), rnd(sinus(added["time_ids"].float().reshape(-1), 256).reshape(B, -1))], -1)
    e = rnd(e + lin(rnd(silu(lin(aug, "add_w1"))), "add_w2"))
    emb = rnd(silu(e))
    x = lin(img, "image_proj", "image_proj_bias").reshape(B, -1, 2048)
    ip = rnd(F.layer_norm(x, (2048,), W["image_ln_w"], W["image_ln_b"], 1e-5))
    x = sample.float().reshape(B, 4, l1, 2, l1, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, l1 * l1, 16)
    h = rnd(x @ W["conv_in"][:, :16].T + lin(emb, "stage_t.0")[:, None, :])
    slot = [0]

    def run(n, h):
        for _ in range(n):
            i = slot[0]
            slot[0] += 1
            p, sp_ = f"slots.{i}.", f"self_slots.{i}."
            C = h.shape[-1]
            heads = C // 64
            qkv = rnd(h @ W[sp_ + "to_qkv"].T)
            a = rnd(attend(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads))
            h = rnd(a @ W[sp_ + "to_out"].T + W[sp_ + "to_out_bias"] + h)
            q = rnd(h @ W[p + "to_q"].T)
            k, v = rnd(text @ W[p + "to_k"].T), rnd(text @ W[p + "to_v"].T)
            kip, vip = rnd(ip @ W[p + "to_k_ip"].T), rnd(ip @ W[p + "to_v_ip"].T)
            a = rnd(attend(q, k, v, heads) + unet.ip_scale * attend(q, kip, vip, heads))
            h = rnd(a @ W[p + "to_out"].T + W[p + "to_out_bias"] + h)
        return h

    h = run(unet.stage_layers[0], h)
    h = h.reshape(B, l2, 2, l2, 2, 640).permute(0, 1, 3, 2, 4, 5).reshape(B, l2 * l2, 2560)
    h = rnd(h @ W["down"].T + lin(emb, "stage_t.1")[:, None, :])
    for s in (1, 2, 3):
        h = run(unet.stage_layers[s], h)
    h = rnd(h @ W["up"].T).reshape(B, l2, l2, 2, 2, 640).permute(0, 1, 3, 2, 4, 5).reshape(B, l1 * l1, 640)
    h = rnd(h + lin(emb, "stage_t.2")[:, None, :])
    h = run(unet.stage_layers[4], h)
    y = rnd(h @ W["conv_out"].T)[..., :16]
    return y.reshape(B, l1, l1, 4, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(B, 4, L, L)


def test_stand_in_with_self_attention_matches_torch_restatement():
    from eeg_image_decode_amd.sdxl import SDXLShapedUNet
    sample, text, added = _unet_inputs(2, 16)
    unet = SDXLShapedUNet(stage_layers=(1, 1, 1, 1, 1), seed=5, self_attention=True).cuda()
    with torch.no_grad():
        out = unet(sample, 999, encoder_hidden_states=text, added_cond_kwargs=added)[0]
        ref = _stand_in_ref(unet, sample, 999, text, added)
    d = (out.float() - ref).abs()
    assert d.max().item() < 1e-2 * max(1.0, ref.abs().max().item()), (d.max().item(), ref.abs().max().item())
    assert d.mean().item() < 1e-3, d.mean().item()
    # and the attn1 path is not a no-op: the default model differs
    base = SDXLShapedUNet(stage_layers=(1, 1, 1, 1, 1), seed=5).cuda()
    with torch.no_grad():
        y0 = base(sample, 999, encoder_hidden_states=text, added_cond_kwargs=added)[0]
    assert (y0.float() - out.float()).abs().max().item() > 1e-2


def test_full_size_ddim_step_with_self_attention_is_finite():
    from eeg_image_decode_amd.sdxl import DDIMScheduler, SDXLShapedUNet, StandInSDXLPipeline
    pipe = StandInSDXLPipeline(SDXLShapedUNet(self_attention=True), DDIMScheduler(), device="cuda", default_sample_size=128)
    emb = torch.randn(2, 1024, generator=torch.Generator().manual_seed(4)).half()
    out = pipe.generate_ip_adapter_embeds(prompt="", ip_adapter_embeds=emb.cuda(), num_inference_steps=1, guidance_scale=5.0,
                                          generator=torch.Generator().manual_seed(12)).images
    assert out.shape == (2, 4, 128, 128)
    assert torch.isfinite(out.float()).all()
