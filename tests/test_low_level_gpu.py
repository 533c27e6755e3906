"""eeg_image_decode_amd.low_level.LowLevelEncoder on the GPU against the fp32 restatement (tests/low_level_ref.py), and its latent through the sampling
pipeline's low-level entry.  Reduced widths (hidden = 64): all six layers to a 64 x 64 latent, and a four-layer stack to 16 x 16.

Measure: relative L2 of the output to the fp32 restatement; allowance 3 x the format's own error = the restatement with its activations rounded to the
16-bit dtype at every layer boundary (measured against the reference, not against the code under test; the rule of tests/test_git_caption_gpu.py).
Measured on an MI355X (relative L2 / format error / allowance = 3 x that), B = 1, 3, 17:
    64 x 64 fp16   6.08e-4 / 6.07e-4 / 1.82e-3,  5.80e-4 / 5.72e-4 / 1.72e-3,  5.84e-4 / 5.79e-4 / 1.74e-3
    64 x 64 bf16   4.71e-3 / 4.71e-3 / 1.41e-2,  4.62e-3 / 4.62e-3 / 1.39e-2,  4.76e-3 / 4.76e-3 / 1.43e-2
    16 x 16 fp16   5.68e-4 / 5.88e-4 / 1.76e-3,  5.84e-4 / 6.00e-4 / 1.80e-3,  5.81e-4 / 5.78e-4 / 1.73e-3
    16 x 16 bf16   4.40e-3 / 4.40e-3 / 1.32e-2,  4.39e-3 / 4.39e-3 / 1.32e-2,  4.45e-3 / 4.45e-3 / 1.34e-2
"""
import pytest
import torch

from low_level_ref import calibrated

pytestmark = pytest.mark.gpu

CH64 = (4032, 128, 64, 64, 64, 64, 4)
CH16 = (4032, 128, 64, 64, 4)
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
_cases = {}


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def case(ch, dt):
    """(product module on the GPU, x (17, 63, 250), fp32 restatement's output, its output with 16-bit activations), built once per configuration"""
    if (ch, dt) not in _cases:
        from eeg_image_decode_amd.low_level import LowLevelEncoder
        ref = calibrated(64, ch, DTYPES[dt], seed=len(ch))
        model = LowLevelEncoder(hidden=64, channels=ch, dtype=DTYPES[dt], device="cuda", seed=9)
        model.load_state_dict(ref.state_dict())
        x = torch.randn(17, 63, 250, generator=torch.Generator().manual_seed(11))
        with torch.no_grad():
            _cases[(ch, dt)] = (model, x, ref(x), ref(x, round_to=DTYPES[dt]), ref)
    return _cases[(ch, dt)]


@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("ch", [CH64, CH16], ids=["64x64", "16x16"])
def test_forward_matches_the_restatement(ch, dt, B):
    model, x, want, fmt, _ = case(ch, dt)
    got = model(x[:B].cuda())
    again = model(x[:B].cuda())
    S = 2 ** (len(ch) - 1)
    assert got.dtype == DTYPES[dt] and tuple(got.shape) == (B, 4, S, S) and torch.isfinite(got).all() and torch.equal(got, again)
    err, e_fmt = rel_l2(got.float().cpu(), want[:B]), rel_l2(fmt[:B], want[:B])
    print(f"low-level encoder {S}x{S} {dt} B={B}: relative L2 {err:.3e}, format error {e_fmt:.3e}, allowance {3 * e_fmt:.3e}")
    assert 0.1 < float(want[:B].abs().mean()) < 10, "the calibrated reference is not O(1)"
    assert err < 3 * e_fmt


def test_caches_follow_buffers_and_state_dict():
    """an in-place change of running_var, and load_state_dict, each change the next forward: the cache keys include the BatchNorm buffers"""
    model, x, _, _, ref = case(CH16, "f16")
    xb = x[:2].cuda()
    base = model(xb).clone()
    model.upsampler[1].running_var.mul_(4.0)
    changed = model(xb).clone()
    assert not torch.equal(changed, base)
    model.load_state_dict(ref.state_dict())
    assert torch.equal(model(xb), base)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    sd["upsampler.4.running_mean"] += 0.5
    sd["upsampler.9.bias"] += 1.0
    model.load_state_dict(sd)
    moved = model(xb).clone()
    assert not torch.equal(moved, base) and float((moved.float() - base.float()).abs().mean()) > 0.5
    model.load_state_dict(ref.state_dict())
    assert torch.equal(model(xb), base)


def test_train_mode_raises():
    from eeg_image_decode_amd._lib import EegclipError
    model, x, _, _, _ = case(CH16, "f16")
    model.train()
    try:
        with pytest.raises(EegclipError):
            model(x[:1].cuda())
    finally:
        model.eval()
    with pytest.raises(EegclipError):
        model(x[:1])                                                             # a CPU tensor: no eager path


def test_latent_starts_the_sampling_loop():
    """the encoder's 16 x 16 latent as low_level_latent: through Generator4Embeds.generate(emb, low_level_latent=) and generate_ip_adapter_embeds directly
    the loop's start (prepare_latents_latent2img's input) is exactly the encoder's output, and the result differs from the run without it"""
    from eeg_image_decode_amd.sdxl import DDIMScheduler, Generator4Embeds, SDXLShapedUNet, StandInSDXLPipeline
    model, x, _, _, _ = case(CH16, "f16")
    lat = model(x[:1].cuda())
    assert tuple(lat.shape) == (1, 4, 16, 16)
    pipe = StandInSDXLPipeline(SDXLShapedUNet(stage_layers=(1, 1, 1, 1, 1)), DDIMScheduler(), default_sample_size=16)
    emb = torch.randn(1, 1024, generator=torch.Generator().manual_seed(4)).cuda().to(pipe.dtype)
    seen = []
    real = pipe.prepare_latents_latent2img
    pipe.prepare_latents_latent2img = lambda l, *a, **k: (seen.append(l.clone()), real(l, *a, **k))[1]
    gen = lambda: torch.Generator(device="cuda").manual_seed(12)  # noqa: E731
    g4 = Generator4Embeds(num_inference_steps=4, pipe=pipe, img2img_strength=0.5)
    via_wrapper = g4.generate(emb, generator=gen(), low_level_latent=lat)
    direct = pipe.generate_ip_adapter_embeds(prompt="", ip_adapter_embeds=emb, num_inference_steps=4, guidance_scale=0.0, img2img_strength=0.5,
                                             low_level_latent=lat, generator=gen(), output_type="latent").images
    assert len(seen) == 2 and all(torch.equal(s, lat) for s in seen)
    assert torch.isfinite(direct).all() and torch.equal(via_wrapper, direct[0])
    without = g4.generate(emb, generator=gen())
    assert len(seen) == 2 and without.shape == via_wrapper.shape and not torch.equal(without, via_wrapper)
    assert g4.low_level_latent is None                                          # the per-call latent did not stick
