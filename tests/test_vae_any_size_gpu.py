"""eeg_image_decode_amd.vae.SDXLShapedVAE at image sizes whose latent H * W is no multiple of 128, and at a larger latent: the mid-block attention is
one flash-style launch (csrc/vae_attn.hip) that takes any number of positions.  Full SDXL layout, seed 3, against oracle/sdxl_vae.py (fp32) on the
16-bit-rounded parameters, at the error budget of tests/test_vae_gpu.py: max <= 3e-2 and mean <= 4e-3 of the reference's max |value|."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _budget(got, ref):
    scale = float(ref.abs().max())
    err = (got - ref).abs()
    print(f"max error {float(err.max()) / scale:.3e} (bound 3e-2), mean error {float(err.mean()) / scale:.3e} (bound 4e-3) of the output scale {scale:.3f}")
    assert float(err.max()) <= 3e-2 * scale and float(err.mean()) <= 4e-3 * scale, (float(err.max()) / scale, float(err.mean()) / scale)


@pytest.fixture(scope="module")
def vae_and_params():
    from eeg_image_decode_amd.vae import SDXLShapedVAE
    vae = SDXLShapedVAE(seed=3).cuda()
    return vae, {k: v.detach().float().cpu() for k, v in vae.state_dict().items()}


def test_decode_18x13_latents(vae_and_params):
    """T = 234 positions: a partial last key tile and a partial last query tile for both images"""
    from oracle import sdxl_vae as ovae
    vae, P = vae_and_params
    z = torch.randn(2, 4, 18, 13, generator=torch.Generator().manual_seed(4))
    img = vae.decode(z.cuda().bfloat16()).float().cpu()
    assert img.shape == (2, 3, 144, 104)
    _budget(img, ovae.decode(P, z.bfloat16().float()))
    assert torch.equal(img, vae.decode(z.cuda().bfloat16()).float().cpu())           # bit-identical, on recycled frames


def test_encode_144x104_image(vae_and_params):
    from oracle import sdxl_vae as ovae
    vae, P = vae_and_params
    x = torch.randn(2, 3, 144, 104, generator=torch.Generator().manual_seed(5))
    mom = vae.encode_moments(x.cuda().bfloat16())
    assert mom.shape == (2, 18, 13, 8)
    got = mom.float().cpu()
    _budget(got.permute(0, 3, 1, 2), ovae.encode_moments(P, x.bfloat16().float()))
    assert torch.equal(got, vae.encode_moments(x.cuda().bfloat16()).float().cpu())


def test_decode_64x64_latents(vae_and_params):
    """T = 4096: parity at a larger latent (fp32 scores; the T x T matrix in the activation dtype is gone)"""
    from oracle import sdxl_vae as ovae
    vae, P = vae_and_params
    z = torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(6))
    img = vae.decode(z.cuda().bfloat16()).float().cpu()
    assert img.shape == (1, 3, 512, 512)
    _budget(img, ovae.decode(P, z.bfloat16().float()))


def test_decode_18x13_latents_fp16():
    from eeg_image_decode_amd.vae import SDXLShapedVAE
    from oracle import sdxl_vae as ovae
    vae = SDXLShapedVAE(seed=3, dtype=torch.float16).cuda()
    P = {k: v.detach().float().cpu() for k, v in vae.state_dict().items()}
    z = torch.randn(1, 4, 18, 13, generator=torch.Generator().manual_seed(7))
    img = vae.decode(z.cuda().half()).float().cpu()
    assert img.shape == (1, 3, 144, 104)
    _budget(img, ovae.decode(P, z.half().float()))
