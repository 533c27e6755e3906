"""LowLevelTrainer's host code with its kernels under the lane emulator (tests/emu_patch.py) against fp32 autograd on the restatement (tests/low_level_ref.py,
tests/low_level_train_common.py): num_channels 2, hidden 64, channels (128, 64, 64, 4) -- an 8 x 8 latent -- at B = 4.

The allowance is 3 x the yardstick's deviation (the reference with 16-bit weights and layer boundaries), per tensor, relative L2.  The reference alone meets
"the loss ends below half its first value" with the learning rate used (2e-3: 1.72 -> 0.025 in thirty steps on the CPU, fp32).
Worst product / allowance on the emulator (one step; printed per tensor with `pytest -s`): bf16 0.575, fp16 0.486, fp16 with loss_scale 256 against bf16's allowance
0.254; the worst product / yardstick ratio of a single tensor is 1.72 (a running variance) of the 3 allowed; the one-step loss is at 0.14 (bf16), 0.33
(fp16) and 0.04 (fp16 x 256) of its allowance of 3 x |yardstick - reference|.  Thirty steps, bf16: 1.7220 -> 0.02483 (reference
0.02517, yardstick 0.02545: the margin 3 x |yardstick - reference| is 8.5e-4, the product is 3.4e-4 off); eval after training: relative L2 3.2e-3 against a format error of 3.1e-3."""
import pytest
import torch

from eeg_image_decode_amd import low_level, vae          # noqa: F401  (before product_on_emulator(): it patches the modules already loaded)
from eeg_image_decode_amd._lib import EegclipError
from emu_patch import product_on_emulator
from low_level_ref import EncoderLowLevelRef
from low_level_train_common import LR, STEPS, WD, check_one_step, references, rel_l2

pytestmark = pytest.mark.emu
NC, HID, CH, B = 2, 64, (128, 64, 64, 4), 4


def make_trainer(ref0, dtype, loss_scale=1.0):
    model = low_level.LowLevelEncoder(num_channels=NC, hidden=HID, channels=CH, dtype=dtype, seed=1)
    model.load_state_dict(ref0.state_dict())
    return model, low_level.LowLevelTrainer(model, lr=LR, weight_decay=WD, loss_scale=loss_scale)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_one_step(dtype):
    ref0, (x, t), (fp32, _), (yard, _) = references(NC, HID, CH, B, dtype, STEPS)
    with product_on_emulator():
        model, tr = make_trainer(ref0, dtype)
        loss = tr.step(x, t)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        check_one_step(tr.grads(), tr.state_dict(), float(loss), fp32[0], yard[0], dtype, label=f"emulator one step {dtype}")
        assert all(int(v) == 1 for k, v in tr.state_dict().items() if k.endswith("num_batches_tracked"))
        assert list(tr.state_dict()) == list(ref0.state_dict())


def test_loss_scale_is_divided_out_exactly():
    """fp16 with loss_scale 256 against the fp32 reference, within the allowance bf16 gets at loss_scale 1"""
    ref0, (x, t), (fp32, _), (yard, _) = references(NC, HID, CH, B, torch.bfloat16, STEPS)
    with product_on_emulator():
        model, tr = make_trainer(ref0, torch.float16, loss_scale=256.0)
        loss = tr.step(x, t)
        check_one_step(tr.grads(), tr.state_dict(), float(loss), fp32[0], yard[0], torch.float16, label="emulator fp16 x 256")
        with pytest.raises(EegclipError):
            low_level.LowLevelTrainer(model, loss_scale=3.0)


@pytest.mark.parametrize("dtype", [torch.bfloat16])
def test_thirty_steps_then_eval(dtype):
    ref0, (x, t), (fp32, ref_end), (yard, _) = references(NC, HID, CH, B, dtype, STEPS)
    assert fp32[-1]["loss"] < 0.5 * fp32[0]["loss"]                                         # the reference itself learns at this rate
    with product_on_emulator():
        model, tr = make_trainer(ref0, dtype)
        losses = [float(tr.step(x, t)) for _ in range(STEPS)]
        margin = 3 * abs(yard[-1]["loss"] - fp32[-1]["loss"])
        print(f"emulator thirty steps {dtype}: product {losses[0]:.4f} -> {losses[-1]:.5f}, reference {fp32[-1]['loss']:.5f}, yardstick {yard[-1]['loss']:.5f}, "
              f"margin {margin:.2e}")
        assert losses[-1] < 0.5 * losses[0]
        assert abs(losses[-1] - fp32[-1]["loss"]) <= margin
        # after training: the model, synchronised, in eval mode against the reference loaded with the trainer's state
        tr.sync_model()
        model.eval()
        got = model(x)
        model.train()
        with pytest.raises(EegclipError):
            model(x)
        model.eval()
    ev = EncoderLowLevelRef(num_channels=NC, hidden=HID, channels=CH)
    ev.load_state_dict(tr.state_dict())
    ev.eval()
    with torch.no_grad():
        want = ev(x)
        fmt = torch.func.functional_call(ev, {k: v.to(dtype).float() for k, v in ev.named_parameters()}, (x,), {"round_to": dtype})
    e_fmt, err = rel_l2(fmt, want), rel_l2(got.float(), want)
    print(f"emulator eval after training {dtype}: relative L2 {err:.3e}, format error {e_fmt:.3e}, allowance {3 * e_fmt:.3e}")
    assert err < 3 * e_fmt


def test_train_low_level_with_vae():
    """the loop with image targets: vae.encode(image) * scaling_factor of a tiny SDXLShapedVAE, a 2-sample loader, two epochs -> two finite losses; the model is
    left in sync with the trainer"""
    g = torch.Generator().manual_seed(4)
    eeg, img = torch.randn(2, NC, 250, generator=g), torch.rand(2, 3, 16, 16, generator=g) * 2 - 1
    with product_on_emulator():
        v = vae.SDXLShapedVAE(block_out_channels=(64, 128), dtype=torch.bfloat16, seed=2)
        model = low_level.LowLevelEncoder(num_channels=NC, hidden=HID, channels=CH, dtype=torch.bfloat16, seed=1)
        before = model.upsampler[0].weight.detach().clone()
        hist = low_level.train_low_level(model, [(eeg, img)], 2, lr=LR, vae=v)
        assert len(hist) == 2 and all(h == h and 0 < h < float("inf") for h in hist)
        assert not torch.equal(before, model.upsampler[0].weight) and int(model.upsampler[1].num_batches_tracked) == 2
        assert not model.training and tuple(model(eeg).shape) == (2, 4, 8, 8)
        with pytest.raises(EegclipError):
            low_level.train_low_level(model, [], 1)
