"""LowLevelTrainer on the MI355X against fp32 autograd on the restatement (tests/low_level_ref.py, tests/low_level_train_common.py, on the CPU): the small
configuration of tests/test_low_level_train_emu.py (hidden 64, channels (128, 64, 64, 4), B = 4) and hidden 128, channels (256, 128, 64, 64, 4) at B = 16 (a
16 x 16 latent; the wide convolution kernels and the split-K slabs of the weight gradient).

The allowance is 3 x the yardstick's deviation (the reference with 16-bit weights and layer boundaries), per tensor, relative L2.  The reference alone meets
"the loss ends below half its first value" with the learning rate used (2e-3; asserted below on its own curve).
Worst product / allowance on the MI355X (one step; printed per tensor with `pytest -s`): hidden 64 bf16 0.575, fp16 0.513; hidden 128 bf16 0.524, fp16 0.615; fp16 with
loss_scale 256 against bf16's allowance 0.254; the worst product / yardstick ratio of a single tensor is 1.84 of the 3 allowed; the one-step loss is at
0.14 / 0.26 (hidden 64, bf16 / fp16), 0.04 / below 0.1 (hidden 128) and 0.04 (fp16 x 256) of its allowance of 3 x |yardstick - reference|.  Thirty steps, bf16: 1.7220 -> 0.02483
(reference 0.02517, yardstick 0.02550: the margin 3 x |yardstick - reference| is 1.0e-3, the product is 3.4e-4 off); eval after training: relative L2 3.2e-3 against a format error of 3.1e-3."""
import pytest
import torch

from eeg_image_decode_amd import low_level, vae
from eeg_image_decode_amd._lib import EegclipError
from low_level_ref import EncoderLowLevelRef
from low_level_train_common import LR, STEPS, WD, check_one_step, references, rel_l2

pytestmark = pytest.mark.gpu
NC = 2
SMALL, LARGE = (64, (128, 64, 64, 4), 4), (128, (256, 128, 64, 64, 4), 16)


def make_trainer(ref0, hidden, channels, dtype, loss_scale=1.0):
    model = low_level.LowLevelEncoder(num_channels=NC, hidden=hidden, channels=channels, dtype=dtype, device="cuda", seed=1)
    model.load_state_dict(ref0.state_dict())
    return model, low_level.LowLevelTrainer(model, lr=LR, weight_decay=WD, loss_scale=loss_scale)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("hidden,channels,B", [SMALL, LARGE])
def test_one_step(hidden, channels, B, dtype):
    ref0, (x, t), (fp32, _), (yard, _) = references(NC, hidden, channels, B, dtype, STEPS if (hidden, dtype) == (64, torch.bfloat16) else 1)
    model, tr = make_trainer(ref0, hidden, channels, dtype)
    loss = tr.step(x.cuda(), t.cuda())
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    check_one_step(tr.grads(), tr.state_dict(), float(loss), fp32[0], yard[0], dtype, label=f"MI355X one step hidden {hidden} {dtype}")
    assert list(tr.state_dict()) == list(ref0.state_dict())
    model2, tr2 = make_trainer(ref0, hidden, channels, dtype)
    tr2.step(x.cuda(), t.cuda())
    assert all(torch.equal(a, b) for a, b in zip(tr.grads().values(), tr2.grads().values())), "two runs differ"


def test_loss_scale_is_divided_out_exactly():
    """fp16 with loss_scale 256 against the fp32 reference, within the allowance bf16 gets at loss_scale 1; and the same bits as fp16 at loss_scale 1 wherever
    no intermediate value leaves fp16's normal range (not asserted: only the allowance is)"""
    hidden, channels, B = SMALL
    ref0, (x, t), (fp32, _), (yard, _) = references(NC, hidden, channels, B, torch.bfloat16, STEPS)
    model, tr = make_trainer(ref0, hidden, channels, torch.float16, loss_scale=256.0)
    loss = tr.step(x.cuda(), t.cuda())
    check_one_step(tr.grads(), tr.state_dict(), float(loss), fp32[0], yard[0], torch.float16, label="MI355X fp16 x 256")


def test_thirty_steps_then_eval():
    hidden, channels, B = SMALL
    dtype = torch.bfloat16
    ref0, (x, t), (fp32, _), (yard, _) = references(NC, hidden, channels, B, dtype, STEPS)
    assert fp32[-1]["loss"] < 0.5 * fp32[0]["loss"]                                         # the reference itself learns at this rate
    model, tr = make_trainer(ref0, hidden, channels, dtype)
    xg, tg = x.cuda(), t.cuda()
    losses = [float(v) for v in [tr.step(xg, tg) for _ in range(STEPS)]]
    margin = 3 * abs(yard[-1]["loss"] - fp32[-1]["loss"])
    print(f"MI355X thirty steps {dtype}: product {losses[0]:.4f} -> {losses[-1]:.5f}, reference {fp32[-1]['loss']:.5f}, yardstick {yard[-1]['loss']:.5f}, margin {margin:.2e}")
    assert losses[-1] < 0.5 * losses[0]
    assert abs(losses[-1] - fp32[-1]["loss"]) <= margin
    tr.sync_model()
    model.eval()
    got = model(xg)
    model.train()
    with pytest.raises(EegclipError):
        model(xg)
    model.eval()
    ev = EncoderLowLevelRef(num_channels=NC, hidden=hidden, channels=channels)
    ev.load_state_dict({k: v.cpu() for k, v in tr.state_dict().items()})
    ev.eval()
    with torch.no_grad():
        want = ev(x)
        fmt = torch.func.functional_call(ev, {k: v.to(dtype).float() for k, v in ev.named_parameters()}, (x,), {"round_to": dtype})
    e_fmt, err = rel_l2(fmt, want), rel_l2(got.float().cpu(), want)
    print(f"MI355X eval after training {dtype}: relative L2 {err:.3e}, format error {e_fmt:.3e}, allowance {3 * e_fmt:.3e}")
    assert err < 3 * e_fmt


def test_train_low_level_with_vae():
    """the loop with image targets: vae.encode(image) * scaling_factor of a tiny SDXLShapedVAE, a 2-sample loader, two epochs -> two finite losses"""
    hidden, channels, _ = SMALL
    g = torch.Generator().manual_seed(4)
    eeg, img = torch.randn(2, NC, 250, generator=g), torch.rand(2, 3, 16, 16, generator=g) * 2 - 1
    v = vae.SDXLShapedVAE(block_out_channels=(64, 128), dtype=torch.bfloat16, seed=2).cuda()
    model = low_level.LowLevelEncoder(num_channels=NC, hidden=hidden, channels=channels, dtype=torch.bfloat16, device="cuda", seed=1)
    before = model.upsampler[0].weight.detach().clone()
    hist = low_level.train_low_level(model, [(eeg, img)], 2, lr=LR, vae=v)
    assert len(hist) == 2 and all(h == h and 0 < h < float("inf") for h in hist)
    assert not torch.equal(before, model.upsampler[0].weight) and int(model.upsampler[1].num_batches_tracked) == 2
    assert not model.training and tuple(model(eeg.cuda()).shape) == (2, 4, 8, 8)
