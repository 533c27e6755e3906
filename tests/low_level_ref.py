"""fp32 torch restatement of the reference's low-level EEG -> VAE-latent encoder (`encoder_low_level`,
Generation/train_vae_latent_512_low_level_no_average.py:219-260), built from nn.Linear / nn.ConvTranspose2d / nn.BatchNorm2d / nn.ReLU in an
nn.Sequential: the reference of tests/test_low_level_*.py.  The reference's source is not available offline; this states the model as SURVEY row 15 and the
upstream repository describe it (per-subject Linear over time, view to (B, 63 * hidden, 1, 1), ConvTranspose2d(4, 2, 1) + BatchNorm2d + ReLU per layer, a bare
ConvTranspose2d last)."""
import torch
import torch.nn as nn


class EncoderLowLevelRef(nn.Module):
    def __init__(self, num_channels=63, sequence_length=250, num_subjects=1, hidden=128, channels=(8064, 1024, 512, 256, 128, 64, 4)):
        super().__init__()
        assert channels[0] == num_channels * hidden
        self.subject_wise_linear = nn.ModuleList([nn.Linear(sequence_length, hidden) for _ in range(num_subjects)])
        layers = []
        for i in range(len(channels) - 2):
            layers += [nn.ConvTranspose2d(channels[i], channels[i + 1], kernel_size=4, stride=2, padding=1), nn.BatchNorm2d(channels[i + 1]), nn.ReLU()]
        layers.append(nn.ConvTranspose2d(channels[-2], channels[-1], kernel_size=4, stride=2, padding=1))
        self.upsampler = nn.Sequential(*layers)

    def forward(self, x, subject_id=0, round_to=None):
        """round_to: a 16-bit dtype -> the activations are rounded to it at every layer boundary (the input, the Linear's output, each ReLU's output and the
        result): the format's own error, the yardstick of the GPU test's allowance"""
        r = (lambda t: t.to(round_to).float()) if round_to is not None else (lambda t: t)
        h = r(self.subject_wise_linear[subject_id](r(x)))
        h = h.reshape(h.shape[0], -1, 1, 1)
        for m in self.upsampler:
            h = m(h)
            if isinstance(m, nn.ReLU):
                h = r(h)
        return r(h)


def calibrated(hidden, channels, dtype, seed=0, batch=8):
    """a restatement whose BatchNorm running statistics are those of one train-mode forward on a fixed batch (momentum 1: exactly that batch's), in eval mode,
    with every floating parameter and buffer rounded to `dtype` -- the values the product module holds after load_state_dict.  Every layer's activations are
    then O(1) and about half the ReLUs are live."""
    g = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        ref = EncoderLowLevelRef(hidden=hidden, channels=channels)
    for m in ref.upsampler:
        if isinstance(m, nn.BatchNorm2d):
            m.momentum = 1.0
            with torch.no_grad():                                   # an affine part that is not the identity
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
    ref.train()
    with torch.no_grad():
        ref(torch.randn(batch, 63, 250, generator=g))
    ref.eval()
    ref.to(dtype).float()
    return ref
