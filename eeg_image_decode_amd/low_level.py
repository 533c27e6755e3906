"""The low-level branch's EEG -> VAE-latent encoder on HIP kernels: (B, 63, 250) EEG -> the (B, 4, 64, 64) SDXL-VAE latent that the pipeline's
`low_level_latent` (sdxl.StandInSDXLPipeline.prepare_latents_latent2img, Generator4Embeds) starts its img2img sampling from.

The reference's model is `encoder_low_level` (Generation/train_vae_latent_512_low_level_no_average.py:219-260).  Its source is not available
offline: the model is RESTATED here from SURVEY row 15 and knowledge of the upstream repository, as sdxl_unet.py restates diffusers' UNet2DConditionModel;
tests/low_level_ref.py is the same restatement in fp32 torch modules, and the state_dict keys and shapes below are the ones its training script saves:

    subject_wise_linear.{s}   nn.Linear(250, hidden) over TIME, one per subject: x (B, 63, 250) -> (B, 63, hidden)
    view(B, 63 * hidden, 1, 1)                             channel = EEG channel * hidden + j
    upsampler                 nn.Sequential of [ConvTranspose2d(c_i, c_{i+1}, 4, 2, 1), BatchNorm2d(c_{i+1}), ReLU] per layer and a bare ConvTranspose2d last
                              (indices 0, 1, 3, 4, 6, 7, ..; published widths 8064 -> 1024 -> 512 -> 256 -> 128 -> 64 -> 4: 1 x 1 -> 64 x 64)

Inference only (eval-mode BatchNorm): a trained state dict is an input, as it is for SDXL, CLIP and GIT; forward() in train() mode raises.  Launches per
forward at the published widths: one csrc/gemm16.hip GEMM (K = 250 padded to 256 in a cached weight copy and a staging buffer), five csrc/convt16.hip
matrix-core launches whose epilogue carries the folded BatchNorm and the ReLU, and the direct 64 -> 4 form that writes the NCHW latent.  The first layer
runs at 1 x 1 pixels: three of the four taps of every phase only ever meet the frame's zero border, and their 198 MB of fp16 weights are never read.
No library GEMM, no eager arithmetic on activations, no fallback; the nn children hold parameters only and are never called.
"""
import torch
import torch.nn as nn

from ._lib import EegclipError, require_cuda
from .ops16 import PackedWeights, conv_transpose16, dtype_code, linear, pack_conv_transpose16, seeded_parameters

_K_PAD = 64             # the GEMMs take K % 64 == 0: 250 time samples are padded to 256 with zero columns


class LowLevelEncoder(nn.Module):
    """`channels[0]` must be num_channels * hidden; every inner width a multiple of 64 (it is the next layer's K), the last
    width < 16 (the direct NCHW form).  The latent side is 2 ** (len(channels) - 1).  Weights get PyTorch's default initialisation under `seed`."""

    def __init__(self, num_channels=63, sequence_length=250, num_subjects=1, hidden=128, channels=(8064, 1024, 512, 256, 128, 64, 4), dtype=torch.float16,
                 device=None, seed=0, eps=1e-5):
        super().__init__()
        channels = tuple(int(c) for c in channels)
        if len(channels) < 2 or channels[0] != num_channels * hidden:
            raise EegclipError(f"LowLevelEncoder: channels[0] must be num_channels * hidden = {num_channels * hidden}; got {channels}")
        if any(c < 64 or c % 64 for c in channels[:-1]) or not 1 <= channels[-1] < 16 or 32 * channels[-1] * channels[-2] > 64 * 1024:
            raise EegclipError(f"LowLevelEncoder: every width but the last must be a multiple of 64 and the last below 16 with 16 * c[-2] * c[-1] weights "
                               f"within 64 KB (csrc/convt16.hip); got {channels}")
        if hidden % 64 or num_subjects < 1 or sequence_length < 1:
            raise EegclipError(f"LowLevelEncoder: hidden must be a multiple of 64 (got {hidden}), num_subjects and sequence_length positive")
        self.num_channels, self.sequence_length, self.hidden, self.channels = num_channels, sequence_length, hidden, channels
        layers = []
        with seeded_parameters(self, dtype, device, seed):
            self.subject_wise_linear = nn.ModuleList([nn.Linear(sequence_length, hidden) for _ in range(num_subjects)])
            for i in range(len(channels) - 2):
                layers += [nn.ConvTranspose2d(channels[i], channels[i + 1], 4, 2, 1), nn.BatchNorm2d(channels[i + 1], eps=eps), nn.ReLU()]
            layers.append(nn.ConvTranspose2d(channels[-2], channels[-1], 4, 2, 1))
            self.upsampler = nn.Sequential(*layers)
        self._cache = PackedWeights()
        self.eval()

    @property
    def dtype(self):
        return self.upsampler[0].weight.dtype

    @property
    def device(self):
        return self.upsampler[0].weight.device

    @property
    def latent_size(self):
        return 2 ** (len(self.channels) - 1)

    # ---- cached, repacked parameters: rebuilt when a parameter or a BatchNorm buffer changes (ops16.PackedWeights.key) -------------------------------------
    def _linear(self, s):
        lin = self.subject_wise_linear[s]
        kp = -(-self.sequence_length // _K_PAD) * _K_PAD

        def make():
            w = torch.zeros(self.hidden, kp, dtype=lin.weight.dtype, device=lin.weight.device)
            w[:, :self.sequence_length] = lin.weight.detach()
            return w, lin.bias.detach().contiguous()
        return self._cache.get(("linear", s), [lin.weight, lin.bias], make)

    def _layer(self, i):
        """(packed weight, scale or None, shift) of transposed convolution i: eval-mode BatchNorm folded with the bias into fp32 vectors, NOT into the 16-bit
        weights (that would change the rounding of every product)"""
        conv = self.upsampler[3 * i]
        bn = self.upsampler[3 * i + 1] if 3 * i + 1 < len(self.upsampler) else None
        ps = [conv.weight, conv.bias] + ([bn.weight, bn.bias, bn.running_mean, bn.running_var] if bn is not None else [])

        def make():
            b = conv.bias.detach().float()
            if bn is None:
                return pack_conv_transpose16(conv.weight), None, b.contiguous()
            scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
            shift = (b - bn.running_mean.detach().float()) * scale + bn.bias.detach().float()
            return pack_conv_transpose16(conv.weight), scale.contiguous(), shift.contiguous()
        return self._cache.get(("convt", i), ps, make)

    # ---- forward ------------------------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, x, subject_id=0):
        """x (B, num_channels, sequence_length) on the GPU, any floating dtype -> (B, channels[-1], S, S) in the module's dtype, S = latent_size"""
        if self.training:
            raise EegclipError("LowLevelEncoder runs in eval mode only (eval-mode BatchNorm; training the encoder is out of scope): call .eval()")
        require_cuda(x, "x")
        dtype_code(self.dtype)
        if x.dim() != 3 or tuple(x.shape[1:]) != (self.num_channels, self.sequence_length) or x.shape[0] < 1:
            raise EegclipError(f"LowLevelEncoder takes (B, {self.num_channels}, {self.sequence_length}); got {tuple(x.shape)}")
        if not 0 <= int(subject_id) < len(self.subject_wise_linear):
            raise EegclipError(f"LowLevelEncoder: subject_id {subject_id} outside [0, {len(self.subject_wise_linear)})")
        B = x.shape[0]
        w, b = self._linear(int(subject_id))
        stage = torch.zeros(B * self.num_channels, w.shape[1], dtype=self.dtype, device=x.device)
        stage[:, :self.sequence_length] = x.reshape(B * self.num_channels, self.sequence_length)            # the cast to 16 bit
        h = linear(stage, w, b)                                                                             # (B * 63, hidden)
        frame = torch.zeros(B, 3, 3, self.channels[0], dtype=self.dtype, device=x.device)                   # the 1 x 1 image inside its zero border
        frame[:, 1, 1] = h.view(B, self.channels[0])                                                        # channel = EEG channel * hidden + j
        n = len(self.channels) - 1
        for i in range(n):
            pw, scale, shift = self._layer(i)
            frame = conv_transpose16(frame, pw, scale, shift, relu=i < n - 1)
        return frame
