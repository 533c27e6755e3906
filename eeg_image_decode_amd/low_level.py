"""The low-level branch's EEG -> VAE-latent encoder on HIP kernels: (B, 63, 250) EEG -> the (B, 4, 64, 64) SDXL-VAE latent that the pipeline's
`low_level_latent` (sdxl.StandInSDXLPipeline.prepare_latents_latent2img, Generator4Embeds) starts its img2img sampling from.

The reference's model is `encoder_low_level` (Generation/train_vae_latent_512_low_level_no_average.py:219-260).  Its source is not available
offline: the model is RESTATED here from SURVEY row 15 and knowledge of the upstream repository, as sdxl_unet.py restates diffusers' UNet2DConditionModel;
tests/low_level_ref.py is the same restatement in fp32 torch modules, and the state_dict keys and shapes below are the ones its training script saves:

    subject_wise_linear.{s}   nn.Linear(250, hidden) over TIME, one per subject: x (B, 63, 250) -> (B, 63, hidden)
    view(B, 63 * hidden, 1, 1)                             channel = EEG channel * hidden + j
    upsampler                 nn.Sequential of [ConvTranspose2d(c_i, c_{i+1}, 4, 2, 1), BatchNorm2d(c_{i+1}), ReLU] per layer and a bare ConvTranspose2d last
                              (indices 0, 1, 3, 4, 6, 7, ..; published widths 8064 -> 1024 -> 512 -> 256 -> 128 -> 64 -> 4: 1 x 1 -> 64 x 64)

LowLevelEncoder itself is the inference path (eval-mode BatchNorm; forward() in train() mode raises).  The reference publishes no checkpoint of this model:
it trains it per data set as an MSE regression onto VAE latents of the stimulus images, and LowLevelTrainer / train_low_level below do that here (fp32 master
weights, 16-bit frames, csrc/convt16_bwd.hip and csrc/bn2d16.hip for the backward of the transposed convolutions and train-mode BatchNorm).  Launches per
forward at the published widths: one csrc/gemm16.hip GEMM (K = 250 padded to 256 in a cached weight copy and a staging buffer), five csrc/convt16.hip
matrix-core launches whose epilogue carries the folded BatchNorm and the ReLU, and the direct 64 -> 4 form that writes the NCHW latent.  The first layer
runs at 1 x 1 pixels: three of the four taps of every phase only ever meet the frame's zero border, and their 198 MB of fp16 weights are never read.
No library GEMM, no eager arithmetic on activations, no fallback; the nn children hold parameters only and are never called.
"""
import collections
import ctypes
import math

import torch
import torch.nn as nn

from . import _abi
from ._lib import EegclipError, check, lib, raw_stream, require_cuda
from .optim import AdamW
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


# ---------------------------------------------------------------------------------------------------------------------------------------- training
def _bwd_live_taps(Hi, Wi):
    """eegclip_convt16_bwd_data's tap_mask (bit 4 ky + kx) without the taps that only meet the zero border of dz: ky in {0, 3} when Hi == 1, kx likewise"""
    return sum(1 << (4 * ky + kx) for ky in range(4) for kx in range(4) if not (ky in (0, 3) and Hi == 1) and not (kx in (0, 3) and Wi == 1))


class LowLevelTrainer:
    """Trains a LowLevelEncoder as the reference's script does (Generation/train_vae_latent_512_low_level_no_average.py: MSE onto VAE latents, AdamW), on HIP
    kernels end to end.  Holds fp32 MASTER copies of every parameter under the reference's state_dict keys (views of one flat buffer, with one flat gradient
    buffer beside it) and optim.AdamW over them; activations and activation gradients are padded NHWC frames in the model's 16-bit dtype.

    loss_scale is a power of two: it multiplies the loss gradient and is divided out, in fp32, where the parameter gradients leave the kernels (exactly: a
    power of two).  bf16 with loss_scale = 1 is the default and needs no scaling; fp16 wants a scale that keeps the small activation gradients above its
    subnormals.  The scale is STATIC: dynamic scaling and skipping steps on overflow are out of scope.

    step() per layer: eegclip_convt16_pack_train (fp32 master -> both 16-bit packings, one launch), eegclip_convt16 (bias in the epilogue), eegclip_bn2d16_fwd;
    then the MSE kernel on fp32, and back: eegclip_bn2d16_bwd, eegclip_convt16_bwd_weight, eegclip_convt16_bwd_data per layer, the Linear's weight and bias
    gradient as ONE fp32 GEMM (the staged input carries a column of ones) and one AdamW launch per contiguous run.  No host synchronisation, no library GEMM;
    eager torch only casts and copies (the EEG into its staging buffer, the selected subject's Linear weight and bias into their persistent 16-bit copies, the
    fp32 view of the 16-bit latent and of the Linear's output gradient)."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, loss_scale=1.0, momentum=0.1):
        if not isinstance(model, LowLevelEncoder):
            raise EegclipError("LowLevelTrainer trains a low_level.LowLevelEncoder")
        ls = float(loss_scale)
        if not ls > 0 or 2.0 ** round(math.log2(ls)) != ls:
            raise EegclipError(f"LowLevelTrainer: loss_scale must be a power of two; got {loss_scale}")
        if not 0.0 <= float(momentum) <= 1.0:
            raise EegclipError(f"LowLevelTrainer: momentum must be in [0, 1]; got {momentum}")
        self.model, self.loss_scale, self.momentum = model, ls, float(momentum)
        self.dtype, dev = model.dtype, model.device
        dtype_code(self.dtype)
        m = model
        self.n_conv = len(m.channels) - 1
        shapes = collections.OrderedDict()
        for s_, lin in enumerate(m.subject_wise_linear):
            shapes[f"subject_wise_linear.{s_}.weight"] = lin.weight
            shapes[f"subject_wise_linear.{s_}.bias"] = lin.bias
        for i in range(self.n_conv):
            shapes[f"upsampler.{3 * i}.weight"] = m.upsampler[3 * i].weight
            shapes[f"upsampler.{3 * i}.bias"] = m.upsampler[3 * i].bias
            if i < self.n_conv - 1:
                shapes[f"upsampler.{3 * i + 1}.weight"] = m.upsampler[3 * i + 1].weight
                shapes[f"upsampler.{3 * i + 1}.bias"] = m.upsampler[3 * i + 1].bias
        offs, total = {}, 0
        for k, p in shapes.items():                                          # every tensor 16-byte aligned in both flat buffers
            offs[k] = total
            total += -(-p.numel() // 4) * 4
        self._flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self._flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.params, self._grads = collections.OrderedDict(), collections.OrderedDict()
        for k, p in shapes.items():
            self.params[k] = self._flat[offs[k]:offs[k] + p.numel()].view(p.shape)
            self._grads[k] = self._flat_grad[offs[k]:offs[k] + p.numel()].view(p.shape)
            self.params[k].copy_(p.detach())
        self.buffers = collections.OrderedDict()
        for i in range(self.n_conv - 1):
            bn = m.upsampler[3 * i + 1]
            self.buffers[f"upsampler.{3 * i + 1}.running_mean"] = bn.running_mean.detach().float().clone()
            self.buffers[f"upsampler.{3 * i + 1}.running_var"] = bn.running_var.detach().float().clone()
        self.num_batches_tracked = [int(m.upsampler[3 * i + 1].num_batches_tracked) for i in range(self.n_conv - 1)]
        self.optimizer = AdamW(list(self.params.values()), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        ch = m.channels
        self._wf = [torch.empty(4, ch[i + 1], 4, ch[i], dtype=self.dtype, device=dev) for i in range(self.n_conv)]
        self._wb = [torch.empty(ch[i], 16, ch[i + 1], dtype=self.dtype, device=dev) for i in range(self.n_conv)]
        self._kp = -(-(m.sequence_length + 1) // _K_PAD) * _K_PAD            # the time samples, a column of ones (the bias gradient), zeros
        self._lin_w16 = torch.zeros(m.hidden, self._kp, dtype=self.dtype, device=dev)      # the selected subject's Linear in 16 bit, K padded with zero columns
        self._lin_b16 = torch.zeros(m.hidden, dtype=self.dtype, device=dev)
        self._work = {}
        self._stepped_subject = None

    # ---- buffers of one batch size ------------------------------------------------------------------------------------------------------------------------
    def _buffers(self, B):
        w = self._work.get(B)
        if w is not None:
            return w
        m, dev, dt = self.model, self.model.device, self.dtype
        ch, n = m.channels, self.n_conv
        L = lib()
        w = {"stage": torch.zeros(B * m.num_channels, self._kp, dtype=dt, device=dev), "stage32": torch.zeros(B * m.num_channels, self._kp, dtype=torch.float32, device=dev),
             "lin_grad": torch.empty(m.hidden, self._kp, dtype=torch.float32, device=dev), "loss": torch.zeros((), dtype=torch.float32, device=dev),
             "dpred": torch.empty(B, ch[-1], m.latent_size, m.latent_size, dtype=torch.float32, device=dev)}
        w["stage"][:, m.sequence_length] = 1.0
        w["stage32"][:, m.sequence_length] = 1.0
        frame = lambda i: torch.zeros(B, 2 ** i + 2, 2 ** i + 2, ch[i], dtype=dt, device=dev)      # noqa: E731
        w["a"] = [frame(i) for i in range(n)]                                # a[i]: the input of convolution i (a[0]: the Linear's output at 1 x 1)
        w["da"] = [frame(i) for i in range(n)]
        w["z"] = [frame(i + 1) for i in range(n - 1)]                        # the raw output of convolution i < n - 1
        w["dz"] = [frame(i + 1) for i in range(n - 1)]
        w["mean"] = [torch.empty(ch[i + 1], dtype=torch.float32, device=dev) for i in range(n - 1)]
        w["rstd"] = [torch.empty(ch[i + 1], dtype=torch.float32, device=dev) for i in range(n - 1)]
        w["slabs"] = [int(L.eegclip_convt16_bwd_weight_slabs(B, 2 ** i, 2 ** i, ch[i], ch[i + 1])) for i in range(n)]
        if min(w["slabs"]) < 1:
            raise EegclipError(f"LowLevelTrainer: csrc/convt16_bwd.hip does not take the widths {ch} (inner widths must be multiples of 64)")
        nws = max([int(L.eegclip_convt16_bwd_weight_workspace_floats(B, 2 ** i, 2 ** i, ch[i], ch[i + 1], w["slabs"][i])) for i in range(n)] +
                  [int(L.eegclip_bn2d16_workspace_floats(B, 2 ** (i + 1), 2 ** (i + 1), ch[i + 1])) for i in range(n - 1)])
        w["ws"], w["nws"] = torch.empty(nws, dtype=torch.float32, device=dev), nws
        self._work[B] = w
        return w

    # ---- one training step --------------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, eeg, target_latent, subject_id=0):
        """eeg (B, num_channels, sequence_length), target_latent (B, channels[-1], S, S), both on the GPU -> the batch's MSE loss before the update, a 0-dim
        fp32 tensor on the GPU.  B * S * S / 4 >= 2 values per channel are needed by the first BatchNorm (B >= 1 suffices: its image is 2 x 2)."""
        m, n, ch = self.model, self.n_conv, self.model.channels
        require_cuda(eeg, "eeg")
        require_cuda(target_latent, "target_latent")
        S = m.latent_size
        if eeg.dim() != 3 or tuple(eeg.shape[1:]) != (m.num_channels, m.sequence_length) or eeg.shape[0] < 1:
            raise EegclipError(f"LowLevelTrainer.step takes eeg (B, {m.num_channels}, {m.sequence_length}); got {tuple(eeg.shape)}")
        B = eeg.shape[0]
        if tuple(target_latent.shape) != (B, ch[-1], S, S):
            raise EegclipError(f"LowLevelTrainer.step takes target_latent ({B}, {ch[-1]}, {S}, {S}); got {tuple(target_latent.shape)}")
        s_ = int(subject_id)
        if not 0 <= s_ < len(m.subject_wise_linear):
            raise EegclipError(f"LowLevelTrainer: subject_id {subject_id} outside [0, {len(m.subject_wise_linear)})")
        w, L, stream, dtc, T = self._buffers(B), lib(), raw_stream(), dtype_code(self.dtype), m.sequence_length
        P, G = self.params, self._grads
        # 1. the 16-bit packings of this step's weights
        for i in range(n):
            check(L.eegclip_convt16_pack_train(P[f"upsampler.{3 * i}.weight"].data_ptr(), self._wf[i].data_ptr(), self._wb[i].data_ptr(), ch[i], ch[i + 1], dtc, stream),
                  "convt16_pack_train")
        # 2. the Linear over time (K padded; column T of the staged input is 1 and meets a zero weight column)
        w["stage"][:, :T] = eeg.reshape(B * m.num_channels, T)                # the cast to 16 bit
        self._lin_w16[:, :T] = P[f"subject_wise_linear.{s_}.weight"]           # the casts of this step's Linear weight and bias (columns >= T stay zero)
        self._lin_b16.copy_(P[f"subject_wise_linear.{s_}.bias"])
        h = linear(w["stage"], self._lin_w16, self._lin_b16)
        w["a"][0][:, 1, 1] = h.view(B, ch[0])
        # 3. / 4. the upsampler: raw convolution (+ bias), train-mode BatchNorm + ReLU into the next frame; the last layer writes the NCHW latent
        pred = None
        for i in range(n):
            bias = P[f"upsampler.{3 * i}.bias"]
            if i == n - 1:
                pred = conv_transpose16(w["a"][i], self._wf[i], None, bias, relu=False)
                break
            conv_transpose16(w["a"][i], self._wf[i], None, bias, relu=False, out=w["z"][i])
            side = 2 ** (i + 1)
            d = _abi.Bn2d16FwdDesc(z=w["z"][i].data_ptr(), a=w["a"][i + 1].data_ptr(), gamma=P[f"upsampler.{3 * i + 1}.weight"].data_ptr(),
                                   beta=P[f"upsampler.{3 * i + 1}.bias"].data_ptr(), mean=w["mean"][i].data_ptr(), rstd=w["rstd"][i].data_ptr(),
                                   running_mean=self.buffers[f"upsampler.{3 * i + 1}.running_mean"].data_ptr(),
                                   running_var=self.buffers[f"upsampler.{3 * i + 1}.running_var"].data_ptr(), workspace=w["ws"].data_ptr(), workspace_floats=w["nws"], N=B, H=side, W=side,
                                   C=ch[i + 1], eps=m.upsampler[3 * i + 1].eps, momentum=self.momentum, dtype=dtc)
            check(L.eegclip_bn2d16_fwd(ctypes.byref(d), stream), "bn2d16_fwd")
            self.num_batches_tracked[i] += 1
        # 5. the loss and its (scaled) gradient, fp32
        pred32, tgt = pred.float(), target_latent.float().contiguous()
        w["loss"].zero_()
        check(L.eegclip_mse_loss_grad_scaled(pred32.data_ptr(), tgt.data_ptr(), pred32.numel(), self.loss_scale, w["loss"].data_ptr(), w["dpred"].data_ptr(), stream),
              "mse_loss_grad_scaled")
        loss = w["loss"] * (1.0 / self.loss_scale)
        # 6. backward through the upsampler
        for i in range(n - 1, -1, -1):
            side = 2 ** i
            if i < n - 1:
                d = _abi.Bn2d16BwdDesc(da=w["da"][i + 1].data_ptr(), a=w["a"][i + 1].data_ptr(), z=w["z"][i].data_ptr(), gamma=P[f"upsampler.{3 * i + 1}.weight"].data_ptr(),
                                       mean=w["mean"][i].data_ptr(), rstd=w["rstd"][i].data_ptr(), dgamma=G[f"upsampler.{3 * i + 1}.weight"].data_ptr(),
                                       dbeta=G[f"upsampler.{3 * i + 1}.bias"].data_ptr(), dz=w["dz"][i].data_ptr(), workspace=w["ws"].data_ptr(), workspace_floats=w["nws"], N=B, H=2 * side,
                                       W=2 * side, C=ch[i + 1], loss_scale=self.loss_scale, dtype=dtc)
                check(L.eegclip_bn2d16_bwd(ctypes.byref(d), stream), "bn2d16_bwd")
            dz = w["dz"][i] if i < n - 1 else w["dpred"]
            d = _abi.Convt16BwdWeightDesc(x=w["a"][i].data_ptr(), dz=dz.data_ptr(), dW=G[f"upsampler.{3 * i}.weight"].data_ptr(), db=G[f"upsampler.{3 * i}.bias"].data_ptr(),
                                          workspace=w["ws"].data_ptr(), workspace_floats=w["nws"], N=B, Hi=side, Wi=side, Cin=ch[i], Cout=ch[i + 1], slabs=w["slabs"][i],
                                          loss_scale=self.loss_scale, dtype=dtc)
            check(L.eegclip_convt16_bwd_weight(ctypes.byref(d), stream), "convt16_bwd_weight")
            d = _abi.Convt16BwdDataDesc(dz=dz.data_ptr(), W=self._wb[i].data_ptr(), dx=w["da"][i].data_ptr(), N=B, Hi=side, Wi=side, Cin=ch[i], Cout=ch[i + 1],
                                        tap_mask=_bwd_live_taps(side, side), dtype=dtc)
            check(L.eegclip_convt16_bwd_data(ctypes.byref(d), stream), "convt16_bwd_data")
        # 7. the selected subject's Linear: [dW | db] = dh^T [x | 1] / loss_scale, one fp32 GEMM (exact products, one K pass: a fixed summation order)
        dh = w["da"][0][:, 1, 1].float().view(B * m.num_channels, m.hidden)
        w["stage32"][:, :T] = w["stage"][:, :T]                               # the ROUNDED input the forward multiplied
        D = _abi.dim
        g = _abi.GemmDesc(M=m.hidden, N=self._kp, K=B * m.num_channels, A=dh.data_ptr(), Am=D(1), Ak=D(m.hidden), B=w["stage32"].data_ptr(), Bk=D(self._kp), Bn=D(1),
                          C=w["lin_grad"].data_ptr(), Cm=D(self._kp), Cn=D(1), Cpre=None, bias_n=None, bias_m=None, R=None, Rm=D(0), Rn=D(0), alpha=1.0 / self.loss_scale,
                          accumulate=0, act=0, drop_p=0.0, seed=0, drop_site=0, split_k=1, precision=_abi.PREC_F32)
        check(L.eegclip_gemm_f32(ctypes.byref(g), stream), "gemm_f32 (Linear weight gradient)")
        G[f"subject_wise_linear.{s_}.weight"].copy_(w["lin_grad"][:, :T])
        G[f"subject_wise_linear.{s_}.bias"].copy_(w["lin_grad"][:, T])
        # 8. AdamW over every parameter that has a gradient: the other subjects' Linears are left alone, as torch leaves parameters without .grad
        for k, p in P.items():
            other = k.startswith("subject_wise_linear.") and int(k.split(".")[1]) != s_
            p.grad = None if other else G[k]
        self.optimizer.step()
        self._stepped_subject = s_
        return loss

    # ---- what a caller reads ------------------------------------------------------------------------------------------------------------------------------
    def grads(self):
        """the parameter gradients of the last step() by state_dict key, fp32, loss scale already divided out (the other subjects' Linears have none)"""
        if self._stepped_subject is None:
            raise EegclipError("LowLevelTrainer.grads(): no step() has run")
        return collections.OrderedDict((k, g.clone()) for k, g in self._grads.items()
                                       if not k.startswith("subject_wise_linear.") or int(k.split(".")[1]) == self._stepped_subject)

    def state_dict(self):
        """fp32 masters, BatchNorm running statistics and num_batches_tracked under the reference's keys, in nn.Module order"""
        out = collections.OrderedDict()
        for k, p in self.params.items():
            out[k] = p.detach().clone()
            parts = k.split(".")
            if parts[0] == "upsampler" and parts[2] == "bias" and f"upsampler.{parts[1]}.running_mean" in self.buffers:
                i = (int(parts[1]) - 1) // 3
                out[f"upsampler.{parts[1]}.running_mean"] = self.buffers[f"upsampler.{parts[1]}.running_mean"].clone()
                out[f"upsampler.{parts[1]}.running_var"] = self.buffers[f"upsampler.{parts[1]}.running_var"].clone()
                out[f"upsampler.{parts[1]}.num_batches_tracked"] = torch.tensor(self.num_batches_tracked[i], dtype=torch.long)
        return out

    @torch.no_grad()
    def sync_model(self):
        """write the parameters and BatchNorm buffers, rounded to the model's dtype, into `model`: model.eval()(x) then uses the trained values (the in-place
        copies move the tensors' versions, so the model's packed-weight cache rebuilds)"""
        own = dict(self.model.named_parameters())
        own.update(dict(self.model.named_buffers()))
        for k, v in self.state_dict().items():
            own[k].copy_(v)
        return self.model


def train_low_level(model, loader, epochs, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, vae=None, subject_id=0, loss_scale=1.0, momentum=0.1,
                    image_size=None):
    """The reference's training loop (Generation/train_vae_latent_512_low_level_no_average.py) on one GPU: `loader` yields (eeg, latent) batches, or with
    `vae` (a vae.SDXLShapedVAE) (eeg, image) batches whose target is vae.encode(image) * vae.scaling_factor, taken without a gradient; with image_size as well, image
    batches that are not float tensors (uint8 (B, H, W, 3) arrays / tensors, lists of PIL images) go through preprocess.vae_preprocess(size=image_size) first:
    the script's Resize((512, 512)) + ToTensor, to the VAE's (-1, 1), in the model's dtype.  Returns the mean loss
    of every epoch; the trained values are written into `model` (LowLevelTrainer.sync_model) before it returns.  Data-parallel training is out of scope."""
    tr = LowLevelTrainer(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, loss_scale=loss_scale, momentum=momentum)
    dev = model.device
    history = []
    for _ in range(int(epochs)):
        losses = []
        for eeg, target in loader:
            if vae is not None and image_size is not None and not (isinstance(target, torch.Tensor) and target.is_floating_point()):
                from .preprocess import vae_preprocess
                target = vae_preprocess(target, size=int(image_size), dtype=vae.dtype, device=dev)
            eeg, target = eeg.to(dev), target.to(dev)
            if vae is not None:
                with torch.no_grad():
                    target = vae.encode(target) * vae.scaling_factor
            losses.append(tr.step(eeg, target, subject_id))
        if not losses:
            raise EegclipError("train_low_level: the loader yielded no batch")
        history.append(float(torch.stack(losses).mean()))               # the epoch's one host synchronisation
    tr.sync_model()
    return history
