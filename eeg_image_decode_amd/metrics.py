"""The reference's reconstruction metrics that need no pretrained network (its metrics notebooks under Generation/, which copy MindEye's
Reconstruction_Metrics): PixCorr, SSIM and two-way identification, on images and features that stay on the GPU (csrc/recon_metrics.hip).

* pixcorr_ssim(images, recons)        both image metrics of every pair from one launch: PixCorr = np.corrcoef of the flattened (3, 425, 425) images, SSIM =
                                      skimage's structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=1.0) on rgb2gray;
* two_way_identification(real, recon) mean over j of #{ i != j : r[i, j] < r[j, j] } / (N - 1), r = np.corrcoef(real, recon)[:N, N:], for any feature matrices;
* clip_two_way(images, recons, tower) the same on the `image_embeds` of a CLIP tower of this package;
* alexnet_two_way(images, recons, net) the AlexNet(2) / AlexNet(5) rows: the same on `features.4` / `features.11` of a metric_nets.AlexNetFeatures;
* correlation_distance(real, recon)   scipy.spatial.distance.correlation of every pair of rows, the score of the notebooks' "distance" rows (EffNet-B, SwAV);
* swav_distance(images, recons, net)  the SwAV row: the mean of that on the `avgpool` node of a metric_nets.ResNetFeatures (swav_resnet50);
* effnet_distance(images, recons, net) the EffNet-B row: the same mean on the `avgpool` node of a metric_nets.EfficientNetFeatures (efficientnet_b1);
* inception_two_way(images, recons, net) the Inception row: two-way identification on the `avgpool` node of a metric_nets.InceptionFeatures (inception_v3);
* reconstruction_metrics(...)         the table: {"PixCorr", "SSIM"}, the two AlexNet rows, the SwAV row, the EffNet-B row and the Inception row when their nets
                                      are given, and one two-way entry per feature net handed in (the CLIP row is such an entry around a tower of this package).

AlexNet's, the SwAV ResNet-50's, EfficientNet-B1's and InceptionV3's architectures are carried (metric_nets.py, csrc/metric_nets.hip, csrc/mbconv.hip) with
seeded weights: load torchvision's state dicts / the SwAV checkpoint into them for the notebooks' rows.  With a CLIP tower as a feature net, all eight rows of
the notebooks' table come from this package.

One difference from the notebooks: they resize with torchvision's Resize(425, BILINEAR) on float tensors; here PIL images, uint8 arrays and float tensors of
another size go through preprocess.resize_crop_normalize(size, filter="bilinear"), PIL's 8-bit antialiased resize (what Resize does to a PIL image), so the
values can differ from the notebooks' in the last digits.  There is no CPU path: CPU tensors without the library raise as everywhere else.  `lib`,
`require_cuda` and `raw_stream` are called as this module's globals (tests/emu_patch.py swaps them).
"""
import torch

from . import _abi, preprocess
from ._lib import EegclipError, check, lib, raw_stream, require_cuda

_DT = {torch.float32: _abi.DT_F32, torch.float16: _abi.DT_F16, torch.bfloat16: _abi.DT_BF16}


def _is_batch(x):
    return isinstance(x, torch.Tensor) and x.is_floating_point() and x.dim() == 4 and x.shape[1] == 3


def _unit_batch(x, size, device, name):
    """-> (N, 3, H, W) float tensor in [0, 1] where the kernels run"""
    if size is None:
        if not _is_batch(x) or x.dtype not in _DT:
            raise EegclipError(f"size=None takes {name} as a float (N, 3, H, W) tensor in [0, 1] (fp32, fp16 or bf16); got "
                               + (f"{tuple(x.shape)} {x.dtype}" if isinstance(x, torch.Tensor) else type(x).__name__))
        return x
    if _is_batch(x) and x.dtype in _DT and preprocess.resized_size(x.shape[2], x.shape[3], size) == (x.shape[2], x.shape[3]):
        return x                                                      # already at `size`: taken as it is (no 8-bit round trip)
    kw = {"in_range": (0.0, 1.0)} if isinstance(x, torch.Tensor) and x.is_floating_point() else {}
    return preprocess.resize_crop_normalize(x, size, filter="bilinear", rescale=1 / 255, device=device, **kw)


def pixcorr_ssim(images, recons, size=425, device=None):
    """-> (pixcorr (N,), ssim (N,)) fp32 on the device, pair i = (images[i], recons[i]).

    images / recons: anything preprocess.resize_crop_normalize takes (PIL images, uint8 (H, W, 3) arrays / tensors or a list of them, a uint8 (N, H, W, 3)
    batch) or a float (N, 3, H, W) tensor in [0, 1].  size: the shortest side after the reference's Resize(425, BILINEAR) (an int, or (h, w)); a float tensor
    already of that size is taken as it is.  size=None: both are float (N, 3, H, W) tensors on the device and are compared as they are (H, W >= 11).
    A constant image gives PixCorr NaN, as numpy does."""
    if device is None:
        device = next((t.device for t in (images, recons) if isinstance(t, torch.Tensor) and t.device.type != "cpu"), "cuda")
    a, b = _unit_batch(images, size, device, "images"), _unit_batch(recons, size, device, "recons")
    if a.shape != b.shape:
        raise EegclipError(f"images and recons differ in shape after the resize: {tuple(a.shape)} and {tuple(b.shape)}")
    if a.dtype != b.dtype:
        a, b = a.float(), b.float()
    a, b = require_cuda(a, "images").contiguous(), require_cuda(b, "recons").contiguous()
    if b.device != a.device:
        raise EegclipError(f"images and recons live on different devices ({a.device}, {b.device})")
    N, _, H, W = a.shape
    if N < 1 or H < 11 or W < 11:
        raise EegclipError(f"SSIM's 11 x 11 window needs at least one pair of images of 11 x 11 or more; got {tuple(a.shape)}")
    L = lib()
    pix, ssm = torch.empty(N, dtype=torch.float32, device=a.device), torch.empty(N, dtype=torch.float32, device=a.device)
    for b0 in range(0, N, 32768):                                     # (the pair index is a grid dimension)
        nb = min(32768, N - b0)
        nbytes = L.eegclip_pixcorr_ssim_workspace_bytes(nb, H, W)
        if nbytes < 0:
            raise EegclipError(f"pixcorr_ssim does not take {nb} pairs of {H} x {W} (code {nbytes})")
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=a.device)
        check(L.eegclip_pixcorr_ssim(a[b0:b0 + nb].data_ptr(), b[b0:b0 + nb].data_ptr(), _DT[a.dtype], nb, H, W, ssm[b0:b0 + nb].data_ptr(),
                                     pix[b0:b0 + nb].data_ptr(), ws.data_ptr(), nbytes, raw_stream()), f"pixcorr_ssim ({nb} pairs of {H} x {W})")
    return pix, ssm


def pixcorr(images, recons, size=425, device=None):
    return pixcorr_ssim(images, recons, size, device)[0]


def ssim(images, recons, size=425, device=None):
    return pixcorr_ssim(images, recons, size, device)[1]


def two_way_identification(real_feats, recon_feats, return_counts=False):
    """the notebooks' two_way_identification on features already computed: r = np.corrcoef(real, recon)[:N, N:], count[j] = #{ i != j : r[i, j] < r[j, j] },
    score = mean(count) / (N - 1) as a float (1.0: every reconstruction is closest to its own image; chance is 0.5).  Trailing dimensions are flattened.
    return_counts=True: (score, count (N,) int32 on the device)."""
    if not isinstance(real_feats, torch.Tensor) or not isinstance(recon_feats, torch.Tensor):
        raise EegclipError("two_way_identification takes two feature tensors (N, ...)")
    if real_feats.shape != recon_feats.shape or real_feats.dim() < 2:
        raise EegclipError(f"real and reconstruction features are two (N, ...) tensors of one shape; got {tuple(real_feats.shape)} and {tuple(recon_feats.shape)}")
    g = require_cuda(real_feats, "real_feats").reshape(real_feats.shape[0], -1).float().contiguous()
    p = require_cuda(recon_feats, "recon_feats").reshape(recon_feats.shape[0], -1).float().contiguous()
    N, D = g.shape
    L = lib()
    nbytes = L.eegclip_two_way_workspace_bytes(N, D)
    if nbytes < 0:
        raise EegclipError(f"two-way identification needs N >= 2 samples (at most 32768) of D >= 2 features; got ({N}, {D})")
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=g.device)
    count = torch.empty(N, dtype=torch.int32, device=g.device)
    check(L.eegclip_two_way(g.data_ptr(), p.data_ptr(), N, D, count.data_ptr(), None, ws.data_ptr(), nbytes, raw_stream()), f"two_way ({N} x {D})")
    score = float(count.sum()) / (N * (N - 1))
    return (score, count) if return_counts else score


def clip_two_way(images, recons, tower, size=224, **kw):
    """two-way identification on the `image_embeds` of `tower` (a clip_vision.CLIPVisionEncoder with a projection), both sides through
    preprocess.clip_image_processor(size) -- the notebooks' CLIP row, with this package's tower in place of OpenAI's ViT-L/14"""
    feats = []
    for x in (images, recons):
        out = tower(preprocess.clip_image_processor(x, size=size, dtype=tower.dtype, device=tower.device))
        if out.image_embeds is None:
            raise EegclipError("clip_two_way needs a tower with a projection (image_embeds)")
        feats.append(out.image_embeds)
    return two_way_identification(feats[0], feats[1], **kw)


def _features(images, recons, net, pre, size):
    """net's output for both sides, each through the row's preprocess.*_preprocess `pre` at `size`, float tensors as values in [0, 1]"""
    feats = []
    for x in (images, recons):
        kw = {"in_range": (0.0, 1.0)} if isinstance(x, torch.Tensor) and x.is_floating_point() else {}
        feats.append(net(pre(x, size=size, dtype=net.dtype, device=net.device, **kw)))
    return feats


def alexnet_two_way(images, recons, net, size=256, return_counts=False):
    """the notebooks' AlexNet(2) and AlexNet(5) rows: {"AlexNet(2)": score, "AlexNet(5)": score}, two-way identification on `features.4` and `features.11` of
    `net` (a metric_nets.AlexNetFeatures; with torchvision's IMAGENET1K_V1 weights loaded, the notebooks' net).  Both sides go through
    preprocess.alexnet_preprocess(size) -- float tensors as values in [0, 1] -- and ONE forward each gives both nodes.  return_counts=True: each entry is
    (score, count (N,) int32 on the device)."""
    real, recon = _features(images, recons, net, preprocess.alexnet_preprocess, size)
    return {row: two_way_identification(real[node], recon[node], return_counts=return_counts)
            for row, node in (("AlexNet(2)", "features.4"), ("AlexNet(5)", "features.11"))}


def correlation_distance(real_feats, recon_feats):
    """scipy.spatial.distance.correlation(real[i], recon[i]) for every i: 1 - the Pearson correlation of the two rows -> (N,) fp32 on the device.  Trailing
    dimensions are flattened; D >= 2 features; a constant row gives NaN, as scipy does.  The notebooks' "distance" rows are np.mean of this."""
    if not isinstance(real_feats, torch.Tensor) or not isinstance(recon_feats, torch.Tensor):
        raise EegclipError("correlation_distance takes two feature tensors (N, ...)")
    if real_feats.shape != recon_feats.shape or real_feats.dim() < 2:
        raise EegclipError(f"real and reconstruction features are two (N, ...) tensors of one shape; got {tuple(real_feats.shape)} and {tuple(recon_feats.shape)}")
    g = require_cuda(real_feats, "real_feats").reshape(real_feats.shape[0], -1).float().contiguous()
    p = require_cuda(recon_feats, "recon_feats").reshape(recon_feats.shape[0], -1).float().contiguous()
    N, D = g.shape
    if N < 1 or D < 2 or p.device != g.device:
        raise EegclipError(f"correlation_distance needs N >= 1 pairs of D >= 2 features on one device; got ({N}, {D}) on {g.device} and {p.device}")
    out = torch.empty(N, dtype=torch.float32, device=g.device)
    check(lib().eegclip_corr_distance(g.data_ptr(), p.data_ptr(), N, D, out.data_ptr(), raw_stream()), f"corr_distance ({N} x {D})")
    return out


def _distance_row(images, recons, net, pre, size, return_distances):
    d = correlation_distance(*_features(images, recons, net, pre, size))
    mean = float(d.mean())
    return (mean, d) if return_distances else mean


def swav_distance(images, recons, net, size=224, return_distances=False):
    """the notebooks' SwAV row: the mean over the pairs of scipy's correlation distance between the `avgpool` features of `net` (a metric_nets.ResNetFeatures;
    swav_resnet50 with the SwAV checkpoint loaded is the notebooks' net) -- lower is better.  Both sides go through preprocess.swav_preprocess(size), float
    tensors as values in [0, 1].  return_distances=True: (mean, distances (N,) fp32 on the device)."""
    return _distance_row(images, recons, net, preprocess.swav_preprocess, size, return_distances)


def effnet_distance(images, recons, net, size=255, return_distances=False):
    """the notebooks' EffNet-B row: the mean over the pairs of scipy's correlation distance between the `avgpool` features of `net` (a
    metric_nets.EfficientNetFeatures; efficientnet_b1 with torchvision's weights loaded is the notebooks' net) -- lower is better.  Both sides go through
    preprocess.effnet_preprocess(size), float tensors as values in [0, 1].  return_distances=True: (mean, distances (N,) fp32 on the device)."""
    return _distance_row(images, recons, net, preprocess.effnet_preprocess, size, return_distances)


def inception_two_way(images, recons, net, size=342, return_counts=False):
    """the notebooks' Inception row: two-way identification on the `avgpool` features (N, 2048) of `net` (a metric_nets.InceptionFeatures; inception_v3 with
    torchvision's weights loaded is the notebooks' net).  Both sides go through preprocess.inception_preprocess(size), float tensors as values in [0, 1].
    return_counts=True: (score, count (N,) int32 on the device)."""
    return two_way_identification(*_features(images, recons, net, preprocess.inception_preprocess, size), return_counts=return_counts)


def reconstruction_metrics(images, recons, feature_nets=None, size=425, device=None, alexnet=None, swav=None, effnet=None, inception=None):
    """the notebooks' table for N pairs: {"PixCorr": mean, "SSIM": mean} plus, with alexnet= a metric_nets.AlexNetFeatures, "AlexNet(2)" and "AlexNet(5)"
    (alexnet_two_way at its default size 256) plus, with swav= a metric_nets.ResNetFeatures, "SwAV" (swav_distance at its default size 224) plus, with effnet= a
    metric_nets.EfficientNetFeatures, "EffNet-B" (effnet_distance at its default size 255) plus, with inception= a metric_nets.InceptionFeatures, "Inception"
    (inception_two_way at its default size 342) plus, per `name: callable` of feature_nets, name: the two-way identification score of callable(images) against
    callable(recons) (each an (N, ...) feature tensor on the device; e.g. the CLIP row: lambda x: tower(preprocess.clip_image_processor(x)).image_embeds)."""
    pix, ssm = pixcorr_ssim(images, recons, size, device)
    out = {"PixCorr": float(pix.mean()), "SSIM": float(ssm.mean())}
    if alexnet is not None:
        out.update(alexnet_two_way(images, recons, alexnet))
    if swav is not None:
        out["SwAV"] = swav_distance(images, recons, swav)
    if effnet is not None:
        out["EffNet-B"] = effnet_distance(images, recons, effnet)
    if inception is not None:
        out["Inception"] = inception_two_way(images, recons, inception)
    for name, net in (feature_nets or {}).items():
        if name in out:
            raise EegclipError(f"feature net name {name!r} is taken by another row of the table")
        out[name] = two_way_identification(net(images), net(recons))
    return out
