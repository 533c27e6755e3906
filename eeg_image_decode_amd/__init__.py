"""eeg_image_decode_amd -- MI355X-native (gfx950) hot path of dongyangli-del/EEG_Image_decode.

Public surface mirrors the reference's Python API for the contrastive-training / diffusion-prior
path.  All arithmetic runs in hand-written HIP kernels reached through the
C-ABI in include/eegclip.h; there is NO CPU fallback: importing the compute modules on a machine
without the built library (or calling them without a GPU) raises.
"""
__version__ = "0.1.0"

# the caption decoder's and the low-level encoder's public names, resolved on first use: importing the package itself stays free of torch (build.py imports it before the library exists)
_LAZY = {"GITCaptioner": "git_caption", "WordPieceDecoder": "git_caption", "caption": "git_caption", "LowLevelEncoder": "low_level", "LowLevelTrainer": "low_level",
         "train_low_level": "low_level", "pixcorr_ssim": "metrics", "pixcorr": "metrics", "ssim": "metrics", "two_way_identification": "metrics",
         "clip_two_way": "metrics", "reconstruction_metrics": "metrics", "alexnet_two_way": "metrics", "AlexNetFeatures": "metric_nets",
         "alexnet_preprocess": "preprocess", "ResNetFeatures": "metric_nets", "swav_resnet50": "metric_nets", "swav_preprocess": "preprocess",
         "correlation_distance": "metrics", "swav_distance": "metrics", "EfficientNetFeatures": "metric_nets", "efficientnet_b1": "metric_nets",
         "effnet_preprocess": "preprocess", "effnet_distance": "metrics", "InceptionFeatures": "metric_nets", "inception_v3": "metric_nets",
         "inception_preprocess": "preprocess", "inception_two_way": "metrics"}
__all__ = sorted(_LAZY)


def __getattr__(name):
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
