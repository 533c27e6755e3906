"""Image preprocessing (eeg_image_decode_amd/preprocess.py, csrc/image_resize.hip) on the GPU.  Prints one JSON object.

  kernel     eegclip_resize_crop_normalize at 500 x 500 -> 224 x 224, bicubic, uint8 in, fp32 out with CLIP's normalisation, B = 1 and B = 64: the kernel's own
             begin .. end (eegclip_time_next_launch: the timestamps of the launch itself) as the median of `--launches` stamped launches after a warm-up, per
             image; beside it the time its bytes (input + output, counted from the shapes) take at 8 TB/s and the ratio of the two; and the same call in
             event-bracketed windows of many launches (dispatch included).
  torch      the same job as torch.nn.functional.interpolate(uint8 NCHW, mode="bicubic", antialias=True) on the same GPU (a resize alone: no crop, no
             normalisation, and not PIL's pixels), in the same windows, alternating with the kernel.
  pil        Image.resize((224, 224), BICUBIC) + the normalisation in NumPy on one CPU core, per image.
  files      datasets.image_features_from_files on `--files` JPEGs of 500 x 500 the tool writes to a temporary directory with PIL, batches of 20, against the
             ViT-H/14 tower: images per second end to end, and the parts measured on their own over the same files: decode (the thread pool alone),
             upload + preprocess, tower.
  The condition: the kernel's time per image at B = 64 must be below the tower's (profiles/clip_vision_bench.json, ip_adapter_image_encoder B64), else
  preprocessing bounds the cache build; `kernel_over_tower_B64` is that ratio.

    python tools/bench_preprocess.py [--out profiles/preprocess_bench.json] [--windows 7] [--files 200]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_clip_vision import spread, update_json, window_us  # noqa: E402

HBM = 8e12
H = W = 500
S = 224
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tower_ms_per_image():
    try:
        with open(os.path.join(ROOT, "profiles", "clip_vision_bench.json")) as f:
            return float(json.load(f)["towers"]["ip_adapter_image_encoder"]["B64"]["hip"]["ms_per_image"])
    except (OSError, KeyError, ValueError):
        return None


def kernel_rows(windows, launches):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from eeg_image_decode_amd import preprocess as P
    from eeg_image_decode_amd._lib import lib
    L = lib()
    e0, e1 = L.eegclip_timing_event_create(), L.eegclip_timing_event_create()
    rows = {}
    for B in (1, 64):
        src = torch.from_numpy(np.random.default_rng(B).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
        nchw = src.permute(0, 3, 1, 2).contiguous()
        ours = lambda: P.open_clip_preprocess(src, size=S)
        theirs, torch_input = (lambda: F.interpolate(nchw, size=(S, S), mode="bicubic", antialias=True)), "uint8"
        try:
            theirs()
        except RuntimeError as e:                                              # (no uint8 antialias kernel in this torch build: its float path instead)
            torch_input = f"float32 (uint8 raised: {str(e).splitlines()[0][:120]})"
            nchw = nchw.float()
            theirs = lambda: F.interpolate(nchw, size=(S, S), mode="bicubic", antialias=True)
        for f in (ours, theirs):
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        stamped = []
        for _ in range(launches):
            L.eegclip_time_next_launch(e0, e1)
            ours()
            torch.cuda.synchronize()
            stamped.append(float(L.eegclip_timing_elapsed_ms(e0, e1)) * 1e3)
        n = max(20, 2000 // B)
        us = {"ours": [], "torch": []}
        for _ in range(windows):
            us["ours"].append(window_us(ours, n))
            us["torch"].append(window_us(theirs, n))
        bytes_moved = B * (H * W * 3 + 3 * S * S * 4)
        k_us = statistics.median(stamped)
        floor_us = bytes_moved / HBM * 1e6
        rows[f"B{B}"] = {"kernel_us": round(k_us, 2), "kernel_min_us": round(min(stamped), 2), "kernel_max_us": round(max(stamped), 2), "stamped_launches": launches,
                         "kernel_us_per_image": round(k_us / B, 3), "bytes_in_plus_out": bytes_moved, "us_at_8TBps": round(floor_us, 3),
                         "kernel_over_bytes_at_8TBps": round(k_us / floor_us, 1), "call_in_windows": dict(spread(us["ours"]), iterations_per_window=n),
                         "torch_interpolate_antialias": dict(spread(us["torch"]), iterations_per_window=n, input=torch_input),
                         "torch_over_ours_window": round(statistics.median(us["torch"]) / statistics.median(us["ours"]), 2)}
        del src, nchw
    L.eegclip_timing_event_destroy(e0)
    L.eegclip_timing_event_destroy(e1)
    return rows


def pil_row(n=20):
    import numpy as np
    from PIL import Image
    try:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})         # one core
    except (AttributeError, OSError):
        pass
    mean, std = np.asarray([0.48145466, 0.4578275, 0.40821073], np.float32), np.asarray([0.26862954, 0.26130258, 0.27577711], np.float32)
    ims = [Image.fromarray(np.random.default_rng(i).integers(0, 256, (H, W, 3), dtype=np.uint8)) for i in range(n)]
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        for im in ims:
            a = np.asarray(im.resize((S, S), Image.BICUBIC), np.float32)
            ((a / 255 - mean) / std).transpose(2, 0, 1).copy()
        t.append((time.perf_counter() - t0) / n * 1e3)
    return {"ms_per_image": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "images": n, "repeats": 3}


def files_row(n_files):
    import numpy as np
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from eeg_image_decode_amd import clip_vision, datasets
    from eeg_image_decode_amd import preprocess as P
    enc = clip_vision.ip_adapter_image_encoder(dtype=torch.float16, device="cuda")
    with tempfile.TemporaryDirectory() as d:
        paths = []
        rng = np.random.default_rng(7)
        base = rng.integers(0, 256, (H // 10, W // 10, 3), dtype=np.uint8)
        for i in range(n_files):
            a = np.asarray(Image.fromarray(np.roll(base, i, axis=1)).resize((W, H), Image.BICUBIC))       # smooth content: JPEGs of a photograph's size
            paths.append(os.path.join(d, f"{i:05d}.jpg"))
            Image.fromarray(a).save(paths[-1], quality=90)
        datasets.image_features_from_files(paths[:40], enc)                     # warm-up: kernels, tables, packed weights
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        feats = datasets.image_features_from_files(paths, enc)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=16) as pool:
            arrays = list(pool.map(datasets._decode, paths))
        decode = time.perf_counter() - t0
        t0 = time.perf_counter()
        px = [P.open_clip_preprocess(arrays[i:i + 20], size=S, device="cuda") for i in range(0, n_files, 20)]
        torch.cuda.synchronize()
        prep = time.perf_counter() - t0
        t0 = time.perf_counter()
        for p in px:
            datasets.image_features(p, enc, batch_size=20)
        torch.cuda.synchronize()
        tower = time.perf_counter() - t0
    return {"files": n_files, "jpeg": "500 x 500, quality 90", "batch_size": 20, "decode_threads": min(16, 20), "images_per_second": round(n_files / total, 1),
            "seconds": round(total, 3), "parts_on_their_own": {"decode_16_threads_s": round(decode, 3), "upload_plus_preprocess_s": round(prep, 3), "tower_s": round(tower, 3)},
            "feature_rows": list(feats.shape)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--files", type=int, default=200)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocess.py measures on the GPU; none found")
    with torch.no_grad():
        out = {"job": f"{H} x {W} -> {S} x {S}, bicubic, uint8 HWC in, fp32 NCHW out, CLIP mean / std",
               "timing": "kernel_us: the launch's own begin / end timestamps, median of stamped launches; windows: device events around many calls, median of the "
                         "windows, min / max = spread",
               "kernel": kernel_rows(a.windows, a.launches), "files": files_row(a.files)}
    out["pil_one_core"] = pil_row()
    tower = tower_ms_per_image()
    k64 = out["kernel"]["B64"]["kernel_us_per_image"] / 1e3
    out["tower_ms_per_image_B64"] = tower if tower is not None else "not found in profiles/clip_vision_bench.json"
    if tower is not None:
        out["kernel_over_tower_B64"] = round(k64 / tower, 4)
        out["kernel_below_tower"] = bool(k64 < tower)
    print(json.dumps(out))
    if a.out:
        update_json(a.out, out)


if __name__ == "__main__":
    main()
