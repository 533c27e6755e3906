"""One training step of the low-level encoder (low_level.LowLevelTrainer) at the published widths (63 x 250 EEG -> 8064 -> 1024 -> 512 -> 256 -> 128 -> 64 -> 4,
1 x 1 -> 64 x 64), bf16, B = 16 and B = 64.  Writes one JSON object (default profiles/low_level_train_bench.json):

* step: LowLevelTrainer.step, synchronised host clock around --steps consecutive steps per sample (divided by their number), median / min / max of --reps samples.
* calls: every C-ABI call of the step in order, timed by an event pair around the call on the step's stream in --reps SEPARATE, instrumented steps (an ABI call
  is one to three launches, so the launch's own timestamps of eegclip_time_next_launch do not apply; an event bracket includes the dispatch gaps, a few us per
  call, which matters for the small calls and not for the large ones).  Each call is set against two bounds: the bytes it must move at the 8.0 TB/s HBM figure
  bench.py uses, and its matrix-core work at 2.5 PFLOP/s (dense bf16).  Bytes: pack 8 B per weight (fp32 in, two 16-bit packings out); convt16 / bwd_data the LIVE
  taps' weights (1 x 1: a quarter) plus the frames; bwd_weight the frames plus the fp32 gradient (dead taps included: their zeros are written); BatchNorm its
  frames once per pass; AdamW 28 B per parameter (p, g, m, v in; p, m, v out).
* yardstick: the same step on tests/low_level_ref.py moved to the same GPU -- torch's own ConvTranspose2d / BatchNorm2d / autograd, torch.optim.AdamW --, fp32 and
  under bf16 autocast, in the same process, alternated with our step sample by sample.
* NOT measured here: the yardstick's per-kernel times, and the split of an ABI call into its launches (BatchNorm partial / finalize / apply, bwd_weight and its
  slab reduction): the event brackets see a call as a whole.

    python tools/bench_low_level_train.py [--reps 7] [--steps 5] [--batches 16,64] [--out profiles/low_level_train_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12
MFMA_FLOPS_PER_S = 2.5e15


def _stats(v, unit="ms"):
    return {f"median_{unit}": round(statistics.median(v), 4), f"min_{unit}": round(min(v), 4), f"max_{unit}": round(max(v), 4),
            "spread": round((max(v) - min(v)) / statistics.median(v), 4)}


class TimedLib:
    """the library handle with an event pair around every call while `on`"""

    def __init__(self, real, torch):
        self.real, self.torch, self.on, self.log = real, torch, False, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.startswith("eegclip_") or name.endswith(("_floats", "_slabs", "_bytes")):
            return fn

        def call(*a):
            if not self.on:
                return fn(*a)
            e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            self.log.append((name, e0, e1))
            return rc
        return call


def live_fraction(side):
    return 0.25 if side == 1 else 1.0


def call_bounds(ch, B, n_params):
    """per ABI call of a step, in call order: (name, label, bytes, flops)"""
    n = len(ch) - 1
    out = [("eegclip_convt16_pack_train", f"layer {i + 1}", 8 * 16 * ch[i] * ch[i + 1], 0) for i in range(n)]
    out.append(("eegclip_gemm16", "subject Linear", 0, 0))
    fr = lambda i: 2 * B * (2 ** i) ** 2 * ch[i]      # noqa: E731  (bytes of frame i's interior)
    for i in range(n):
        S = 2 ** i
        w = 2 * 16 * ch[i] * ch[i + 1] * live_fraction(S)
        fl = 2 * B * S * S * 16 * ch[i] * ch[i + 1] * live_fraction(S)
        out.append(("eegclip_convt16", f"layer {i + 1}", w + fr(i) + fr(i + 1), fl))
        if i < n - 1:
            out.append(("eegclip_bn2d16_fwd", f"layer {i + 1}", 3 * fr(i + 1), 0))
    out.append(("eegclip_mse_loss_grad_scaled", "loss", 0, 0))
    for i in range(n - 1, -1, -1):
        S = 2 ** i
        dzb = fr(i + 1) if i < n - 1 else 4 * B * (2 * S) ** 2 * ch[i + 1]
        fl = 2 * B * S * S * 16 * ch[i] * ch[i + 1] * live_fraction(S)
        if i < n - 1:
            out.append(("eegclip_bn2d16_bwd", f"layer {i + 1}", 7 * fr(i + 1), 0))
        out.append(("eegclip_convt16_bwd_weight", f"layer {i + 1}", fr(i) + dzb + 4 * 16 * ch[i] * ch[i + 1], fl))
        out.append(("eegclip_convt16_bwd_data", f"layer {i + 1}", 2 * 16 * ch[i] * ch[i + 1] * live_fraction(S) + dzb + fr(i), fl))
    out.append(("eegclip_gemm_f32", "subject Linear, weight + bias gradient", 0, 0))
    out.append(("eegclip_adamw_step", "all parameters", 28 * n_params, 0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5, help="consecutive steps per timing sample")
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "low_level_train_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from eeg_image_decode_amd import _lib, low_level, ops16, optim
    from low_level_ref import EncoderLowLevelRef
    if not torch.cuda.is_available():
        raise SystemExit("bench_low_level_train.py measures on the GPU; none found")
    timed = TimedLib(_lib.lib(), torch)
    for mod in (low_level, ops16, optim):
        mod.lib = lambda: timed
    model = low_level.LowLevelEncoder(device="cuda", dtype=torch.bfloat16)
    ch = model.channels
    trainer = low_level.LowLevelTrainer(model, lr=1e-4)
    n_params = sum(p.numel() for p in trainer.params.values())
    refs = {}
    for mode in ("fp32", "bf16_autocast"):
        r = EncoderLowLevelRef().cuda().train()
        refs[mode] = (r, torch.optim.AdamW(r.parameters(), lr=1e-4))

    def ref_step(mode, x, t):
        r, opt = refs[mode]
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "bf16_autocast"):
            pred = r(x)
        loss = torch.nn.functional.mse_loss(pred.float(), t)
        loss.backward()
        opt.step()
        return loss

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    cases = []
    for B in [int(b) for b in args.batches.split(",")]:
        g = torch.Generator(device="cuda").manual_seed(B)
        x = torch.randn(B, 63, 250, device="cuda", generator=g)
        t = torch.randn(B, ch[-1], model.latent_size, model.latent_size, device="cuda", generator=g)
        fns = {"ours": lambda: trainer.step(x, t), "fp32": lambda: ref_step("fp32", x, t), "bf16_autocast": lambda: ref_step("bf16_autocast", x, t)}
        for k, f in fns.items():
            f(), f()
            torch.cuda.synchronize()
            print(f"B = {B}: {k} warmed up", file=sys.stderr, flush=True)
        times = {k: [] for k in fns}
        for _ in range(args.reps):                                           # alternated
            for k, f in fns.items():
                times[k].append(clock(f))
        print(f"B = {B}: step times taken", file=sys.stderr, flush=True)
        bounds = call_bounds(ch, B, n_params)
        per_call = [[] for _ in bounds]
        for _ in range(args.reps):
            timed.log, timed.on = [], True
            trainer.step(x, t)
            timed.on = False
            torch.cuda.synchronize()
            names = [nm for nm, _, _ in timed.log]
            assert names == [b[0] for b in bounds], (names, [b[0] for b in bounds])
            for j, (_, e0, e1) in enumerate(timed.log):
                per_call[j].append(e0.elapsed_time(e1) * 1e3)
        calls, tot = [], 0.0
        for (name, label, nbytes, flops), v in zip(bounds, per_call):
            med = statistics.median(v)
            tot += med
            hb, mb = nbytes / HBM_BYTES_PER_S * 1e6, flops / MFMA_FLOPS_PER_S * 1e6
            calls.append({"call": name, "what": label, "us": round(med, 2), "min_us": round(min(v), 2), "bytes": int(nbytes), "hbm_bound_us": round(hb, 2),
                          "mfma_bound_us": round(mb, 3), "bound_over_time": round(max(hb, mb) / med, 4) if nbytes else None})
        by_kind = {}
        for c in calls:
            by_kind[c["call"]] = round(by_kind.get(c["call"], 0.0) + c["us"], 2)
        hbm_total = sum(b[2] for b in bounds) / HBM_BYTES_PER_S * 1e3
        ours = statistics.median(times["ours"])
        cases.append({"B": B, "dtype": "bfloat16", "repetitions": args.reps, "step": _stats(times["ours"]), "abi_calls_per_step": len(bounds),
                      "sum_of_calls_ms": round(tot / 1e3, 4), "sum_by_call_us": by_kind, "hbm_bound_ms": round(hbm_total, 4), "hbm_bound_over_step": round(hbm_total / ours, 4),
                      "yardstick": {k: dict(_stats(times[k]), ours_over_yardstick=round(ours / statistics.median(times[k]), 4)) for k in ("fp32", "bf16_autocast")},
                      "calls": calls})
    res = {"hbm_bytes_per_s": HBM_BYTES_PER_S, "mfma_flops_per_s": MFMA_FLOPS_PER_S, "parameters": n_params,
           "model": "LowLevelEncoder() defaults (the reference's encoder_low_level widths), seeded weights, random batch",
           "yardstick": "tests/low_level_ref.py on the same GPU: torch ConvTranspose2d / BatchNorm2d / autograd + torch.optim.AdamW", "steps_per_sample": args.steps,
           "not_measured": ["the yardstick's per-kernel times", "the launches inside one ABI call (BatchNorm partial / finalize / apply; bwd_weight and its slab reduction)",
                            "fp16 timings", "hardware counters"],
           "cases": cases}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"cases": [{k: v for k, v in c.items() if k != "calls"} for c in cases]}))


if __name__ == "__main__":
    main()
