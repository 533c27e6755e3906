"""low_level.LowLevelEncoder at the published widths (63 x 250 EEG -> 8064 -> 1024 -> 512 -> 256 -> 128 -> 64 -> 4 channels, 1 x 1 -> 64 x 64; fp16), B = 1 and
B = 16.  Writes one JSON object (default profiles/low_level_bench.json):

* forward: one forward (the subject Linear, the staging copies and the six csrc/convt16.hip launches), synchronised host clock, median / min / max of --reps.
* layers: each transposed convolution alone, the kernel's own begin .. end timestamps (eegclip_time_next_launch), median and min of 15 launches; the bytes of
  the packed weight the launch reads (live taps only) and that over the kernel time.
* weight_streaming_bound: the live packed weights of the six layers over the 8.0 TB/s HBM figure bench.py and DESIGN.md use, and bound / (sum of the six kernel
  times).  (Apart from the first layer's 66 MB the weights fit the 256 MiB Infinity Cache across launches: the bound is the HBM figure all the same.)
* yardstick: the same six layers through the kernels the library had before csrc/convt16.hip, alternated with convt16 in one process: layer 1 (1 x 1 input) as
  ONE csrc/caption.hip skinny GEMM over the four live taps ((4 Cout, Cin) weight, M = B); layers 2 - 6 as four csrc/vae.hip conv16 launches each, a phase's
  2 x 2 taps embedded in a 3 x 3 kernel with five zero taps (conv16 takes KS 1 | 3 only: 9/4 of the weight and the FLOPs).  `max_abs_diff` is the yardstick's
  output against convt16's on the same input (both without epilogue).

    python tools/bench_low_level.py [--reps 9] [--out profiles/low_level_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12


def _stats(v, unit="ms"):
    return {f"median_{unit}": round(statistics.median(v), 4), f"min_{unit}": round(min(v), 4), f"max_{unit}": round(max(v), 4),
            "spread": round((max(v) - min(v)) / statistics.median(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "low_level_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from eeg_image_decode_amd import _abi
    from eeg_image_decode_amd._lib import check, lib, raw_stream
    from eeg_image_decode_amd.low_level import LowLevelEncoder
    from eeg_image_decode_amd.ops16 import conv_transpose16, conv_transpose_live_taps, linear16_skinny
    if not torch.cuda.is_available():
        raise SystemExit("bench_low_level.py measures on the GPU; none found")
    L_ = lib()
    model = LowLevelEncoder(device="cuda", dtype=torch.float16)
    ch = model.channels
    n = len(ch) - 1
    packed = [model._layer(i)[0] for i in range(n)]
    e0, e1 = L_.eegclip_timing_event_create(), L_.eegclip_timing_event_create()

    def stamped(f):
        """the NEXT launch's own begin .. end, in us (f launches exactly one kernel)"""
        torch.cuda.synchronize()
        assert L_.eegclip_time_next_launch(e0, e1) == 0
        f()
        torch.cuda.synchronize()
        return float(L_.eegclip_timing_elapsed_ms(e0, e1)) * 1e3

    def conv16_phase(frame, w3, out):
        N, Hp, Wp, Cin = frame.shape
        d = _abi.Conv16Desc(in_=frame.data_ptr(), W=w3.data_ptr(), out=out.data_ptr(), bias=None, residual=None, N=N, Hi=Hp - 2, Wi=Wp - 2, Cin=Cin, in_pad=1,
                            Ho=Hp - 2, Wo=Wp - 2, Cout=w3.shape[0], out_pad=0, KS=3, stride=1, pad_top=1, pad_left=1, upsample=0, dtype=_abi.DT_F16)
        check(L_.eegclip_conv16(d, raw_stream()), "conv16 (yardstick)")

    def embed3x3(pw, phase):
        """a phase's (Cout, 4 taps, Cin) as a 3 x 3 convolution's (Cout, 9, Cin): tap half 0 in the centre, half 1 at the neighbour's side"""
        py, px = phase >> 1, phase & 1
        w3 = torch.zeros(pw.shape[1], 3, 3, pw.shape[3], dtype=pw.dtype, device=pw.device)
        for tap in range(4):
            dy, dx = ((1 if py else -1) if tap >> 1 else 0), ((1 if px else -1) if tap & 1 else 0)
            w3[:, 1 + dy, 1 + dx] = pw[phase, :, tap]
        return w3.reshape(pw.shape[1], 9, pw.shape[3]).contiguous()

    w_skinny = packed[0][:, :, 0, :].reshape(4 * ch[1], ch[0]).contiguous()                    # layer 1's live taps: [phase][co] rows
    w3 = [None] + [[embed3x3(packed[i], p) for p in range(4)] for i in range(1, n)]
    cases = []
    for B in (1, 16):
        g = torch.Generator(device="cuda").manual_seed(B)
        x = torch.randn(B, 63, 250, device="cuda", generator=g)
        for _ in range(3):
            model(x)
        fwd = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model(x)
            torch.cuda.synchronize()
            fwd.append((time.perf_counter() - t0) * 1e3)
        layers, tot_new, tot_old, live_bytes = [], 0.0, 0.0, 0
        for i in range(n):
            S = 2 ** i
            frame = torch.zeros(B, S + 2, S + 2, ch[i], dtype=torch.float16, device="cuda")
            frame[:, 1:-1, 1:-1] = torch.randn(B, S, S, ch[i], device="cuda", generator=g).half()
            out = (torch.zeros(B, 2 * S + 2, 2 * S + 2, ch[i + 1], dtype=torch.float16, device="cuda") if ch[i + 1] >= 16 else
                   torch.empty(B, ch[i + 1], 2 * S, 2 * S, dtype=torch.float16, device="cuda"))
            new = lambda: conv_transpose16(frame, packed[i], out=out)                        # noqa: E731
            taps = bin(conv_transpose_live_taps(S, S)).count("1")
            wbytes = 2 * taps * ch[i] * ch[i + 1]
            live_bytes += wbytes
            if i == 0:
                xs = frame[:, 1, 1].contiguous()
                ys = torch.empty(B, 4 * ch[1], dtype=torch.float16, device="cuda")
                old_fns = [lambda: linear16_skinny(xs, w_skinny, out=ys)]
            else:
                outs = [torch.empty(B, S, S, ch[i + 1], dtype=torch.float16, device="cuda") for _ in range(4)]
                old_fns = [(lambda p=p: conv16_phase(frame, w3[i][p], outs[p])) for p in range(4)]
            for f in [new] + old_fns:
                f(), f()
            t_new, t_old = [], []
            for _ in range(15):                                                              # alternated
                t_new.append(stamped(new))
                t_old.append(sum(stamped(f) for f in old_fns))
            torch.cuda.synchronize()
            if ch[i + 1] >= 16:
                got = out[:, 1:-1, 1:-1].float()                                             # (B, 2S, 2S, Cout)
            else:
                got = out.permute(0, 2, 3, 1).float()
            if i == 0:
                old = ys.view(B, 2, 2, ch[1]).float()
            else:
                old = torch.empty_like(got)
                for p in range(4):
                    old[:, (p >> 1)::2, (p & 1)::2] = outs[p].float()
            diff = float((got - old).abs().max())
            mn, mo = statistics.median(t_new), statistics.median(t_old)
            tot_new += mn
            tot_old += mo
            layers.append({"layer": i + 1, "Cin": ch[i], "Cout": ch[i + 1], "input": f"{S}x{S}", "pixels_per_phase": B * S * S, "live_taps_of_16": taps,
                           "live_weight_bytes": wbytes, "convt16_us": round(mn, 2), "convt16_min_us": round(min(t_new), 2),
                           "weight_TBps": round(wbytes / mn / 1e6, 3), "yardstick": "gemm16_skinny over the 4 live taps" if i == 0 else "4 x conv16 3x3 (5 zero taps)",
                           "yardstick_us": round(mo, 2), "yardstick_min_us": round(min(t_old), 2), "convt16_over_yardstick": round(mn / mo, 4),
                           "max_abs_diff": diff})
        bound_us = live_bytes / HBM_BYTES_PER_S * 1e6
        cases.append({"B": B, "dtype": "float16", "repetitions": args.reps, "forward": _stats(fwd), "launches_per_forward": 1 + n, "layers": layers,
                      "sum_convt16_us": round(tot_new, 2), "sum_yardstick_us": round(tot_old, 2), "convt16_over_yardstick": round(tot_new / tot_old, 4),
                      "weight_streaming_bound": {"live_weight_bytes": live_bytes, "bound_us": round(bound_us, 2),
                                                 "bound_over_sum_convt16": round(bound_us / tot_new, 4)}})
    L_.eegclip_timing_event_destroy(e0), L_.eegclip_timing_event_destroy(e1)
    res = {"hbm_bytes_per_s": HBM_BYTES_PER_S, "model": "LowLevelEncoder() defaults (the reference's encoder_low_level widths), seeded weights", "cases": cases}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
