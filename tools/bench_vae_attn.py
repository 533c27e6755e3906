"""csrc/vae_attn.hip and the VAE decode around it.  Writes one JSON object (default profiles/vae_attn_bench.json):

* kernel: eegclip_vae_attn_fwd alone at head_dim 512, B = 1, T = 4096 and 16384 (the mid block of a 512 x 512 and of a 1024 x 1024 decode), fp16 and bf16:
  ms, TFLOP/s from 4 T^2 D, and the share of the 2.5 PF/s dense 16-bit MFMA peak.  Device events around a window of >= 0.3 s after a warm-up.
* decode: vae.bench_decode at latent 64 and 128, and torch.cuda.max_memory_allocated over one 1024 x 1024 decode.  With --parent-tree DIR (a built
  checkout of the commit to compare with) the same runs there too: one worker process per tree, repetitions ALTERNATED between the two, median / min
  of each and the parent's run-to-run spread ((max - min) / median).

    python tools/bench_vae_attn.py [--parent-tree DIR] [--reps 10] [--out profiles/vae_attn_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 2.5e15
LATENTS = (64, 128)


def ev_ms(f, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def bench_kernel():
    import torch
    from eeg_image_decode_amd.ops16 import vae_attention
    rows, D = [], 512
    for dt in (torch.float16, torch.bfloat16):
        for T in (4096, 16384):
            g = torch.Generator(device="cuda").manual_seed(T)
            qkv = torch.randn(1, T, 3 * D, device="cuda", dtype=dt, generator=g)          # the packed projection's layout, consumed in place
            q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
            o = torch.empty(1, T, D, device="cuda", dtype=dt)
            run = lambda: vae_attention(q, k, v, out=o)          # noqa: E731
            for _ in range(3):
                run()
            n = max(10, int(300.0 / ev_ms(run, 5)))              # a window of >= 0.3 s
            ms = ev_ms(run, n)
            flop = 4.0 * T * T * D
            rows.append({"dtype": str(dt).split(".")[-1], "B": 1, "T": T, "head_dim": D, "launches_timed": n, "ms": round(ms, 4),
                         "TFLOPs": round(flop / ms / 1e9, 1), "fraction_of_peak": round(flop / ms / 1e-3 / PEAK, 3), "finite": bool(torch.isfinite(o).all())})
            del qkv, o
            torch.cuda.empty_cache()
    return rows


def worker():
    """one line in, one JSON line out: `kernel` -> bench_kernel(); `decode L` -> vae.bench_decode(latent=L); `mem` -> peak bytes of one 1024 x 1024
    decode.  (All GPU work happens in workers: the parent process starts them before anything touches a device and never opens one itself.)"""
    import torch
    from eeg_image_decode_amd import _abi, vae
    if not torch.cuda.is_available():
        raise SystemExit("bench_vae_attn.py measures on the GPU; none found")
    print(json.dumps({"ready": f"ABI {_abi.ABI_VERSION}"}), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd:
            continue
        if cmd[0] == "kernel":
            with torch.no_grad():
                r = bench_kernel()
        elif cmd[0] == "decode":
            r = vae.bench_decode(images=1, latent=int(cmd[1]), reps=3)
        else:
            m = vae.SDXLShapedVAE().cuda()
            z = torch.randn(1, 4, 128, 128, device="cuda", dtype=torch.bfloat16)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            m.decode(z)
            torch.cuda.synchronize()
            r = {"max_memory_allocated_MB": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), "allocated_before_MB": round(base / 2 ** 20, 1)}
            del m, z
        torch.cuda.empty_cache()
        print(json.dumps(r), flush=True)


class Tree:
    def __init__(self, root):
        env = dict(os.environ, PYTHONPATH=root)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], cwd=root, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  text=True)
        line = self.p.stdout.readline()
        if not line:
            raise SystemExit(f"the worker in {root} did not start (exit status {self.p.wait()})")
        self.where = json.loads(line)["ready"]                          # the tree's ABI version: tells the two libraries apart

    def ask(self, cmd):
        self.p.stdin.write(cmd + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError(f"the worker in {self.where} ended on `{cmd}` (exit status {self.p.wait()})")
        return json.loads(line)

    def close(self):
        self.p.stdin.close()
        self.p.wait()


def bench_decode(parent_tree, reps):
    trees = {"this": Tree(ROOT)}
    if parent_tree:
        trees["parent"] = Tree(os.path.abspath(parent_tree))
    out = {"libraries": {n: t.where for n, t in trees.items()}, "repetitions": reps, "decodes_per_repetition": 3}
    try:
        kernel = trees["this"].ask("kernel")
        for L in LATENTS:
            ms = {n: [] for n in trees}
            for n, t in trees.items():
                t.ask(f"decode {L}")                                 # warm-up: code objects, the allocator's pool
            for _ in range(reps):
                for n, t in trees.items():                           # alternated
                    ms[n].append(t.ask(f"decode {L}")["ms_per_decode"])
            row = {}
            for n, v in ms.items():
                row[n] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                          "spread": round((max(v) - min(v)) / statistics.median(v), 4)}
            if "parent" in row:
                row["this_over_parent_median"] = round(row["this"]["median_ms"] / row["parent"]["median_ms"], 4)
            out[f"latent_{L}"] = row
        out["decode_1024_memory"] = {n: t.ask("mem") for n, t in trees.items()}
    finally:
        for t in trees.values():
            t.close()
    if not parent_tree:
        out["parent"] = "not measured"
    return kernel, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_attn_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.getcwd() if args.worker else ROOT)
    if args.worker:
        return worker()
    kernel, decode = bench_decode(args.parent_tree, args.reps)
    out = {"peak_dense_16bit_TFLOPs": PEAK / 1e12, "kernel": kernel, "decode": decode}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
