"""VAE decode of two builds of the package, alternated in fresh processes: the decoded image of one seeded latent must be bit-identical, and the ms per decode
(vae.bench_decode, latent 128 = 1024 x 1024) is reported per run so that the two builds' spreads can be compared.

    python tools/compare_vae_builds.py --other PATH_TO_OTHER_TREE [--rounds 2] [--out profiles/vae_build_compare.json]

PATH_TO_OTHER_TREE is another checkout with its library already built (e.g. the parent commit)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
import torch
from eeg_image_decode_amd import vae
torch.manual_seed(0)
m = vae.SDXLShapedVAE().cuda()
z = torch.randn(1, 4, 128, 128, generator=torch.Generator().manual_seed(7)).to("cuda", torch.bfloat16)
img = m.decode(z)
torch.cuda.synchronize()
digest = hashlib.sha256(img.view(torch.int16).cpu().numpy().tobytes()).hexdigest()
b = vae.bench_decode(latent=128, reps=5)
print(json.dumps({"sha256": digest, "ms_per_decode": b["ms_per_decode"]}))
"""


def run(tree):
    out = subprocess.run([sys.executable, "-c", CHILD, tree], capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        raise SystemExit(f"decode under {tree} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_build_compare.json"))
    a = ap.parse_args()
    runs = []
    for _ in range(a.rounds):
        for name, tree in (("other", os.path.abspath(a.other)), ("this", ROOT)):
            r = run(tree)
            r["build"] = name
            runs.append(r)
            print(json.dumps(r), flush=True)
    same = len({r["sha256"] for r in runs}) == 1
    res = {"what": "SDXLShapedVAE.decode of one seeded 128 x 128 latent (bf16) and vae.bench_decode(latent=128), two builds alternated in fresh processes",
           "bit_identical": same, "runs": runs,
           "ms_other": [r["ms_per_decode"] for r in runs if r["build"] == "other"], "ms_this": [r["ms_per_decode"] for r in runs if r["build"] == "this"]}
    print(json.dumps({"bit_identical": same, "ms_other": res["ms_other"], "ms_this": res["ms_this"]}))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if not same:
        raise SystemExit("decode outputs differ between the builds")


if __name__ == "__main__":
    main()
