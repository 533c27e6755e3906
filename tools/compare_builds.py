"""The generation stack under two builds of the package (this tree and another checkout, e.g. the parent commit, with its library built), alternated in
fresh processes: per case a sha256 of the outputs, which must be identical across every run of both trees (these paths are bit-reproducible), and a time.

    python tools/compare_builds.py --other PATH_TO_OTHER_TREE [--rounds 3] [--cases vae_decode,text_encoder,...] [--out profiles/build_compare.json]

Cases (the child uses public names only, so it runs under both trees):
  weights          CPU only: sdxl_text_encoder(seed=3), a reduced SDXLUNet, SDXLShapedVAE(seed=3) -- sha256 over the state_dict (same weights from the same seed)
  vae_decode       SDXLShapedVAE.decode of one seeded 128 x 128 latent (bf16); ms = vae.bench_decode(latent=128, reps=5)
  unet_512_b1      SDXLUNet forward (SDXL config + IP-Adapter, fp16) at the shapes of tools/bench_sdxl_unet.py; ms = median of 5 forwards (CUDA events)
  unet_1024_b2
  text_encoder     forward of each SDXL text encoder, B = 1, output_hidden_states=True; ms = median of 30 forwards (host clock + synchronise: host-bound)
  text_encoder_2
  standin_loop     4-step seeded DDIM run of the stand-in pipeline (2 images, guidance 5, 32 x 32 latents), without / with self_attention=True;
  standin_loop_sa  ms = median of 5 further runs, host clock
  git_caption      a reduced GITCaptioner (2 layers, hidden 128, fp16): forward of 2 x 6 ids over 9 visual tokens and a greedy generate to length 8 -- sha256 over
                   the logits and the ids; ms = median of 5 further forward + generate runs, host clock
  low_level        a reduced-width LowLevelEncoder (hidden 128, widths 256-128-64-64-4, bf16, B = 16): forward, then one LowLevelTrainer.step -- sha256 over
                   the latent and every parameter gradient (the loss is an atomic sum); ms = median of 5 further steps, host clock
  clip_vision      two reduced CLIPVisionEncoders (2 layers, fp16) on 2 seeded 224 x 224 images (257 tokens): hidden 640 = 8 heads of 80 with a projection
                   and hidden 512 = 8 heads of 64 without one (post_layernorm on every token) -- sha256 over image_embeds / last_hidden_state and
                   the hidden states; ms = median of 5 further forwards of both, host clock

Time: the other tree's own runs are the reference.  This tree's median per case must lie within the other tree's [min, max] widened on both sides by
its spread (max - min); `within_range` records it.  Exit status 1 if a digest differs or a case is outside its range."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("weights", "vae_decode", "unet_512_b1", "unet_1024_b2", "text_encoder", "text_encoder_2", "standin_loop", "standin_loop_sa", "git_caption",
         "low_level", "clip_vision")

CHILD = r"""
import hashlib, json, statistics, sys, time
sys.path.insert(0, sys.argv[1])
cases = sys.argv[2].split(",")
import torch


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def host_ms(fn, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms)


def event_ms(fn, reps):
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def weights():
    from eeg_image_decode_amd.clip_text import sdxl_text_encoder
    from eeg_image_decode_amd.sdxl_unet import SDXLUNet
    from eeg_image_decode_amd.vae import SDXLShapedVAE
    unet = SDXLUNet(block_out_channels=(64, 128), transformer_layers_per_block=1, down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"),
                    up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"), seed=3)
    return {"sha256": sha(*[v for m in (sdxl_text_encoder(seed=3), unet, SDXLShapedVAE(seed=3)) for v in m.state_dict().values()])}


def vae_decode():
    from eeg_image_decode_amd import vae
    m = vae.SDXLShapedVAE().cuda()
    z = torch.randn(1, 4, 128, 128, generator=torch.Generator().manual_seed(7)).to("cuda", torch.bfloat16)
    img = m.decode(z)
    torch.cuda.synchronize()
    digest = sha(img)
    del m
    return {"sha256": digest, "ms": vae.bench_decode(latent=128, reps=5)["ms_per_decode"]}


_unet = []


def unet(B, L):
    from eeg_image_decode_amd.sdxl_unet import SDXLUNet
    if not _unet:
        _unet.append(SDXLUNet(dtype=torch.float16, device="cuda", ip_adapter=True))
    m = _unet[0]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 4, L, L, generator=g).to("cuda", m.dtype)
    ehs = (torch.randn(B, 77, 2048, generator=g) * 0.5).to("cuda", m.dtype)
    added = {"text_embeds": (torch.randn(B, 1280, generator=g) * 0.5).to("cuda", m.dtype),
             "time_ids": torch.tensor([[8 * L, 8 * L, 0, 0, 8 * L, 8 * L]] * B, dtype=m.dtype, device="cuda"),
             "image_embeds": torch.randn(B, 1024, generator=g).to("cuda", m.dtype)}
    run = lambda: m(x, 999, encoder_hidden_states=ehs, added_cond_kwargs=added)[0]
    digest = sha(run())
    run()
    return {"sha256": digest, "ms": event_ms(run, 5)}


def text_encoder(which):
    from eeg_image_decode_amd import clip_text
    enc = (clip_text.sdxl_text_encoder, clip_text.sdxl_text_encoder_2)[which](dtype=torch.float16, device="cuda")
    ids = torch.tensor([[clip_text.BOS_ID] + list(range(1000, 1009)) + [clip_text.EOS_ID] + [0 if which else clip_text.EOS_ID] * 66])
    run = lambda: enc(ids, output_hidden_states=True)
    out = run()
    digest = sha(*out.hidden_states, out.last_hidden_state, out.pooler_output, *([out.text_embeds] if out.text_embeds is not None else []))
    for _ in range(3):
        run()
    return {"sha256": digest, "ms": host_ms(run, 30)}


def standin_loop(sa):
    from eeg_image_decode_amd.sdxl import DDIMScheduler, SDXLShapedUNet, StandInSDXLPipeline
    pipe = StandInSDXLPipeline(SDXLShapedUNet(dtype=torch.float16, self_attention=sa), DDIMScheduler(), device="cuda", dtype=torch.float16,
                               default_sample_size=32)
    emb = torch.randn(2, 1024, generator=torch.Generator().manual_seed(1)).to("cuda", torch.float16)
    run = lambda: pipe.generate_ip_adapter_embeds(prompt="", ip_adapter_embeds=emb, num_inference_steps=4, guidance_scale=5.0,
                                                  generator=torch.Generator(device="cuda").manual_seed(0)).images
    digest = sha(run())
    return {"sha256": digest, "ms": host_ms(run, 5)}


def git_caption():
    from eeg_image_decode_amd.git_caption import GITCaptioner
    m = GITCaptioner(vocab_size=515, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, max_position_embeddings=64,
                     vision_hidden_size=128, dtype=torch.float16, device="cuda", seed=0)
    g = torch.Generator().manual_seed(5)
    vis = torch.randn(2, 9, 128, generator=g).to("cuda", torch.float16)
    ids = torch.randint(0, 515, (2, 6), generator=g)
    run = lambda: (m(ids, vis), m.generate(vis, max_length=8))
    logits, out = run()
    digest = sha(logits, out)
    return {"sha256": digest, "ms": host_ms(run, 5)}


def low_level():
    from eeg_image_decode_amd.low_level import LowLevelEncoder, LowLevelTrainer
    m = LowLevelEncoder(num_channels=2, hidden=128, channels=(256, 128, 64, 64, 4), dtype=torch.bfloat16, device="cuda", seed=1)
    g = torch.Generator().manual_seed(6)
    x, target = torch.randn(16, 2, 250, generator=g).cuda(), torch.randn(16, 4, 16, 16, generator=g).cuda()
    latent = m(x)
    trainer = LowLevelTrainer(m, lr=1e-3)
    trainer.step(x, target)
    digest = sha(latent, *trainer.grads().values())             # not the loss: its workgroups' partial sums are added with atomics, in any order
    return {"sha256": digest, "ms": host_ms(lambda: trainer.step(x, target), 5)}


def clip_vision():
    from eeg_image_decode_amd.clip_vision import CLIPVisionEncoder
    towers = (CLIPVisionEncoder(640, 1280, 2, 8, "gelu", 128, dtype=torch.float16, device="cuda", seed=2),
              CLIPVisionEncoder(512, 1024, 2, 8, "quick_gelu", None, post_layernorm_all=True, dtype=torch.float16, device="cuda", seed=2))
    px = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(8)).to("cuda", torch.float16)
    run = lambda: [m(px, output_hidden_states=True) for m in towers]
    h80, h64 = run()
    digest = sha(h80.image_embeds, h80.last_hidden_state, *h80.hidden_states, h64.last_hidden_state, *h64.hidden_states)
    return {"sha256": digest, "ms": host_ms(run, 5)}


table = {"weights": weights, "vae_decode": vae_decode, "unet_512_b1": lambda: unet(1, 64), "unet_1024_b2": lambda: unet(2, 128),
         "text_encoder": lambda: text_encoder(0), "text_encoder_2": lambda: text_encoder(1), "standin_loop": lambda: standin_loop(False),
         "standin_loop_sa": lambda: standin_loop(True), "git_caption": git_caption, "low_level": low_level,
         "clip_vision": clip_vision}
res = {}
for c in cases:
    if not c.startswith("unet"):
        _unet.clear()                       # (the two UNet cases share one model)
    res[c] = table[c]()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()
print(json.dumps(res))
"""


def run(tree, cases):
    out = subprocess.run([sys.executable, "-c", CHILD, tree, ",".join(cases)], capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(f"the cases under {tree} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "build_compare.json"))
    a = ap.parse_args()
    cases = a.cases.split(",")
    if any(c not in CASES for c in cases):
        raise SystemExit(f"--cases takes a subset of {CASES}")
    runs = {c: {"other": [], "this": []} for c in cases}
    for _ in range(a.rounds):
        for name, tree in (("other", os.path.abspath(a.other)), ("this", ROOT)):
            r = run(tree, cases)
            for c in cases:
                runs[c][name].append(r[c])
            print(json.dumps({"build": name, **r}), flush=True)
    res, ok = {}, True
    for c in cases:
        both = runs[c]["other"] + runs[c]["this"]
        row = {"bit_identical": len({r["sha256"] for r in both}) == 1, "sha256": sorted({r["sha256"] for r in both})}
        if "ms" in both[0]:
            o, t = [r["ms"] for r in runs[c]["other"]], [r["ms"] for r in runs[c]["this"]]
            spread = max(o) - min(o)
            row.update(ms_other=o, ms_this=t, range_other=[min(o), max(o)], range_this=[min(t), max(t)], median_this=statistics.median(t),
                       allowed=[min(o) - spread, max(o) + spread])
            row["within_range"] = row["allowed"][0] <= row["median_this"] <= row["allowed"][1]
        ok = ok and row["bit_identical"] and row.get("within_range", True)
        res[c] = row
    out = {"what": "two builds of the package alternated in fresh processes (tools/compare_builds.py): sha256 of each case's outputs and its ms per run; "
                   "allowed = the other build's [min, max] widened by its own spread, against this build's median",
           "rounds": a.rounds, "all_bit_identical": all(r["bit_identical"] for r in res.values()),
           "all_within_range": all(r.get("within_range", True) for r in res.values()), "cases": res}
    print(json.dumps({c: {k: r[k] for k in ("bit_identical", "within_range", "ms_other", "ms_this") if k in r} for c, r in res.items()}))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not ok:
        raise SystemExit("a case differs between the builds or falls outside the other build's range")


if __name__ == "__main__":
    main()
