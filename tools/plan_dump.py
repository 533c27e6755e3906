"""Every launch plan of the training paths as text, so that two trees can be compared record for record (CPU only: the plans are built on the lane
emulator, as the `-m "not gpu"` suite builds them).

    python tools/plan_dump.py --out dump.json                                              # this tree
    python tools/plan_dump.py --other PATH_TO_OTHER_TREE --out profiles/plan_dump.json     # this tree against another built checkout (e.g. the parent commit)

Plans are read through Plan.ops, Plan._seed_slots and Plan._seed_descs only, so this file runs unchanged against an older tree (a child process per tree, as
tools/compare_builds.py does).  Per plan one record per op:
    the entry point's name and side flag; every non-pointer argument verbatim (floats as float.hex); every pointer argument as (label, byte offset) when it
    lies in a tensor reachable from the engine, the step plan or the plan (labelled by the attribute path of the first tensor seen on that storage), otherwise
    as ("ptr", n), n = order of first appearance in the plan; ctypes structs behind byref() and struct arrays field by field under the same rule;
then the seed slots and the ops whose descriptor takes the run's seed.

Matrix: the ATMS forward and backward plans for EEGCLIP_GEMM_PRECISION unset | f32, single-subject | joint-subject model, B = 3 | 32, train | eval; the step plans
of the retrieval and reconstruction objectives and of a joint-subject batch that mixes subjects, B = 32, after one run() (the per-step patches are in); the
diffusion prior's training step plans after Pipe.train, and its sampling plans after one generate().  With --other: exit status 1 unless both trees give the same records.
"""
import argparse
import bisect
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Labels:
    """device pointer -> (attribute path of the first tensor seen on that storage, byte offset)"""

    def __init__(self):
        self.start, self.info, self.seen = [], [], set()

    def add(self, path, obj, depth=0):
        import torch
        if isinstance(obj, torch.Tensor):
            st = obj.untyped_storage()
            if st.nbytes() and st.data_ptr() not in self.seen:
                self.seen.add(st.data_ptr())
                i = bisect.bisect(self.start, st.data_ptr())
                self.start.insert(i, st.data_ptr())
                self.info.insert(i, (st.nbytes(), path))
        elif depth < 4 and isinstance(obj, dict):
            for k, v in obj.items():
                self.add(f"{path}[{k!r}]", v, depth + 1)
        elif depth < 4 and isinstance(obj, (list, tuple)):
            for k, v in enumerate(obj):
                self.add(f"{path}[{k}]", v, depth + 1)

    def add_attrs(self, path, obj, first=()):
        for k in list(first) + sorted(vars(obj)):
            self.add(f"{path}.{k}", getattr(obj, k, None))

    def find(self, p):
        i = bisect.bisect(self.start, p) - 1
        if i >= 0 and p < self.start[i] + self.info[i][0]:
            return [self.info[i][1], p - self.start[i]]
        return None


def dump_plan(pl, labels):
    from eeg_image_decode_amd import _abi
    fns = _abi.plan_functions()
    order = {}

    def pointer(v):
        if v is None or isinstance(v, int):
            if not v:
                return v
            return labels.find(v) or ["ptr", order.setdefault(v, len(order))]
        if hasattr(v, "_obj"):                                   # ctypes.byref(struct)
            return struct(v._obj)
        if isinstance(v, ctypes.Array):
            return [struct(e) if isinstance(e, (ctypes.Structure, ctypes.Union)) else pointer(e) for e in v]
        if isinstance(v, ctypes.Structure):
            return struct(v)
        raise TypeError(f"{pl.name}: pointer argument of type {type(v).__name__}")

    def scalar(t, v):
        return float(v).hex() if t in (ctypes.c_float, ctypes.c_double) else int(v)

    def struct(s):
        out = {}
        for k, t in s._fields_:
            v = getattr(s, k)
            out[k] = struct(v) if issubclass(t, ctypes.Structure) else pointer(v) if t is ctypes.c_void_p else scalar(t, v)
        return out

    ops = []
    for fn, args, name, side in pl.ops:
        if fn is None:
            rec = [pointer(args[0].data_ptr()), args[0].numel() * args[0].element_size()] if name == "memset" else []
        else:
            rec = [pointer(v) if _abi.plan_slot(t) == "p" else scalar(t, v) for t, v in zip(fns[name], args)]
            assert len(args) == len(fns[name]) + 1, (pl.name, name, len(args))          # (+ the stream)
        ops.append({"fn": name, "side": int(side), "args": rec})
    descs = []
    for d in pl._seed_descs:
        descs.append(next((i for i, op in enumerate(pl.ops) if op[0] is not None and getattr(op[1][0], "_obj", None) is d), -1))
    return {"ops": ops, "seed_slots": sorted(list(s) for s in pl._seed_slots), "seed_descs": descs}


def child(out_path):
    """dump every plan of the tree that is first on sys.path"""
    import numpy as np
    import torch
    from emu_patch import product_on_emulator
    from eeg_image_decode_amd import synthetic as syn
    result = {}

    def T(a):
        return torch.from_numpy(np.ascontiguousarray(a))

    def engine_labels(eng):
        lab = Labels()
        lab.add_attrs("eng", eng, first=("flat", "gflat"))
        return lab

    with product_on_emulator():
        from eeg_image_decode_amd import optim, retrieval, step_plan
        from eeg_image_decode_amd import prior as eprior
        from eeg_image_decode_amd.atms import ATMS
        from eeg_image_decode_amd.retrieval_joint import ATMS as JointATMS
        # ---- encoder plans
        for prec in ("bf16x3", "f32"):
            os.environ.pop("EEGCLIP_GEMM_PRECISION", None)
            if prec == "f32":
                os.environ["EEGCLIP_GEMM_PRECISION"] = "f32"
            for joint in (False, True):
                torch.manual_seed(7)
                m = JointATMS(joint_train=True) if joint else ATMS()
                eng = m._engine()
                for B in (3, 32):
                    eng.bufs[B] = b = eng._alloc(B)
                    plans = {}
                    for train in (True, False):
                        probs = m.train(train).drop_probs(train)
                        plans["fwd", train] = eng._build_fwd(B, train, False, probs)
                        if "ds" not in b:
                            eng._alloc_bwd(B, b)
                        plans["bwd", train] = eng._build_bwd(B, False, probs, False, False, train)
                    lab = engine_labels(eng)
                    for (kind, train), pl in plans.items():
                        lab.add_attrs(f"{kind}{int(train)}", pl)
                    for (kind, train), pl in plans.items():
                        result[f"atms/{prec}/{'joint' if joint else 'single'}/B{B}/{'train' if train else 'eval'}/{kind}"] = dump_plan(pl, lab)
        os.environ.pop("EEGCLIP_GEMM_PRECISION", None)
        # ---- step plans: two ordinary steps, the third through the plan (tests/test_product_on_emulator.py)
        step_plan._runtime_ok = lambda: True
        step_plan._on_device = lambda t: True
        step_plan.StepPlan.WARM_STEPS = 2
        B, NC = 32, 40
        rng = np.random.default_rng(1)
        cls = T(syn.unit_features(4, NC, tag="c"))
        data = [(T(syn.eeg_batch(100 + i, B)), T(syn.unit_features(200 + i, B, tag="i")), T(syn.unit_features(300 + i, B, tag="t")),
                 T(rng.integers(0, NC, size=B).astype(np.int64))) for i in range(3)]
        mixed = rng.integers(1, 5, B).tolist()
        for variant in ("retrieval", "reconstruction", "joint_mixed"):
            objective = "reconstruction" if variant == "reconstruction" else "retrieval"
            os.environ.pop("EEGCLIP_WGRAD_ADAMW", None)
            if variant == "reconstruction":
                os.environ["EEGCLIP_WGRAD_ADAMW"] = "1"               # (the opt-in form: the slab reduction steps the optimizer)
            torch.manual_seed(5)
            m = (JointATMS(joint_train=True) if variant == "joint_mixed" else ATMS()).train()
            opt = optim.AdamW(m.parameters(), lr=3e-4)
            acc, correct = [], torch.zeros(1, dtype=torch.int32)
            for x, img, txt, lab_ in data:
                retrieval.contrastive_step(m, opt, x, mixed if variant == "joint_mixed" else 1, img, txt, lab_, cls, acc, correct,
                                           alpha=0.9 if objective == "reconstruction" else 0.99, objective=objective)
            sp, = retrieval.step_plans_of(m)
            lab = engine_labels(sp.eng)
            lab.add_attrs("step", sp)
            lab.add_attrs("pl", sp.pl)
            lab.add("opt", opt.state_dict()["state"])
            lab.add("cls", cls)
            result[f"step/{variant}/B{B}"] = dump_plan(sp.pl, lab)
        os.environ.pop("EEGCLIP_WGRAD_ADAMW", None)
        # ---- the prior: training step plans (one per condition key) and the sampling plans
        built = []
        real_init = eprior._TrainStepPlan.__init__

        def keeping_init(self, *a, **k):
            real_init(self, *a, **k)
            built.append(self)
        eprior._TrainStepPlan.__init__ = keeping_init
        N, E, Cd = 64, 128, 64
        rng = np.random.default_rng(21)
        pdata = [{"c_embedding": T(rng.standard_normal((N, Cd)).astype(np.float32)), "h_embedding": T(rng.standard_normal((N, E)).astype(np.float32))}
                 for _ in range(9)]
        torch.manual_seed(5)
        pm = eprior.DiffusionPriorUNet(embed_dim=E, cond_dim=Cd, hidden_dim=[128, 64, 64], time_embed_dim=64, dropout=0.1)
        pipe = eprior.Pipe(pm, device="cpu")
        pipe.cond_drop_prob = 0.3
        torch.manual_seed(11)
        pipe.train(pdata, num_epochs=1, learning_rate=1e-3)
        eprior._TrainStepPlan.__init__ = real_init
        peng = pm._engine()
        for tp in built:
            lab = engine_labels(peng)
            lab.add_attrs("train", tp)
            lab.add_attrs("pl", tp.pl)
            result[f"prior/train/{tp.key}"] = dump_plan(tp.pl, lab)
        pm.eval()
        pipe.generate(c_embeds=pdata[0]["c_embedding"][:2], num_inference_steps=3, guidance_scale=2.0, generator=torch.Generator().manual_seed(3))
        for key, val in peng.plans.items():
            if isinstance(val, tuple):                               # sampling: (hoisted plan, per-step plan, buffers)
                lab = engine_labels(peng)
                lab.add("b", val[2])
                result[f"prior/sampling/{key}/hoist"] = dump_plan(val[0], lab)
                result[f"prior/sampling/{key}/step"] = dump_plan(val[1], lab)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=0, sort_keys=True)


def run_child(tree, out_path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([tree, os.path.join(tree, "tests")]))
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", "--out", out_path], env=env, cwd=tree)
    with open(out_path) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="another built checkout to compare with")
    ap.add_argument("--out", required=True)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.out = os.path.abspath(a.out)
    if a.child:
        return child(a.out)
    if not a.other:
        run_child(ROOT, a.out)
        return 0
    this = run_child(ROOT, a.out + ".this.tmp")
    other = run_child(os.path.abspath(a.other), a.out + ".other.tmp")
    os.remove(a.out + ".this.tmp")
    os.remove(a.out + ".other.tmp")
    differ = {}
    for k in sorted(set(this) | set(other)):
        if this.get(k) != other.get(k):
            ta, tb = this.get(k, {}).get("ops", []), other.get(k, {}).get("ops", [])
            first = next((i for i, (x, y) in enumerate(zip(ta, tb)) if x != y), min(len(ta), len(tb)))
            differ[k] = {"first_differing_op": first, "this": ta[first] if first < len(ta) else None, "other": tb[first] if first < len(tb) else None}
    res = {"what": "tools/plan_dump.py: every plan of the matrix in its docstring, this tree against the other one, record for record",
           "plans": len(this), "ops": sum(len(v["ops"]) for v in this.values()), "seed_slots": sum(len(v["seed_slots"]) for v in this.values()),
           "seeded_descriptors": sum(len(v["seed_descs"]) for v in this.values()),
           "ops_per_plan": {k: len(v["ops"]) for k, v in sorted(this.items())}, "equal": not differ, "differ": differ}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("plans", "ops", "seed_slots", "seeded_descriptors", "equal")}))
    return 0 if not differ else 1


if __name__ == "__main__":
    sys.exit(main())
