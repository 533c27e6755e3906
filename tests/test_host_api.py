"""CPU-side checks of the host layer: reference-compatible state_dict, C-ABI symbol coverage, fail-loudly behaviour."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch

from conftest import GOLDEN, ROOT


def test_atms_state_dict_matches_reference_keys_and_shapes():
    from eeg_image_decode_amd.atms import ATMS
    m = ATMS()
    with open(os.path.join(GOLDEN, "atms_keys.json")) as f:
        ref = json.load(f)
    ours = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert list(ours.keys()) == list(ref["keys"].keys())          # same keys, same ORDER
    assert ours == ref["keys"]
    assert sum(p.numel() for p in m.parameters()) == ref["n_params"]
    assert abs(float(m.logit_scale) - 2.6592600) < 1e-5            # log(1/0.07), used raw


def test_header_abi_and_library_agree():
    from eeg_image_decode_amd import _abi
    hdr = open(os.path.join(ROOT, "include", "eegclip.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|float|void\s*\*)\s*(eegclip_\w+)\s*\(", hdr))
    assert declared == set(_abi.PROTOTYPES), (declared ^ set(_abi.PROTOTYPES))
    libpath = os.path.join(ROOT, "eeg_image_decode_amd", "csrc", "libeegclip_hip.so")
    if not os.path.exists(libpath):
        from eeg_image_decode_amd import build
        build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath], text=True)
    exported = set(re.findall(r" T (eegclip_\w+)", out))
    assert declared <= exported, declared - exported
    lib = _abi.declare(ctypes.CDLL(libpath))                        # loads without a GPU; no compute call here
    assert lib.eegclip_abi_version() == _abi.ABI_VERSION
    # every header entry cites the reference lines it replaces
    assert hdr.count(".py:") >= 12
    # the prototypes are read from the header: types, names and return types of a few entry points spelled out, one of each kind
    I, L, F, U64, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_ulonglong, ctypes.c_void_p
    assert _abi.PROTOTYPES["eegclip_adamw_step_zero_grad"] == [P, P, P, P, L, F, F, F, F, F, L, F, P, P]
    assert _abi.PARAMS["eegclip_adamw_step_zero_grad"] == ("p", "g", "m", "v", "n", "lr", "beta1", "beta2", "eps", "weight_decay", "step", "grad_scale",
                                                           "grad_scale_dev", "stream")
    assert _abi.PROTOTYPES["eegclip_dropout_scale"] == [P, L, F, U64, ctypes.c_uint, P]
    assert _abi.PROTOTYPES["eegclip_bn_finalize"][1] is ctypes.c_double
    assert _abi.PROTOTYPES["eegclip_gemm_f32"] == [ctypes.POINTER(_abi.GemmDesc), P] and _abi.PROTOTYPES["eegclip_plan_events"] == [I, P]
    assert _abi.PARAMS["eegclip_maxpool16"][0] == "in_" and _abi.PARAMS["eegclip_abi_version"] == ()
    for name, res in _abi.RESTYPES.items():
        want = {"eegclip_timing_event_create": P, "eegclip_timing_elapsed_ms": F, "eegclip_cstack_bwd_rows_count": L}.get(
            name, L if name.endswith(("_floats", "_bytes")) else I)
        assert res is want and getattr(lib, name).restype is want, name
        assert list(getattr(lib, name).argtypes) == _abi.PROTOTYPES[name] and len(_abi.PARAMS[name]) == len(_abi.PROTOTYPES[name])
    # a declaration that cannot be mapped is an error that names the function, never a gap in the table
    for bad in ("int eegclip_x(short a, void* stream);", "int eegclip_x(int);", "struct s eegclip_x(int a);", "int eegclip_x(int a[4]);"):
        with pytest.raises(TypeError, match="eegclip_x"):
            _abi._parse_prototypes(bad)


def _header_structs():
    """typedef name -> [(field, kind)] of include/eegclip.h; kind: pointer | i32 | u32 | i64 | u64 | f32 | f64 | a struct's name | (struct name, array length)"""
    from eeg_image_decode_amd import _abi
    text = _abi.header_text()
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(\w+)\s+\(?(-?\d+)\)?\s*$", text, re.M)}
    kinds = {"int": "i32", "unsigned int": "u32", "long long": "i64", "unsigned long long": "u64", "float": "f32", "double": "f64"}
    out = {}
    for body, name in re.findall(r"typedef\s+(?:struct|union)\s*\{(.*?)\}\s*(\w+)\s*;", text, re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"(?:const\s+)?([\w \t]+?)\s*((?:\*\s*)*\w+(?:\[\w+\])?(?:\s*,\s*\**\s*\w+)*)", decl, re.S)
            assert m, (name, decl)
            base = " ".join(m.group(1).split())
            for d in m.group(2).split(","):
                fname, arr = re.fullmatch(r"[\s*]*(\w+)(?:\[(\w+)\])?\s*", d).groups()
                kind = "pointer" if "*" in d else kinds.get(base, base)
                assert kind in kinds.values() or kind == "pointer" or kind in out, (name, decl)
                fields.append((fname, (kind, macros[arr] if arr in macros else int(arr)) if arr else kind))
        out[name] = fields
    return out


def test_ctypes_struct_mirrors_match_the_header():
    from eeg_image_decode_amd import _abi
    hdr = _header_structs()
    classes = [c for c in vars(_abi).values() if isinstance(c, type) and issubclass(c, (ctypes.Structure, ctypes.Union))
               and c not in (ctypes.Structure, ctypes.Union)]
    unnamed = [c.__name__ for c in classes if not hasattr(c, "_c_name_")]
    assert not unnamed, f"ctypes classes without the header's struct name (_c_name_): {unnamed}"
    mirrors = {c._c_name_: c for c in classes}
    assert len(mirrors) == len(classes) and set(mirrors) == set(hdr), sorted(set(mirrors) ^ set(hdr))
    assert issubclass(mirrors["eegclip_plan_arg"], ctypes.Union) and issubclass(mirrors["eegclip_plan_op"], ctypes.Structure)
    scalar = {ctypes.c_void_p: "pointer", ctypes.c_int: "i32", ctypes.c_uint: "u32", ctypes.c_longlong: "i64", ctypes.c_ulonglong: "u64",
              ctypes.c_float: "f32", ctypes.c_double: "f64"}

    def kind(t):
        if t in scalar:
            return scalar[t]
        if issubclass(t, ctypes.Array):
            return (t._type_._c_name_, t._length_)
        return t._c_name_

    for name, cls in mirrors.items():
        ours = [(k[:-1] if k.endswith("_") else k, kind(t)) for k, t in cls._fields_]
        theirs = [(k[:-1] if k.endswith("_") else k, t) for k, t in hdr[name]]
        assert ours == theirs, (name, [(a, b) for a, b in zip(ours, theirs) if a != b], len(ours), len(theirs))
    assert hdr["eegclip_plan_op"][-1] == ("a", ("eegclip_plan_arg", _abi.PLAN_MAX_ARGS))


def test_generated_plan_dispatcher_is_the_committed_one():
    from eeg_image_decode_amd import build
    with open(os.path.join(build.CSRC, "plan_exec_gen.inc")) as f:
        assert f.read() == build.plan_dispatch_text()


def test_parameter_names_carry_the_plan_conventions():
    """what Plan.call(seeded=True) and the plan executor rest on: a dispatchable entry point ends in `stream`, its only unsigned long long is `seed`"""
    from eeg_image_decode_amd import _abi, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    lib = _abi.declare(ctypes.CDLL(build.LIB))
    dispatchable = _abi.plan_functions()
    for name, params in _abi.PARAMS.items():
        assert len(set(params)) == len(params), (name, params)
        assert (lib.eegclip_plan_fn_id(name.encode()) >= 0) == (name in dispatchable) == (params[-1:] == ("stream",)), name
        if name in dispatchable:
            u64 = [p for p, t in zip(params, _abi.PROTOTYPES[name]) if t is ctypes.c_ulonglong]
            assert u64 in ([], ["seed"]), (name, u64)
            assert len(params) - 1 <= _abi.PLAN_MAX_ARGS
        assert ("seed" in params) == (ctypes.c_ulonglong in _abi.PROTOTYPES[name]), name
    assert "eegclip_proj1x1_fwd_rows_planes" in dispatchable and "eegclip_plan_run" not in dispatchable


def test_plan_arguments_by_name():
    from emu_patch import product_on_emulator
    from eeg_image_decode_amd import _abi
    adam = dict(lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.0, step=0, grad_scale=1.0, grad_scale_dev=None)
    with product_on_emulator():
        from eeg_image_decode_amd.plan import Plan
        pl = Plan("by_name", precision=_abi.PREC_F32)
        with pytest.raises(TypeError, match="eegclip_adamw_step_zero_grad.*'nope'"):                 # unknown keyword
            pl.call("eegclip_adamw_step_zero_grad", 1, 2, 3, 4, 5, nope=1, **adam)
        with pytest.raises(TypeError, match="eegclip_adamw_step_zero_grad.*'n'.*twice"):            # positional and keyword
            pl.call("eegclip_adamw_step_zero_grad", 1, 2, 3, 4, 5, n=5, **adam)
        with pytest.raises(TypeError, match="eegclip_adamw_step_zero_grad.*'eps'.*missing"):
            pl.call("eegclip_adamw_step_zero_grad", 1, 2, 3, 4, 5, **{k: v for k, v in adam.items() if k != "eps"})
        with pytest.raises(TypeError, match="eegclip_adamw_step_zero_grad takes 13"):
            pl.call("eegclip_adamw_step_zero_grad", 1, 2, 3, 4, 5)
        with pytest.raises(TypeError, match="eegclip_adamw_step_zero_grad takes 13"):
            pl.call("eegclip_adamw_step_zero_grad", *range(14))
        with pytest.raises(TypeError, match="eegclip_gemm_workspace_bytes"):                         # no stream: not a plan op
            pl.call("eegclip_gemm_workspace_bytes", None)
        assert pl.ops == [] and pl._seed_slots == []
        pl.call("eegclip_adamw_step_zero_grad", 1, 2, 3, 4, 5, **adam)
        pl.call("eegclip_residual_layernorm_fwd_slabs", 1, 2, 3, 0.5, 0, 6, 7, 8, y=0, mean=9, rstd=10, gamma2=None, beta2=None, y2=None, mean2=None,
                rstd2=None, rows=4, cols=8, eps=1e-5, y_hi=None, y_lo=None, nslabs=2, slab_stride=32, x_bias=None, seeded=True)
        pl.call("eegclip_proj1x1_fwd_rows_planes", *([0] * 23), riders=None, n_riders=0, seeded=True)
        assert pl.ops[0][1] == [1, 2, 3, 4, 5, 1e-3, 0.9, 0.99, 1e-8, 0.0, 0, 1.0, None, None] and len(pl.ops[1][1]) == 25
        assert pl._seed_slots == [(1, 4), (2, 19)]                  # (19: the position earlier versions spelled out for this entry point)
        assert pl.arg_index("eegclip_adamw_step_zero_grad", "lr") == pl.arg_index(0, "lr") == 5
        with pytest.raises(KeyError, match="eegclip_adamw_step_zero_grad"):
            pl.set_arg(0, "rows", 1)
        with pytest.raises(KeyError, match="eegclip_adamw_step_zero_grad"):
            pl.arg_index("eegclip_adamw_step_zero_grad", "rows")
        # by name and by number write the same slot, in the op list and -- once the plan is compiled -- in the executor's array
        cases = [(0, "n", 4, "i", 77, 78), (0, "lr", 5, "f", 0.25, 0.5), (0, "g", 1, "p", 4096, 8192), (1, "seed", 4, "u", 2 ** 63 + 5, 2 ** 63 + 6),
                 (1, "rows", 16, "i32", 12, 13), (1, "y", 8, "p", 64, 128)]
        for compiled in (False, True):
            if compiled:
                pl._compile()
            for op, name, j, slot, v1, v2 in cases:
                pl.set_arg(op, name, v1)
                assert pl.ops[op][1][j] == v1 and pl.ops[op][1].count(v1) == 1
                if compiled:
                    assert getattr(pl._c["arr"][op].a[j], slot) == v1
                pl.set_arg(op, j, v2)
                assert pl.ops[op][1][j] == v2
                if compiled:
                    assert getattr(pl._c["arr"][op].a[j], slot) == v2
        pl.close()


def test_no_cpu_fallback():
    from eeg_image_decode_amd._lib import EegclipError
    from eeg_image_decode_amd.atms import ATMS
    from eeg_image_decode_amd.loss import ClipLoss
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    m = ATMS()
    with pytest.raises(EegclipError):
        m(torch.zeros(2, 63, 250), torch.ones(2, dtype=torch.long))
    with pytest.raises(EegclipError):
        ClipLoss()(torch.zeros(4, 8), torch.zeros(4, 8), 1.0)
    with pytest.raises(EegclipError):
        m.encoder(torch.zeros(1))                                    # holders have no eager path


def test_product_never_imports_oracle_or_emulator():
    pkg = os.path.join(ROOT, "eeg_image_decode_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+(oracle|hipemu|tests)\b", src, re.M), f
                assert "/root/reference" not in src, f
