"""ctypes mirror of include/eegclip.h (struct layouts + prototypes).  Pure declarations, no compute."""
import ctypes as C
import keyword
import os
import re

BIG = 1 << 62


class Dim(C.Structure):
    _c_name_ = "eegclip_dim"
    _fields_ = [("div", C.c_longlong), ("so", C.c_longlong), ("si", C.c_longlong)]


def dim(si, div=BIG, so=0):
    """offset(i) = (i // div) * so + (i % div) * si   (plain stride when div is omitted)."""
    return Dim(int(div), int(so), int(si))


class GemmDesc(C.Structure):
    _c_name_ = "eegclip_gemm_desc"
    _fields_ = [
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("A", C.c_void_p), ("Am", Dim), ("Ak", Dim),
        ("B", C.c_void_p), ("Bk", Dim), ("Bn", Dim),
        ("C", C.c_void_p), ("Cm", Dim), ("Cn", Dim),
        ("Cpre", C.c_void_p),
        ("bias_n", C.c_void_p), ("bias_m", C.c_void_p),
        ("R", C.c_void_p), ("Rm", Dim), ("Rn", Dim),
        ("alpha", C.c_float), ("accumulate", C.c_int), ("act", C.c_int),
        ("drop_p", C.c_float), ("seed", C.c_ulonglong), ("drop_site", C.c_uint),
        ("split_k", C.c_int),
        ("rowsum_a", C.c_void_p),
        ("precision", C.c_int),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_longlong),
    ]


class SplitItem(C.Structure):
    _c_name_ = "eegclip_split_item"
    _fields_ = [("src", C.c_void_p), ("hi", C.c_void_p), ("lo", C.c_void_p), ("rows", C.c_int), ("cols", C.c_int), ("ld_src", C.c_longlong),
                ("ld_out", C.c_longlong), ("transpose", C.c_int), ("copy", C.c_void_p), ("ld_copy", C.c_longlong)]


class InfonceProblem(C.Structure):
    _c_name_ = "eegclip_infonce_problem"
    _fields_ = [("q_hi", C.c_void_p), ("q_lo", C.c_void_p), ("k_hi", C.c_void_p), ("k_lo", C.c_void_p), ("col0", C.c_int), ("weight", C.c_float),
                ("part", C.c_void_p), ("diag", C.c_void_p), ("lse", C.c_void_p), ("lse_k", C.c_void_p), ("G", C.c_void_p), ("ldg", C.c_longlong),
                ("part_k", C.c_void_p), ("diag_k", C.c_void_p), ("G_hi", C.c_void_p), ("G_lo", C.c_void_p)]


class TokenBlockDesc(C.Structure):
    _c_name_ = "eegclip_token_block_desc"
    _fields_ = ([("B", C.c_int), ("x", C.c_void_p), ("packed", C.c_void_p), ("bv", C.c_void_p), ("pe", C.c_void_p), ("tokens", C.c_void_p), ("ids", C.c_void_p)]
                + [(k, C.c_void_p) for k in ("bqkv", "bo", "ln1_g", "ln1_b", "b1", "b2", "ln2_g", "ln2_b", "ln3_g", "ln3_b")]
                + [(k, C.c_void_p) for k in ("h", "qkv", "r1", "mu1", "rs1", "f1", "r2", "n2", "mu2", "rs2", "n3", "mu3", "rs3")]
                + [(k, C.c_void_p) for k in ("xp", "hp", "ctxp", "n1p", "g1p")]
                + [("drop_p", C.c_float), ("eps", C.c_float), ("scale", C.c_float), ("seed", C.c_ulonglong)]
                + [(k, C.c_uint) for k in ("site_embed", "site_attn", "site_attn_out", "site_ffn_act", "site_ffn_out")]
                + [("packed_embed", C.c_void_p), ("embed_subject", C.c_void_p), ("bv_stride", C.c_longlong)]
                + [("cs_w25", C.c_void_p), ("cs_bias", C.c_void_p), ("cs_rows", C.c_void_p), ("cs_H", C.c_int)])


class TokenBlockBwdDesc(C.Structure):
    _c_name_ = "eegclip_token_block_bwd_desc"
    _fields_ = ([("B", C.c_int), ("packed", C.c_void_p)]
                + [(k, C.c_void_p) for k in ("dn3", "n2", "r2", "r1", "f1", "mu1", "rs1", "mu2", "rs2", "mu3", "rs3", "ln1_g", "ln2_g", "ln2_b", "ln3_g")]
                + [(k, C.c_void_p) for k in ("dr1", "dctx", "partials", "df2p", "dg1p", "da1p", "dr1p", "dqkvp")]
                + [(k, C.c_void_p) for k in ("dln3_g", "dln3_b", "dln2_g", "dln2_b", "dln1_g", "dln1_b")]
                + [("drop_p", C.c_float), ("seed", C.c_ulonglong)]
                + [(k, C.c_uint) for k in ("site_embed", "site_attn_out", "site_ffn_act", "site_ffn_out")])


class GemmPlanesDesc(C.Structure):
    _c_name_ = "eegclip_gemm_planes_desc"
    _fields_ = [("a_hi", C.c_void_p), ("a_lo", C.c_void_p), ("b_hi", C.c_void_p), ("b_lo", C.c_void_p), ("lda", C.c_longlong), ("ldb", C.c_longlong),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("C", C.c_void_p), ("ldc", C.c_longlong), ("Cpre", C.c_void_p), ("ldcpre", C.c_longlong),
                ("bias", C.c_void_p), ("R", C.c_void_p), ("ldr", C.c_longlong), ("p_hi", C.c_void_p), ("p_lo", C.c_void_p), ("ldp", C.c_longlong),
                ("act", C.c_int), ("accumulate", C.c_int), ("planes_of", C.c_int)]


class HeadGemmDesc(C.Structure):
    _c_name_ = "eegclip_head_gemm_desc"
    _fields_ = [("a_hi", C.c_void_p), ("a_lo", C.c_void_p), ("b_hi", C.c_void_p), ("b_lo", C.c_void_p), ("lda", C.c_longlong), ("ldb", C.c_longlong),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("slices", C.c_int), ("slab_stride", C.c_longlong), ("bias", C.c_void_p),
                ("Cpre", C.c_void_p), ("ldcpre", C.c_longlong), ("act", C.c_int), ("aux", C.c_void_p), ("ldaux", C.c_longlong), ("R", C.c_void_p),
                ("ldr", C.c_longlong), ("C", C.c_void_p), ("ldc", C.c_longlong), ("p_hi", C.c_void_p), ("p_lo", C.c_void_p), ("ldp", C.c_longlong),
                ("b_kmajor", C.c_int)]


class Conv16Desc(C.Structure):
    _c_name_ = "eegclip_conv16_desc"
    _fields_ = [("in_", C.c_void_p), ("W", C.c_void_p), ("out", C.c_void_p), ("bias", C.c_void_p), ("residual", C.c_void_p),
                ("N", C.c_int), ("Hi", C.c_int), ("Wi", C.c_int), ("Cin", C.c_int), ("in_pad", C.c_int),
                ("Ho", C.c_int), ("Wo", C.c_int), ("Cout", C.c_int), ("out_pad", C.c_int),
                ("KS", C.c_int), ("stride", C.c_int), ("pad_top", C.c_int), ("pad_left", C.c_int), ("upsample", C.c_int), ("dtype", C.c_int),
                ("chan_bias", C.c_void_p)]


class ConvRelu16Desc(C.Structure):
    _c_name_ = "eegclip_convrelu16_desc"
    _fields_ = [("in_", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
                ("N", C.c_int), ("Hi", C.c_int), ("Wi", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int),
                ("KS", C.c_int), ("stride", C.c_int), ("pad", C.c_int), ("out_pad", C.c_int), ("dtype", C.c_int)]


class ConvBn16Desc(C.Structure):
    _c_name_ = "eegclip_convbn16_desc"
    _fields_ = [("in_", C.c_void_p), ("W", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p), ("residual", C.c_void_p), ("out", C.c_void_p),
                ("N", C.c_int), ("Hi", C.c_int), ("Wi", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int),
                ("KS", C.c_int), ("stride", C.c_int), ("pad", C.c_int), ("out_pad", C.c_int), ("relu", C.c_int), ("dtype", C.c_int)]


class ConvBnAct16Desc(C.Structure):
    _c_name_ = "eegclip_convbnact16_desc"
    _fields_ = [("in_", C.c_void_p), ("W", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p), ("residual", C.c_void_p), ("out", C.c_void_p),
                ("N", C.c_int), ("Hi", C.c_int), ("Wi", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int),
                ("KS", C.c_int), ("stride", C.c_int), ("pad", C.c_int), ("in_pad", C.c_int), ("out_pad", C.c_int), ("act", C.c_int), ("dtype", C.c_int)]


class ConvBnCat16Desc(C.Structure):
    _c_name_ = "eegclip_convbncat16_desc"
    _fields_ = [("in_", C.c_void_p), ("W", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p), ("out", C.c_void_p),
                ("N", C.c_int), ("Hi", C.c_int), ("Wi", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int),
                ("KH", C.c_int), ("KW", C.c_int), ("stride", C.c_int), ("pad_h", C.c_int), ("pad_w", C.c_int), ("in_pad", C.c_int),
                ("out_pad", C.c_int), ("out_stride", C.c_int), ("out_c0", C.c_int), ("relu", C.c_int), ("dtype", C.c_int)]


class Convt16Desc(C.Structure):
    _c_name_ = "eegclip_convt16_desc"
    _fields_ = [("in_", C.c_void_p), ("W", C.c_void_p), ("out", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p),
                ("N", C.c_int), ("Hi", C.c_int), ("Wi", C.c_int), ("Cin", C.c_int), ("Ho", C.c_int), ("Wo", C.c_int), ("Cout", C.c_int),
                ("KS", C.c_int), ("stride", C.c_int), ("pad", C.c_int), ("relu", C.c_int), ("tap_mask", C.c_int), ("dtype", C.c_int)]


class Convt16BwdDataDesc(C.Structure):
    _c_name_ = "eegclip_convt16_bwd_data_desc"
    _fields_ = [("dz", C.c_void_p), ("W", C.c_void_p), ("dx", C.c_void_p), ("N", C.c_int), ("Hi", C.c_int), ("Wi", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int),
                ("tap_mask", C.c_int), ("dtype", C.c_int)]


class Convt16BwdWeightDesc(C.Structure):
    _c_name_ = "eegclip_convt16_bwd_weight_desc"
    _fields_ = [("x", C.c_void_p), ("dz", C.c_void_p), ("dW", C.c_void_p), ("db", C.c_void_p), ("workspace", C.c_void_p), ("workspace_floats", C.c_longlong),
                ("N", C.c_int), ("Hi", C.c_int), ("Wi", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("slabs", C.c_int), ("loss_scale", C.c_float),
                ("dtype", C.c_int)]


class Bn2d16FwdDesc(C.Structure):
    _c_name_ = "eegclip_bn2d16_fwd_desc"
    _fields_ = [("z", C.c_void_p), ("a", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p),
                ("running_mean", C.c_void_p), ("running_var", C.c_void_p), ("workspace", C.c_void_p), ("workspace_floats", C.c_longlong), ("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int),
                ("eps", C.c_float), ("momentum", C.c_float), ("dtype", C.c_int)]


class Bn2d16BwdDesc(C.Structure):
    _c_name_ = "eegclip_bn2d16_bwd_desc"
    _fields_ = [("da", C.c_void_p), ("a", C.c_void_p), ("z", C.c_void_p), ("gamma", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p), ("dgamma", C.c_void_p),
                ("dbeta", C.c_void_p), ("dz", C.c_void_p), ("workspace", C.c_void_p), ("workspace_floats", C.c_longlong), ("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int),
                ("loss_scale", C.c_float), ("dtype", C.c_int)]


class WgradTokProblem(C.Structure):
    _c_name_ = "eegclip_wgrad_tok_problem"
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("a_group_stride", C.c_longlong), ("m_groups", C.c_int), ("heads_m", C.c_int), ("heads_n", C.c_int),
                ("M", C.c_int), ("N", C.c_int), ("out", C.c_void_p), ("ldo", C.c_longlong), ("bias_out", C.c_void_p), ("bias_mfma", C.c_int),
                ("sample0", C.c_int), ("samples", C.c_int), ("sample_index", C.c_void_p)]


class CstackFwdDesc(C.Structure):
    _c_name_ = "eegclip_cstack_fwd_desc"
    _fields_ = [("B", C.c_int), ("H", C.c_int), ("x", C.c_void_p), ("xs_b", C.c_longlong), ("xs_h", C.c_longlong), ("w25", C.c_void_p), ("bias1", C.c_void_p),
                ("stat1", C.c_void_p), ("nstat1", C.c_int), ("count1", C.c_double), ("eps", C.c_float), ("momentum", C.c_float),
                ("gamma1", C.c_void_p), ("beta1", C.c_void_p), ("mean1", C.c_void_p), ("rstd1", C.c_void_p), ("run_mean1", C.c_void_p),
                ("run_var1", C.c_void_p), ("nbt1", C.c_void_p), ("packed", C.c_void_p), ("bias2", C.c_void_p), ("y2", C.c_void_p), ("stat2", C.c_void_p)]


class CstackBwdDesc(C.Structure):
    _c_name_ = "eegclip_cstack_bwd_desc"
    _fields_ = [("B", C.c_int), ("H", C.c_int), ("x", C.c_void_p), ("xs_b", C.c_longlong), ("xs_h", C.c_longlong), ("w25", C.c_void_p), ("bias1", C.c_void_p),
                ("mean1", C.c_void_p), ("rstd1", C.c_void_p), ("gamma1", C.c_void_p), ("beta1", C.c_void_p), ("packed_t", C.c_void_p), ("dy2", C.c_void_p),
                ("rows_out", C.c_void_p), ("stat", C.c_void_p), ("nstat", C.c_int), ("count", C.c_double), ("stat_local", C.c_void_p),
                ("nstat_local", C.c_int), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("dx", C.c_void_p), ("dw_partials", C.c_void_p), ("dw25", C.c_void_p)]


class WgradPlanesProblem(C.Structure):
    _c_name_ = "eegclip_wgrad_planes_problem"
    _fields_ = [("a_hi", C.c_void_p), ("a_lo", C.c_void_p), ("lda", C.c_longlong), ("b_hi", C.c_void_p), ("b_lo", C.c_void_p), ("ldb", C.c_longlong),
                ("rows", C.c_int), ("M", C.c_int), ("N", C.c_int), ("out", C.c_void_p), ("ldo", C.c_longlong), ("bias_out", C.c_void_p), ("slices", C.c_int)]


PLAN_MAX_ARGS = 28
PLAN_MEMSET, PLAN_JOIN, PLAN_SIDE, PLAN_SKIP, PLAN_SIDE2 = -2, -3, 1, 2, 4


class PlanArg(C.Union):
    _c_name_ = "eegclip_plan_arg"
    _fields_ = [("p", C.c_void_p), ("i", C.c_longlong), ("u", C.c_ulonglong), ("d", C.c_double), ("f", C.c_float), ("i32", C.c_int), ("u32", C.c_uint)]


class PlanOp(C.Structure):
    _c_name_ = "eegclip_plan_op"
    _fields_ = [("fn", C.c_int), ("flags", C.c_int), ("a", PlanArg * PLAN_MAX_ARGS)]


ACT_NONE, ACT_GELU, ACT_SILU, ACT_GELU_GRAD = 0, 1, 2, 3
PREC_F32, PREC_BF16X3 = 0, 1
ABI_VERSION = 26
DT_BF16, DT_F16, DT_F32 = 0, 1, 2
SRC_U8_HWC, RESIZE_BILINEAR, RESIZE_BICUBIC = 3, 2, 3
SSIM_TILE_H, SSIM_TILE_W = 32, 32

# ---- prototypes: read from include/eegclip.h, the single description of the entry points
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eegclip.h")
SCALARS = {"int": C.c_int, "unsigned int": C.c_uint, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "float": C.c_float,
           "double": C.c_double}


def header_text():
    """include/eegclip.h without its comments"""
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)


def _parse_prototypes(text):
    """every `<ret> eegclip_name(<params>);` -> argument ctypes, parameter names, return ctypes.  A pointer to a struct mirrored above is POINTER(its class)
    (takes the struct itself, byref(), an array of it, None -- and refuses another struct); any other pointer is c_void_p (byref(), ctypes arrays, ints,
    bytes, None).  A declaration that does not map raises: nothing is skipped."""
    protos, params, restypes = {}, {}, {}
    structs = {c._c_name_: C.POINTER(c) for c in globals().values() if isinstance(c, type) and issubclass(c, C.Structure) and hasattr(c, "_c_name_")}
    for ret, name, plist in re.findall(r"([\w \t*]+?)\b(eegclip_\w+)\s*\(([^()]*)\)\s*;", text):
        ret = " ".join(ret.replace("*", " * ").split())
        if ret not in SCALARS and ret != "void *":
            raise TypeError(f"{name}: return type {ret!r} is not int | long long | float | void*")
        types, names = [], []
        for p in ([] if plist.strip() == "void" else plist.split(",")):
            m = re.fullmatch(r"\s*(?:const\s+)?([\w \t]+?)\s*((?:\*\s*(?:const\s*)?)*)(\w+)\s*", p)
            base, stars = (" ".join(m.group(1).split()), m.group(2).count("*")) if m else (None, 0)
            ctype = (structs.get(base, C.c_void_p) if stars == 1 else C.c_void_p) if stars else SCALARS.get(base)
            if not ctype:
                raise TypeError(f"{name}: cannot map parameter {p.strip()!r}")
            types.append(ctype)
            names.append(m.group(3) + "_" * keyword.iskeyword(m.group(3)))
        protos[name], params[name], restypes[name] = types, tuple(names), SCALARS.get(ret, C.c_void_p)
    missed = set(re.findall(r"\b(eegclip_\w+)\s*\(", text)) - set(protos)
    if missed:
        raise TypeError(f"include/eegclip.h: cannot parse the declaration of {sorted(missed)}")
    return protos, params, restypes


# name -> argument ctypes | parameter names (a Python keyword gets a trailing underscore: eegclip_maxpool16's `in_`) | return ctypes
PROTOTYPES, PARAMS, RESTYPES = _parse_prototypes(header_text())
ARG_INDEX = {name: {p: i for i, p in enumerate(names)} for name, names in PARAMS.items()}


def plan_params(name):
    """parameter names of a dispatchable entry point, f(..., void* stream), WITHOUT the trailing stream, which the executor supplies"""
    if PARAMS.get(name, ())[-1:] != ("stream",):
        raise TypeError(f"{name} is not an entry point that ends in `void* stream`")
    return PARAMS[name][:-1]


def plan_functions():
    """entry points the plan executor can dispatch: name -> argument ctypes WITHOUT the trailing stream"""
    return {n: a[:-1] for n, a in PROTOTYPES.items() if PARAMS[n][-1:] == ("stream",)}


def plan_slot(t):
    """PlanArg field for a ctypes parameter type"""
    return {C.c_int: "i32", C.c_uint: "u32", C.c_longlong: "i", C.c_ulonglong: "u", C.c_float: "f", C.c_double: "d"}.get(t, "p")


def declare(lib):
    """Attach prototypes; raises AttributeError if the library lacks a symbol the header declares."""
    for name, args in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = RESTYPES[name]
        fn.argtypes = args
    return lib
