"""The 16-bit host layer of the generation stack: what sdxl.py (processors, stand-in UNet), sdxl_unet.py, clip_text.py and vae.py share.

* thin wrappers over the 16-bit entry points, free functions taking tensors: linear16 / linear (csrc/gemm16.hip, csrc/vae.hip conv16 as a 1 x 1
  convolution), linear16_skinny / decode_attention (csrc/caption.hip), self_attention (csrc/self_attn.hip, head dims 64 and 80), vae_attention (csrc/vae_attn.hip), cross_attention (csrc/cross_attn.hip), layernorm16 / geglu16 / concat16 (csrc/unet.hip),
  act16 / gather_rows16 (csrc/clip_text.hip), patch_rows16 / embed_ln16 (csrc/clip_vision.hip), conv_transpose16 (csrc/convt16.hip).  No library GEMM, no eager fallback: a shape a kernel does not take raises.
* PackedWeights: the one cache of repacked weights and the one statement of its key.
* seeded_parameters: the construction of a module whose nn children hold parameters only and are never called.
* what both UNets do around their attention stacks: image_embeds_of, text_time_embedding, TokenKV.

`lib`, `require_cuda` and `raw_stream` are called as this module's globals: tests/emu_patch.py swaps them to run these wrappers on the lane emulator.
"""
import contextlib
import math
import typing

import torch

from . import _abi
from ._lib import EegclipError, check, lib, raw_stream, require_cuda

_CODES = {torch.float16: _abi.DT_F16, torch.bfloat16: _abi.DT_BF16}


def dtype_code(t):
    """the C ABI's dtype code of a tensor or a torch.dtype"""
    dtype = t.dtype if isinstance(t, torch.Tensor) else t
    code = _CODES.get(dtype) if isinstance(dtype, torch.dtype) else None
    if code is None:
        raise EegclipError(f"the 16-bit kernels run in fp16 or bf16 (the pipeline dtype of the reference: custom_pipeline.py:459, "
                           f"custom_pipeline_low_level.py:576); got {dtype!r}")
    return code


# ---------------------------------------------------------------------------------------------------------------------- kernel wrappers
def linear16(x, weight, bias=None, residual=None, r_div=0):
    """y = x @ weight.T (+ bias) (+ residual) on the 16-bit matrix cores.  x (..., K), weight (N, K) (nn.Linear layout), residual shaped like y,
    or (rows / r_div, N) with r_div > 0 (one row per block of r_div consecutive rows: a per-sample embedding).  N % 128 == 0, K % 64 == 0."""
    require_cuda(x, "x")
    dt = dtype_code(x)
    K = x.shape[-1]
    N = weight.shape[0]
    if weight.shape[1] != K or weight.dtype != x.dtype:
        raise EegclipError(f"linear16: weight {tuple(weight.shape)} {weight.dtype} does not match input (..., {K}) {x.dtype}")
    if N % 128 or K % 64:
        raise EegclipError(f"linear16 takes N % 128 == 0 and K % 64 == 0 (got N = {N}, K = {K}); pad the layer")
    x2 = x.reshape(-1, K)
    if x2.stride(1) != 1 or x2.stride(0) % 8:
        x2 = x2.contiguous()
    w = weight if weight.is_contiguous() else weight.contiguous()
    M = x2.shape[0]
    out = torch.empty(M, N, dtype=x.dtype, device=x.device)
    r2 = None
    if residual is not None:
        r2 = residual.reshape(-1, N)
        if r2.stride(1) != 1 or r2.stride(0) % 4:
            r2 = r2.contiguous()
        if r2.shape[0] != (M if r_div == 0 else (M + r_div - 1) // r_div):
            raise EegclipError("linear16: residual rows do not match")
    b = bias.contiguous() if bias is not None else None
    check(lib().eegclip_gemm16(x2.data_ptr(), x2.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), N, b.data_ptr() if b is not None else None,
                               r2.data_ptr() if r2 is not None else None, r2.stride(0) if r2 is not None else 0, int(r_div), M, N, K, dt, raw_stream()), "gemm16")
    return out.reshape(*x.shape[:-1], N)


def linear(x, weight, bias=None, residual=None):
    """x (M, K) rows -> (M, N) = x W^T + b (+ residual): gemm16 when N % 128 == 0, else conv16 as a 1 x 1 convolution over M pixels (Cout % 64)"""
    N = weight.shape[0]
    if N % 128 == 0:
        return linear16(x, weight, bias, residual)
    M, K = x.shape
    x = x.contiguous()
    out = torch.empty(M, N, dtype=x.dtype, device=x.device)
    r = residual.contiguous() if residual is not None else None
    d = _abi.Conv16Desc(in_=x.data_ptr(), W=weight.data_ptr(), out=out.data_ptr(), bias=bias.data_ptr() if bias is not None else None,
                        residual=r.data_ptr() if r is not None else None, N=1, Hi=M, Wi=1, Cin=K, in_pad=0, Ho=M, Wo=1, Cout=N, out_pad=0, KS=1, stride=1,
                        pad_top=0, pad_left=0, upsample=0, dtype=dtype_code(x))
    check(lib().eegclip_conv16(d, raw_stream()), "conv16 (1 x 1 linear)")
    return out


def cross_attention(q, k, v, heads, k_ip=None, v_ip=None, ip_scale=1.0):
    """softmax(q k^T/8) v + ip_scale * softmax(q k_ip^T/8) v_ip, head_dim 64.  q (B,HW,C); k,v (B,S,C); k_ip,v_ip (B,S_ip,C)."""
    require_cuda(q, "q")
    dt = dtype_code(q)
    B, HW, C = q.shape
    if C != heads * 64:
        raise EegclipError(f"head_dim must be 64 (C={C}, heads={heads})")
    q, k, v = q.contiguous(), k.to(q.dtype).contiguous(), v.to(q.dtype).contiguous()
    S = k.shape[1]
    S_ip = 0
    kp = vp = None
    if k_ip is not None:
        k_ip, v_ip = k_ip.to(q.dtype).contiguous(), v_ip.to(q.dtype).contiguous()
        S_ip = k_ip.shape[1]
        kp, vp = k_ip.data_ptr(), v_ip.data_ptr()
    out = torch.empty_like(q)
    check(lib().eegclip_cross_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), kp, vp, out.data_ptr(), B, HW, heads, 64, S, S_ip,
                                       float(ip_scale), dt, raw_stream()), "cross_attn_fwd")
    return out


def _row_layout(t, name):
    """(B, T, C) view -> (tensor, row stride in elements) as csrc/self_attn.hip addresses it: unit column stride, sample b's rows from b * T * ld.
    Column slices of a fused (B, T, 3C) projection qualify as they are; anything else is made contiguous first."""
    B, T, C = t.shape
    ld = t.stride(1) if T > 1 else (t.stride(0) if B > 1 else C)
    if t.stride(2) != 1 or (B > 1 and t.stride(0) != T * ld) or ld < C or ld % 8 or t.data_ptr() % 16:
        if name == "out":
            raise EegclipError("attention: `out` must be (B, T, C) rows with unit column stride, a row stride that is a multiple of 8 and a "
                               "16-byte aligned base")
        t = t.contiguous()
        ld = C
    return t, ld


def _flash_operands(name, q, k, v, out, check_shapes):
    """what self_attention and vae_attention (`name`, for the messages) do with their tensors ahead of the launch, in the order both always had: q, k, v on
    the GPU in one 16-bit dtype; the caller's own shape rules (`check_shapes()`: rank, head dim, matching and non-empty shapes; it raises); each tensor brought
    to _row_layout; `out`, shaped like q, allocated, or checked against q when given.  Returns (q, ldq, k, ldk, v, ldv, out, ldo)."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        require_cuda(t, n)
    if q.dtype not in _CODES or k.dtype != q.dtype or v.dtype != q.dtype:
        raise EegclipError(f"{name} runs in fp16 or bf16 with one dtype for q, k, v (got {q.dtype}, {k.dtype}, {v.dtype})")
    check_shapes()
    q, ldq = _row_layout(q, "q")
    k, ldk = _row_layout(k, "k")
    v, ldv = _row_layout(v, "v")
    if out is None:
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    elif out.shape != q.shape or out.dtype != q.dtype or out.device != q.device:
        raise EegclipError(f"{name}: out {tuple(out.shape)} {out.dtype} does not match {tuple(q.shape)} {q.dtype}")
    out, ldo = _row_layout(out, "out")
    return q, ldq, k, ldk, v, ldv, out, ldo


def self_attention(q, k, v, heads, scale=None, out=None, causal=False, prefix=None, head_dim=64):
    """softmax(scale * q k^T) v per head of `head_dim` (flash-style: no T x T buffer): 64 or 80, both csrc/self_attn.hip (80: eegclip_attn80_fwd, CLIP ViT-H/14; no
    mask: causal / prefix raise).  q (B, Tq, C), k / v (B, Tk, C), C = heads * head_dim,
    fp16 or bf16; the three may be column slices of one fused (B, T, 3C) projection (consumed in place).  scale defaults to head_dim ** -0.5 (diffusers'
    attn.scale: 1/8 at 64).  causal: key j reaches query i only if j <= i (CLIP's text encoders; Tq == Tk).  prefix (an int in [0, T]; Tq == Tk): key j reaches
    query i iff j < max(i + 1, prefix) (GIT's caption decoder: `prefix` image tokens ahead of causal text).  Returns `out` (B, Tq, C), which may be given."""
    if prefix is not None:
        if causal:
            raise EegclipError("self_attention: give `causal` or `prefix`, not both (prefix=0 is the causal mask)")
        causal = True
    if head_dim not in (64, 80):
        raise EegclipError(f"self_attention: head_dim must be 64 or 80 (got {head_dim})")
    if head_dim == 80 and causal:
        raise EegclipError("self_attention: head_dim 80 has no causal / prefix form")
    def check_shapes():
        if q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
            raise EegclipError("self_attention takes (B, T, C) tensors")
        B, Tq, C = q.shape
        Tk = k.shape[1]
        if C != heads * head_dim:
            raise EegclipError(f"head_dim must be {head_dim} (C={C}, heads={heads})")
        if tuple(k.shape) != (B, Tk, C) or tuple(v.shape) != (B, Tk, C):
            raise EegclipError(f"self_attention: k {tuple(k.shape)} / v {tuple(v.shape)} do not match q {tuple(q.shape)}")
        if B * Tq * Tk == 0:
            raise EegclipError("self_attention: empty input")
        if causal and Tq != Tk:
            raise EegclipError(f"self_attention: the causal form takes Tq == Tk (got {Tq}, {Tk})")
    q, ldq, k, ldk, v, ldv, out, ldo = _flash_operands("self_attention", q, k, v, out, check_shapes)
    (B, Tq, C), Tk = q.shape, k.shape[1]
    scale = 1.0 / math.sqrt(head_dim) if scale is None else float(scale)
    if head_dim == 80:
        check(lib().eegclip_attn80_fwd(q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, out.data_ptr(), ldo, B, Tq, Tk, heads, scale, _CODES[q.dtype],
                                       raw_stream()), "attn80_fwd")
        return out
    if prefix is not None:
        if not 0 <= int(prefix) <= Tk:
            raise EegclipError(f"self_attention: prefix must be in [0, {Tk}]; got {prefix}")
        check(lib().eegclip_self_attn_prefix_fwd(q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, out.data_ptr(), ldo, B, Tq, int(prefix), heads, 64, scale,
                                                 _CODES[q.dtype], raw_stream()), "self_attn_prefix_fwd")
        return out
    fwd = lib().eegclip_self_attn_causal_fwd if causal else lib().eegclip_self_attn_fwd
    check(fwd(q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, out.data_ptr(), ldo, B, Tq, Tk, heads, 64, scale, _CODES[q.dtype], raw_stream()),
          "self_attn_causal_fwd" if causal else "self_attn_fwd")
    return out


def decode_attention(q, cache, Tk, heads, scale=None):
    """one query row per sample against the first Tk rows of a key / value cache (csrc/caption.hip decode_attn16): q (B, C) -- a column slice of a (B, 3C)
    projection qualifies --, cache (B, Tmax, 2C) rows [k | v], C = heads * 64; every key is visible.  Returns (B, C)."""
    require_cuda(q, "q")
    require_cuda(cache, "cache")
    dt = dtype_code(q)
    C = heads * 64
    if q.dim() != 2 or q.shape[1] != C or cache.dim() != 3 or cache.shape[0] != q.shape[0] or cache.shape[2] != 2 * C or cache.dtype != q.dtype:
        raise EegclipError(f"decode_attention: q {tuple(q.shape)} {q.dtype} / cache {tuple(cache.shape)} {cache.dtype} are not (B, {C}) / (B, Tmax, {2 * C})")
    B, Tmax = q.shape[0], cache.shape[1]
    if not 1 <= Tk <= Tmax:
        raise EegclipError(f"decode_attention: Tk must be in [1, {Tmax}]; got {Tk}")
    if q.stride(1) != 1 or cache.stride(2) != 1:
        raise EegclipError("decode_attention: q and cache must have unit column stride")
    out = torch.empty(B, C, dtype=q.dtype, device=q.device)
    scale = 1.0 / math.sqrt(64) if scale is None else float(scale)
    check(lib().eegclip_decode_attn16(q.data_ptr(), q.stride(0) if B > 1 else max(q.stride(0), C), cache.data_ptr(), cache.stride(1),
                                      cache.stride(0) if B > 1 else max(cache.stride(0), Tk * cache.stride(1)), out.data_ptr(), C, B, int(Tk), heads, 64, scale, dt,
                                      raw_stream()), "decode_attn16")
    return out


def linear16_skinny(x, weight, bias=None, residual=None, out=None, out_f32=False):
    """y = x @ weight.T (+ bias) (+ residual) for few rows (csrc/caption.hip gemm16_skinny: the weight is streamed once; 16 rows per launch, more rows
    take one launch per 16).  x (M, K), weight (N, K) with any N, K % 64 == 0; residual (M, N); `out` (M, N) may be given as a view with any row
    stride (a cache row per sample); out_f32: fp32 output (the LM head's logits)."""
    require_cuda(x, "x")
    dt = dtype_code(x)
    if x.dim() != 2 or weight.dim() != 2 or weight.shape[1] != x.shape[1] or weight.dtype != x.dtype:
        raise EegclipError(f"linear16_skinny: weight {tuple(weight.shape)} {weight.dtype} does not match input {tuple(x.shape)} {x.dtype}")
    M, K = x.shape
    N = weight.shape[0]
    if K % 64 or M < 1:
        raise EegclipError(f"linear16_skinny takes K % 64 == 0 and at least one row (got M = {M}, K = {K})")
    if x.stride(1) != 1 or x.stride(0) % 8:
        x = x.contiguous()
    w = weight if weight.is_contiguous() else weight.contiguous()
    odt = torch.float32 if out_f32 else x.dtype
    if out is None:
        out = torch.empty(M, N, dtype=odt, device=x.device)
    elif tuple(out.shape) != (M, N) or out.dtype != odt or out.stride(1) != 1 or out.device != x.device:
        raise EegclipError(f"linear16_skinny: out {tuple(out.shape)} {out.dtype} is not ({M}, {N}) {odt} rows with unit column stride")
    r = None
    if residual is not None:
        r = residual if residual.stride(1) == 1 else residual.contiguous()
        if tuple(r.shape) != (M, N) or r.dtype != x.dtype:
            raise EegclipError("linear16_skinny: residual does not match the output")
    if bias is not None and (bias.dtype != x.dtype or bias.numel() != N):
        raise EegclipError("linear16_skinny: bias does not match the output")
    b = bias.contiguous() if bias is not None else None
    ldc = out.stride(0) if M > 1 else max(out.stride(0), N)
    for m0 in range(0, M, 16):
        mm = min(16, M - m0)
        check(lib().eegclip_gemm16_skinny(x.data_ptr() + 2 * m0 * x.stride(0), max(x.stride(0), K), w.data_ptr(), K, out.data_ptr() + out.element_size() * m0 * ldc,
                                          ldc, b.data_ptr() if b is not None else None, r.data_ptr() + 2 * m0 * r.stride(0) if r is not None else None,
                                          max(r.stride(0), N) if r is not None else 0, mm, N, K, int(out_f32), dt, raw_stream()), "gemm16_skinny")
    return out


def vae_attention(q, k, v, scale=None, out=None):
    """softmax(scale * q k^T) v with ONE head of head_dim = C in {128, 256, 384, 512} (flash-style, csrc/vae_attn.hip: no T x T buffer; the VAE's
    mid-block attention).  q, k, v (B, T, C), fp16 or bf16, any T >= 1; the three may be column slices of one packed (B, T, 3C) projection (consumed
    in place).  scale defaults to 1 / sqrt(C).  Returns `out` (B, T, C), which may be given."""
    def check_shapes():
        if q.dim() != 3 or tuple(k.shape) != tuple(q.shape) or tuple(v.shape) != tuple(q.shape):
            raise EegclipError(f"vae_attention takes three (B, T, C) tensors of one shape (got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)})")
        B, T, C = q.shape
        if C % 128 or not 128 <= C <= 512:
            raise EegclipError(f"vae_attention: head_dim must be 128, 256, 384 or 512 (got {C})")
        if B * T == 0:
            raise EegclipError("vae_attention: empty input")
    q, ldq, k, ldk, v, ldv, out, ldo = _flash_operands("vae_attention", q, k, v, out, check_shapes)
    B, T, C = q.shape
    scale = 1.0 / math.sqrt(C) if scale is None else float(scale)
    check(lib().eegclip_vae_attn_fwd(q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, out.data_ptr(), ldo, B, T, C, scale, _CODES[q.dtype],
                                     raw_stream()), "vae_attn_fwd")
    return out


def layernorm16(x, weight, bias, eps):
    """LayerNorm over the rows of x (M, C)"""
    M, C = x.shape
    y = torch.empty_like(x)
    check(lib().eegclip_layernorm16(x.data_ptr(), x.stride(0), weight.data_ptr(), bias.data_ptr(), y.data_ptr(), C, M, C, float(eps), dtype_code(x),
                                    raw_stream()), "layernorm16")
    return y


def geglu16(f):
    """f (M, 2 D) = [a | g] -> a * gelu_erf(g) (M, D)"""
    M, D2 = f.shape
    y = torch.empty(M, D2 // 2, dtype=f.dtype, device=f.device)
    check(lib().eegclip_geglu16(f.data_ptr(), y.data_ptr(), M, D2 // 2, dtype_code(f), raw_stream()), "geglu16")
    return y


def act16(f, kind):
    """f (M, D) -> act(f) in place; kind: 0 quick_gelu, 1 erf gelu (clip_text.ACT_KINDS)"""
    M, D = f.shape
    check(lib().eegclip_act16(f.data_ptr(), f.stride(0), f.data_ptr(), f.stride(0), M, D, kind, dtype_code(f), raw_stream()), "act16")
    return f


def gather_rows16(table, idx, rows, add=None, add_rows=0):
    """out[r] = table[idx[r]] (+ add[r % add_rows]): the token + position embedding, and the pooling"""
    C = table.shape[1]
    out = torch.empty(rows, C, dtype=table.dtype, device=table.device)
    check(lib().eegclip_gather_rows16(table.data_ptr(), table.shape[0], idx.data_ptr(), 1, add.data_ptr() if add is not None else None, add_rows,
                                      out.data_ptr(), rows, C, dtype_code(table), raw_stream()), "gather_rows16")
    return out


_PIXEL_CODES = {torch.float32: _abi.DT_F32, **_CODES}


def patch_rows16(pixels, patch, dtype, scale=None, shift=None):
    """NCHW pixels (B, 3, H, W) in fp32 / fp16 / bf16 -> the patch convolution's GEMM operand in `dtype`: (B (1 + P), Kpad) rows, Kpad = 3 patch^2 rounded up
    to a multiple of 64; row b (1 + P) is zero (the class slot), row b (1 + P) + 1 + p is patch p in (c, i, j) order, zero-padded (csrc/clip_vision.hip).
    scale / shift: fp32 (3) per channel, both or neither: pixel * scale[c] + shift[c] before the one rounding."""
    require_cuda(pixels, "pixels")
    dt = dtype_code(dtype)
    if pixels.dim() != 4 or pixels.shape[1] != 3 or pixels.dtype not in _PIXEL_CODES or pixels.numel() == 0:
        raise EegclipError(f"patch_rows16 takes (B, 3, H, W) pixels in fp32, fp16 or bf16; got {tuple(pixels.shape)} {pixels.dtype}")
    B, _, H, W = pixels.shape
    if patch < 1 or H % patch or W % patch:
        raise EegclipError(f"patch_rows16: the image ({H} x {W}) is not a whole number of {patch} x {patch} patches")
    if (scale is None) != (shift is None):
        raise EegclipError("patch_rows16 takes scale and shift together")
    for v, n in ((scale, "scale"), (shift, "shift")):
        if v is not None and (v.dtype != torch.float32 or v.numel() != 3 or not v.is_contiguous() or v.device != pixels.device):
            raise EegclipError(f"patch_rows16: {n} must be a contiguous fp32 vector of 3 on the pixels' device")
    pixels = pixels.contiguous()
    kpad = (3 * patch * patch + 63) // 64 * 64
    out = torch.empty(B * (1 + (H // patch) * (W // patch)), kpad, dtype=dtype, device=pixels.device)
    check(lib().eegclip_patch_rows16(pixels.data_ptr(), _PIXEL_CODES[pixels.dtype], scale.data_ptr() if scale is not None else None,
                                     shift.data_ptr() if shift is not None else None, out.data_ptr(), B, H, W, int(patch), dt, raw_stream()), "patch_rows16")
    return out


def embed_ln16(x, pos, weight, bias, eps):
    """LayerNorm(x[r] + pos[r % T]) over the rows of x (M, C), pos (T, C) (csrc/clip_vision.hip: the position embedding and pre_layrnorm in one pass)"""
    require_cuda(x, "x")
    dt = dtype_code(x)
    if x.dim() != 2 or x.shape[0] == 0:
        raise EegclipError(f"embed_ln16 takes (M, C) rows; got {tuple(x.shape)}")
    M, C = x.shape
    if x.stride(1) != 1 or x.stride(0) % 8:
        x = x.contiguous()
    if pos.dim() != 2 or pos.shape[1] != C or pos.dtype != x.dtype or not pos.is_contiguous() or pos.device != x.device:
        raise EegclipError(f"embed_ln16: pos {tuple(pos.shape)} {pos.dtype} does not match rows of {C} {x.dtype}")
    for v, n in ((weight, "weight"), (bias, "bias")):
        if v.dtype != x.dtype or v.numel() != C or not v.is_contiguous() or v.device != x.device:
            raise EegclipError(f"embed_ln16: {n} must be a contiguous vector of {C} {x.dtype} on the rows' device")
    y = torch.empty(M, C, dtype=x.dtype, device=x.device)
    check(lib().eegclip_embed_ln16(x.data_ptr(), max(x.stride(0), C), pos.data_ptr(), pos.shape[0], weight.data_ptr(), bias.data_ptr(), y.data_ptr(), C, M, C,
                                   float(eps), dt, raw_stream()), "embed_ln16")
    return y


def concat16(a, b, out):
    """padded NHWC frames a (N, H + 2, W + 2, Ca), b (.., Cb) -> the caller's frame `out` (.., Ca + Cb): the skip concatenation"""
    N, Hp, Wp, Ca = a.shape
    check(lib().eegclip_concat16(a.data_ptr(), b.data_ptr(), out.data_ptr(), N, Hp - 2, Wp - 2, 1, Ca, b.shape[3], 1, dtype_code(a), raw_stream()), "concat16")
    return out


_CONVT_K = ((1, 3), (2, 0))     # [phase half][tap half] -> index into the 4-wide kernel along that axis (include/eegclip.h, eegclip_convt16)


def pack_conv_transpose16(weight):
    """nn.ConvTranspose2d(.., 4, 2, 1)'s weight (Cin, Cout, 4, 4) -> the kernel's [phase 2 py + px][Cout][tap 2 ty + tx][Cin] (K contiguous)"""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (4, 4):
        raise EegclipError(f"pack_conv_transpose16 takes a (Cin, Cout, 4, 4) weight; got {tuple(weight.shape)}")
    w = weight.detach()
    return torch.stack([torch.stack([w[:, :, _CONVT_K[py][ty], _CONVT_K[px][tx]].t() for ty in (0, 1) for tx in (0, 1)], dim=1)
                        for py in (0, 1) for px in (0, 1)], dim=0).contiguous()


def conv_transpose_live_taps(Hi, Wi):
    """eegclip_convt16's tap_mask without the taps whose source is in the zero border for every pixel: the neighbour row when Hi == 1, the neighbour column
    when Wi == 1 (at 1 x 1 three of four taps, and their weights, are never read)"""
    nib = sum(1 << t for t in range(4) if not ((t >> 1) and Hi == 1) and not ((t & 1) and Wi == 1))
    return nib * 0x1111


def conv_transpose16(x_frame, packed_w, scale=None, shift=None, relu=False, out=None):
    """ConvTranspose2d(kernel 4, stride 2, padding 1) + y * scale[co] + shift[co] (+ ReLU) on csrc/convt16.hip.  x_frame: padded NHWC (N, Hi + 2, Wi + 2, Cin)
    with a zero border; packed_w: pack_conv_transpose16's (4, Cout, 4, Cin); scale / shift: fp32 (Cout) or None (1 / 0).  Cout % 16 == 0: returns the padded
    NHWC frame (N, 2 Hi + 2, 2 Wi + 2, Cout) of the next layer (`out`, if given, must already have a zero border: only its interior is written);
    Cout < 16: returns unpadded NCHW (N, Cout, 2 Hi, 2 Wi)."""
    require_cuda(x_frame, "x_frame")
    dt = dtype_code(x_frame)
    if x_frame.dim() != 4 or packed_w.dim() != 4 or packed_w.shape[0] != 4 or packed_w.shape[2] != 4 or packed_w.shape[3] != x_frame.shape[3] or \
            packed_w.dtype != x_frame.dtype or min(x_frame.shape[1:3]) < 3:
        raise EegclipError(f"conv_transpose16: frame {tuple(x_frame.shape)} {x_frame.dtype} / packed weight {tuple(packed_w.shape)} {packed_w.dtype} do not match "
                           f"(N, Hi + 2, Wi + 2, Cin) / (4, Cout, 4, Cin)")
    N, Hi, Wi, Cin = x_frame.shape[0], x_frame.shape[1] - 2, x_frame.shape[2] - 2, x_frame.shape[3]
    Cout = packed_w.shape[1]
    x_frame, packed_w = x_frame.contiguous(), packed_w.contiguous()
    shape = (N, 2 * Hi + 2, 2 * Wi + 2, Cout) if Cout >= 16 else (N, Cout, 2 * Hi, 2 * Wi)
    if out is None:
        out = (torch.zeros if Cout >= 16 else torch.empty)(shape, dtype=x_frame.dtype, device=x_frame.device)
    elif tuple(out.shape) != shape or out.dtype != x_frame.dtype or out.device != x_frame.device or not out.is_contiguous():
        raise EegclipError(f"conv_transpose16: out {tuple(out.shape)} {out.dtype} is not a contiguous {shape} {x_frame.dtype}")
    for v, n in ((scale, "scale"), (shift, "shift")):
        if v is not None and (v.dtype != torch.float32 or v.numel() != Cout or not v.is_contiguous() or v.device != x_frame.device):
            raise EegclipError(f"conv_transpose16: {n} must be a contiguous fp32 vector of {Cout} on the input's device")
    d = _abi.Convt16Desc(in_=x_frame.data_ptr(), W=packed_w.data_ptr(), out=out.data_ptr(), scale=scale.data_ptr() if scale is not None else None,
                         shift=shift.data_ptr() if shift is not None else None, N=N, Hi=Hi, Wi=Wi, Cin=Cin, Ho=2 * Hi, Wo=2 * Wi, Cout=Cout, KS=4, stride=2, pad=1,
                         relu=int(bool(relu)), tap_mask=conv_transpose_live_taps(Hi, Wi), dtype=dt)
    check(lib().eegclip_convt16(d, raw_stream()), "convt16")
    return out


# ---------------------------------------------------------------------------------------------------------------------- modules and their weights
class PackedWeights:
    """Repacked weights (concatenated q | k | v, stacked time_emb_proj, convolution weights in the kernel's order), made once per state of the
    parameters they come from.  The key is (id, _version, data_ptr) per parameter: identity and version catch load_state_dict and in-place edits, the
    address a `.data =` swap (same object, same version).  The entry holds the parameters themselves, so their ids cannot be recycled for other
    tensors while it lives.  None entries (optional biases) are part of the key."""

    def __init__(self):
        self._entries = {}

    @staticmethod
    def key(params):
        return tuple((id(p), p._version, p.data_ptr()) if p is not None else None for p in params)

    def get(self, tag, params, make):
        key = self.key(params)
        hit = self._entries.get(tag)
        if hit is None or hit[0] != key:
            hit = self._entries[tag] = (key, params, make())
        return hit[2]


@contextlib.contextmanager
def seeded_parameters(module, dtype, device=None, seed=0):
    """Build `module`'s children inside the block: PyTorch's default initialisation under `seed` on `device` (the caller's RNG streams are left as they
    were); afterwards the module is cast to `dtype` (fp16 / bf16) and frozen.  For modules whose nn children hold parameters only."""
    dtype_code(dtype)
    dev = torch.device(device) if device is not None else torch.device("cpu")
    rng_devs = [dev.index if dev.index is not None else torch.cuda.current_device()] if dev.type == "cuda" else []
    with torch.random.fork_rng(devices=rng_devs), dev:
        torch.manual_seed(seed)
        yield
    module.to(dtype)
    for p in module.parameters():
        p.requires_grad_(False)


# ---------------------------------------------------------------------------------------------------------------------- shared by the two UNets
def _sinusoid(t, dim, flip_sin_to_cos=True):
    """diffusers Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin] of t * exp(-ln(1e4) i / (dim/2))"""
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32, device=t.device) / half)
    arg = t.float()[..., None] * freqs
    return torch.cat([arg.cos(), arg.sin()] if flip_sin_to_cos else [arg.sin(), arg.cos()], dim=-1)


def image_embeds_of(added_cond_kwargs):
    """added_cond_kwargs["image_embeds"] as (B, dim) or None: diffusers passes a list of (B, n_images, dim) tensors, one per adapter"""
    e = (added_cond_kwargs or {}).get("image_embeds")
    if isinstance(e, (list, tuple)):
        e = e[0]
    return e[:, 0] if e is not None and e.dim() == 3 else e


def text_time_embedding(timestep, B, added, time_mlp, add_mlp, time_dim, add_dim, dtype, device):
    """silu(time_embedding(Timesteps(time_dim)(t)) + add_embedding(cat(text_embeds, Timesteps(add_dim)(time_ids)))): (B, 4 C0), what every time
    projection reads (addition_embed_type "text_time").  time_mlp / add_mlp: (w1, b1, w2, b2) of linear_1, SiLU, linear_2; the biases may be None."""
    if added is None or "text_embeds" not in added or "time_ids" not in added:
        raise EegclipError("the UNet needs added_cond_kwargs with 'text_embeds' and 'time_ids' (addition_embed_type 'text_time')")
    silu = torch.nn.functional.silu
    t = torch.as_tensor(timestep, device=device).reshape(-1).float().expand(B)
    w1, b1, w2, b2 = time_mlp
    e = linear16(silu(linear16(_sinusoid(t, time_dim).to(dtype), w1, b1)), w2, b2)
    text_embeds = added["text_embeds"].to(device=device, dtype=dtype)
    time_ids = added["time_ids"].to(device=device)
    aug = torch.cat([text_embeds, _sinusoid(time_ids.flatten(), add_dim).reshape(B, -1).to(dtype)], dim=-1)          # (B, 1280 + 6 * 256) in SDXL
    w1, b1, w2, b2 = add_mlp
    if aug.shape[1] != w1.shape[1]:
        raise EegclipError(f"text_embeds + time_ids give {aug.shape[1]} features; add_embedding takes {w1.shape[1]}")
    return silu(e + linear16(silu(linear16(aug, w1, b1)), w2, b2))


class TokenKV(typing.NamedTuple):
    """K / V of the text tokens (and of the IP-Adapter's image tokens) at every cross-attention position: they do not change between denoising steps, so
    they are projected once per sampling run.  `entries` is the list of (k, v, k_ip, v_ip) per position.  A hit needs THE SAME two token tensors
    (identity and _version; the entry holds them, so an address recycled by the allocator cannot match) and an equal `extra` (the caller's: batch
    size, key of the projection weights).  A UNet's `_kv` is one of these, or None before the first projection."""
    text: torch.Tensor
    text_version: int
    image: typing.Optional[torch.Tensor]
    image_version: typing.Optional[int]
    extra: object
    entries: list

    @classmethod
    def project(cls, text_src, image_src, extra, text, ip, weights):
        """weights: (to_k, to_v, to_k_ip, to_v_ip) per position; text (B, S, X) / ip (B, S_ip, X) or None: the token matrices of the two sources"""
        entries = [(linear16(text, wk), linear16(text, wv)) + ((linear16(ip, wki), linear16(ip, wvi)) if ip is not None else (None, None))
                   for wk, wv, wki, wvi in weights]
        return cls(text_src, text_src._version, image_src, None if image_src is None else image_src._version, extra, entries)

    def hit(self, text_src, image_src, extra):
        return self.text is text_src and self.text_version == text_src._version and self.image is image_src and \
            self.image_version == (None if image_src is None else image_src._version) and self.extra == extra
