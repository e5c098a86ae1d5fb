"""Checked Python entry points over the libvmc C ABI (include/vmc.h).

PyTorch is used for device memory and streams only: every function here enqueues HIP kernels on the
current stream and returns tensors allocated by the caching allocator.  No function has a PyTorch
compute fallback.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import ACT_GELU_ERF, ACT_NONE, ACT_QUICKGELU, ACT_RELU, F32, check, dt, lib, ptr, stream  # noqa: F401


def _kpad(k: int) -> int:
    return (k + 63) // 64 * 64


def cast_weight(w: torch.Tensor, dtype16: torch.dtype, transposed: bool = False, pad_k: bool = False):
    """fp32 [rows, cols] parameter -> 16-bit compute copy (optionally the transposed copy instead).
    pad_k pads the K (= last) dimension of the copy with zeros up to a multiple of 64."""
    w2 = w.detach().reshape(w.shape[0], -1)
    if w2.dtype != torch.float32 or not w2.is_contiguous():
        w2 = w2.float().contiguous()
    rows, cols = w2.shape
    if transposed:
        ld = _kpad(rows) if pad_k else rows
        out = (torch.zeros if ld != rows else torch.empty)((cols, ld), dtype=dtype16, device=w.device)
        check(lib.vmc_cast_weight(ptr(w2), None, ptr(out), rows, cols, 0, ld, dt(dtype16), stream()), "cast_weight")
    else:
        ld = _kpad(cols) if pad_k else cols
        out = (torch.zeros if ld != cols else torch.empty)((rows, ld), dtype=dtype16, device=w.device)
        check(lib.vmc_cast_weight(ptr(w2), ptr(out), None, rows, cols, ld, 0, dt(dtype16), stream()), "cast_weight")
    return out


def cast_weight_both(w: torch.Tensor, dtype16: torch.dtype):
    """One launch for both 16-bit copies a training step needs: [rows, cols(+pad to 64)] for the forward and the
    transposed [cols, rows(+pad to 64)] for the dgrad (K padding only where the contraction length is not a multiple of 64)."""
    w2 = w.detach().reshape(w.shape[0], -1)
    if w2.dtype != torch.float32 or not w2.is_contiguous():
        w2 = w2.float().contiguous()
    rows, cols = w2.shape
    ld = _kpad(cols) if cols % 64 else cols
    ldt = _kpad(rows) if rows % 64 else rows
    out = (torch.zeros if ld != cols else torch.empty)((rows, ld), dtype=dtype16, device=w.device)
    out_t = (torch.zeros if ldt != rows else torch.empty)((cols, ldt), dtype=dtype16, device=w.device)
    check(lib.vmc_cast_weight(ptr(w2), ptr(out), ptr(out_t), rows, cols, ld, ldt, dt(dtype16), stream()), "cast_weight")
    return out, out_t


def cast16(x: torch.Tensor, dtype16: torch.dtype) -> torch.Tensor:
    if x.dtype == dtype16:
        return x
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=dtype16, device=x.device)
    check(lib.vmc_cast_f32_to_16(ptr(x), ptr(y), x.numel(), dt(dtype16), stream()), "cast_f32_to_16")
    return y


def cast32(x: torch.Tensor) -> torch.Tensor:
    if x.dtype == torch.float32:
        return x
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(lib.vmc_cast_16_to_f32(ptr(x), ptr(y), x.numel(), dt(x), stream()), "cast_16_to_f32")
    return y


def linear(a: torch.Tensor, w16: torch.Tensor, bias=None, res=None, act: int = ACT_NONE, alpha: float = 1.0,
           out_dtype=None, out=None, out_row_group: int = 0, res_row_mod: int = 0, out_rows=None,
           lda=None, z_out=None, variant=None) -> torch.Tensor:
    """C = alpha * act(A @ W^T + bias) + res   (vmc_linear).  a: [M,K] 16-bit (row stride lda), w16: [N,K].
    z_out: optional 16-bit [M,N] tensor that receives A @ W^T + bias before the activation (vmc_linear_preact)."""
    M = a.shape[0]
    K = w16.shape[1]
    N = w16.shape[0]
    lda = a.stride(0) if lda is None else lda
    if a.stride(-1) != 1 or w16.stride(-1) != 1:
        raise ValueError("linear: operands must be contiguous in K")
    out_dtype = out_dtype or (out.dtype if out is not None else a.dtype)
    if out is None:
        out = torch.empty((out_rows or M, N), dtype=out_dtype, device=a.device)
    if bias is not None and bias.dtype != torch.float32:
        raise TypeError("linear: bias must be float32")
    if z_out is not None:
        check(lib.vmc_linear_preact(ptr(a), ptr(w16), ptr(bias), ptr(res), ptr(out), ptr(z_out), M, N, K, lda, w16.stride(0), out.stride(0),
                                    res.stride(0) if res is not None else 0, z_out.stride(0), act, float(alpha), dt(out),
                                    dt(res) if res is not None else 0, out_row_group, res_row_mod, dt(a), stream()), "linear_preact")
        return out
    if variant is not None:         # A/B measurements: large-problem kernel / epilogue options chosen per call (vmc_linear_variant)
        check(lib.vmc_linear_variant(ptr(a), ptr(w16), ptr(bias), ptr(res), ptr(out), M, N, K, lda, w16.stride(0), out.stride(0),
                                     res.stride(0) if res is not None else 0, act, float(alpha), dt(out), dt(res) if res is not None else 0,
                                     out_row_group, res_row_mod, dt(a), int(variant), stream()), "linear_variant")
        return out
    check(lib.vmc_linear(ptr(a), ptr(w16), ptr(bias), ptr(res), ptr(out), M, N, K, lda, w16.stride(0), out.stride(0),
                         res.stride(0) if res is not None else 0, act, float(alpha), dt(out), dt(res) if res is not None else 0,
                         out_row_group, res_row_mod, dt(a), stream()), "linear")
    return out


def linear_wgrad(a: torch.Tensor, w16: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[M,N] (f32, contiguous, overwritten) = a[M,K] @ w16[N,K]^T for weight gradients: split-K when the output is
    small and the contraction long (vmc_linear_splitk_f32), the plain tiled GEMM otherwise."""
    M, K = a.shape
    N = w16.shape[0]
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if out.is_contiguous() and tiles < 384 and K >= 1024:
        nbytes = lib.vmc_linear_splitk_workspace_bytes(M, N, K)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=a.device) if nbytes else None
        check(lib.vmc_linear_splitk_f32(ptr(a), ptr(w16), ptr(out), M, N, K, a.stride(0), w16.stride(0), ptr(ws), nbytes, dt(a), stream()),
              "linear_splitk_f32")
        return out
    return linear(a, w16, out=out)


def wgrad_tn(dy: torch.Tensor, x: torch.Tensor, out: torch.Tensor, dbias: torch.Tensor = None) -> torch.Tensor:
    """out[N,K] (f32, contiguous, overwritten) = dy[M,N]^T @ x[M,K] (vmc_linear_wgrad_bias_tn): no transposed copies.
    dbias[N] (f32, optional, overwritten) = column sums of dy, from the same launch."""
    M, N = dy.shape
    K = x.shape[1]
    nbytes = lib.vmc_linear_wgrad_tn_workspace_bytes(M, N, K)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dy.device) if nbytes else None
    check(lib.vmc_linear_wgrad_bias_tn(ptr(dy), ptr(x), ptr(out), ptr(dbias), M, N, K, dy.stride(0), x.stride(0), ptr(ws), nbytes, dt(dy),
                                       stream()), "linear_wgrad_bias_tn")
    return out


class WgradProblem(ctypes.Structure):          # vmc_wgrad_tn_problem (include/vmc.h)
    _fields_ = [("dY", ctypes.c_void_p), ("X", ctypes.c_void_p), ("C", ctypes.c_void_p), ("dbias", ctypes.c_void_p),
                ("M", ctypes.c_int), ("N", ctypes.c_int), ("K", ctypes.c_int), ("lddy", ctypes.c_int), ("ldx", ctypes.c_int),
                ("reserved", ctypes.c_int)]


WGRAD_GROUP_MAX = 32


def wgrad_group_ok(dy: torch.Tensor, x: torch.Tensor, out: torch.Tensor) -> bool:
    """Shapes vmc_linear_wgrad_tn_group takes (whole 128-token pairs, 8-column granularity, < 2 GiB operands, contiguous f32 output)."""
    M, N = dy.shape
    K = x.shape[1]
    return (M >= 256 and M % 128 == 0 and N % 8 == 0 and K % 8 == 0 and dy.stride(0) % 8 == 0 and x.stride(0) % 8 == 0
            and dy.stride(1) == 1 and x.stride(1) == 1 and out.is_contiguous() and out.dtype == torch.float32
            and M * dy.stride(0) * 2 < (1 << 31) and M * x.stride(0) * 2 < (1 << 31)
            and (dy.data_ptr() | x.data_ptr() | out.data_ptr()) % 16 == 0)


def wgrad_tn_group(problems, dtype16) -> None:
    """problems: list of (dy [M,N], x [M,K], out [N,K] f32, dbias [N] f32 or None), at most WGRAD_GROUP_MAX: every out = dy^T @ x and
    dbias = column sums of dy from ONE launch (vmc_linear_wgrad_tn_group: no token slices, no workspace, no reduce)."""
    n = len(problems)
    arr = (WgradProblem * n)()
    for i, (dy, x, out, db) in enumerate(problems):
        arr[i] = WgradProblem(dy.data_ptr(), x.data_ptr(), out.data_ptr(), db.data_ptr() if db is not None else None,
                              dy.shape[0], dy.shape[1], x.shape[1], dy.stride(0), x.stride(0), 0)
    check(lib.vmc_linear_wgrad_tn_group(ctypes.cast(arr, ctypes.c_void_p), n, dt(dtype16), stream()), "linear_wgrad_tn_group")


def layernorm(x: torch.Tensor, gamma, beta, dtype16, *, out16=True, out32=False, y32=None, rows=None, ldx=None,
              eps: float = 1e-5, save_stats: bool = False):
    """LayerNorm over the last dim of x viewed as [rows, D] with row stride ldx.  Returns (y16, y32, mean, rstd)."""
    D = gamma.shape[0]
    rows = x.numel() // D if rows is None else rows
    ldx = D if ldx is None else ldx
    y16 = torch.empty((rows, D), dtype=dtype16, device=x.device) if out16 else None
    if out32 and y32 is None:
        y32 = torch.empty((rows, D), dtype=torch.float32, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    check(lib.vmc_layernorm_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y16), ptr(y32), ptr(mean), ptr(rstd), rows, D, ldx,
                                float(eps), dt(x), dt(dtype16), stream()), "layernorm_fwd")
    return y16, y32, mean, rstd


def add_layernorm_(x32: torch.Tensor, branch16: torch.Tensor, gamma, beta, *, rows=None, ldx=None, ldb=None, write_x=True,
                   eps: float = 1e-5, branch0=None) -> torch.Tensor:
    """x32 += branch16 (in place, fp32 residual stream) and return LN(x32) in branch16's dtype (vmc_add_layernorm_fwd).
    branch0: a second 16-bit branch added FIRST, x32 = (x32 + branch0) + branch16 (vmc_add2_layernorm_fwd): the add an earlier
    call with write_x=False left out of the stored stream."""
    D = gamma.shape[0]
    rows = x32.numel() // D if rows is None else rows
    y = torch.empty((rows, D), dtype=branch16.dtype, device=x32.device)
    if branch0 is not None:
        check(lib.vmc_add2_layernorm_fwd(ptr(x32), ptr(branch0), ptr(branch16), ptr(gamma), ptr(beta), ptr(y), rows, D, ldx or D, D, ldb or D,
                                         float(eps), int(write_x), dt(branch16), stream()), "add2_layernorm_fwd")
        return y
    check(lib.vmc_add_layernorm_fwd(ptr(x32), ptr(branch16), ptr(gamma), ptr(beta), ptr(y), rows, D, ldx or D, ldb or D, float(eps),
                                    int(write_x), dt(branch16), stream()), "add_layernorm_fwd")
    return y


def attention_vit(qkv: torch.Tensor, F: int, N: int, H: int, want_lse: bool = False):
    D = H * 64
    out = torch.empty((F * N, D), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((F, H, N), dtype=torch.float32, device=qkv.device) if want_lse else None
    check(lib.vmc_attention_vit_fwd(ptr(qkv), ptr(out), ptr(lse), F, N, H, dt(qkv), stream()), "attention_vit_fwd")
    return out, lse


def attention_vit_cls(q_cls: torch.Tensor, kv: torch.Tensor, F: int, N: int, H: int) -> torch.Tensor:
    """Attention of the class-token queries only: q_cls [F, D], kv [F*N, 2D] (K | V of every token) -> [F, D]."""
    out = torch.empty((F, H * 64), dtype=kv.dtype, device=kv.device)
    check(lib.vmc_attention_vit_cls_fwd(ptr(q_cls), ptr(kv), ptr(out), F, N, H, dt(kv), stream()), "attention_vit_cls_fwd")
    return out


def attention(q, k, v, key_mask_u8, B, H, Tq, Tk, dh, want_lse=False, dropout_p=0.0, dropout_seed=0):
    """Generic masked attention.  q/k/v are 2-D 16-bit views [B*T, ld] whose first H*dh columns are used."""
    out = torch.empty((B * Tq, H * dh), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, Tq), dtype=torch.float32, device=q.device) if want_lse else None
    check(lib.vmc_attention_fwd(ptr(q), ptr(k), ptr(v), ptr(key_mask_u8), ptr(out), ptr(lse), B, H, Tq, Tk, dh,
                                q.stride(0), k.stride(0), v.stride(0), out.stride(0), float(dropout_p), int(dropout_seed),
                                dt(q), stream()), "attention_fwd")
    return out, lse


# vmc_<entry>: (source channels, kpad-wide parts of a patch row, u8 source with a wrap_quirk argument)
_PATCH_ENTRIES = {"preprocess_patches_u8": (3, 1, True), "preprocess_patches_gray_u8": (1, 1, True),
                  "patches_u8_exact": (3, 2, True), "patches_gray_u8_exact": (1, 2, True),
                  "patches_f32": (3, 1, False), "patches_f32_split": (3, 3, False)}


def _patches(entry: str, x: torch.Tensor, patch: int, dtype16, wrap_quirk: bool = False) -> torch.Tensor:
    """x [F,C,R,R] -> the 16-bit patch matrix [F*g*g, parts*kpad] of lib.vmc_<entry> (include/vmc.h), g = R // patch."""
    channels, parts, u8 = _PATCH_ENTRIES[entry]
    F, C, R, R2 = x.shape
    if C != channels or R != R2 or (u8 and x.dtype != torch.uint8):
        raise ValueError(f"frames must be u8 [F,{channels},R,R]" if u8 else "pixel_values must be [F,3,R,R]")
    x = (x if u8 else x.float()).contiguous()
    g = R // patch
    kpad = _kpad(3 * patch * patch)
    out = torch.empty((F * g * g, parts * kpad), dtype=dtype16, device=x.device)
    wrap = (int(wrap_quirk),) if u8 else ()
    check(getattr(lib, "vmc_" + entry)(ptr(x), ptr(out), F, R, patch, kpad, *wrap, dt(dtype16), stream()), entry)
    return out


def preprocess_patches_u8(frames_u8: torch.Tensor, patch: int, dtype16, wrap_quirk: bool) -> torch.Tensor:
    return _patches("preprocess_patches_u8", frames_u8, patch, dtype16, wrap_quirk)


def patches_f32(pixel_values: torch.Tensor, patch: int, dtype16) -> torch.Tensor:
    return _patches("patches_f32", pixel_values, patch, dtype16)


def patches_u8_exact(frames_u8: torch.Tensor, patch: int, dtype16, wrap_quirk: bool) -> torch.Tensor:
    """[F*g*g, 2*kpad] = [v | v]: raw pixels as exact 16-bit integers (vmc_patches_u8_exact)."""
    return _patches("patches_u8_exact", frames_u8, patch, dtype16, wrap_quirk)


def patches_f32_split(pixel_values: torch.Tensor, patch: int, dtype16) -> torch.Tensor:
    """[F*g*g, 3*kpad] = [x_hi | x_lo | x_hi] (vmc_patches_f32_split)."""
    return _patches("patches_f32_split", pixel_values, patch, dtype16)


def preprocess_patches_gray_u8(gray_u8: torch.Tensor, patch: int, dtype16, wrap_quirk: bool) -> torch.Tensor:
    """preprocess_patches_u8 of the plane given three times, read once (vmc_preprocess_patches_gray_u8).  gray_u8: u8 [F,1,R,R]."""
    return _patches("preprocess_patches_gray_u8", gray_u8, patch, dtype16, wrap_quirk)


def patches_gray_u8_exact(gray_u8: torch.Tensor, patch: int, dtype16, wrap_quirk: bool) -> torch.Tensor:
    """patches_u8_exact of the plane given three times, read once (vmc_patches_gray_u8_exact).  gray_u8: u8 [F,1,R,R]."""
    return _patches("patches_gray_u8_exact", gray_u8, patch, dtype16, wrap_quirk)


GRAY_WEIGHTS_CV8 = (9798, 19235, 3735, 15)      # OpenCV 4.x 8-bit COLOR_BGR2GRAY: R, G, B weights and the shift
GRAY_WEIGHTS_14BIT = (4899, 9617, 1868, 14)     # the 14-bit constants of other OpenCV builds
FRAME_DIFF_MIN_SEG = 8                          # VMC_FRAME_DIFF_MIN_SEG (include/vmc.h): shortest time segment of the kernel


def frame_diff_gray(frames: torch.Tensor, prev: torch.Tensor = None, channels: int = 1, weights=GRAY_WEIGHTS_CV8,
                    layout: str = "nchw", out: torch.Tensor = None) -> torch.Tensor:
    """Frame-difference motion frames |gray(f[t+1]) - gray(f[t])| of RGB frames (vmc_frame_diff_gray_u8), the arithmetic of the
    reference's utils/generate_frame_diff_video.py before its lossy encode.
    frames: u8 device tensor, [T,3,H,W] (layout="nchw") or [T,H,W,3] (layout="nhwc"), any strides (views are read in place).
    prev:   one frame [3,H,W] / [H,W,3] that precedes frames[0] (the previous chunk's last frame), or None.
    Returns u8 [n_out, channels, H, W], n_out = T - 1 + (prev is not None); empty when n_out == 0.
    out:    optional contiguous u8 device tensor of that shape to write into (e.g. one clip's slice of a batch)."""
    if layout not in ("nchw", "nhwc"):
        raise ValueError("layout must be 'nchw' or 'nhwc'")
    if frames.dtype != torch.uint8 or frames.dim() != 4:
        raise ValueError("frames must be a 4-D u8 tensor")
    if layout == "nhwc":
        frames = frames.permute(0, 3, 1, 2)
        if prev is not None:
            prev = prev.permute(2, 0, 1)
    T, C, H, W = frames.shape
    if C != 3:
        raise ValueError(f"frames must have 3 channels, got {C} (layout={layout!r})")
    if channels not in (1, 3):
        raise ValueError("channels must be 1 or 3")
    if prev is not None:
        if prev.dtype != torch.uint8 or tuple(prev.shape) != (3, H, W) or prev.device != frames.device:
            raise ValueError("prev must be one u8 frame of the frames' shape, layout and device")
        if prev.stride() != frames.stride()[1:]:
            prev = _restride_like(prev, frames)
    n_out = T - 1 + (prev is not None)
    shape = (max(n_out, 0), channels, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=frames.device)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != frames.device:
        raise ValueError(f"out must be a contiguous u8 tensor of shape {shape} on the frames' device")
    if n_out <= 0 or H == 0 or W == 0:
        return out
    w_r, w_g, w_b, shift = (int(v) for v in weights)
    st, sc, sy, sx = frames.stride()
    check(lib.vmc_frame_diff_gray_u8(ptr(frames), ptr(prev), ptr(out), T, H, W, st, sc, sy, sx, w_r, w_g, w_b, shift, channels, stream()),
          "frame_diff_gray_u8")
    return out


def _restride_like(prev: torch.Tensor, frames: torch.Tensor) -> torch.Tensor:
    """One-frame copy of prev [3,H,W] with the channel / row / pixel strides of frames [T,3,H,W] (the kernel addresses both with one
    stride triple).  Memory plumbing: a single frame."""
    buf = torch.empty_strided(prev.shape, frames.stride()[1:], dtype=prev.dtype, device=prev.device)
    buf.copy_(prev)
    return buf


RESIZE_RECIPES = {"aten": 0, "separable": 2, "weights4": 4}      # VMC_RESIZE_SEPARABLE / VMC_RESIZE_WEIGHTS4 (include/vmc.h)
RESIZE_ATEN_SMALL = 128                                          # VMC_RESIZE_ATEN_SMALL


def resize_bilinear_u8(frames_u8: torch.Tensor, size, out: torch.Tensor = None, as_u8: bool = False, recipe: str = "aten") -> torch.Tensor:
    """Bilinear resize of u8 frames (vmc_resize_bilinear_u8), bit-exact with the reference's dataset_frame_diff_mn.py
    ``F.interpolate(frames.float() / 255, size, mode="bilinear", align_corners=False)`` on the CPU.
    recipe: aten's CPU kernel has two operation orders (DESIGN.md "Bilinear resize").  "aten" takes the one aten takes in a
    multi-threaded process ("weights4" when OH + OW <= RESIZE_ATEN_SMALL, else "separable"); a one-thread process, such as a
    DataLoader worker, runs "weights4" on three-channel frames of any size.
    frames_u8: u8 device tensor [F,C,H,W], C 1 or 3, any strides (a permuted [T,H,W,3] stack is read in place).
    Returns contiguous [F,C,OH,OW]: f32 in [0,1], or with as_u8 the u8 pixels ``to_pil_image`` makes of it (``.mul(255).byte()``).
    out: optional contiguous device tensor of that shape and dtype to write into (e.g. one sample's slice of a batch)."""
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4:
        raise ValueError("frames must be a 4-D u8 tensor [F,C,H,W]")
    F, C, H, W = frames_u8.shape
    if C not in (1, 3):
        raise ValueError(f"frames must have 1 or 3 channels, got {C}")
    OH, OW = (int(v) for v in size)
    if OH < 1 or OW < 1:
        raise ValueError("size must be positive")
    if recipe not in RESIZE_RECIPES:
        raise ValueError(f"recipe must be one of {sorted(RESIZE_RECIPES)}")
    shape, dtype = (F, C, OH, OW), (torch.uint8 if as_u8 else torch.float32)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=frames_u8.device)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous() or out.device != frames_u8.device:
        raise ValueError(f"out must be a contiguous {dtype} tensor of shape {shape} on the frames' device")
    src, dst = ptr(frames_u8), ptr(out)
    if F == 0:
        return out
    if H < 1 or W < 1:
        raise ValueError("frames must not be empty")
    s_f, s_c, s_y, s_x = frames_u8.stride()
    check(lib.vmc_resize_bilinear_u8(src, dst, F, C, H, W, OH, OW, s_f, s_c, s_y, s_x, int(as_u8) | RESIZE_RECIPES[recipe], stream()),
          "resize_bilinear_u8")
    return out


def unit_f32_to_u8(x: torch.Tensor) -> torch.Tensor:
    """u8 tensor of x's shape with (int)trunc(x * 255) & 255 (vmc_unit_f32_to_u8): the pixels ``to_pil_image`` makes of a float picture.
    [0,1] floats give their PIL pixels; integer-valued floats v in 0..255 give (256 - v) mod 256."""
    if x.dtype != torch.float32:
        raise ValueError("x must be float32")
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    src = ptr(x)
    if x.numel():
        check(lib.vmc_unit_f32_to_u8(src, ptr(out), x.numel(), stream()), "unit_f32_to_u8")
    return out


def set_class_rows(x: torch.Tensor, a, b, F: int, D: int, row_stride: int, dtype16):
    check(lib.vmc_set_class_rows(ptr(x), ptr(a), ptr(b), F, D, row_stride, dt(x), dt(dtype16), stream()), "set_class_rows")


def pool_len_tensor(pool_len, device):
    """The logical pool length of include/vmc.h ("POOL LENGTH") as the one-element int32 device tensor the kernels read.
    None stays None (mean over all rows); an int becomes a new tensor -- do that once, outside any graph capture."""
    if pool_len is None:
        return None
    if torch.is_tensor(pool_len):
        if pool_len.dtype != torch.int32 or pool_len.numel() != 1 or not pool_len.is_cuda:
            raise TypeError("pool_len must be an int or a one-element int32 device tensor")
        return pool_len
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("pool_len given as an int during a graph capture: pass a device tensor (the value would be frozen)")
    return torch.tensor([int(pool_len)], dtype=torch.int32, device=device)


def concat_tokens_bwd(dx: torch.Tensor, T_rgb: int, T_motion: int, len_rgb=None, len_motion=None):
    """(d rgb [B, T_rgb, D], d motion [B, T_motion, D]) = vmc_concat_tokens_len_bwd: the rows of ``dx`` [B, T_out, D] f32 scattered back to
    the two streams at the lengths ``concat_tokens`` read; exact zeros on every row that fed nothing.  Only enqueues."""
    if dx.dtype != torch.float32 or not dx.is_contiguous() or dx.dim() != 3:
        raise ValueError("concat_tokens_bwd: need a contiguous float32 [B, T_out, D] gradient")
    B, T_out, D = dx.shape
    drgb = torch.empty((B, int(T_rgb), D), dtype=torch.float32, device=dx.device)
    dmotion = torch.empty((B, int(T_motion), D), dtype=torch.float32, device=dx.device)
    check(lib.vmc_concat_tokens_len_bwd(ptr(dx), ptr(drgb), ptr(dmotion), B, int(T_rgb), int(T_motion), T_out, D, ptr(len_rgb),
                                        ptr(len_motion), stream()), "concat_tokens_len_bwd")
    return drgb, dmotion


def mean_pool(x: torch.Tensor, B: int, T: int, D: int, dtype16, out16=True, out32=False, pool_len=None):
    """pool_len (one-element int32 device tensor or None): the mean runs over the first pool_len rows of every clip."""
    o16 = torch.empty((B, D), dtype=dtype16, device=x.device) if out16 else None
    o32 = torch.empty((B, D), dtype=torch.float32, device=x.device) if out32 else None
    check(lib.vmc_mean_pool_len(ptr(x), ptr(o16), ptr(o32), B, T, D, ptr(pool_len), dt(x), dt(dtype16), stream()), "mean_pool")
    return o16, o32


def concat_tokens(rgb: torch.Tensor, motion: torch.Tensor, mask_rgb, mask_motion, T_out: int, len_rgb=None, len_motion=None, out=None):
    """(x [B, T_out, D] f32, mask [B, T_out] u8, pool_len [1] i32) = vmc_concat_tokens_len (include/vmc.h K19): the token
    concatenation ``cat([rgb[:, :-1], motion], 1)`` at the streams' own lengths, real rows first, zeros behind them.
    ``len_rgb`` / ``len_motion``: one-element int32 device tensors (``pool_len_tensor``) or None (the tensors' full lengths);
    ``mask_rgb`` / ``mask_motion``: [B, T] one-byte masks (bool or uint8) or None (all real).  ``out``: (x, mask, pool_len) buffers
    to write into; fresh ``torch.empty`` ones otherwise -- the kernel writes every element.  Only enqueues."""
    B, T_rgb, D = rgb.shape
    T_motion, T_out = int(motion.shape[1]), int(T_out)
    if motion.shape[0] != B or motion.shape[2] != D:
        raise ValueError("concat_tokens: rgb [B, T_rgb, D] and motion [B, T_motion, D] must agree in B and D")
    for t in (rgb, motion):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("concat_tokens: need contiguous float32 token tensors")
    masks = []
    for m, T in ((mask_rgb, T_rgb), (mask_motion, T_motion)):
        if m is not None:
            if tuple(m.shape) != (B, T) or m.element_size() != 1 or not m.is_contiguous():
                raise ValueError("concat_tokens: masks must be contiguous one-byte tensors of shape [B, T]")
        masks.append(m)
    for n in (len_rgb, len_motion):
        if n is not None and (not torch.is_tensor(n) or n.dtype != torch.int32 or n.numel() != 1 or not n.is_cuda):
            raise TypeError("concat_tokens: lengths must be one-element int32 device tensors (ops.pool_len_tensor)")
    if out is None:
        out = (torch.empty((B, T_out, D), dtype=torch.float32, device=rgb.device),
               torch.empty((B, T_out), dtype=torch.uint8, device=rgb.device),
               torch.empty(1, dtype=torch.int32, device=rgb.device))
    x, mask, pool_len = out
    if tuple(x.shape) != (B, T_out, D) or x.dtype != torch.float32 or not x.is_contiguous() or tuple(mask.shape) != (B, T_out) \
            or mask.element_size() != 1 or not mask.is_contiguous() or pool_len.dtype != torch.int32 or pool_len.numel() != 1:
        raise ValueError(f"concat_tokens: output buffers do not match B = {B}, T_out = {T_out}, D = {D}")
    check(lib.vmc_concat_tokens_len(ptr(rgb), ptr(motion), ptr(masks[0]), ptr(masks[1]), ptr(x), ptr(mask), ptr(pool_len), B, T_rgb,
                                    T_motion, T_out, D, ptr(len_rgb), ptr(len_motion), stream()), "concat_tokens_len")
    return x, mask, pool_len


def add_sinusoidal_pe_(x: torch.Tensor):
    B, T, D = x.shape
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("add_sinusoidal_pe_: need contiguous float32 [B,T,D]")
    check(lib.vmc_add_sinusoidal_pe(ptr(x), B, T, D, stream()), "add_sinusoidal_pe")
    return x


def transpose16(x: torch.Tensor) -> torch.Tensor:
    rows, cols = x.shape
    out = torch.empty((cols, rows), dtype=x.dtype, device=x.device)
    check(lib.vmc_transpose16(ptr(x), ptr(out), rows, cols, x.stride(0), rows, stream()), "transpose16")
    return out


def colsum(x: torch.Tensor) -> torch.Tensor:
    M, N = x.shape
    out = torch.empty(N, dtype=torch.float32, device=x.device)
    nbytes = lib.vmc_colsum_workspace_bytes(M, N)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    check(lib.vmc_colsum(ptr(x), ptr(out), M, N, x.stride(0), dt(x), ptr(ws), nbytes, stream()), "colsum")
    return out


def act_fwd(x: torch.Tensor, act: int) -> torch.Tensor:
    y = torch.empty_like(x)
    check(lib.vmc_act_fwd(ptr(x), ptr(y), x.numel(), act, dt(x), stream()), "act_fwd")
    return y


def act_bwd(x: torch.Tensor, dy: torch.Tensor, act: int) -> torch.Tensor:
    dx = torch.empty_like(x)
    check(lib.vmc_act_bwd(ptr(x), ptr(dy), ptr(dx), x.numel(), act, dt(x), stream()), "act_bwd")
    return dx


LORA_TAIL = 64      # columns the adapter term occupies behind the K columns of a concat buffer


def lora_down_concat(x: torch.Tensor, a16: torch.Tensor, r: int, scale: float, out: torch.Tensor = None, copy_x: bool = True,
                     col0: int = None) -> torch.Tensor:
    """out [M, K + 64] = [ x | round16(scale * x @ a16[:r]^T) | 0 ] (vmc_lora_down_concat).  x [M, K] 16-bit (row stride free),
    a16 [>= r, K].  out given with copy_x=False: only the 64 tail columns at col0 (default K) are written."""
    M, K = x.shape
    col0 = K if col0 is None else col0
    if out is None:
        out = torch.empty((M, col0 + LORA_TAIL), dtype=x.dtype, device=x.device)
    if x.stride(1) != 1 or a16.stride(1) != 1 or out.stride(1) != 1 or a16.dtype != x.dtype or out.dtype != x.dtype:
        raise ValueError("lora_down_concat: operands must share one 16-bit dtype and be contiguous in their last dimension")
    check(lib.vmc_lora_down_concat(ptr(x), x.stride(0), ptr(a16), a16.stride(0), ptr(out), out.stride(0), M, K, int(r), col0, float(scale),
                                   int(copy_x), dt(x), stream()), "lora_down_concat")
    return out


def lora_wgrad_tn(t: torch.Tensor, x: torch.Tensor, out: torch.Tensor, transpose_out: bool = False) -> torch.Tensor:
    """out [r, C] (or [C, r] with transpose_out; f32, contiguous, overwritten) = t[M, r]^T @ x[M, C] (vmc_lora_wgrad_tn); t and x may be
    column windows of wider buffers."""
    M, r = t.shape
    C = x.shape[1]
    if x.shape[0] != M or t.stride(1) != 1 or x.stride(1) != 1 or t.dtype != x.dtype:
        raise ValueError("lora_wgrad_tn: t and x need the same rows, one 16-bit dtype and unit column stride")
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != r * C:
        raise ValueError("lora_wgrad_tn: out must be contiguous float32 with r * C elements")
    nbytes = lib.vmc_lora_wgrad_tn_workspace_bytes(M, r, C)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=t.device) if nbytes else None
    check(lib.vmc_lora_wgrad_tn(ptr(t), t.stride(0), ptr(x), x.stride(0), ptr(out), M, r, C, int(transpose_out), ptr(ws), nbytes, dt(t),
                                stream()), "lora_wgrad_tn")
    return out


# ---- patch dropout in the student's training stem (include/vmc.h) --------------------------------------------------
PATCH_KEEP_MAX_G = 1024


def patch_keep_count(patches_per_frame: int, p: float) -> int:
    """Kp = max(1, int(G (1 - p))): open_clip's PatchDropout rule."""
    return max(1, int(patches_per_frame * (1.0 - p)))


def _check_keep(keep: torch.Tensor, F: int, G: int) -> int:
    if keep.dtype != torch.int32 or keep.dim() != 2 or keep.shape[0] != F or not keep.is_contiguous():
        raise ValueError(f"keep must be a contiguous int32 [F, Kp] tensor with F = {F}, got {keep.dtype} {tuple(keep.shape)}")
    Kp = keep.shape[1]
    if not 1 <= Kp <= G:
        raise ValueError(f"keep holds {Kp} patches per frame, the frames have {G}")
    return Kp


def patch_keep_sample(seed: int, F: int, G: int, Kp: int, device) -> torch.Tensor:
    """int32 [F, Kp]: per frame the Kp of G patches with the smallest (hash32(seed, f G + n), n), ascending (vmc_patch_keep_sample).
    seed: a value below 2^63 or a device address with bit 63 set (FusedAdam.seed_address)."""
    keep = torch.empty((F, Kp), dtype=torch.int32, device=device)
    check(lib.vmc_patch_keep_sample(int(seed), F, G, Kp, ptr(keep), stream()), "patch_keep_sample")
    return keep


def gather_rows16(src: torch.Tensor, keep: torch.Tensor, G: int) -> torch.Tensor:
    """src 16-bit [F*G, cols] (row stride free) -> [F*Kp, cols], row f Kp + j = src row f G + keep[f, j] (vmc_gather_rows16)."""
    F = src.shape[0] // G
    Kp = _check_keep(keep, F, G)
    if src.dim() != 2 or src.shape[0] != F * G or src.stride(1) != 1 or src.element_size() != 2:
        raise ValueError("gather_rows16: src must be a 16-bit [F*G, cols] matrix with unit column stride")
    cols = src.shape[1]
    dst = torch.empty((F * Kp, cols), dtype=src.dtype, device=src.device)
    check(lib.vmc_gather_rows16(ptr(src), src.stride(0), ptr(keep), G, ptr(dst), cols, cols, F, Kp, stream()), "gather_rows16")
    return dst


def assemble_tokens_keep(xp: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, keep: torch.Tensor, out_dtype) -> torch.Tensor:
    """[F*(Kp+1), D]: per frame cls + pos[0], then xp[f Kp + j] + pos[keep[f, j] + 1] (vmc_assemble_tokens_keep)."""
    F, G, D = keep.shape[0], pos.shape[0] - 1, xp.shape[1]
    Kp = _check_keep(keep, F, G)
    if xp.shape[0] != F * Kp or not xp.is_contiguous() or pos.shape[1] != D or cls.numel() != D:
        raise ValueError("assemble_tokens_keep: xp must be contiguous [F*Kp, D], cls [D], pos [G+1, D]")
    x = torch.empty((F * (Kp + 1), D), dtype=out_dtype, device=xp.device)
    check(lib.vmc_assemble_tokens_keep(ptr(xp), ptr(cls), ptr(pos), ptr(keep), ptr(x), F, G, Kp, D, dt(x), dt(xp), stream()),
          "assemble_tokens_keep")
    return x


def assemble_tokens_keep_bwd(dx: torch.Tensor, keep: torch.Tensor, G: int, dtype16, dcls: torch.Tensor = None, dpos: torch.Tensor = None):
    """dx [F*(Kp+1), D] -> (dxp 16-bit [F*Kp, D], dcls f32 [D], dpos f32 [G+1, D]) (vmc_assemble_tokens_keep_bwd).  dcls / dpos given:
    contiguous f32 destinations (gradient arena slots), overwritten."""
    F = keep.shape[0]
    Kp = _check_keep(keep, F, G)
    D = dx.shape[1]
    if dx.shape[0] != F * (Kp + 1) or not dx.is_contiguous():
        raise ValueError("assemble_tokens_keep_bwd: dx must be contiguous [F*(Kp+1), D]")
    dxp = torch.empty((F * Kp, D), dtype=dtype16, device=dx.device)
    dcls = torch.empty(D, dtype=torch.float32, device=dx.device) if dcls is None else dcls
    dpos = torch.empty((G + 1, D), dtype=torch.float32, device=dx.device) if dpos is None else dpos
    nbytes = lib.vmc_assemble_tokens_keep_bwd_workspace_bytes(F, G, D)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dx.device)
    check(lib.vmc_assemble_tokens_keep_bwd(ptr(dx), ptr(keep), ptr(dxp), ptr(dcls), ptr(dpos), F, G, Kp, D, dt(dx), dt(dtype16), ptr(ws),
                                           nbytes, stream()), "assemble_tokens_keep_bwd")
    return dxp, dcls, dpos


# ---- stochastic depth that skips dropped frames (include/vmc.h) -----------------------------------------------------
DROP_PATH_MAX_F = 8192


def drop_path_rate(p: float, block: int, layers: int) -> float:
    """p_l = p l / max(1, L - 1): the linear rule, block 0 never drops."""
    return float(p) * block / max(1, layers - 1)


def drop_path_keep_count(frames: int, p_l: float) -> int:
    """K_l = max(1, int(F (1 - p_l))): the rounding of ``patch_keep_count``."""
    return patch_keep_count(frames, p_l)


def _check_frames(name: str, x: torch.Tensor, rows: int = None) -> int:
    """x is a contiguous [rows, row] matrix of frames; returns row."""
    if x.dim() != 2 or not x.is_contiguous() or x.dtype not in (torch.float32, torch.bfloat16, torch.float16) or x.shape[1] < 1 \
            or (rows is not None and x.shape[0] != rows):
        raise ValueError(f"{name}: expected a contiguous f32 / bf16 / f16 matrix"
                         f"{'' if rows is None else f' of {rows} frames'}, got {x.dtype} {tuple(x.shape)}")
    return x.shape[1]


def _check_index(name: str, t: torch.Tensor, n: int = None) -> int:
    if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.numel() < 1 or (n is not None and t.numel() != n):
        raise ValueError(f"{name} must be a contiguous int32 vector{'' if n is None else f' of {n}'}, got {t.dtype} {tuple(t.shape)}")
    return t.numel()


def drop_path_sample(seed: int, block: int, F: int, K: int, device):
    """(keep int32 [K], slot int32 [F]): the K of F frames with the smallest (hash32(seed, block F + f), f), ascending, and the
    position of every frame in keep (-1: dropped) (vmc_drop_path_sample).  seed: a value below 2^63 or a device address with bit 63."""
    if F > DROP_PATH_MAX_F:
        raise ValueError(f"drop path draws among at most {DROP_PATH_MAX_F} frames per forward, got {F}: split the batch")
    keep = torch.empty(K, dtype=torch.int32, device=device)
    slot = torch.empty(F, dtype=torch.int32, device=device)
    check(lib.vmc_drop_path_sample(int(seed), int(block), F, K, ptr(keep), ptr(slot), stream()), "drop_path_sample")
    return keep, slot


def frame_gather(src: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
    """src [F, row] -> [K, row], row j = src row keep[j], bit copies (vmc_frame_gather)."""
    row, K = _check_frames("frame_gather: src", src), _check_index("keep", keep)
    dst = torch.empty((K, row), dtype=src.dtype, device=src.device)
    check(lib.vmc_frame_gather(ptr(src), ptr(keep), ptr(dst), src.shape[0], K, row, dt(src), stream()), "frame_gather")
    return dst


def frame_scatter_add(dpass: torch.Tensor, dsub: torch.Tensor, slot: torch.Tensor) -> torch.Tensor:
    """dx[f] = dpass[f] + dsub[slot[f]] where slot[f] >= 0, dpass[f] elsewhere (vmc_frame_scatter_add)."""
    row, F = _check_frames("frame_scatter_add: dpass", dpass), _check_index("slot", slot, dpass.shape[0])
    if _check_frames("frame_scatter_add: dsub", dsub) != row or dsub.dtype != dpass.dtype or dsub.shape[0] > F:
        raise ValueError("frame_scatter_add: dsub must hold at most F frames of dpass's row length and dtype")
    dx = torch.empty_like(dpass)
    check(lib.vmc_frame_scatter_add(ptr(dpass), ptr(dsub), ptr(slot), ptr(dx), F, row, dt(dpass), stream()), "frame_scatter_add")
    return dx


def drop_path_merge(x: torch.Tensor, y: torch.Tensor, slot: torch.Tensor, s: float) -> torch.Tensor:
    """out[f] = (1 - s) x[f] + s y[slot[f]] where slot[f] >= 0, x[f] (the same bits) elsewhere (vmc_drop_path_merge)."""
    row, F = _check_frames("drop_path_merge: x", x), _check_index("slot", slot, x.shape[0])
    if _check_frames("drop_path_merge: y", y) != row or y.dtype != x.dtype or y.shape[0] > F:
        raise ValueError("drop_path_merge: y must hold at most F frames of x's row length and dtype")
    out = torch.empty_like(x)
    check(lib.vmc_drop_path_merge(ptr(x), ptr(y), ptr(slot), ptr(out), F, row, 1.0 - s, s, dt(x), stream()), "drop_path_merge")
    return out


def drop_path_merge_bwd(dout: torch.Tensor, keep: torch.Tensor, slot: torch.Tensor, s: float):
    """(dx [F, row], dy [K, row]): dx[f] = (1 - s) dout[f] for a kept frame, dout[f] (the same bits) for a dropped one;
    dy[j] = s dout[keep[j]] (vmc_drop_path_merge_bwd, one launch)."""
    row, K = _check_frames("drop_path_merge_bwd: dout", dout), _check_index("keep", keep)
    F = _check_index("slot", slot, dout.shape[0])
    dx = torch.empty_like(dout)
    dy = torch.empty((K, row), dtype=dout.dtype, device=dout.device)
    check(lib.vmc_drop_path_merge_bwd(ptr(dout), ptr(keep), ptr(slot), ptr(dx), ptr(dy), F, K, row, 1.0 - s, s, dt(dout), stream()),
          "drop_path_merge_bwd")
    return dx, dy
