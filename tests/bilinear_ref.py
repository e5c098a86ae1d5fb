"""numpy restatement of the bilinear-resize recipes (DESIGN.md "Bilinear resize"): aten's CPU upsample_bilinear2d on frames / 255 with
align_corners=False, then to_pil_image's mul(255).byte().  aten has two operation orders and picks by output size and thread count;
both are here.  float32 throughout, one rounding per operation; an FMA a * b + c is
f32(f64(c) + f64(a) * f64(b)) (the product of two f32 is exact in f64).  tests/test_bilinear_host.py pins this against
F.interpolate on the CPU and against the stored fixture; the GPU tests compare the kernels with it and never call torch's CPU
kernel (its bits may depend on the host's vector ISA)."""
import numpy as np

f32, f64 = np.float32, np.float64


def fma(a, b, c):
    """f32 a * b + c with one rounding (to f64 precision first: a * b is exact there)."""
    return (np.asarray(c, f32).astype(f64) + np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64)).astype(f32)


def axis_table(n_in: int, n_out: int):
    """(i0, i1, l0, l1) of every output index along one axis."""
    scale = f32(n_in) / f32(n_out)
    d = np.arange(n_out, dtype=f32)
    src = fma(scale, d + f32(0.5), f32(-0.5))
    src = np.where(src < 0, f32(0), src).astype(f32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = np.clip(src - i0.astype(f32), f32(0), f32(1)).astype(f32)
    l0 = (f32(1) - l1).astype(f32)
    return i0, i1, l0, l1


def unit(v_u8):
    """p(v) = (float)v / 255, correctly rounded."""
    return (np.asarray(v_u8).astype(f32) / f32(255)).astype(f32)


ATEN_SMALL = 128          # VMC_RESIZE_ATEN_SMALL (include/vmc.h)


def aten_recipe(size) -> str:
    """The recipe aten's CPU kernel (torch 2.10, AVX-512) uses on contiguous frames in a multi-threaded process."""
    return "weights4" if size[0] + size[1] <= ATEN_SMALL else "separable"


def resize_f32(frames_u8: np.ndarray, size, recipe: str = "aten") -> np.ndarray:
    """u8 [..., H, W] -> f32 [..., OH, OW] in [0,1]: the dataset's _resize_frames.
    recipe "separable": rows first, then columns, one FMA each (aten's generic kernel); "weights4": four products of the axis weights,
    then a chain of FMAs (aten's channels-last kernel: small outputs, and three-channel frames in a one-thread process);
    "aten": aten_recipe(size)."""
    H, W = frames_u8.shape[-2:]
    OH, OW = size
    y0, y1, ly0, ly1 = axis_table(H, OH)
    x0, x1, lx0, lx1 = axis_table(W, OW)
    p = unit(frames_u8)
    recipe = aten_recipe(size) if recipe == "aten" else recipe
    if recipe == "separable":
        rows = fma(lx0, p[..., x0], (lx1 * p[..., x1]).astype(f32))                # [..., H, OW]
        return fma(ly0[:, None], rows[..., y0, :], (ly1[:, None] * rows[..., y1, :]).astype(f32))
    if recipe != "weights4":
        raise ValueError(recipe)
    top, bot = p[..., y0, :], p[..., y1, :]
    p00, p01, p10, p11 = top[..., x0], top[..., x1], bot[..., x0], bot[..., x1]
    ly0, ly1 = ly0[:, None], ly1[:, None]
    w00, w01, w10, w11 = ((a * b).astype(f32) for a, b in ((ly0, lx0), (ly0, lx1), (ly1, lx0), (ly1, lx1)))
    return fma(w11, p11, fma(w10, p10, fma(w00, p00, (w01 * p01).astype(f32))))


def to_u8(x_f32: np.ndarray) -> np.ndarray:
    """to_pil_image on a float picture: mul(255) rounded to f32, truncated, taken mod 256."""
    return (np.trunc((np.asarray(x_f32, f32) * f32(255)).astype(f32)).astype(np.int64) & 255).astype(np.uint8)


def resize_u8(frames_u8: np.ndarray, size, recipe: str = "aten") -> np.ndarray:
    return to_u8(resize_f32(frames_u8, size, recipe))
