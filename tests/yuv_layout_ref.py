"""Float64 restatement of the YUV conversions of Img2Img::renderYuv for every YuvLayout: the test reference of gather_yuv_kernel,
compose_yuv_kernel and compose_yuv444_kernel.  Built on yuv_ref's levels and MATRICES; for "i420" the operations and their order are yuv_ref's, so
the results are yuv_ref's to the bit.

  i420  Y, U, V; chroma ceil(H/2) x ceil(W/2), sited at luma (x = 2j, y = 2i + 1/2)          yuv420p / yuv420p10le
  i422  Y, U, V; chroma H x ceil(W/2), sited at luma (x = 2j, y = i)                          yuv422p / yuv422p10le
  i444  Y, U, V; chroma H x W                                                                 yuv444p / yuv444p10le
  nv12  Y, UV;   i420's samples with U and V interleaved (U first) in one plane of ceil(H/2) x 2 ceil(W/2); at 10 bits (P010) every uint16 of Y
        and UV holds its code in the HIGH 10 bits                                             nv12 / p010le

Decode: i444 takes Cb, Cr at the pixel; i422 interpolates columns as i420 does (even x C[x/2], odd x the mean of C[(x-1)/2] and C[min((x+1)/2, cw-1)])
and takes chroma row y for luma row y; nv12 is i420 on the de-interleaved samples.  Encode: Y per pixel from the clamped RGB in every layout; i444
codes Cb, Cr from the pixel's own clamped RGB; i422 filters the clamped RGB of row y over columns 2j-1, 2j, 2j+1 (1/4, 1/2, 1/4, clamped indices);
nv12 is i420's encode, interleaved.  Rounding half to even, codes clamped to the code range."""
import numpy as np

import yuv_ref
from yuv_ref import MATRICES, levels

LAYOUTS = ("i420", "i422", "i444", "nv12")


def plane_shapes(rows, cols, layout):
    """[(rows, samples per row)] of the layout's planes"""
    ch, cw = (rows + 1) // 2, (cols + 1) // 2
    if layout == "nv12":
        return [(rows, cols), (ch, 2 * cw)]
    c = {"i420": (ch, cw), "i422": (rows, cw), "i444": (rows, cols)}[layout]
    return [(rows, cols), c, c]


def pack_nv12(y, u, v, bits=None):
    """i420 planes -> (Y, UV) of nv12 (8 bits) / p010le (10 bits: codes << 6)"""
    bits = bits or (8 if np.asarray(y).dtype == np.uint8 else 10)
    uv = np.empty((u.shape[0], 2 * u.shape[1]), u.dtype)
    uv[:, 0::2] = u
    uv[:, 1::2] = v
    if bits == 10:
        return np.ascontiguousarray(y << 6), uv << 6
    return np.ascontiguousarray(y), uv


def unpack_nv12(y, uv, bits=None):
    """(Y, UV) of nv12 / p010le -> i420 planes (10 bits: v >> 6, the low six bits ignored)"""
    bits = bits or (8 if np.asarray(y).dtype == np.uint8 else 10)
    sh = 6 if bits == 10 else 0
    return np.ascontiguousarray(y >> sh), np.ascontiguousarray(uv[:, 0::2] >> sh), np.ascontiguousarray(uv[:, 1::2] >> sh)


def upsample_cols(c, cols):
    c = np.asarray(c, np.float64)
    x = np.arange(cols)
    j = x // 2
    j1 = np.where(x % 2 == 1, np.minimum(j + 1, c.shape[1] - 1), j)
    return 0.5 * (c[:, j] + c[:, j1])


def upsample_rows(h, rows):
    y = np.arange(rows)
    k, odd = y // 2, y % 2 == 1
    r0 = np.where(odd, k, np.maximum(k - 1, 0))
    r1 = np.where(odd, np.minimum(k + 1, h.shape[0] - 1), k)
    w0 = np.where(odd, 0.75, 0.25)[:, None]
    return w0 * h[r0] + (1.0 - w0) * h[r1]


def decode(planes, layout, *, matrix="bt709", full_range=False, bits=None):
    """the layout's codes -> float64 RGB (H x W x 3) clamped to [0, 1]"""
    bits = bits or (8 if np.asarray(planes[0]).dtype == np.uint8 else 10)
    if layout == "nv12":
        planes, layout = unpack_nv12(*planes, bits=bits), "i420"
    y, u, v = planes
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    yo, ys, co, cs = levels(bits, full_range)
    rows, cols = np.asarray(y).shape

    def up(c):
        if layout == "i444":
            return np.asarray(c, np.float64)
        h = upsample_cols(c, cols)
        return upsample_rows(h, rows) if layout == "i420" else h
    Y = (np.asarray(y, np.float64) - yo) / ys
    cb = (up(u) - co) / cs
    cr = (up(v) - co) / cs
    r = Y + 2 * (1 - kr) * cr
    b = Y + 2 * (1 - kb) * cb
    g = (Y - kr * r - kb * b) / kg
    return np.clip(np.stack([r, g, b], -1), 0.0, 1.0)


def encode(rgb, layout, *, matrix="bt709", full_range=False, bits=8):
    """float RGB (H x W x 3) -> the layout's planes of codes"""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    yo, ys, co, cs = levels(bits, full_range)
    top = 2 ** bits - 1
    dt = np.uint8 if bits == 8 else np.uint16
    x = np.clip(np.asarray(rgb, np.float64), 0.0, 1.0)
    rows, cols = x.shape[:2]
    code = lambda off, scale, val: np.ascontiguousarray(np.clip(np.rint(off + scale * val), 0, top).astype(dt))
    Y = code(yo, ys, kr * x[..., 0] + kg * x[..., 1] + kb * x[..., 2])
    if layout == "i444":
        f = x
    else:
        if layout == "i422":
            vert = x
        else:
            i = np.arange((rows + 1) // 2)
            vert = 0.5 * (x[2 * i] + x[np.minimum(2 * i + 1, rows - 1)])
        j = np.arange((cols + 1) // 2)
        f = 0.25 * vert[:, np.maximum(2 * j - 1, 0)] + 0.5 * vert[:, 2 * j] + 0.25 * vert[:, np.minimum(2 * j + 1, cols - 1)]
    fy = kr * f[..., 0] + kg * f[..., 1] + kb * f[..., 2]
    U = code(co, cs, (f[..., 2] - fy) / (2 * (1 - kb)))
    V = code(co, cs, (f[..., 0] - fy) / (2 * (1 - kr)))
    return pack_nv12(Y, U, V, bits) if layout == "nv12" else (Y, U, V)


def random_planes(rows, cols, bits, seed, layout, full_range=False):
    """noise planes of the layout within the range's legal codes"""
    rng = np.random.default_rng(seed)
    yo, ys, co, cs = levels(bits, full_range)
    dt = np.uint8 if bits == 8 else np.uint16
    shapes = plane_shapes(rows, cols, "i420" if layout == "nv12" else layout)
    y = rng.integers(int(yo), int(yo + ys) + 1, shapes[0]).astype(dt)
    u = rng.integers(int(co - cs / 2), int(co + cs / 2) + 1, shapes[1]).astype(dt)
    v = rng.integers(int(co - cs / 2), int(co + cs / 2) + 1, shapes[2]).astype(dt)
    return pack_nv12(y, u, v, bits) if layout == "nv12" else (y, u, v)


def smooth_rgb(rows, cols, seed):
    """yuv_ref.smooth_planes' picture before it is encoded"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    ph = rng.random(6) * 6.28
    return np.stack([0.5 + 0.45 * np.sin(xx / (7 + 5 * k) + yy / (11 + 3 * k) + ph[k]) for k in range(3)], -1)


def smooth_planes(rows, cols, bits, seed, layout, matrix="bt709", full_range=False):
    return encode(smooth_rgb(rows, cols, seed), layout, matrix=matrix, full_range=full_range, bits=bits)
