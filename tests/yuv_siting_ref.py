"""Float64 restatement of the YUV conversions of Img2Img::renderYuv for every (YuvLayout, YuvSiting): the test reference of the sited
instantiations of gather_yuv_kernel, compose_yuv_kernel and the resample_yuv kernels.  Built on yuv_layout_ref and yuv_ref (levels, MATRICES, pack_nv12).

A siting is a pair of 1-D rules, one per subsampled axis:

  siting    columns (i420, i422, nv12)   rows (i420, nv12)    chroma (i, j) sits at luma
  left      co-sited                     centred              x = 2j,       y = 2i + 1/2
  center    centred                      centred              x = 2j + 1/2, y = 2i + 1/2
  topleft   co-sited                     co-sited             x = 2j,       y = 2i

i422 has the column rule only (topleft is left there), i444 none.

Decode along an axis of cn chroma samples, luma index n, indices clamped to the plane:
  co-sited  even n takes C[n/2]; odd n takes 1/2 (C[(n-1)/2] + C[min((n+1)/2, cn-1)])
  centred   n = 2k takes 1/4 C[max(k-1, 0)] + 3/4 C[k]; n = 2k+1 takes 3/4 C[k] + 1/4 C[min(k+1, cn-1)]
columns first, then rows.  Encode along an axis of n luma samples, site j, on the RGB clamped to [0, 1]:
  co-sited  1/4 v[max(2j-1, 0)] + 1/2 v[2j] + 1/4 v[min(2j+1, n-1)]
  centred   1/2 v[2j] + 1/2 v[min(2j+1, n-1)]
rows first, then columns; Y per pixel, Cb / Cr from the filtered RGB.  At "left" every operation and its order is yuv_layout_ref's, so the results are
yuv_layout_ref's to the bit."""
import numpy as np

import yuv_layout_ref as ylr
from yuv_ref import MATRICES, levels

SITINGS = ("left", "center", "topleft")
COLS_CENTRED = {"left": False, "center": True, "topleft": False}
ROWS_CENTRED = {"left": True, "center": True, "topleft": False}


def effective(layout, siting):
    """the siting the layout can tell apart: i444 none, i422 the column rule alone"""
    if siting not in SITINGS:
        raise ValueError(siting)
    if layout == "i444" or (layout == "i422" and siting == "topleft"):
        return "left"
    return siting


def upsample_axis(c, n, centred, axis):
    """chroma samples along `axis` -> n luma samples, by the rule"""
    c = np.moveaxis(np.asarray(c, np.float64), axis, 0)
    cn = c.shape[0]
    i = np.arange(n)
    k, odd = i // 2, i % 2 == 1
    shape = (-1,) + (1,) * (c.ndim - 1)
    if centred:
        r0 = np.where(odd, k, np.maximum(k - 1, 0))
        r1 = np.where(odd, np.minimum(k + 1, cn - 1), k)
        w0 = np.where(odd, 0.75, 0.25).reshape(shape)
        out = w0 * c[r0] + (1.0 - w0) * c[r1]
    else:
        k1 = np.where(odd, np.minimum(k + 1, cn - 1), k)
        out = 0.5 * (c[k] + c[k1])
    return np.moveaxis(out, 0, axis)


def downsample_axis(v, centred, axis):
    """n luma samples along `axis` -> ceil(n / 2) sites, by the rule"""
    v = np.moveaxis(np.asarray(v, np.float64), axis, 0)
    n = v.shape[0]
    j = np.arange((n + 1) // 2)
    if centred:
        out = 0.5 * (v[2 * j] + v[np.minimum(2 * j + 1, n - 1)])
    else:
        out = 0.25 * v[np.maximum(2 * j - 1, 0)] + 0.5 * v[2 * j] + 0.25 * v[np.minimum(2 * j + 1, n - 1)]
    return np.moveaxis(out, 0, axis)


def upsample(c, rows, cols, layout, siting):
    """a chroma plane of the layout (not nv12: de-interleave first) on the luma grid"""
    if layout == "i444":
        return np.asarray(c, np.float64)
    h = upsample_axis(c, cols, COLS_CENTRED[siting], 1)
    return upsample_axis(h, rows, ROWS_CENTRED[siting], 0) if layout == "i420" else h


def decode(planes, layout, siting="left", *, matrix="bt709", full_range=False, bits=None):
    """the layout's codes, chroma sited by `siting` -> float64 RGB (H x W x 3) clamped to [0, 1]"""
    siting = effective(layout, siting)
    bits = bits or (8 if np.asarray(planes[0]).dtype == np.uint8 else 10)
    if layout == "nv12":
        planes, layout = ylr.unpack_nv12(*planes, bits=bits), "i420"
    y, u, v = planes
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    yo, ys, co, cs = levels(bits, full_range)
    rows, cols = np.asarray(y).shape
    Y = (np.asarray(y, np.float64) - yo) / ys
    cb = (upsample(u, rows, cols, layout, siting) - co) / cs
    cr = (upsample(v, rows, cols, layout, siting) - co) / cs
    r = Y + 2 * (1 - kr) * cr
    b = Y + 2 * (1 - kb) * cb
    g = (Y - kr * r - kb * b) / kg
    return np.clip(np.stack([r, g, b], -1), 0.0, 1.0)


def site_rgb(rgb, layout, siting):
    """the clamped RGB filtered onto the layout's chroma sites"""
    siting = effective(layout, siting)
    x = np.clip(np.asarray(rgb, np.float64), 0.0, 1.0)
    if layout == "i444":
        return x
    vert = x if layout == "i422" else downsample_axis(x, ROWS_CENTRED[siting], 0)
    return downsample_axis(vert, COLS_CENTRED[siting], 1)


def encode(rgb, layout, siting="left", *, matrix="bt709", full_range=False, bits=8):
    """float RGB (H x W x 3) -> the layout's planes of codes, chroma sited by `siting`"""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    yo, ys, co, cs = levels(bits, full_range)
    top = 2 ** bits - 1
    dt = np.uint8 if bits == 8 else np.uint16
    x = np.clip(np.asarray(rgb, np.float64), 0.0, 1.0)
    code = lambda off, scale, val: np.ascontiguousarray(np.clip(np.rint(off + scale * val), 0, top).astype(dt))
    Y = code(yo, ys, kr * x[..., 0] + kg * x[..., 1] + kb * x[..., 2])
    f = site_rgb(x, "i420" if layout == "nv12" else layout, siting)
    fy = kr * f[..., 0] + kg * f[..., 1] + kb * f[..., 2]
    U = code(co, cs, (f[..., 2] - fy) / (2 * (1 - kb)))
    V = code(co, cs, (f[..., 0] - fy) / (2 * (1 - kr)))
    return ylr.pack_nv12(Y, U, V, bits) if layout == "nv12" else (Y, U, V)


# The frames of tests/test_gpu_yuv_siting.py, which tests/test_yuv_siting_host.py shows to tell the sitings apart: (rows, cols) -> seed of the noise frame
# (yuv_layout_ref.random_planes) and seed of the smooth picture (yuv_layout_ref.smooth_rgb)
GPU_FRAMES = {(45, 67): (11, 12), (9, 141): (13, 14)}


def gpu_noise(rows, cols, layout="i420", bits=8):
    """the noise frame of that size in `layout` ("nv12": the i420 frame's samples, interleaved)"""
    planes = ylr.random_planes(rows, cols, bits, GPU_FRAMES[(rows, cols)][0], "i420" if layout == "nv12" else layout)
    return ylr.pack_nv12(*planes, bits) if layout == "nv12" else planes


def gpu_smooth(rows, cols, layout, siting):
    """the smooth picture of that size encoded for (layout, siting), 8 bits"""
    return smooth_planes(rows, cols, 8, GPU_FRAMES[(rows, cols)][1], layout, siting)


def smooth_planes(rows, cols, bits, seed, layout, siting="left", matrix="bt709", full_range=False):
    """yuv_layout_ref.smooth_rgb's picture encoded for (layout, siting)"""
    return encode(ylr.smooth_rgb(rows, cols, seed), layout, siting, matrix=matrix, full_range=full_range, bits=bits)
