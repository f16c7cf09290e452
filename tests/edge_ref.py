"""The edge rule (include/w2x/c_api_edge.h) in numpy, written from its statement and not from the engine's code: the source index, the frame
extended through it, the un-truncated tap table of the antialiased resize, the colour bleed whose neighbours go round the frame, and the float64 reference of a
resize under a mode.

    replicate: min(max(i, 0), n - 1)
    wrap:      ((i % n) + n) % n
    mirror:    reflection without repeating the edge sample (numpy's "reflect": -1 -> 1, n -> n - 2), period 2 (n - 1), as often as needed; n == 1 gives 0
"""
import numpy as np
import torch
import torch.nn.functional as F

import rgba_ref

MODES = ("replicate", "wrap", "mirror")
NP_PAD = {"replicate": "edge", "wrap": "wrap", "mirror": "reflect"}


def index(mode, i, n):
    """the source index of coordinate(s) i in a dimension of n samples; i any integer array"""
    i = np.asarray(i, np.int64)
    if mode == "replicate":
        return np.clip(i, 0, n - 1)
    if mode == "wrap":
        return np.mod(i, n)                      # (numpy's mod takes the sign of the divisor: already in [0, n))
    if mode == "mirror":
        if n == 1:
            return np.zeros_like(i)
        p = 2 * (n - 1)
        r = np.mod(i, p)
        return np.where(r < n, r, p - r)
    raise ValueError(mode)


def extend(a, mode, pad):
    """[H, W, ...] -> [H + 2 pad, W + 2 pad, ...]: the frame with `pad` samples per side taken through the rule"""
    h, w = a.shape[:2]
    ys, xs = index(mode, np.arange(-pad, h + pad), h), index(mode, np.arange(-pad, w + pad), w)
    return a[ys][:, xs]


def pad_roi(mode):
    """oracle.pipeline.pad_roi under `mode`: the crop of rect r with the out-of-frame part taken through the rule"""
    def f(img, r):
        h, w = img.shape[:2]
        return img[index(mode, np.arange(r.y, r.y + r.h), h)][:, index(mode, np.arange(r.x, r.x + r.w), w)]
    return f


def _filter(x, filt):
    x = np.abs(x)
    if filt == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a, 0.0))


def taps(n_in, n_out, filt):
    """The un-truncated tap table of the antialiased resize of one axis (PIL's convolution resampler as torch computes it, with no clipping at the border):
    (first[out] int64 - may be negative -, weights[out, taps] float64 normalised per row over ALL taps, zero past the taps a row has)."""
    scale = n_in / n_out
    half = 2.0 if filt == "bicubic" else 1.0
    support = half * scale if scale >= 1.0 else half
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    k = int(np.ceil(support)) * 2 + 1
    first = np.zeros(n_out, np.int64)
    w = np.zeros((n_out, k), np.float64)
    for i in range(n_out):
        c = scale * (i + 0.5)
        x0 = int(np.floor(c - support + 0.5))
        n = min(int(np.floor(c + support + 0.5)) - x0, k)
        v = _filter((np.arange(n) + x0 - c + 0.5) * inv, filt)
        first[i] = x0
        w[i, :n] = v / v.sum()
    return first, w


def resize_axis(a, n_out, filt, mode, axis, dtype=np.float64):
    """one axis of the resize by the table above, every tap read through the rule; accumulation in `dtype` in tap order"""
    a = np.moveaxis(np.asarray(a, dtype), axis, 0)
    first, w = taps(a.shape[0], n_out, filt)
    out = np.zeros((n_out,) + a.shape[1:], dtype)
    for k in range(w.shape[1]):
        wk = w[:, k].astype(dtype).reshape((-1,) + (1,) * (a.ndim - 1))
        out = (out + wk * a[index(mode, first + k, a.shape[0])]).astype(dtype)
    return np.moveaxis(out, 0, axis)


def resized_by_taps(canvas, size, filt, mode, dtype=np.float64):
    """[H, W, C] -> [size[0], size[1], C]: columns first, then rows - the engine's order; float32: the restatement of the same rule in fp32 with fp32 weights"""
    return resize_axis(resize_axis(canvas, size[1], filt, mode, 1, dtype), size[0], filt, mode, 0, dtype)


def resized(canvas, size, filt, mode, dtype=np.float64):
    """The reference of a resize under `mode`: the canvas padded by its own size per side with np.pad in the mode, torch's antialiased resize to three times the
    target, the middle third.  The ratio is the same, so the sample grids coincide, and the support (at most 8 samples per side at a factor of 4) never reaches
    the padded array's own border."""
    h, w = canvas.shape[:2]
    x = np.pad(np.asarray(canvas, dtype), ((h, h), (w, w), (0, 0)), mode=NP_PAD[mode])
    tt = torch.from_numpy(np.ascontiguousarray(x)).permute(2, 0, 1)[None]
    y = F.interpolate(tt, size=(3 * size[0], 3 * size[1]), mode=filt, antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()
    return np.ascontiguousarray(y[size[0]:2 * size[0], size[1]:2 * size[1]]).astype(dtype)


def codes(V, bits):
    """sat(rint(V * maxcode)): the undithered quantisation"""
    m = (1 << bits) - 1
    return np.clip(np.rint(np.asarray(V, np.float64) * m), 0, m).astype(np.uint8 if bits == 8 else np.uint16)


def bleed(bgr, alpha, radius, mode):
    """The colour bleed under `mode`.  wrap: rgba_ref.bleed of the frame extended by radius + 1 pixels per side through the rule, cropped - the bleed is local
    (a pixel after R iterations depends on the radius-R neighbourhood alone), so this is exact.  replicate and mirror: the plain bleed."""
    if mode != "wrap" or radius == 0:
        return rgba_ref.bleed(bgr, alpha, radius)
    p = radius + 1
    out = rgba_ref.bleed(np.ascontiguousarray(extend(bgr, mode, p)), np.ascontiguousarray(extend(alpha, mode, p)), radius)
    return np.ascontiguousarray(out[p:-p, p:-p])
