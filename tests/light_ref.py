"""The rule of the resize in linear light (include/w2x/c_api_resize_light.h) in numpy, written from its statement and not from the engine's code.

A curve is four constants (t, k, a, g):
    decode(e) = e / k   for e < t,      else ((e + a) / (1 + a))^g
    encode(l) = k l     for l < t / k,  else (1 + a) l^(1/g) - a
A resized frame under a curve is clip01 -> decode -> the antialiased resize (torch F.interpolate(antialias=True), what the engine's tap tables are) -> clip01 ->
encode; under "gamma" it is the resize alone (the callers clamp where they quantise).  dtype float64 is the reference; float32 - every step of the chain rounded
to float32 - is the model of an ideal fp32 implementation, whose distance from float64 the GPU tests measure per case and grant the device twice over.
"""
import numpy as np
import torch
import torch.nn.functional as F

CURVES = {
    "srgb": (0.04045, 12.92, 0.055, 2.4),
    "bt709": (0.0812428583, 4.5, 0.0992968268, 1.0 / 0.45),
}
MODES = ("gamma", "srgb", "bt709")


def decode(e, mode, dtype=np.float64):
    e = np.asarray(e, dtype)
    if mode == "gamma":
        return e
    t, k, a, g = (dtype(c) for c in CURVES[mode])
    one = dtype(1)
    return np.where(e < t, e / k, np.power((e + a) / (one + a), g, dtype=dtype)).astype(dtype)


def encode(l, mode, dtype=np.float64):
    l = np.asarray(l, dtype)
    if mode == "gamma":
        return l
    t, k, a, g = (dtype(c) for c in CURVES[mode])
    one = dtype(1)
    return np.where(l < t / k, k * l, (one + a) * np.power(l, one / g, dtype=dtype) - a).astype(dtype)


def interpolate(x, size, filt, dtype=np.float64):
    """[H, W, C] -> [size[0], size[1], C]: torch's antialiased separable resize in `dtype`"""
    tt = torch.from_numpy(np.ascontiguousarray(x, dtype)).permute(2, 0, 1)[None]
    return F.interpolate(tt, size=tuple(size), mode=filt, antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy().astype(dtype)


def linear_resized(canvas, size, filt, mode, dtype=np.float64):
    """the resized values V in [0, 1] of an [H, W, C] canvas under `mode` (the stores quantise V); "gamma": the clamped resize"""
    x = np.asarray(canvas, dtype)
    if mode == "gamma":
        return np.clip(interpolate(x, size, filt, dtype), 0, 1).astype(dtype)
    L = decode(np.clip(x, 0, 1), mode, dtype)
    return encode(np.clip(interpolate(L, size, filt, dtype), 0, 1), mode, dtype)


def codes(V, bits):
    """sat(rint(V * maxcode)): the undithered quantisation"""
    m = (1 << bits) - 1
    return np.clip(np.rint(np.asarray(V, np.float64) * m), 0, m).astype(np.uint8 if bits == 8 else np.uint16)


def other_modes(mode):
    return [m for m in MODES if m != mode]
