"""Float64 restatement of the YUV 4:2:0 conversions of Img2Img::renderYuv: the test reference of gather_yuv_kernel and
compose_yuv_kernel.

Planes as ffmpeg's yuv420p / yuv420p10le lay them out: Y of H x W, U (Cb) and V (Cr) of ceil(H/2) x ceil(W/2); 8-bit codes as uint8, 10-bit as
uint16.  Chroma siting MPEG-2 "left": chroma (i, j) sits at luma (x = 2j, y = 2i + 1/2).  Indices are clamped to the plane at every edge.

With n bits, Y' = Kr R + Kg G + Kb B, Cb' = (B - Y') / (2 (1 - Kb)), Cr' = (R - Y') / (2 (1 - Kr)):
  limited range  Y = 2^(n-8) (16 + 219 Y'),   C = 2^(n-8) (128 + 224 C')
  full range     Y = (2^n - 1) Y',            C = 2^(n-1) + (2^n - 1) C'
"""
import numpy as np

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}   # (Kr, Kb); Kg = 1 - Kr - Kb


def levels(bits, full_range):
    """(y_off, y_scale, c_off, c_scale): code = off + scale * normalised value"""
    q, top = 2.0 ** (bits - 8), 2.0 ** bits - 1
    if full_range:
        return 0.0, top, 2.0 ** (bits - 1), top
    return 16 * q, 219 * q, 128 * q, 224 * q


def plane_shapes(rows, cols):
    return [(rows, cols), ((rows + 1) // 2, (cols + 1) // 2), ((rows + 1) // 2, (cols + 1) // 2)]


def upsample(c, rows, cols):
    """chroma plane -> luma grid: columns even x C[x/2], odd x (C[(x-1)/2] + C[(x+1)/2]) / 2; rows 2k 1/4 C[k-1] + 3/4 C[k], 2k+1 3/4 C[k] + 1/4 C[k+1]"""
    c = np.asarray(c, np.float64)
    ch, cw = c.shape
    x = np.arange(cols)
    j = x // 2
    j1 = np.where(x % 2 == 1, np.minimum(j + 1, cw - 1), j)
    h = 0.5 * (c[:, j] + c[:, j1])
    y = np.arange(rows)
    k, odd = y // 2, y % 2 == 1
    r0 = np.where(odd, k, np.maximum(k - 1, 0))
    r1 = np.where(odd, np.minimum(k + 1, ch - 1), k)
    w0 = np.where(odd, 0.75, 0.25)[:, None]
    return w0 * h[r0] + (1.0 - w0) * h[r1]


def decode(y, u, v, *, matrix="bt709", full_range=False, bits=None):
    """YUV 4:2:0 codes -> float64 RGB (H x W x 3) clamped to [0, 1] (the values gather_yuv_kernel puts in place of u8 * fl32(1/255))"""
    bits = bits or (8 if np.asarray(y).dtype == np.uint8 else 10)
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    yo, ys, co, cs = levels(bits, full_range)
    rows, cols = np.asarray(y).shape
    Y = (np.asarray(y, np.float64) - yo) / ys
    cb = (upsample(u, rows, cols) - co) / cs
    cr = (upsample(v, rows, cols) - co) / cs
    r = Y + 2 * (1 - kr) * cr
    b = Y + 2 * (1 - kb) * cb
    g = (Y - kr * r - kb * b) / kg
    return np.clip(np.stack([r, g, b], -1), 0.0, 1.0)


def encode(rgb, *, matrix="bt709", full_range=False, bits=8):
    """float RGB (H x W x 3, the canvas render() would quantise) -> (Y, U, V) codes: R, G, B clamped to [0, 1]; Y per pixel; Cb / Cr of the RGB
    filtered onto chroma site (i, j): columns 2j-1, 2j, 2j+1 with 1/4, 1/2, 1/4, rows 2i, 2i+1 with 1/2, 1/2 (clamped); rint (half to even), clamped"""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    yo, ys, co, cs = levels(bits, full_range)
    top = 2 ** bits - 1
    dt = np.uint8 if bits == 8 else np.uint16
    x = np.clip(np.asarray(rgb, np.float64), 0.0, 1.0)
    rows, cols = x.shape[:2]
    code = lambda off, scale, val: np.ascontiguousarray(np.clip(np.rint(off + scale * val), 0, top).astype(dt))
    Y = code(yo, ys, kr * x[..., 0] + kg * x[..., 1] + kb * x[..., 2])
    i = np.arange((rows + 1) // 2)
    vert = 0.5 * (x[2 * i] + x[np.minimum(2 * i + 1, rows - 1)])
    j = np.arange((cols + 1) // 2)
    f = 0.25 * vert[:, np.maximum(2 * j - 1, 0)] + 0.5 * vert[:, 2 * j] + 0.25 * vert[:, np.minimum(2 * j + 1, cols - 1)]
    fy = kr * f[..., 0] + kg * f[..., 1] + kb * f[..., 2]
    U = code(co, cs, (f[..., 2] - fy) / (2 * (1 - kb)))
    V = code(co, cs, (f[..., 0] - fy) / (2 * (1 - kr)))
    return Y, U, V


def random_planes(rows, cols, bits, seed, full_range=False):
    """noise planes within the range's legal codes"""
    rng = np.random.default_rng(seed)
    yo, ys, co, cs = levels(bits, full_range)
    dt = np.uint8 if bits == 8 else np.uint16
    (r, c), (cr_, cc) = plane_shapes(rows, cols)[:2]
    y = rng.integers(int(yo), int(yo + ys) + 1, (r, c)).astype(dt)
    u = rng.integers(int(co - cs / 2), int(co + cs / 2) + 1, (cr_, cc)).astype(dt)
    v = rng.integers(int(co - cs / 2), int(co + cs / 2) + 1, (cr_, cc)).astype(dt)
    return y, u, v


def smooth_planes(rows, cols, bits, seed, matrix="bt709", full_range=False):
    """a smooth RGB picture encoded by encode(): the kind of frame video carries"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    ph = rng.random(6) * 6.28
    rgb = np.stack([0.5 + 0.45 * np.sin(xx / (7 + 5 * k) + yy / (11 + 3 * k) + ph[k]) for k in range(3)], -1)
    return encode(rgb, matrix=matrix, full_range=full_range, bits=bits)
