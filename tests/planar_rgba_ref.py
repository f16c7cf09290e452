"""Planar RGBA frames: the numpy restatement of the colour bleed on codes of any integer depth, and the frames the host and the GPU tests share.
The bleed: every code clamped to maxcode, known_0 = alpha > 0, `radius` Jacobi iterations over the eight neighbours inside the frame, a filled pixel takes
(sum + (n >> 1)) // n per channel, a known pixel never changes."""
import numpy as np

DTYPES = {8: np.uint8, 10: np.uint16, 12: np.uint16, 16: np.uint16, 32: np.float32}
# The codes whose half-precision tile sample depends on how code * float32(1 / maxcode) is rounded to a half: once, from the exact product, or twice, through
# fp32 (rounding_codes() enumerates them).  gather_planes_kernel of k_planar.hip rounds the first two elements of a tile pixel twice and the third once.
ROUNDING_CODES = {12: (2047, 4094), 16: (65455, 65519)}
TILE_W, TILE_H = 64, 32                                            # the bleed kernel's workgroup tile (kernels.h kBleedTileW / kBleedTileH)


def rounding_codes(bits):
    """the codes of `bits` for which float16(float32(code) * float32(1 / maxcode)) and float16(code * float32(1 / maxcode)), the product exact, differ"""
    m = (1 << bits) - 1
    c = np.arange(m + 1)
    inv = np.float32(1.0 / m)
    twice = (c.astype(np.float32) * inv).astype(np.float16)
    once = (c.astype(np.float64) * np.float64(inv)).astype(np.float16)       # (a 16-bit code times a 24-bit significand is exact in a double)
    return tuple(int(v) for v in c[twice != once])


def bleed_planes(planes, maxcode, radius, iterations=None):
    """planes: (R, G, B, A) 2-D integer arrays of one shape -> the three bled colour planes, of the dtype of planes[0].  iterations: a list that receives, per
    pixel, the iteration at which it was filled (0: visible from the start, -1: never)."""
    dt = planes[0].dtype
    col = np.stack([np.minimum(p.astype(np.int64), maxcode) for p in planes[:3]])
    known = np.minimum(planes[3].astype(np.int64), maxcode) > 0
    when = np.where(known, 0, -1)
    H, W = known.shape
    for it in range(1, radius + 1):
        k = np.pad(known, 1)
        c = np.pad(col * known, ((0, 0), (1, 1), (1, 1)))
        n = np.zeros((H, W), np.int64)
        s = np.zeros((3, H, W), np.int64)
        for dy in range(3):
            for dx in range(3):
                if dy == 1 and dx == 1:
                    continue
                n += k[dy:dy + H, dx:dx + W]
                s += c[:, dy:dy + H, dx:dx + W]
        fill = ~known & (n > 0)
        if not fill.any():
            break
        nn = np.maximum(n, 1)
        col = np.where(fill, (s + (nn >> 1)) // nn, col)
        known = known | fill
        when[fill] = it
    if iterations is not None:
        iterations.append(when)
    return tuple(col[k].astype(dt) for k in range(3))


def alpha_plane(rows, cols, bits, pattern, seed):
    """an alpha plane of codes of `bits`: "random" about half zero, "sparse" about 6 % visible, in a few discs, "zero", "opaque" (all non-zero, not
    uniform), "corner" one visible pixel at the bottom right"""
    rng = np.random.default_rng(seed)
    m = (1 << bits) - 1
    a = rng.integers(1, m + 1, (rows, cols))
    if pattern == "random":
        a[rng.random((rows, cols)) < 0.5] = 0
    elif pattern == "sparse":                                      # a few discs: most of the frame lies further than any radius from a visible pixel
        n = max(1, rows * cols // 2500)
        r2 = 0.06 * rows * cols / (n * np.pi)
        yy, xx = np.mgrid[0:rows, 0:cols]
        keep = np.zeros((rows, cols), bool)
        for cy, cx in zip(rng.integers(0, rows, n), rng.integers(0, cols, n)):
            keep |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r2
        a[~keep] = 0
    elif pattern == "zero":
        a[:] = 0
    elif pattern == "corner":
        a[:] = 0
        a[-1, -1] = m
    else:
        assert pattern == "opaque"
    return a.astype(DTYPES[bits])


def colour_planes(rows, cols, bits, seed):
    """three planes of random codes of `bits`, the extremes included"""
    rng = np.random.default_rng(seed)
    p = [rng.integers(0, 1 << bits, (rows, cols)).astype(DTYPES[bits]) for _ in range(3)]
    p[0].flat[:2] = (0, (1 << bits) - 1)[:p[0].size]
    return tuple(p)


def frame(rows, cols, bits, pattern, seed):
    """(R, G, B, A) of `bits`"""
    return colour_planes(rows, cols, bits, seed) + (alpha_plane(rows, cols, bits, pattern, seed + 1000),)


def padded(planes, seed=0):
    """the same planes as views into wider buffers, every plane padded its own way (rows of different steps, the samples starting off the buffer's start)"""
    out = []
    for k, p in enumerate(planes):
        buf = np.full((p.shape[0], p.shape[1] + 4 * k + 5), 0xEE if p.dtype != np.float32 else 0.25, p.dtype)
        view = buf[:, k + 1:k + 1 + p.shape[1]]
        view[...] = p
        out.append(view)
    return tuple(out)


def crosses_a_tile_at_full_radius(alpha, radius=16):
    """True when some pixel is filled in iteration `radius` exactly and every visible pixel within `radius` of it lies in another workgroup tile of the bleed
    kernel: its colour crossed a tile border through the whole depth of the halo"""
    when = []
    z = np.zeros_like(alpha)
    bleed_planes((z, z, z, alpha), int(np.iinfo(alpha.dtype).max), radius, when)
    ys, xs = np.nonzero(when[0] == radius)
    vis = alpha > 0
    for y, x in zip(ys, xs):
        y0, y1, x0, x1 = max(y - radius, 0), y + radius + 1, max(x - radius, 0), x + radius + 1
        sy, sx = np.nonzero(vis[y0:y1, x0:x1])
        if len(sy) and all(((y0 + a) // TILE_H, (x0 + b) // TILE_W) != (y // TILE_H, x // TILE_W) for a, b in zip(sy, sx)):
            return True
    return False
