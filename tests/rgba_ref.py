"""The colour bleed of the RGBA renders, restated in numpy: the reference for the host function (w2x_alpha_bleed), the device kernel
(alpha_bleed_kernel) and renderRgba's colour.  Integer and exact; shares nothing with the implementation.

Inputs: an 8-bit BGR frame C, an 8-bit alpha plane A of the same size, a radius R in [0, 16].  known_0 = A > 0, col_0 = C.  Iteration it = 1..R reads
state it - 1 and writes state it: a pixel unknown in state it - 1 with n > 0 of its eight neighbours inside the frame and known in state it - 1 takes, per
channel, (sum of their colours + (n >> 1)) // n and becomes known; every other pixel keeps colour and flag.  The result is col_R."""
import numpy as np

MAX_RADIUS = 16
NEIGHBOURS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]


def bleed(bgr: np.ndarray, alpha: np.ndarray, radius: int) -> np.ndarray:
    """padded shifts: every state is padded by one pixel of `unknown`, so a pixel outside the frame is never known"""
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3 and alpha.dtype == np.uint8 and alpha.shape == bgr.shape[:2]
    assert 0 <= radius <= MAX_RADIUS
    rows, cols = alpha.shape
    col = bgr.astype(np.int64)
    known = alpha > 0
    for _ in range(radius):
        pk = np.zeros((rows + 2, cols + 2), bool)
        pk[1:-1, 1:-1] = known
        pc = np.zeros((rows + 2, cols + 2, 3), np.int64)
        pc[1:-1, 1:-1] = col
        n = np.zeros((rows, cols), np.int64)
        total = np.zeros((rows, cols, 3), np.int64)
        for dy, dx in NEIGHBOURS:
            k = pk[1 + dy:1 + dy + rows, 1 + dx:1 + dx + cols]
            n += k
            total += pc[1 + dy:1 + dy + rows, 1 + dx:1 + dx + cols] * k[..., None]
        fill = ~known & (n > 0)
        mean = (total + (n >> 1)[..., None]) // np.maximum(n, 1)[..., None]
        col = np.where(fill[..., None], mean, col)
        known = known | fill
    return col.astype(np.uint8)


def bleed_loops(bgr: np.ndarray, alpha: np.ndarray, radius: int) -> np.ndarray:
    """the same with plain loops (small frames: the two statements check each other in tests/test_rgba_host.py)"""
    rows, cols = alpha.shape
    col = [[tuple(int(v) for v in bgr[y, x]) for x in range(cols)] for y in range(rows)]
    known = [[bool(alpha[y, x] > 0) for x in range(cols)] for y in range(rows)]
    for _ in range(radius):
        ncol = [row[:] for row in col]
        nknown = [row[:] for row in known]
        for y in range(rows):
            for x in range(cols):
                if known[y][x]:
                    continue
                near = [col[y + dy][x + dx] for dy, dx in NEIGHBOURS if 0 <= y + dy < rows and 0 <= x + dx < cols and known[y + dy][x + dx]]
                n = len(near)
                if n:
                    ncol[y][x] = tuple((sum(c[ch] for c in near) + (n >> 1)) // n for ch in range(3))
                    nknown[y][x] = True
        col, known = ncol, nknown
    return np.array(col, np.uint8).reshape(rows, cols, 3)


def cases():
    """(name, bgr, alpha, radii): the frames and masks of the host and the device tests - seeded, so both see the same bytes"""
    out = []
    rng = np.random.default_rng(20260)
    radii = (0, 1, 2, 5, 16)
    for rows, cols in ((1, 1), (1, 17), (17, 1), (64, 64), (100, 70)):
        bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        # a random mask of random alpha values, about half of it transparent
        a = rng.integers(0, 256, (rows, cols), dtype=np.uint8) * (rng.random((rows, cols)) < 0.5)
        out.append((f"random {rows}x{cols}", bgr, a.astype(np.uint8), radii))
        # sparse: a few known pixels, so that every neighbour count 1..8 occurs as the fronts meet
        s = (rng.random((rows, cols)) < 0.06).astype(np.uint8) * 200
        out.append((f"sparse {rows}x{cols}", bgr, s, radii))
        out.append((f"all zero {rows}x{cols}", bgr, np.zeros((rows, cols), np.uint8), radii))
        out.append((f"all non-zero {rows}x{cols}", bgr, rng.integers(1, 256, (rows, cols), dtype=np.uint8), radii))
    # holes wider than 2R: the core is out of reach and keeps its colour
    bgr = rng.integers(0, 256, (100, 70, 3), dtype=np.uint8)
    a = np.full((100, 70), 255, np.uint8)
    a[10:60, 8:50] = 0          # 50 x 42: wider than 2 * 16 both ways
    a[70:95, 55:70] = 0         # touches the right edge
    out.append(("wide holes 100x70", bgr, a, radii))
    # a single known pixel in a corner
    for rows, cols in ((64, 64), (100, 70)):
        bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        for cy, cx in ((0, 0), (rows - 1, cols - 1)):
            a = np.zeros((rows, cols), np.uint8)
            a[cy, cx] = 1
            out.append((f"corner ({cy},{cx}) {rows}x{cols}", bgr, a, radii))
    # dense small neighbourhoods: 3 x 3 patterns around an unknown centre with exactly n known neighbours, n = 1..8, several colours each
    bgr = rng.integers(0, 256, (36, 48, 3), dtype=np.uint8)
    a = np.zeros((36, 48), np.uint8)
    for n in range(1, 9):
        for rep in range(6):
            cy, cx = 2 + 4 * n, 2 + 6 * rep + (n % 2)
            pick = rng.permutation(8)[:n]
            for k in pick:
                dy, dx = NEIGHBOURS[k]
                a[cy + dy, cx + dx] = 255
    out.append(("neighbour counts 36x48", bgr, a, (1, 2)))
    return out


def neighbour_counts(alpha: np.ndarray) -> set:
    """the known-neighbour counts the first iteration meets on unknown pixels"""
    known = np.pad(alpha > 0, 1)
    rows, cols = alpha.shape
    n = sum(known[1 + dy:1 + dy + rows, 1 + dx:1 + dx + cols].astype(int) for dy, dx in NEIGHBOURS)
    return set(int(v) for v in n[alpha == 0])
