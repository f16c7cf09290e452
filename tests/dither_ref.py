"""The rule of the dithered output (include/w2x/c_api_dither.h) in numpy float32, written from its statement and not from the engine's code.

A destination sample of an integer depth in plane c at (x, y) is  min(max(floor(fl32(V + t)), 0), maxcode),  t = (rank + 0.5) / N.
  ordered:   N = 64,   rank = B8[(y + dy) & 7][(x + dx) & 7], the recursive 8 x 8 Bayer matrix by its closed form (bayer_rank);
  bluenoise: N = 4096, rank = T[(y + dy) & 63][(x + dx) & 63], T handed in by the caller (the package's dither_table("bluenoise"));
  dx = 17 c + 23 phase, dy = 29 c + 41 phase.
V is the value the undithered engine rounds to nearest: for a plane of values v in [0, 1] it is fl32(v * fl32(maxcode)).
"""
import numpy as np

DTYPES = {8: np.uint8, 10: np.uint16, 12: np.uint16, 16: np.uint16}
LEVELS = {"ordered": 64, "bluenoise": 4096}


def bayer_rank(u, v):
    """rank of cell (u, v) of the recursive 8 x 8 Bayer matrix: q_b = ((u_b ^ v_b) << 1) | v_b for the bits b = 0, 1, 2, rank = q_0 << 4 | q_1 << 2 | q_2"""
    u, v = np.asarray(u) & 7, np.asarray(v) & 7
    rank = np.zeros(np.broadcast(u, v).shape, np.int64)
    for b in range(3):
        ub, vb = (u >> b) & 1, (v >> b) & 1
        rank |= (((ub ^ vb) << 1) | vb) << (4 - 2 * b)
    return rank


def offsets(c, phase):
    return 17 * c + 23 * phase, 29 * c + 41 * phase


def ranks(mode, shape, c, phase, table=None, offsets_dropped=False):
    """the ranks of a plane of `shape` with plane index c; offsets_dropped: the mutant that forgets the plane offsets (every plane as plane 0)"""
    dx, dy = offsets(0 if offsets_dropped else c, phase)
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    if mode == "ordered":
        return bayer_rank(x + dx, y + dy)
    assert mode == "bluenoise" and table is not None and table.shape == (64, 64)
    return table[(y + dy) & 63, (x + dx) & 63].astype(np.int64)


def thresholds(mode, shape, c, phase, table=None, offsets_dropped=False):
    """t = (rank + 0.5) / N as float32 (exact)"""
    t = (ranks(mode, shape, c, phase, table, offsets_dropped).astype(np.float64) + 0.5) / LEVELS[mode]
    t32 = t.astype(np.float32)
    assert (t32.astype(np.float64) == t).all()
    return t32


def code_of(V, t, bits):
    """min(max(floor(fl32(V + t)), 0), maxcode) for float32 arrays V and t"""
    assert V.dtype == np.float32 and t.dtype == np.float32
    m = (1 << bits) - 1
    s = (V + t).astype(np.float32)                                 # one rounded fp32 addition
    return np.clip(np.floor(s.astype(np.float64)), 0, m).astype(DTYPES[bits])


def dither_plane(v, bits, mode, c, phase=0, table=None, offsets_dropped=False):
    """the dithered plane of float32 values v: V = fl32(v * fl32(maxcode)); mode "none": clip(rint(V))"""
    v = np.asarray(v)
    assert v.dtype == np.float32
    m = (1 << bits) - 1
    V = (v * np.float32(m)).astype(np.float32)
    if mode == "none":
        return np.clip(np.rint(V), 0, m).astype(DTYPES[bits])
    return code_of(V, thresholds(mode, v.shape, c, phase, table, offsets_dropped), bits)


def dither_planes(planes, bits, mode, phase=0, table=None, offsets_dropped=False, indices=(0, 1, 2)):
    """planes k of a frame with plane index indices[k] (R, G, B = 0, 1, 2; a gray frame: (1,))"""
    return tuple(dither_plane(p, bits, mode, c, phase, table, offsets_dropped) for p, c in zip(planes, indices))
