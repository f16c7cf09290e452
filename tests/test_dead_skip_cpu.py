"""Dead-skip extents (csrc/liveness.cpp) against a brute-force mask propagation.  No GPU.

w2x_dead_skip_extents reports, per plan op and tile, the part of the op's row map that some kept output pixel depends on, in the form
columns [0, cx) U [W - wx, W) x rows [0, cy) U [H - wy, H).  The check pushes a per-token boolean mask backwards through the same op list, op by op,
with the rules of the design - per-token ops widen nothing, an attention window is needed as soon as one of its tokens is and then needs all of its
tokens (masked keys included), convolutions need their taps, a tensor with several readers needs the union - and asks for EQUAL sets at every op.
The one place where the form cannot hold the exact set is an op whose reader crops its input (the stem in front of the patch convolution: the needed
columns start at the crop offset, not at 0): there the extents must cover the mask and be the whole axis."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

OVERLAP = (0.0625, 0.0625)
SCALE = 4


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    import synth_models as sm
    work = str(tmp_path_factory.mktemp("dead_skip"))
    out = {}
    for tile, batch in ((64, 2), (256, 1)):
        path = sm.model_path(os.path.join(work, f"t{tile}"), "swin_unet/art", SCALE, 3)
        sm.export_onnx(sm.make_model("swin_unet/art", SCALE, seed=1237), path, batch=batch, tile=tile)
        out[tile] = (path, batch)
    return out


def expand(n, c, w):
    a = np.zeros(n, bool)
    a[:min(c, n)] = True
    if w > 0:
        a[n - w:] = True
    return a


def op_set(e):
    return np.outer(expand(e["H"], e["cy"], e["wy"]), expand(e["W"], e["cx"], e["wx"]))


def is_all(e):
    return e["cx"] >= e["W"] and e["cy"] >= e["H"]


def brute_force(ops, kept_w, kept_h):
    """per op: the boolean mask [H][W] over its row map of the rows some kept output pixel depends on"""
    need = {}

    def add(t, m):
        need[t] = m if t not in need else (need[t] | m)

    last = ops[-1]
    m = np.zeros((last["out_H"], last["out_W"]), bool)
    m[:kept_h, :kept_w] = True
    add(last["t_out"], m)
    rows = [None] * len(ops)
    for i in range(len(ops) - 1, -1, -1):
        e = ops[i]
        H, W = e["H"], e["W"]
        o = need[e["t_out"]]
        if e["kind"] == 0:
            r = e["r"]
            assert o.shape == (H * r, W * r)
            live = o.reshape(H, r, W, r).any(axis=(1, 3))
            if e["t_res"] >= 0:
                add(e["t_res"], np.repeat(np.repeat(live, r, axis=0), r, axis=1))
            src = np.zeros((e["in_H"], e["in_W"]), bool)
            s = e["stride"]
            ys, xs = np.nonzero(live)
            for ky in range(e["kh"]):
                for kx in range(e["kw"]):
                    src[e["y0"] + s * ys + ky, e["x0"] + s * xs + kx] = True
            add(e["t_in"], src)
        elif e["kind"] == 4:
            live = o.copy()
            add(e["t_in"], live)
        elif e["kind"] == 5:
            ws = e["ws"]
            yy = (np.arange(H) + e["ry"]) % H          # window-order row y holds pixel row (y + ry) % H
            xx = (np.arange(W) + e["rx"]) % W
            rolled = o[np.ix_(yy, xx)]
            win = rolled.reshape(H // ws, ws, W // ws, ws).any(axis=(1, 3))
            full = np.repeat(np.repeat(win, ws, axis=0), ws, axis=1)     # a needed window needs every key, masked or not
            live = np.zeros((H, W), bool)
            live[np.ix_(yy, xx)] = full
            add(e["t_in"], live)
        else:
            raise AssertionError(f"op kind {e['kind']}")
        rows[i] = live
    return rows



def grid_of(pkg, tile, tout, w, h):
    n, rin, rout = pkg.calculate_tiles(w, h, w * SCALE, h * SCALE, tile, tout, SCALE, OVERLAP)
    return n, rin, rout


def tile_out(pkg, path, batch, tile):
    ops = pkg.dead_skip_extents(path, batch, tile, tile, tile, SCALE, OVERLAP, -1)
    return ops[-1]["out_W"]


def check_frame(pkg, path, batch, tile, w, h, expect_all=False):
    tout = tile_out(pkg, path, batch, tile)
    n, _, rout = grid_of(pkg, tile, tout, w, h)
    assert n > 0
    seen = set()
    some_dead = False
    for t in range(n):
        kw, kh = int(rout[t][2]), int(rout[t][3])
        if (kw, kh) in seen:
            continue
        seen.add((kw, kh))
        ops = pkg.dead_skip_extents(path, batch, tile, w, h, SCALE, OVERLAP, t)
        if kw >= tout and kh >= tout or expect_all:
            assert all(is_all(e) for e in ops), (w, h, t)
            assert all(e["live_units"] == e["total_units"] for e in ops)
            if expect_all:
                assert kw >= tout and kh >= tout, "the frame was meant to be an exact multiple of the stride"
            continue
        masks = brute_force(ops, kw, kh)
        for i, (e, m) in enumerate(zip(ops, masks)):
            got = op_set(e)
            cropped_reader = i + 1 < len(ops) and ops[i + 1]["t_in"] == e["t_out"] and (ops[i + 1]["x0"] or ops[i + 1]["y0"])
            if cropped_reader:
                assert (got | m).sum() == got.sum(), (w, h, t, i)                     # covers the mask
                for axis, (c, wd, nn) in enumerate(((e["cy"], e["wy"], e["H"]), (e["cx"], e["wx"], e["W"]))):
                    line = m.any(axis=1 - axis)
                    exact = np.array_equal(line, expand(nn, c, wd))
                    assert exact or (c >= nn), (w, h, t, i, axis)                     # exact where the form holds it, else the whole axis
                continue
            assert np.array_equal(got, m), (w, h, t, i, e)
            units = e["live_units"]
            if e["kind"] == 5:
                assert units * e["ws"] ** 2 == m.sum()
            else:
                assert units == m.sum()
            some_dead = some_dead or units < e["total_units"]
    return some_dead


def stride_in(pkg, path, batch, tile):
    tout = tile_out(pkg, path, batch, tile)
    return round(tout / SCALE) - round(tile * OVERLAP[0])        # input pixels between tile origins (tiles.cpp calculate_tiles)


@pytest.mark.parametrize("tile", [64, 256])
def test_exact_multiples_are_all(pkg, models, tile):
    path, batch = models[tile]
    s = stride_in(pkg, path, batch, tile)
    ov = round(tile * OVERLAP[0])
    for nx, ny in ((1, 1), (2, 1), (2, 3)):
        check_frame(pkg, path, batch, tile, nx * s + ov, ny * s + ov, expect_all=True)


@pytest.mark.parametrize("tile", [64, 256])
def test_infer_and_tta_are_all(pkg, models, tile):
    path, batch = models[tile]
    for ops in (pkg.dead_skip_extents(path, batch, tile, 100, 70, SCALE, OVERLAP, -1), pkg.dead_skip_extents(path, batch, tile, 100, 70, SCALE, OVERLAP, 0, tta=True)):
        assert ops and all(is_all(e) for e in ops)


@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("dx,dy", [(1, 0), (0, 1), (1, 1)])
def test_one_pixel_into_the_last_tile(pkg, models, tile, dx, dy):
    path, batch = models[tile]
    s = stride_in(pkg, path, batch, tile)
    ov = round(tile * OVERLAP[0])
    assert check_frame(pkg, path, batch, tile, 2 * s + ov + dx, 2 * s + ov + dy)


@pytest.mark.parametrize("tile,w,h", [(64, 100, 70), (64, 380, 290), (64, 1920, 1080), (64, 65, 65), (256, 100, 70), (256, 380, 290), (256, 1920, 1080)])
def test_extents_equal_brute_force(pkg, models, tile, w, h):
    path, batch = models[tile]
    check_frame(pkg, path, batch, tile, w, h)


def test_no_dead_skip_switch_makes_everything_all(pkg, models):
    path, batch = models[64]
    with pkg.debug_switches(no_dead_skip=1):
        ops = pkg.dead_skip_extents(path, batch, 64, 100, 70, SCALE, OVERLAP, 0)
    assert all(is_all(e) for e in ops)


def test_1080p_decoder_runs_fewer_units(pkg, models):
    """tile 256, 1920 x 1080: the last tile column and the last tile row run strictly fewer units than they have in every decoder launch"""
    path, batch = models[256]
    tout = tile_out(pkg, path, batch, 256)
    n, _, rout = grid_of(pkg, 256, tout, 1920, 1080)
    assert n == 45
    last_col, last_row = n - 2, 4             # column-major: tile (8, 3) and tile (0, 4)
    assert rout[last_col][2] < tout and rout[last_col][3] == tout
    assert rout[last_row][2] == tout and rout[last_row][3] < tout
    for t in (last_col, last_row, n - 1):
        ops = pkg.dead_skip_extents(path, batch, 256, 1920, 1080, SCALE, OVERLAP, t)
        up = [i for i, e in enumerate(ops) if e["kind"] == 0 and e["r"] == 2]
        assert len(up) == 2
        decoder = ops[up[0]:]
        assert len(decoder) >= 10
        for e in decoder:
            assert e["live_units"] < e["total_units"], e
