"""Planar RGBA frames on the GPU (Img2Img::renderPlanarRgba / renderPlanarRgbaResized / renderSequencePlanarRgba*).  The contract: the colour planes
are render_planar() of the bled colour, the alpha plane is the G plane of render_planar() of (A, A, A), at the same depths; at 8 / 8 bits the planes are
render_rgba()'s bytes.  The references are the engine's own render_planar() / render_rgba() / render_gray(), which the rest of the suite holds to the oracle, and
the host bleed, which tests/test_planar_rgba_host.py holds to numpy.  Every comparison is equality on every byte or every float bit: there is no tolerance.
Engines: the small synthetic graphs at tile 64 of test_gpu_gray.CONFIGS."""
import ctypes as C
import json
import math
import subprocess

import numpy as np
import pytest

import planar_rgba_ref as ref
from test_gpu_gray import CONFIGS, TAG, engines, w2x_setup  # noqa: F401  (engines: the module-scoped fixture, made again for this module)
from test_gpu_parity import smooth_frame
from test_gpu_planar import DTYPES, TARGETS, as_float, fake_tools, quantised
from test_gpu_rgba import W2X, rgba_frame

pytestmark = pytest.mark.gpu


def same(tag, got, want):
    if isinstance(got, tuple):
        assert len(got) == len(want), (tag, len(got), len(want))
        for k in range(len(got)):
            same(f"{tag} plane {k}", got[k], want[k])
        return
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:                                    # every float bit
        got, want = got.view(np.uint32), want.view(np.uint32)
    bad = got != want
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {bad.size} samples differ, first at {tuple(np.argwhere(bad)[0])}"


# every frame of 12 and 16 bits holds ref.ROUNDING_CODES in every plane, so that no comparison below passes by the luck of its seed
ROUNDING_CODES = ref.ROUNDING_CODES


def frame(rows, cols, bits, seed, pattern="random"):
    """(R, G, B, A) of `bits`, ROUNDING_CODES planted in every plane; 32: the float frame of a 16-bit one"""
    if bits == 32:
        return as_float(frame(rows, cols, 16, seed, pattern), 16)
    planes = ref.frame(rows, cols, bits, pattern, seed)
    for p in planes:
        p[1, :2] = ROUNDING_CODES.get(bits, p[1, :2])
    return planes


def expected(pkg, eng, planes, bits, out_bits, bleed, size=None, filt="bicubic"):
    """the two render_planar() calls render_planar_rgba replaces: (R, G, B, A) planes"""
    colour = planes[:3] if bleed == 0 else pkg.alpha_bleed_planes(planes, bleed, bits=bits)
    a3 = (planes[3],) * 3
    if size is None:
        return eng.render_planar(colour, bits=bits, out_bits=out_bits) + (eng.render_planar(a3, bits=bits, out_bits=out_bits)[1],)
    return eng.render_planar_resized(colour, size, bits=bits, out_bits=out_bits, filter=filt) + (eng.render_planar_resized(a3, size, bits=bits, out_bits=out_bits, filter=filt)[1],)


def tile_count(pkg, eng, rows, cols, scale, kw):
    n, _, _ = pkg.calculate_tiles(cols, rows, cols * scale, rows * scale, 64, eng.output_tile_size, scale, kw.get("overlap", (0.0625, 0.0625)))
    return n


# ---- 1. the bleed kernel alone
SPARSE_SEEDS = {(33, 65): 1, (70, 150): 1, (100, 70): 1}                 # seeds for which the two assertions on the CPU reference below hold


@pytest.mark.parametrize("bits", [8, 10, 12, 16])
def test_device_bleed_matches_the_host(engines, pkg, bits):
    """frames that straddle the kernel's 64 x 32 tile in both directions with ragged edges, planes padded each its own way; the sparse frames first shown, on the
    CPU reference alone, to need the last iteration and the whole halo"""
    eng, _ = engines("swin_x4_b2_blend")
    m = (1 << bits) - 1
    for (rows, cols), seed in SPARSE_SEEDS.items():
        sparse = ref.alpha_plane(rows, cols, bits, "sparse", seed + 1000)
        col = ref.colour_planes(rows, cols, bits, seed)
        assert any((a != b).any() for a, b in zip(ref.bleed_planes(col + (sparse,), m, 16), ref.bleed_planes(col + (sparse,), m, 15))), (rows, cols)
        assert ref.crosses_a_tile_at_full_radius(sparse), (rows, cols)
        for pattern in ("random", "sparse", "zero", "opaque", "corner"):
            planes = ref.padded(ref.frame(rows, cols, bits, pattern, seed))
            assert len({p.strides[0] for p in planes}) == 4
            a = np.minimum(planes[3].astype(np.int64), m)
            for radius in (0, 1, 2, 7, 16):
                got, words = eng.alpha_bleed_planes_device(planes, radius, bits=bits, words=True)
                same(f"{bits} bits {rows}x{cols} {pattern} radius {radius}", got, pkg.alpha_bleed_planes(planes, radius, bits=bits))
                assert words == (int(a.max()), m - int(a.min())), (pattern, radius, words)
    # codes above 2^bits - 1 act as 2^bits - 1, alpha included (10 and 12 bits: the planes are uint16)
    if bits in (10, 12):
        wild = ref.frame(70, 150, 16, "sparse", 9)
        assert (wild[0] > m).any() and (wild[3] > m).any()
        tame = tuple(np.minimum(p, m) for p in wild)
        same("codes above the depth", eng.alpha_bleed_planes_device(wild, 7, bits=bits), eng.alpha_bleed_planes_device(tame, 7, bits=bits))
        same("codes above the depth, host", eng.alpha_bleed_planes_device(wild, 7, bits=bits), pkg.alpha_bleed_planes(tame, 7, bits=bits))


def test_device_bleed_copies_float_planes_and_reduces_their_range(engines):
    eng, _ = engines("swin_x4_b2_blend")
    rng = np.random.default_rng(5)
    planes = tuple(rng.uniform(-0.5, 1.5, (33, 65)).astype(np.float32) for _ in range(4))
    planes[3][0, :5] = (np.nan, -0.0, np.inf, -np.inf, 0.25)
    got, words = eng.alpha_bleed_planes_device(planes, 0, words=True)
    same("float planes are copied", got, planes[:3])
    a = np.where(np.isnan(planes[3]), np.float32(0), np.clip(planes[3], 0, 1)).astype(np.float32) + np.float32(0)       # (-0.0 + 0.0 = +0.0)
    assert words == (int(a.max().view(np.uint32)), 0x3F800000 - int(a.min().view(np.uint32)))
    flat = planes[:3] + (np.full((33, 65), 0.3, np.float32),)
    w = eng.alpha_bleed_planes_device(flat, 0, words=True)[1]
    assert w[0] + w[1] == 0x3F800000 and w[0] == int(np.float32(0.3).view(np.uint32))


# ---- 2. the colour and alpha contract
CASES = [("swin_x4_b2_blend", 45, 57), ("swin_x4_b2_blend", 40, 141), ("cunet_x2_b3_noblend_tta", 61, 83), ("cunet_x2_b1_fp32", 57, 70)]
DEPTHS = [(8, 8), (10, 10), (12, 16), (16, 16), (16, 8), (8, 32), (32, 32)]


@pytest.mark.parametrize("bits,out_bits", DEPTHS)
@pytest.mark.parametrize("name,rows,cols", CASES)
def test_colour_and_alpha_are_two_planar_renders(engines, pkg, name, rows, cols, bits, out_bits):
    eng, scale = engines(name)
    planes = frame(rows, cols, bits, 7 * bits + rows)
    for bleed in ((0,) if bits == 32 else (0, 4, 16)):
        out = eng.render_planar_rgba(planes, bits=bits, out_bits=out_bits, bleed=bleed)
        assert len(out) == 4 and out[0].shape == (rows * scale, cols * scale) and out[0].dtype == DTYPES[out_bits]
        same(f"{name} {bits}/{out_bits} bleed {bleed}", out, expected(pkg, eng, planes, bits, out_bits, bleed))
        if (bits, out_bits) == (8, 8):                             # the interleaved planes are render_rgba's bytes
            bgra = np.ascontiguousarray(np.stack([planes[2], planes[1], planes[0], planes[3]], axis=2))
            same(f"{name} render_rgba bleed {bleed}", np.stack([out[2], out[1], out[0], out[3]], axis=2), eng.render_rgba(bgra, bleed=bleed))
        if (bits, out_bits) == (16, 16):
            same(f"{name} alpha is render_gray", out[3], eng.render_gray(planes[3]))
    if bits != 32:                                                 # the bleed changed what the network saw
        assert not all(np.array_equal(a, b) for a, b in zip(eng.render_planar_rgba(planes, bits=bits, out_bits=out_bits, bleed=4)[:3],
                                                              eng.render_planar_rgba(planes, bits=bits, out_bits=out_bits)[:3]))


# ---- 3. quantisation and input reading
@pytest.mark.parametrize("name,rows,cols", [CASES[0], CASES[3]])
def test_quantisation_and_input_reading(engines, name, rows, cols):
    eng, _ = engines(name)
    src = frame(rows, cols, 10, 21)
    for bleed in (0, 4):
        f = eng.render_planar_rgba(src, bits=10, out_bits=32, bleed=bleed)
        assert all(p.dtype == np.float32 and p.min() >= 0 and p.max() <= 1 for p in f)
        for b in (8, 10, 12, 16):
            same(f"{name} out_bits {b} bleed {bleed}", eng.render_planar_rgba(src, bits=10, out_bits=b, bleed=bleed), tuple(quantised(p, b) for p in f))
    for b in (10, 12):                                             # codes above 2^b - 1 act as 2^b - 1, alpha included
        m = (1 << b) - 1
        over = frame(rows, cols, 16, 30 + b)
        assert all((p > m).any() for p in over)
        for ob in (b, 32):
            same(f"{name} codes above {m} -> {ob}", eng.render_planar_rgba(over, bits=b, out_bits=ob, bleed=4), eng.render_planar_rgba(tuple(np.minimum(p, m) for p in over), bits=b, out_bits=ob, bleed=4))
    rng = np.random.default_rng(40)                                # float samples below 0, above 1, NaN, infinities and -0.0 act as their clamped frame
    wild = tuple(rng.uniform(-0.5, 1.5, (rows, cols)).astype(np.float32) for _ in range(4))
    for p in wild:
        p[rng.integers(0, rows, 40), rng.integers(0, cols, 40)] = np.nan
        p[0, :4] = (-np.inf, np.inf, -0.0, 2.0)
    tame = tuple(np.where(np.isnan(p), np.float32(0), np.clip(p, 0, 1)).astype(np.float32) for p in wild)
    for ob in (8, 16, 32):
        same(f"{name} wild floats -> {ob}", eng.render_planar_rgba(wild, out_bits=ob), eng.render_planar_rgba(tame, out_bits=ob))
    # an alpha plane of NaN is invisible: uniform 0, also to the shortcut
    nan = wild[:3] + (np.full((rows, cols), np.nan, np.float32),)
    out = eng.render_planar_rgba(nan, out_bits=16, skip_uniform_alpha=True)
    assert not out[3].any()
    same("NaN alpha, colour", out[:3], eng.render_planar(tame[:3], out_bits=16))


@pytest.mark.parametrize("bits", [8, 10, 12, 16])
@pytest.mark.parametrize("name,rows,cols", [CASES[0], CASES[3]])
def test_integer_input_is_its_float_frame(engines, pkg, name, rows, cols, bits):
    """Integer input equals its float frame float32(code) * float32(1 / (2^bits - 1)) at radius 0, at every output depth - wherever render_planar(), which
    defines both sides, has that property.

    The cases.  On an fp16 engine a tile pixel is three halves, and gather_planes_kernel rounds code * inv to a half TWICE (through fp32) for the first two
    elements of the pixel and ONCE (from the exact product) for the third - B, and for the frame (A, A, A) the third copy of A -, while the three elements of a
    float frame are each converted from their fp32 value, which is the twice-rounded result.  The two roundings differ for exactly two codes of 12 bits (2047,
    4094) and two of 16 (65455, 65519) and for none of 8 or 10 (ROUNDING_CODES; the host test of tests/test_planar_rgba_host.py finds them by enumeration).  So
    the reference itself, render_planar(), gives an integer frame and its float frame different bytes where the B plane holds one of the four - and
    render_planar_rgba(), held to render_planar() byte for byte on both kinds of input, inherits exactly that, in B and in A.  The frames of the equality are
    therefore: every code of the depth in R and G, the four codes included (planted), and every code but those four in B and A on an fp16 engine; on the fp32
    engine, which converts nothing to half, every code in every plane.  On the frames WITH the four codes in B and A the test asserts what does hold there:
    both kinds of input follow render_planar() bit for bit (measured on an MI355X, swin_x4_b2_blend 45 x 57, two of the codes planted in each plane: integer and
    float input then differ in 854 of 41040 samples of a plane at 12 bits and 856 at 16, through render_planar() and through this format alike)."""
    eng, _ = engines(name)
    planted = frame(rows, cols, bits, 30 + bits)
    fl = as_float(planted, bits)
    same(f"{name} bits {bits}: the integer frame follows render_planar", eng.render_planar_rgba(planted, bits=bits, out_bits=32), expected(pkg, eng, planted, bits, 32, 0))
    same(f"{name} bits {bits}: the float frame follows render_planar", eng.render_planar_rgba(fl, out_bits=32), expected(pkg, eng, fl, 32, 32, 0))
    src = planted
    if CONFIGS[name][5] is None and bits in ROUNDING_CODES:       # an fp16 engine: B and A without the codes render_planar() rounds two ways
        src = planted[:2] + tuple(np.where(np.isin(p, ROUNDING_CODES[bits]), p - 1, p).astype(p.dtype) for p in planted[2:])
        assert all(np.isin(p, ROUNDING_CODES[bits]).any() for p in src[:2]) and not any(np.isin(p, ROUNDING_CODES[bits]).any() for p in src[2:])
        fl = as_float(src, bits)
    for ob in (8, 16, 32):
        same(f"{name} bits {bits} -> {ob}", eng.render_planar_rgba(src, bits=bits, out_bits=ob), eng.render_planar_rgba(fl, out_bits=ob))
        # and the reference has the property on the same frame: the equality above is render_planar()'s own
        same(f"{name} bits {bits} -> {ob}, render_planar", expected(pkg, eng, src, bits, ob, 0), expected(pkg, eng, fl, 32, ob, 0))


# ---- 4. resized
@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
def test_resized_is_two_resized_planar_renders(engines, pkg, filt):
    eng, scale = engines("swin_x4_b2_blend")
    r, c = 45, 57
    for bits, out_bits in ((8, 8), (16, 16), (8, 32)):
        planes = frame(r, c, bits, 50 + bits)
        for size in TARGETS:
            out = eng.render_planar_rgba_resized(planes, size, bits=bits, out_bits=out_bits, bleed=4, filter=filt)
            assert out[0].shape == size
            same(f"{bits}/{out_bits} -> {size} {filt}", out, expected(pkg, eng, planes, bits, out_bits, 4, size, filt))
        same(f"{bits}/{out_bits} scaled size", eng.render_planar_rgba_resized(planes, (r * scale, c * scale), bits=bits, out_bits=out_bits, bleed=4, filter=filt),
             eng.render_planar_rgba(planes, bits=bits, out_bits=out_bits, bleed=4))
        # a uniform alpha plane, with the shortcut and without
        m = (1 << bits) - 1
        flat = planes[:3] + (np.full((r, c), m // 3, DTYPES[bits]),)
        want = expected(pkg, eng, flat, bits, out_bits, 0, TARGETS[0], filt)
        same(f"{bits}/{out_bits} uniform, tiles run", eng.render_planar_rgba_resized(flat, TARGETS[0], bits=bits, out_bits=out_bits, filter=filt), want)
        out = eng.render_planar_rgba_resized(flat, TARGETS[0], bits=bits, out_bits=out_bits, filter=filt, skip_uniform_alpha=True)
        same(f"{bits}/{out_bits} uniform, shortcut: colour", out[:3], want[:3])
        v = np.float32(m // 3) * np.float32(1.0 / m)
        assert (out[3] == (v if out_bits == 32 else quantised(v, out_bits))).all()
    bgra = rgba_frame(r, c, 55)                                    # 8 / 8: render_rgba_resized's bytes
    out = eng.render_planar_rgba_resized(tuple(np.ascontiguousarray(bgra[..., k]) for k in (2, 1, 0, 3)), TARGETS[1], bleed=3, filter=filt)
    same("render_rgba_resized", np.stack([out[2], out[1], out[0], out[3]], axis=2), eng.render_rgba_resized(bgra, TARGETS[1], bleed=3, filter=filt))


# ---- 5. progress and the uniform shortcut
@pytest.mark.parametrize("name", ["swin_x4_b2_blend", "cunet_x2_b3_noblend_tta"])
def test_progress_totals_and_the_uniform_shortcut(engines, pkg, name):
    eng, scale = engines(name)
    _, _, batch, _, _, _, kw = CONFIGS[name]
    steps = 8 if kw.get("tta") else 1
    seen = []
    eng.setProgressCallback(lambda cur, total, speed: seen.append((cur, total)))
    try:
        rows, cols = 71, 103
        n = tile_count(pkg, eng, rows, cols, scale, kw)
        both, colour_only = math.ceil(2 * n * steps / batch), math.ceil(n * steps / batch)
        planes = frame(rows, cols, 10, 60)
        for skip in (False, True):                                 # a plane that is not uniform: the whole schedule either way
            for call in (lambda: eng.render_planar_rgba(planes, bits=10, skip_uniform_alpha=skip), lambda: eng.render_planar_rgba_resized(planes, (100, 150), bits=10, out_bits=8, skip_uniform_alpha=skip)):
                seen.clear()
                call()
                assert seen == [(k + 1, both) for k in range(both)], (name, skip, seen)
        # the value rule across depths: sat(rint(v * (2^out_bits - 1))), float: v, v the sample as the gather reads it
        for bits, out_bits, code in ((8, 16, 37), (16, 8, 40000), (10, 32, 1023), (10, 32, 0), (32, 8, None), (12, 12, 2049), (16, 16, 65535)):
            base = frame(rows, cols, bits, 61)
            a = np.full((rows, cols), 0.3, np.float32) if code is None else np.full((rows, cols), code, DTYPES[bits])
            v = np.float32(0.3) if code is None else np.float32(code) * np.float32(1.0 / ((1 << bits) - 1))
            flat = base[:3] + (a,)
            seen.clear()
            out = eng.render_planar_rgba(flat, bits=bits, out_bits=out_bits, skip_uniform_alpha=True)
            assert seen == [(k + 1, colour_only) for k in range(colour_only)], (name, bits, out_bits, seen)
            want = v if out_bits == 32 else quantised(v, out_bits)
            assert out[3].dtype == DTYPES[out_bits] and (out[3] == want).all(), (bits, out_bits, code, out[3][0, 0], want)
            if bits == out_bits and code is not None:
                assert (out[3] == code).all()
            same(f"{bits}/{out_bits} uniform: colour", out[:3], eng.render_planar(base[:3], bits=bits, out_bits=out_bits))
            seen.clear()                                           # with the shortcut off the same frame gives the network's alpha
            out = eng.render_planar_rgba(flat, bits=bits, out_bits=out_bits)
            assert seen == [(k + 1, both) for k in range(both)]
            same(f"{bits}/{out_bits} uniform without the shortcut", out, expected(pkg, eng, flat, bits, out_bits, 0))
        # a code above the depth everywhere is one value: 2^bits - 1
        over = frame(rows, cols, 10, 62)[:3] + (np.random.default_rng(1).integers(1023, 65536, (rows, cols)).astype(np.uint16),)
        seen.clear()
        out = eng.render_planar_rgba(over, bits=10, skip_uniform_alpha=True)
        assert seen[-1] == (colour_only, colour_only) and (out[3] == 1023).all()
        # one pixel off: not uniform
        flat = frame(rows, cols, 16, 63)[:3] + (np.zeros((rows, cols), np.uint16),)
        flat[3][rows - 1, cols - 1] = 1
        seen.clear()
        eng.render_planar_rgba(flat, skip_uniform_alpha=True, bleed=16)
        assert seen and seen[-1] == (both, both)
    finally:
        eng.setProgressCallback(None)


def test_a_pass_holds_tiles_of_both_kinds(engines, pkg):
    """3 tiles at batch 2: 6 tiles in 3 batches, the second of which is the last colour tile and the first alpha tile"""
    eng, scale = engines("swin_x4_b2_blend")
    _, _, batch, _, _, _, kw = CONFIGS["swin_x4_b2_blend"]
    cols = next(c for c in range(1, 400) if tile_count(pkg, eng, 20, c, scale, kw) == 3)
    assert 3 % batch
    planes = frame(20, cols, 12, 64)
    seen = []
    eng.setProgressCallback(lambda cur, total, speed: seen.append((cur, total)))
    out = eng.render_planar_rgba(planes, bits=12, out_bits=16, bleed=2)
    eng.setProgressCallback(None)
    assert seen == [(1, 3), (2, 3), (3, 3)], seen
    same("3 tiles at batch 2", out, expected(pkg, eng, planes, 12, 16, 2))


# ---- 6. sequences
@pytest.mark.parametrize("bits,out_bits", [(8, 8), (16, 10), (8, 32)])
@pytest.mark.parametrize("pinned", [False, True])
def test_sequence_matches_single_frames(engines, pinned, bits, out_bits):
    eng, scale = engines("swin_x4_b2_blend")
    r, c = 45, 57
    m = (1 << bits) - 1
    frames = [frame(r, c, bits, 70 + k, "random" if k % 2 else "sparse") for k in range(5)]
    frames[1] = frames[1][:3] + (np.full((r, c), m // 2, DTYPES[bits]),)          # uniform frames among the others: the shortcut is decided per frame
    frames[3] = frames[3][:3] + (np.zeros((r, c), DTYPES[bits]),)
    kw = dict(bits=bits, out_bits=out_bits, bleed=3, skip_uniform_alpha=True)
    for size in (None, (113, 150)):
        want = [eng.render_planar_rgba(f, **kw) if size is None else eng.render_planar_rgba_resized(f, size, **kw) for f in frames]
        for attempt in range(2):
            got = eng.render_sequence_planar_rgba(frames, size, pinned=pinned, **kw)
            assert len(got) == 5
            for k in range(5):
                same(f"{size} attempt {attempt} frame {k}", got[k], want[k])
        wide = [ref.padded(f) for f in frames[:3]]
        steps = [p.strides[0] for p in wide[0]]
        assert all([p.strides[0] for p in w] == steps for w in wide) and len(set(steps)) == 4
        for k, o in enumerate(eng.render_sequence_planar_rgba(wide, size, **kw)):
            same(f"padded rows {size} {k}", o, want[k])
    mine = [tuple(np.zeros((4 * r, 4 * c), DTYPES[out_bits]) for _ in range(4)) for _ in range(2)]
    assert eng.render_sequence_planar_rgba(frames[:2], outs=mine, **kw) is mine
    same("caller's buffers", mine[1], eng.render_planar_rgba(frames[1], **kw))
    gbra = eng.render_sequence_planar_rgba([(f[1], f[2], f[0], f[3]) for f in frames[:2]], order="gbra", **kw)
    w = eng.render_planar_rgba(frames[0], **kw)
    same("order gbra", gbra[0], (w[1], w[2], w[0], w[3]))


def test_outputs_are_untouched_after_a_refused_sequence(engines):
    eng, _ = engines("swin_x4_b2_blend")
    frames = [frame(45, 57, 8, 80 + k) for k in range(2)]
    outs = [tuple(np.full((180, 228), 0xAB, np.uint8) for _ in range(4)) for _ in range(2)]
    L, h = eng._L, eng._h
    sp = (C.c_void_p * 8)(*[p.ctypes.data for p in frames[0]], frames[1][0].ctypes.data, None, frames[1][2].ctypes.data, frames[1][3].ctypes.data)   # frame 1 lacks a plane
    dp = (C.c_void_p * 8)(*[p.ctypes.data for o in outs for p in o])
    n = len(eng.messages)
    assert L.w2x_render_sequence_rgbap(h, sp, (C.c_size_t * 4)(57, 57, 57, 57), 45, 57, 8, dp, (C.c_size_t * 4)(228, 228, 228, 228), 180, 228, 8, 2, 0, 0) == 0
    assert eng.messages[n:][-1][1].endswith("Input image has a missing plane or an invalid step.")
    assert all((p == 0xAB).all() for o in outs for p in o)


# ---- 7. kinds do not leak into each other
def test_kinds_do_not_leak(engines):
    eng, scale = engines("swin_x4_b2_blend")
    r, c = 48, 64
    bgr = smooth_frame(r, c, 30)
    bgra = rgba_frame(r, c, 33)
    g = np.ascontiguousarray(bgra[..., 1])
    p8 = frame(r, c, 8, 35)
    p16 = frame(r, c, 16, 36)
    first = None
    for rnd in range(3):
        got = [eng.render(bgr), eng.render_planar_rgba(p8, bleed=2), eng.render_rgba(bgra, bleed=2), eng.render_planar(p8[:3]), eng.render_planar_rgba(p16, out_bits=32),
               eng.render_gray(g), eng.render_planar_rgba(p8, out_bits=16), eng.render_planar(p16[:3]), eng.render_planar_rgba(p16, bleed=5), eng.render(bgr)]
        got = [x if isinstance(x, tuple) else (x,) for x in got]
        if first is None:
            first = got
        for k, (a, b) in enumerate(zip(got, first)):
            same(f"round {rnd} call {k}", a, b)
    same("bgr twice", first[0], first[9])
    res = np.empty((r * scale, c * scale, 3), np.uint8)
    eng.render_planar_rgba(p8)
    assert eng.bench_resident(2) < 0 and not eng.resident_output(res)          # a planar RGBA frame is not replayed, like an RGBA one
    want = eng.render(bgr)
    assert eng.bench_resident(2) > 0 and eng.resident_output(res)
    same("render() frames are still replayed", res, want)
    same("planar RGBA after a replay", eng.render_planar_rgba(p8, bleed=2), first[1])


# ---- 8. refusals, through the C entries
def test_refusals_leave_the_engine_usable(engines, pkg):
    eng, scale = engines("swin_x4_b2_blend")
    err = int(pkg.Severity.error)
    R, Cc = 40, 50
    src = frame(R, Cc, 8, 90)
    src16 = tuple(p.astype(np.uint16) * 257 for p in src)
    srcf = as_float(src, 8)
    before = (eng.render_planar_rgba(src, bleed=3), eng.render_planar_rgba(src16, out_bits=32), eng.render_planar_rgba_resized(src, (100, 150)))
    L, h = eng._L, eng._h
    out = tuple(np.zeros((170, 210), np.float32) for _ in range(4))            # larger than any destination below

    def ptrs(planes, null=None, off=0):
        return (C.c_void_p * 4)(*[None if k == null else p.ctypes.data + off for k, p in enumerate(planes)])

    def steps(*v):
        return (C.c_size_t * 4)(*v)

    def plain(rows=R, cols=Cc, bits=8, sp=None, ss=None, orows=None, ocols=None, obits=8, dp=None, ds=None, planes=src, bleed=0):
        orows, ocols = rows * scale if orows is None else orows, cols * scale if ocols is None else ocols
        return L.w2x_render_rgbap(h, ptrs(planes) if sp is None else sp, steps(*[planes[0].strides[0]] * 4) if ss is None else ss, rows, cols, bits,
                                  ptrs(out) if dp is None else dp, steps(*[840] * 4) if ds is None else ds, orows, ocols, obits, bleed, 0)

    def resized(orows=100, ocols=150, filt=0, bits=8, obits=8, sp=None, dp=None, rows=R, bleed=0):
        return L.w2x_render_rgbap_resized(h, ptrs(src) if sp is None else sp, steps(50, 50, 50, 50), rows, Cc, bits, ptrs(out) if dp is None else dp, steps(840, 840, 840, 840),
                                          orows, ocols, obits, bleed, 0, filt)

    eight = (C.c_void_p * 8)(*[p.ctypes.data for p in src + src])
    outs8 = (C.c_void_p * 8)(*[p.ctypes.data for p in out + out])

    def seq(srcs=eight, dsts=outs8, count=2, bits=8, orows=160, ocols=200, bleed=0):
        return L.w2x_render_sequence_rgbap(h, srcs, steps(50, 50, 50, 50), R, Cc, bits, dsts, steps(840, 840, 840, 840), orows, ocols, 8, count, bleed, 0)

    def seq_resized(srcs=eight, dsts=outs8, count=2, orows=100, ocols=150, filt=0):
        return L.w2x_render_sequence_rgbap_resized(h, srcs, steps(50, 50, 50, 50), R, Cc, 8, dsts, steps(840, 840, 840, 840), orows, ocols, 8, count, 0, 0, filt)

    BITS = "Planar frames must have 8, 10, 12, 16 or 32 (float) bits."
    EMPTY = "Input image is empty."
    IN_PLANE = "Input image has a missing plane or an invalid step."
    OUT_PLANE = "Output image has a missing plane or an invalid step."
    SIZE = "Output image has invalid size: expected 200x160."
    RANGE = "Output image has invalid size for a resize: {}x{} is not between 50x40 and 200x160."
    FILTER = "Unknown resize filter {}."
    BLEED = "Alpha bleed radius {} is not in [0, 16]."
    FLOAT = "Colour bleed takes integer samples."
    cases = [
        ("source depth 9", lambda: plain(bits=9), BITS), ("destination depth 14", lambda: plain(obits=14), BITS), ("sequence: source depth 24", lambda: seq(bits=24), BITS),
        ("no rows", lambda: plain(rows=0), EMPTY), ("no columns", lambda: plain(cols=0), EMPTY), ("resized: no rows", lambda: resized(rows=0), EMPTY),
        ("null alpha plane", lambda: plain(sp=ptrs(src, 3)), IN_PLANE), ("null source plane 0", lambda: plain(sp=ptrs(src, 0)), IN_PLANE),
        ("short alpha step", lambda: plain(ss=steps(50, 50, 50, 49)), IN_PLANE), ("16-bit: odd source step", lambda: plain(bits=10, planes=src16, ss=steps(100, 100, 100, 101)), IN_PLANE),
        ("16-bit: odd source address", lambda: plain(bits=16, sp=ptrs(src16, off=1), ss=steps(100, 100, 100, 100)), IN_PLANE),
        ("float: source address 2 mod 4", lambda: plain(bits=32, sp=ptrs(out, off=2), ss=steps(840, 840, 840, 840)), IN_PLANE),
        ("null destination alpha", lambda: plain(dp=ptrs(out, 3)), OUT_PLANE), ("short destination step", lambda: plain(ds=steps(200, 200, 200, 199)), OUT_PLANE),
        ("float: destination step 2 mod 4", lambda: plain(obits=32, ds=steps(840, 840, 840, 842)), OUT_PLANE),
        ("resized: null destination plane", lambda: resized(dp=ptrs(out, 2)), OUT_PLANE),
        ("one row too many", lambda: plain(orows=161), SIZE), ("one column short", lambda: plain(ocols=199), SIZE), ("sequence: one row too many", lambda: seq(orows=161), SIZE),
        ("resized: one row too many", lambda: resized(orows=161), RANGE.format(150, 161)), ("resized: fewer rows than the input", lambda: resized(orows=39), RANGE.format(150, 39)),
        ("sequence: too large", lambda: seq_resized(orows=161), RANGE.format(150, 161)),
        ("filter 2", lambda: resized(filt=2), FILTER.format(2)), ("sequence: filter -1", lambda: seq_resized(filt=-1), FILTER.format(-1)),
        ("bleed 17", lambda: plain(bleed=17), BLEED.format(17)), ("bleed -1", lambda: resized(bleed=-1), BLEED.format(-1)), ("sequence: bleed 99", lambda: seq(bleed=99), BLEED.format(99)),
        ("bleed on float samples", lambda: plain(bits=32, planes=srcf, bleed=1), FLOAT),
        ("sequence: a null plane in frame 1", lambda: seq(srcs=(C.c_void_p * 8)(*[p.ctypes.data for p in src], src[0].ctypes.data, None, src[2].ctypes.data, src[3].ctypes.data)), IN_PLANE),
        # the order of the checks: the filter (at the entry), the depths, the empty frame, the target, per frame source before destination, then the bleed
        ("filter before depth", lambda: resized(filt=5, bits=9), FILTER.format(5)), ("depth before empty", lambda: plain(bits=9, rows=0), BITS),
        ("target before a null source plane", lambda: resized(orows=161, sp=ptrs(src, 1)), RANGE.format(150, 161)),
        ("source plane before the output size", lambda: plain(sp=ptrs(src, 1), orows=161), IN_PLANE), ("output size before the bleed", lambda: plain(ocols=201, bleed=40), SIZE),
        ("destination plane before the bleed", lambda: plain(dp=ptrs(out, 0), bleed=40), OUT_PLANE),
    ]
    for name, call, text in cases:
        n = len(eng.messages)
        assert call() == 0, name
        new = [m for s, m in eng.messages[n:] if s == err]
        assert len(new) == 1, (name, new)
        assert new[0].startswith("[") and "@" in new[0].split("]")[0] and new[0].split("] ", 1)[1] == text, (name, new[0])
    # the bleed hook's own refusals
    n = len(eng.messages)
    with pytest.raises(pkg.W2xError, match="integer samples"):
        eng.alpha_bleed_planes_device(srcf, 2)
    with pytest.raises(pkg.W2xError, match="not in"):
        eng.alpha_bleed_planes_device(src, 17)
    # frames of a sequence that differ: the wrapper's ValueError names size, depth and strides
    with pytest.raises(ValueError, match="one size, one depth"):
        eng.render_sequence_planar_rgba([src, tuple(np.zeros((R, Cc + 1), np.uint8) for _ in range(4))])
    with pytest.raises(ValueError, match="one size, one depth"):
        eng.render_sequence_planar_rgba([src16, src], bits=16)
    n = len(eng.messages)
    assert seq(count=-1) == 0 and seq(srcs=None) == 0 and seq(dsts=None) == 0 and seq_resized(count=-1) == 0 and seq_resized(srcs=None, filt=7) == 0
    assert seq(count=0, srcs=None, dsts=None) == 1 and seq_resized(count=0, srcs=None, dsts=None) == 1
    assert len(eng.messages) == n
    fresh = pkg.Img2Img()
    assert fresh.render_planar_rgba(src, dst=tuple(np.zeros((160, 200), np.uint8) for _ in range(4))) is False and "before a successful load" in fresh.last_error()
    fresh.close()
    after = (eng.render_planar_rgba(src, bleed=3), eng.render_planar_rgba(src16, out_bits=32), eng.render_planar_rgba_resized(src, (100, 150)))
    for k, (a, b) in enumerate(zip(after, before)):
        same(f"after the refusals, call {k}", a, b)
    same("a sequence after the refusals", eng.render_sequence_planar_rgba([src, src], bleed=3)[1], before[0])


# ---- 9. the command line
def test_cli_planar_rgba_video(pkg, tmp_path):
    """`w2x render --rgba-in gbrap10le --rgba-out gbrap16le --alpha-bleed 4` on a clip read through ffmpeg (the fake ffmpeg / ffprobe scripts of
    test_gpu_planar stand in for the pipes and log their arguments): raw frames in - planes G, B, R, A, contiguous -, renderSequencePlanarRgba[Resized] in the
    chunks of the bgr24 loop (6 frames: a full chunk of 4 and a ragged one), raw frames out"""
    W, H, N = 100, 70, 6
    frames = [frame(H, W, 10, 100 + k, "sparse" if k % 2 else "random") for k in range(N)]         # (R, G, B, A)
    frames[2] = frames[2][:3] + (np.full((H, W), 1023, np.uint16),)                                 # an opaque frame among them
    (tmp_path / "clip.mkv").write_bytes(b"".join(f[k].tobytes() for f in frames for k in (1, 2, 0, 3)))
    log, env = fake_tools(tmp_path, W, H, N)
    common, eng = w2x_setup(pkg, tmp_path, env)
    for k, (extra, size, tag) in enumerate((((), (4 * H, 4 * W), ""), (("--outsize", "250x175", "--alpha-skip-uniform"), (175, 250), "(250x175)"))):
        log.write_text("")
        out = tmp_path / f"v{k}"; out.mkdir()
        r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "clip.mkv"), "-o", str(out), "--rgba-in", "gbrap10le", "--rgba-out", "gbrap16le", "--alpha-bleed", "4", *extra],
                           capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr
        raw = np.frombuffer((out / f"clip{TAG}{tag}.mp4").read_bytes(), np.uint16)
        assert raw.size == N * 4 * size[0] * size[1]
        got = raw.reshape(N, 4, *size)
        want = eng.render_sequence_planar_rgba(frames, None if not extra else size, bits=10, out_bits=16, bleed=4, skip_uniform_alpha=bool(extra))
        for i in range(N):
            same(f"video frame {i} {extra}", (got[i, 2], got[i, 0], got[i, 1], got[i, 3]), want[i])
        calls = [json.loads(line) for line in log.read_text().splitlines()]
        reader = next(c for c in calls if c[c.index("-i") + 1] != "-")
        writer = next(c for c in calls if c[c.index("-i") + 1] == "-")
        assert reader[reader.index("-pix_fmt") + 1] == "gbrap10le" and reader[reader.index("-f") + 1] == "rawvideo"
        i = writer.index("-i")
        assert writer[writer.index("-f") + 1] == "rawvideo" and writer.index("-f") < i
        assert writer[writer.index("-pix_fmt") + 1] == "gbrap16le" and writer.index("-pix_fmt") < i
        assert writer[writer.index("-s") + 1] == f"{size[1]}x{size[0]}" and writer.index("-s") < i
        # no --pix_fmt given: the encoder's format defaults to the --rgba-out format
        assert writer[i + 1:].count("-pix_fmt") == 1 and writer[i + 1:][writer[i + 1:].index("-pix_fmt") + 1] == "gbrap16le"
    eng.close()


def test_cli_planar_rgba_leaves_a_still_read_through_ffmpeg_alone(pkg, tmp_path):
    """a single frame read through ffmpeg is a still like any other: under --rgba-in / --rgba-out the reader is still asked for bgr24 and the bytes are render()'s"""
    W, H = 100, 70
    bgr = smooth_frame(H, W, 95)
    (tmp_path / "cover.jpg").write_bytes(bgr.tobytes())
    log, env = fake_tools(tmp_path, W, H, 1)
    common, eng = w2x_setup(pkg, tmp_path, env)
    want = eng.render(bgr)
    log.write_text("")
    out = tmp_path / "s"; out.mkdir()
    r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "cover.jpg"), "-o", str(out), "--rgba-in", "gbrap", "--rgba-out", "gbrapf32le"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    raw = np.frombuffer((out / f"cover{TAG}.png").read_bytes(), np.uint8)
    assert raw.size == want.size
    same("a still through ffmpeg", raw.reshape(want.shape), want)
    calls = [json.loads(line) for line in log.read_text().splitlines()]
    reader = next(c for c in calls if c[c.index("-i") + 1] != "-")
    writer = next(c for c in calls if c[c.index("-i") + 1] == "-")
    assert reader[reader.index("-pix_fmt") + 1] == "bgr24" and writer[writer.index("-pix_fmt") + 1] == "bgr24"
    eng.close()
