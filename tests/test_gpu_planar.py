"""Planar RGB frames on the GPU (Img2Img::renderPlanar / renderPlanarResized / renderSequencePlanar*).  The contract: at 8 / 8 and 16 / 16 bits
render_planar gives the planes of render() of the interleaved frame and render_planar_resized those of render_resized(); the other depths are the same
expressions widened - every integer output is the quantisation of the float output, every integer input the bytes of its float frame.  The reference is the
engine's own render() / render_resized(), which the rest of the suite holds to the oracle, and every comparison is equality on every byte or every float bit:
there is no tolerance.  Engines: the small synthetic graphs at tile 64 of test_gpu_gray.CONFIGS."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from test_gpu_gray import CONFIGS, FAKE_FFMPEG, TAG, engines, w2x_setup  # noqa: F401  (engines: the module-scoped fixture, made again for this module)
from test_gpu_parity import make_engine, smooth_frame
from test_gpu_rgba import W2X, rgba_frame

pytestmark = pytest.mark.gpu

DTYPES = {8: np.uint8, 10: np.uint16, 12: np.uint16, 16: np.uint16, 32: np.float32}


def bgr_frame(rows, cols, seed, kind="smooth", dtype=np.uint8):
    if kind == "smooth":
        f = smooth_frame(rows, cols, seed)
        return f if dtype == np.uint8 else f.astype(np.uint16) * 257
    return np.random.default_rng(seed).integers(0, np.iinfo(dtype).max + 1, (rows, cols, 3), dtype=dtype)


def planes_of(bgr):
    """the R, G, B planes of an interleaved BGR frame"""
    return tuple(np.ascontiguousarray(bgr[..., k]) for k in (2, 1, 0))


def codes(rows, cols, bits, seed):
    """three planes of random codes of `bits`, the extremes included"""
    rng = np.random.default_rng(seed)
    p = [rng.integers(0, 1 << bits, (rows, cols)).astype(DTYPES[bits]) for _ in range(3)]
    p[0][0, :2] = (0, (1 << bits) - 1)
    return tuple(p)


def as_float(planes, bits):
    """the float frame of an integer one: float32(code) * float32(1 / (2^bits - 1))"""
    return tuple(p.astype(np.float32) * np.float32(1.0 / ((1 << bits) - 1)) for p in planes)


def quantised(f, bits):
    """clip(rint(f * float32(2^bits - 1))) in numpy float32"""
    m = (1 << bits) - 1
    return np.clip(np.rint(f * np.float32(m)), 0, m).astype(DTYPES[bits])


def same(tag, got, want):
    if isinstance(got, tuple):
        assert len(got) == len(want) == 3, tag
        for k in range(3):
            same(f"{tag} plane {k}", got[k], want[k])
        return
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:                                    # every float bit
        got, want = got.view(np.uint32), want.view(np.uint32)
    bad = got != want
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {bad.size} samples differ, first at {tuple(np.argwhere(bad)[0])}"


# ---- 1. 8 / 8 against render(), 16 / 16 against the 16-bit render()
CASES = [("swin_x4_b2_blend", 45, 57), ("swin_x4_b2_blend", 40, 141), ("cunet_x2_b3_noblend_tta", 61, 83), ("cunet_x1_b2_blend", 37, 541), ("cunet_x2_b1_fp32", 57, 70)]


@pytest.mark.parametrize("name,rows,cols", CASES)
def test_render_planar_gives_the_planes_of_render(engines, name, rows, cols):
    eng, scale = engines(name)
    for seed, kind in ((1, "smooth"), (2, "noise")):
        bgr = bgr_frame(rows, cols, seed, kind)
        out = eng.render_planar(planes_of(bgr))
        assert out[0].shape == (rows * scale, cols * scale) and out[0].dtype == np.uint8
        same(f"{name} {rows}x{cols} {kind}", out, planes_of(eng.render(bgr)))
    bgr16 = bgr_frame(rows, cols, 3, "noise", np.uint16)
    out = eng.render_planar(planes_of(bgr16))
    assert out[0].dtype == np.uint16
    same(f"{name} {rows}x{cols} 16-bit", out, planes_of(eng.render(bgr16)))


# ---- 2. the output depths are quantisations of one canvas
@pytest.mark.parametrize("name,rows,cols", [CASES[0], CASES[2], CASES[3], CASES[4]])
def test_output_depths_quantise_one_canvas(engines, name, rows, cols):
    eng, scale = engines(name)
    bgr = bgr_frame(rows, cols, 5, "noise")
    src = planes_of(bgr)
    f = eng.render_planar(src, out_bits=32)
    assert all(p.dtype == np.float32 and p.min() >= 0 and p.max() <= 1 for p in f)
    for b in (8, 10, 12, 16):
        same(f"{name} out_bits {b}", eng.render_planar(src, out_bits=b), tuple(quantised(p, b) for p in f))
    same(f"{name} 8 bits is render()", eng.render_planar(src, out_bits=8), planes_of(eng.render(bgr)))


# ---- 3. the input depths are the bytes of their float frames
@pytest.mark.parametrize("name,rows,cols", [CASES[0], CASES[4]])
def test_input_depths_are_their_float_frames(engines, name, rows, cols):
    eng, scale = engines(name)
    for b in (8, 10, 12, 16):
        src = codes(rows, cols, b, 10 + b)
        fl = as_float(src, b)
        for ob in (8, 10, 12, 16, 32):
            same(f"{name} bits {b} -> {ob}", eng.render_planar(src, bits=b, out_bits=ob), eng.render_planar(fl, out_bits=ob))
    for b in (10, 12):                                             # codes above 2^b - 1 act as 2^b - 1
        m = (1 << b) - 1
        src = codes(rows, cols, 16, 30 + b)
        assert (src[0] > m).any()
        for ob in (b, 32):
            same(f"{name} codes above {m} -> {ob}", eng.render_planar(src, bits=b, out_bits=ob), eng.render_planar(tuple(np.minimum(p, m) for p in src), bits=b, out_bits=ob))
    rng = np.random.default_rng(40)                                # float samples below 0, above 1 and NaN act as 0, 1 and 0
    wild = tuple(rng.uniform(-0.5, 1.5, (rows, cols)).astype(np.float32) for _ in range(3))
    for p in wild:
        p[rng.integers(0, rows, 40), rng.integers(0, cols, 40)] = np.nan
    wild[1][0, :4] = (-np.inf, np.inf, -0.0, 2.0)
    tame = tuple(np.where(np.isnan(p), np.float32(0), np.clip(p, 0, 1)).astype(np.float32) for p in wild)
    assert all(np.isnan(p).any() and (p[~np.isnan(p)] < 0).any() and (p[~np.isnan(p)] > 1).any() for p in wild)
    for ob in (8, 16, 32):
        same(f"{name} wild floats -> {ob}", eng.render_planar(wild, out_bits=ob), eng.render_planar(tame, out_bits=ob))


# ---- 4. resized
TARGETS = [(71, 103), (150, 200), (100, 201), (180, 228), (113, 150)]        # of a 45 x 57 frame at x4: every residue of the width mod 4, heights off 16


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
def test_resized_gives_the_planes_of_render_resized(engines, filt):
    eng, scale = engines("swin_x4_b2_blend")
    assert {c % 4 for _, c in TARGETS} == {0, 1, 2, 3} and any(r % 16 for r, _ in TARGETS)
    r, c = 45, 57
    bgr, bgr16 = bgr_frame(r, c, 50, "noise"), bgr_frame(r, c, 51, "noise", np.uint16)
    src, src16 = planes_of(bgr), planes_of(bgr16)
    for size in TARGETS:
        out = eng.render_planar_resized(src, size, filter=filt)
        assert out[0].shape == size
        same(f"8 / 8 -> {size} {filt}", out, planes_of(eng.render_resized(bgr, size, filt)))
        same(f"16 / 16 -> {size} {filt}", eng.render_planar_resized(src16, size, filter=filt), planes_of(eng.render_resized(bgr16, size, filt)))
    for size in TARGETS[:2]:                                       # the output depths quantise one resized canvas
        f = eng.render_planar_resized(src, size, out_bits=32, filter=filt)
        assert all(p.min() >= 0 and p.max() <= 1 for p in f)
        for b in (8, 10, 12, 16):
            same(f"resized out_bits {b} {size}", eng.render_planar_resized(src, size, out_bits=b, filter=filt), tuple(quantised(p, b) for p in f))
    for ob in (8, 10, 32):                                         # at the scaled size the resized call is the plain one
        same(f"scaled size {ob}", eng.render_planar_resized(src, (r * scale, c * scale), out_bits=ob, filter=filt), eng.render_planar(src, out_bits=ob))


def test_resized_fp32_engine_and_tta(engines):
    eng, _ = engines("cunet_x2_b1_fp32")
    bgr = bgr_frame(57, 70, 52, "noise")
    for size, filt in (((90, 113), "bilinear"), ((57, 139), "bicubic")):
        same(f"fp32 -> {size}", eng.render_planar_resized(planes_of(bgr), size, filter=filt), planes_of(eng.render_resized(bgr, size, filt)))
    eng, _ = engines("cunet_x2_b3_noblend_tta")
    bgr = bgr_frame(61, 83, 53)
    same("tta -> (100, 131)", eng.render_planar_resized(planes_of(bgr), (100, 131)), planes_of(eng.render_resized(bgr, (100, 131))))


# ---- 5. sequences
def sequence_frames(bits):
    if bits == 8:
        return [planes_of(bgr_frame(90, 130, 60 + k, "noise" if k % 2 else "smooth")) for k in range(5)]
    return [planes_of(bgr_frame(90, 130, 70 + k, "noise" if k % 2 else "smooth", np.uint16)) for k in range(5)]


@pytest.mark.parametrize("bits,out_bits", [(8, 8), (8, 10), (16, 32)])
@pytest.mark.parametrize("pinned", [False, True])
def test_rolling_sequence_matches_single_frames(pkg, onnx_model, monkeypatch, pinned, bits, out_bits):
    """five 90 x 130 frames on swin x4 with TTA (48 slots of one pass: the sequence rolls, compose_planes_kernel - resized: the canvas compose and
    resample_planes_kernel - on the second group's stream): the bytes of the per-frame calls, with W2X_NO_ROLLING=1 and without, on a repeated call, pageable
    and page-locked, and with source rows wider than the frame"""
    path = onnx_model("swin_unet/art", 4, 2, 64, small=True)
    frames = sequence_frames(bits)
    size = (270, 391)
    kw = dict(out_bits=out_bits)
    monkeypatch.setenv("W2X_NO_ROLLING", "1")
    plain = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625), tta=True)
    unrolled = plain.render_sequence_planar(frames, pinned=pinned, **kw), plain.render_sequence_planar(frames, size, pinned=pinned, **kw)
    plain.close()
    monkeypatch.delenv("W2X_NO_ROLLING")
    eng = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625), tta=True)
    want = [eng.render_planar(f, **kw) for f in frames], [eng.render_planar_resized(f, size, **kw) for f in frames]
    for which, sz in enumerate((None, size)):
        for k in range(5):
            same(f"unrolled {sz} {k}", unrolled[which][k], want[which][k])
        for attempt in range(2):
            got = eng.render_sequence_planar(frames, sz, pinned=pinned, **kw)
            assert len(got) == 5
            for k in range(5):
                same(f"rolling {sz} attempt {attempt} frame {k}", got[k], want[which][k])
        wide = [tuple(np.pad(p, ((0, 0), (0, 24)))[:, :130] for p in f) for f in frames[:3]]
        assert wide[0][0].strides[0] == 154 * wide[0][0].itemsize
        for k, o in enumerate(eng.render_sequence_planar(wide, sz, **kw)):
            same(f"wide rows {sz} {k}", o, want[which][k])
    got = eng.render_sequence_planar(frames[:1], size, filter="bilinear", **kw)
    same("one frame, bilinear", got[0], eng.render_planar_resized(frames[0], size, filter="bilinear", **kw))
    mine = [tuple(np.zeros(size, DTYPES[out_bits]) for _ in range(3)) for _ in range(2)]
    assert eng.render_sequence_planar(frames[:2], size, outs=mine, **kw) is mine
    same("caller's buffers", mine[1], want[1][1])
    eng.close()


# ---- 6. destination views and plane orders
@pytest.mark.parametrize("out_bits", [8, 12, 32])
def test_destination_views_and_orders(engines, out_bits):
    eng, scale = engines("swin_x4_b2_blend")
    src = planes_of(bgr_frame(45, 57, 80, "noise"))
    want = eng.render_planar(src, out_bits=out_bits)
    H, W = want[0].shape
    dt = DTYPES[out_bits]
    # three planes cut out of ONE buffer: padded rows, plane k starting k + 1 samples into its rows
    block = np.zeros((3, H, W + 13), dt)
    views = tuple(block[k, :, k + 1:k + 1 + W] for k in range(3))
    assert eng.render_planar(src, out_bits=out_bits, dst=views) is True
    same("offset, padded views", views, want)
    for k in range(3):
        assert not block[k, :, :k + 1].any() and not block[k, :, k + 1 + W:].any()
    # every second row of a taller buffer
    tall = np.zeros((3, 2 * H, W), dt)
    assert eng.render_planar(src, out_bits=out_bits, dst=tuple(tall[k, ::2] for k in range(3))) is True
    same("every second row", tuple(tall[k, ::2] for k in range(3)), want)
    assert not tall[:, 1::2].any()
    # a padded source, and the planes in ffmpeg's order on both sides
    padded = tuple(np.pad(p, ((0, 0), (3, 20)))[:, 3:60] for p in src)
    same("padded source", eng.render_planar(padded, out_bits=out_bits), want)
    gbr = eng.render_planar((src[1], src[2], src[0]), out_bits=out_bits, order="gbr")
    same("order gbr", gbr, (want[1], want[2], want[0]))
    size = (101, 131)
    want = eng.render_planar_resized(src, size, out_bits=out_bits)
    wide = np.zeros((3, size[0], size[1] + 5), dt)
    views = tuple(wide[k, :, 1:1 + size[1]] for k in range(3))
    assert eng.render_planar_resized((src[1], src[2], src[0]), size, out_bits=out_bits, order="gbr", dst=(views[1], views[2], views[0])) is True
    same("resized, one sample in, gbr", views, want)
    assert not wide[:, :, 0].any() and not wide[:, :, 1 + size[1]:].any()
    seq = eng.render_sequence_planar([(src[1], src[2], src[0])] * 2, out_bits=out_bits, order="gbr")
    same("sequence, gbr", seq[1], gbr)


# ---- 7. kinds do not leak into each other: the captured passes of every kind on one engine and one frame size
def test_kinds_do_not_leak(engines):
    eng, scale = engines("swin_x4_b2_blend")
    r, c = 48, 64
    bgr = smooth_frame(r, c, 30)
    g = np.ascontiguousarray(bgr_frame(r, c, 31, "noise")[..., 1])
    bgra = rgba_frame(r, c, 33)
    rng = np.random.default_rng(34)
    yuv = (rng.integers(16, 236, (r, c), dtype=np.uint8), rng.integers(16, 241, (r // 2, c // 2), dtype=np.uint8), rng.integers(16, 241, (r // 2, c // 2), dtype=np.uint8))
    p8 = planes_of(bgr_frame(r, c, 35, "noise"))
    p10 = codes(r, c, 10, 36)
    first = None
    for rnd in range(3):
        got = [eng.render(bgr), eng.render_planar(p8), eng.render_yuv(*yuv), eng.render_planar(p10, bits=10, out_bits=32), eng.render_rgba(bgra), eng.render_planar(p8, out_bits=16),
               eng.render_gray(g), eng.render_planar(p10, bits=10), eng.render(bgr)]
        if first is None:
            first = got
        for k, (a, b) in enumerate(zip(got, first)):
            same(f"round {rnd} call {k}", a, b)
    same("bgr twice", first[0], first[8])
    same("planar 8", first[1], planes_of(eng.render(np.ascontiguousarray(np.stack(p8[::-1], axis=2)))))
    same("planar 10 -> float", first[3], eng.render_planar(as_float(p10, 10), out_bits=32))
    same("planar 10 -> 10", first[7], tuple(quantised(p, 10) for p in first[3]))
    same("gray", first[6], eng.render(np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2)))[..., 1])
    # a planar frame is not replayed, like a gray one
    res = np.empty((r * scale, c * scale, 3), np.uint8)
    eng.render_gray(g)
    after_gray = (eng.bench_resident(2) < 0, eng.resident_output(res))
    eng.render_planar(p8)
    assert (eng.bench_resident(2) < 0, eng.resident_output(res)) == after_gray == (True, False)
    want = eng.render(bgr)
    assert eng.bench_resident(2) > 0 and eng.resident_output(res)
    same("render() frames are still replayed", res, want)
    same("planar after a replay", eng.render_planar(p8), first[1])


# ---- 8. refusals: every text and the order of the checks, through the C entries
def test_refusals_leave_the_engine_usable(engines, pkg):
    eng, scale = engines("swin_x4_b2_blend")
    err = int(pkg.Severity.error)
    R, Cc = 40, 50
    src = planes_of(bgr_frame(R, Cc, 90, "noise"))
    src16 = tuple(p.astype(np.uint16) * 257 for p in src)
    bgr = smooth_frame(R, Cc, 91)
    before = (eng.render_planar(src), eng.render_planar(src16, out_bits=32), eng.render_planar_resized(src, (100, 150)), eng.render(bgr))
    L, h = eng._L, eng._h
    out = tuple(np.zeros((170, 210), np.float32) for _ in range(3))     # larger than any destination below

    def ptrs(planes, null=None, off=0):
        return (C.c_void_p * 3)(*[None if k == null else p.ctypes.data + off for k, p in enumerate(planes)])

    def steps(*v):
        return (C.c_size_t * 3)(*v)

    def plain(rows=R, cols=Cc, bits=8, sp=None, ss=None, orows=None, ocols=None, obits=8, dp=None, ds=None, planes=src):
        bps, obps = (4 if bits == 32 else 2 if bits > 8 else 1), (4 if obits == 32 else 2 if obits > 8 else 1)
        orows, ocols = rows * scale if orows is None else orows, cols * scale if ocols is None else ocols
        return L.w2x_render_planar(h, ptrs(planes) if sp is None else sp, steps(*[planes[0].strides[0]] * 3) if ss is None else ss, rows, cols, bits,
                                   ptrs(out) if dp is None else dp, steps(*[840] * 3) if ds is None else ds, orows, ocols, obits)

    def resized(orows=100, ocols=150, filt=0, bits=8, obits=8, sp=None, ss=None, dp=None, ds=None, rows=R, cols=Cc):
        return L.w2x_render_planar_resized(h, ptrs(src) if sp is None else sp, steps(50, 50, 50) if ss is None else ss, rows, cols, bits,
                                           ptrs(out) if dp is None else dp, steps(840, 840, 840) if ds is None else ds, orows, ocols, obits, filt)

    six = (C.c_void_p * 6)(*[p.ctypes.data for p in src + src])
    outs6 = (C.c_void_p * 6)(*[p.ctypes.data for p in out + out])

    def seq(srcs=six, dsts=outs6, count=2, rows=R, cols=Cc, bits=8, obits=8, ss=None, ds=None, orows=160, ocols=200):
        return L.w2x_render_sequence_planar(h, srcs, steps(50, 50, 50) if ss is None else ss, rows, cols, bits, dsts, steps(840, 840, 840) if ds is None else ds, orows, ocols, obits, count)

    def seq_resized(srcs=six, dsts=outs6, count=2, orows=100, ocols=150, filt=0, bits=8):
        return L.w2x_render_sequence_planar_resized(h, srcs, steps(50, 50, 50), R, Cc, bits, dsts, steps(840, 840, 840), orows, ocols, 8, count, filt)

    BITS = "Planar frames must have 8, 10, 12, 16 or 32 (float) bits."
    EMPTY = "Input image is empty."
    IN_PLANE = "Input image has a missing plane or an invalid step."
    OUT_PLANE = "Output image has a missing plane or an invalid step."
    SIZE = "Output image has invalid size: expected 200x160."
    RANGE = "Output image has invalid size for a resize: {}x{} is not between 50x40 and 200x160."
    FILTER = "Unknown resize filter {}."
    odd = np.zeros(64, np.uint8)
    cases = [
        # one thing wrong
        ("source depth 9", lambda: plain(bits=9), BITS), ("source depth 0", lambda: plain(bits=0), BITS), ("destination depth 14", lambda: plain(obits=14), BITS),
        ("destination depth 64", lambda: resized(obits=64), BITS), ("sequence: source depth 24", lambda: seq(bits=24), BITS),
        ("no rows", lambda: plain(rows=0), EMPTY), ("no columns", lambda: plain(cols=0), EMPTY), ("resized: no rows", lambda: resized(rows=0), EMPTY),
        ("sequence: no rows", lambda: seq(rows=0), EMPTY),
        ("null source plane 0", lambda: plain(sp=ptrs(src, 0)), IN_PLANE), ("null source plane 2", lambda: plain(sp=ptrs(src, 2)), IN_PLANE),
        ("null source array", lambda: L.w2x_render_planar(h, None, steps(50, 50, 50), R, Cc, 8, ptrs(out), steps(840, 840, 840), 160, 200, 8), IN_PLANE),
        ("short source step", lambda: plain(ss=steps(50, 49, 50)), IN_PLANE), ("16-bit: short source step", lambda: plain(bits=16, planes=src16, ss=steps(100, 100, 99)), IN_PLANE),
        ("16-bit: odd source step", lambda: plain(bits=10, planes=src16, ss=steps(100, 101, 100)), IN_PLANE),
        ("16-bit: odd source address", lambda: plain(bits=16, sp=ptrs(src16, off=1), ss=steps(100, 100, 100)), IN_PLANE),
        ("float: source address 2 mod 4", lambda: plain(bits=32, sp=ptrs(out, off=2), ss=steps(840, 840, 840)), IN_PLANE),
        ("null destination plane 1", lambda: plain(dp=ptrs(out, 1)), OUT_PLANE), ("short destination step", lambda: plain(ds=steps(200, 199, 200)), OUT_PLANE),
        ("16-bit: short destination step", lambda: plain(obits=12, ds=steps(400, 400, 399)), OUT_PLANE),
        ("float: short destination step", lambda: plain(obits=32, ds=steps(796, 800, 800)), OUT_PLANE),
        ("float: destination step 2 mod 4", lambda: plain(obits=32, ds=steps(840, 842, 840)), OUT_PLANE),
        ("float: destination address 2 mod 4", lambda: plain(obits=32, dp=ptrs(out, off=2)), OUT_PLANE),
        ("resized: null destination plane", lambda: resized(dp=ptrs(out, 2)), OUT_PLANE), ("resized: short destination step", lambda: resized(ds=steps(149, 150, 150)), OUT_PLANE),
        ("one row too many", lambda: plain(orows=161), SIZE), ("one column short", lambda: plain(ocols=199), SIZE), ("the input's size", lambda: plain(orows=40, ocols=50), SIZE),
        ("sequence: one row too many", lambda: seq(orows=161), SIZE),
        ("resized: one row too many", lambda: resized(orows=161), RANGE.format(150, 161)), ("resized: one column too many", lambda: resized(ocols=201), RANGE.format(201, 100)),
        ("resized: fewer rows than the input", lambda: resized(orows=39), RANGE.format(150, 39)), ("resized: no columns", lambda: resized(ocols=0), RANGE.format(0, 100)),
        ("sequence: too large", lambda: seq_resized(orows=161), RANGE.format(150, 161)),
        ("filter 2", lambda: resized(filt=2), FILTER.format(2)), ("filter -1", lambda: resized(filt=-1), FILTER.format(-1)), ("sequence: filter 2", lambda: seq_resized(filt=2), FILTER.format(2)),
        ("sequence: a null plane in frame 1", lambda: seq(srcs=(C.c_void_p * 6)(*[p.ctypes.data for p in src], src[0].ctypes.data, None, src[2].ctypes.data)), IN_PLANE),
        ("sequence: a null destination plane in frame 1", lambda: seq(dsts=(C.c_void_p * 6)(*[p.ctypes.data for p in out], out[0].ctypes.data, out[1].ctypes.data, None)), OUT_PLANE),
        # two things wrong: the order of the checks - the filter (at the entry), the depths, the empty frame, the target, then per frame source before destination
        ("filter before depth", lambda: resized(filt=5, bits=9), FILTER.format(5)), ("depth before empty", lambda: plain(bits=9, rows=0), BITS),
        ("destination depth before empty", lambda: plain(obits=9, cols=0), BITS), ("empty before a null plane", lambda: plain(rows=0, sp=ptrs(src, 0)), EMPTY),
        ("depth before the target", lambda: resized(obits=11, orows=500), BITS), ("empty before the target", lambda: resized(rows=0, orows=500), EMPTY),
        ("target before a null source plane", lambda: resized(orows=161, sp=ptrs(src, 1)), RANGE.format(150, 161)),
        ("target before a null destination plane", lambda: resized(ocols=49, dp=ptrs(out, 0)), RANGE.format(49, 100)),
        ("source plane before the output size", lambda: plain(sp=ptrs(src, 1), orows=161), IN_PLANE), ("source step before destination plane", lambda: plain(ss=steps(49, 50, 50), dp=ptrs(out, 0)), IN_PLANE),
        ("output size before destination plane", lambda: plain(ocols=201, dp=ptrs(out, 0)), SIZE), ("output size before destination step", lambda: plain(orows=159, ds=steps(1, 1, 1)), SIZE),
    ]
    for name, call, text in cases:
        n = len(eng.messages)
        assert call() == 0, name
        new = [m for s, m in eng.messages[n:] if s == err]
        assert len(new) == 1, (name, new)
        assert new[0].startswith("[") and "@" in new[0].split("]")[0] and new[0].split("] ", 1)[1] == text, (name, new[0])
    # frames of a sequence that differ, through the C++ record the ABI cannot express: the wrapper's ValueError names size, depth and strides
    with pytest.raises(ValueError, match="one size, one depth"):
        eng.render_sequence_planar([src, tuple(np.zeros((R, Cc + 1), np.uint8) for _ in range(3))])
    with pytest.raises(ValueError, match="one size, one depth"):
        eng.render_sequence_planar([src16, src], bits=16)
    # the count and the arrays of the sequence entries: what the neighbouring entries answer - 0 without a message for a negative count or a null array of a
    # non-empty sequence; an empty sequence is done, and touches nothing
    n = len(eng.messages)
    assert seq(count=-1) == 0 and seq(srcs=None) == 0 and seq(dsts=None) == 0
    assert seq_resized(count=-1) == 0 and seq_resized(srcs=None) == 0 and seq_resized(dsts=None) == 0
    assert seq(count=0, srcs=None, dsts=None) == L.w2x_render_sequence(h, None, 40, 50, 150, None, 600, 0) == 1
    assert seq_resized(count=0, srcs=None, dsts=None) == 1
    assert len(eng.messages) == n
    # the wrapper: a destination of another size is refused with the engine's message, a filter it does not know raises
    for shape in ((161, 200), (160, 199)):
        n = len(eng.messages)
        assert eng.render_planar(src, dst=tuple(np.zeros(shape, np.uint8) for _ in range(3))) is False
        assert [m for s, m in eng.messages[n:] if s == err][-1].endswith(SIZE)
    with pytest.raises(ValueError):
        eng.render_planar_resized(src, (100, 150), filter="lanczos")
    with pytest.raises(pkg.W2xError, match="not between"):
        eng.render_planar_resized(src, (161, 150))
    fresh = pkg.Img2Img()
    assert fresh.render_planar(src, dst=tuple(np.zeros((160, 200), np.uint8) for _ in range(3))) is False and "before a successful load" in fresh.last_error()
    fresh.close()
    after = (eng.render_planar(src), eng.render_planar(src16, out_bits=32), eng.render_planar_resized(src, (100, 150)), eng.render(bgr))
    for k, (a, b) in enumerate(zip(after, before)):
        same(f"after the refusals, call {k}", a, b)
    same("a sequence after the refusals", eng.render_sequence_planar([src, src])[1], before[0])


def test_single_calls_report_progress_like_render(engines):
    eng, scale = engines("cunet_x2_b3_noblend_tta")
    bgr = bgr_frame(61, 83, 95)
    seen = {}
    for name, call in (("render", lambda: eng.render(bgr)), ("planar", lambda: eng.render_planar(planes_of(bgr), out_bits=10)),
                       ("resized", lambda: eng.render_planar_resized(planes_of(bgr), (100, 131), out_bits=32))):
        prog = []
        eng.setProgressCallback(lambda c, t, s: prog.append((c, t)))
        call()
        eng.setProgressCallback(None)
        seen[name] = prog
    assert seen["render"] and seen["planar"] == seen["render"] == seen["resized"]


# ---- 9. the command line
FAKE_FFPROBE = """#!/usr/bin/env python3
# stand-in for ffprobe on a raw clip: width,height,r_frame_rate,nb_read_packets like `-of csv=p=0`
import os
print(f"{os.environ['FAKE_W']},{os.environ['FAKE_H']},30/1,{os.environ['FAKE_FRAMES']}")
"""


def fake_tools(tmp_path, W, H, frames):
    bindir = tmp_path / "bin"; bindir.mkdir()
    for name, text in (("ffprobe", FAKE_FFPROBE), ("ffmpeg", FAKE_FFMPEG)):
        (bindir / name).write_text(text); (bindir / name).chmod(0o755)
    log = tmp_path / "argv.jsonl"
    return log, dict(os.environ, PATH=f"{bindir}:{os.environ['PATH']}", FAKE_W=str(W), FAKE_H=str(H), FAKE_FRAMES=str(frames), FAKE_LOG=str(log))


def test_cli_planar_video(pkg, tmp_path):
    """`w2x render --rgb-in gbrp10le --rgb-out gbrp16le` on a clip read through ffmpeg (fake ffmpeg / ffprobe scripts stand in for the pipes and log their
    arguments): raw planar frames in - planes G, B, R, contiguous -, renderSequencePlanar[Resized] in the chunks of the bgr24 loop (6 frames: a full chunk of 4
    and a ragged one), raw planar frames out"""
    W, H, N = 100, 70, 6
    frames = [codes(H, W, 10, 100 + k) for k in range(N)]                                   # (R, G, B)
    (tmp_path / "clip.mkv").write_bytes(b"".join(f[k].tobytes() for f in frames for k in (1, 2, 0)))
    log, env = fake_tools(tmp_path, W, H, N)
    common, eng = w2x_setup(pkg, tmp_path, env)
    for k, (extra, size, tag) in enumerate((((), (4 * H, 4 * W), ""), (("--outsize", "250x175"), (175, 250), "(250x175)"))):
        log.write_text("")
        out = tmp_path / f"v{k}"; out.mkdir()
        r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "clip.mkv"), "-o", str(out), "--rgb-in", "gbrp10le", "--rgb-out", "gbrp16le", *extra],
                           capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr
        raw = np.frombuffer((out / f"clip{TAG}{tag}.mp4").read_bytes(), np.uint16)
        assert raw.size == N * 3 * size[0] * size[1]
        got = raw.reshape(N, 3, *size)
        want = eng.render_sequence_planar(frames, None if not extra else size, bits=10, out_bits=16)
        for i in range(N):
            same(f"video frame {i} {extra}", (got[i, 2], got[i, 0], got[i, 1]), want[i])
        calls = [json.loads(line) for line in log.read_text().splitlines()]
        reader = next(c for c in calls if c[c.index("-i") + 1] != "-")
        writer = next(c for c in calls if c[c.index("-i") + 1] == "-")
        assert reader[reader.index("-pix_fmt") + 1] == "gbrp10le" and reader[reader.index("-f") + 1] == "rawvideo"
        i = writer.index("-i")
        assert writer[writer.index("-f") + 1] == "rawvideo" and writer.index("-f") < i
        assert writer[writer.index("-pix_fmt") + 1] == "gbrp16le" and writer.index("-pix_fmt") < i
        assert writer[writer.index("-s") + 1] == f"{size[1]}x{size[0]}" and writer.index("-s") < i
        # no --pix_fmt given: the encoder's format defaults to the --rgb-out format
        assert writer[i + 1:].count("-pix_fmt") == 1 and writer[i + 1:][writer[i + 1:].index("-pix_fmt") + 1] == "gbrp16le"
    eng.close()


def test_cli_planar_leaves_a_still_read_through_ffmpeg_alone(pkg, tmp_path):
    """a single frame read through ffmpeg is a still like any other: under --rgb-in / --rgb-out the reader is still asked for bgr24 and the bytes are render()'s"""
    W, H = 100, 70
    bgr = smooth_frame(H, W, 95)
    (tmp_path / "cover.jpg").write_bytes(bgr.tobytes())
    log, env = fake_tools(tmp_path, W, H, 1)
    common, eng = w2x_setup(pkg, tmp_path, env)
    want = eng.render(bgr)
    log.write_text("")
    out = tmp_path / "s"; out.mkdir()
    r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "cover.jpg"), "-o", str(out), "--rgb-in", "gbrp", "--rgb-out", "gbrpf32le"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    raw = np.frombuffer((out / f"cover{TAG}.png").read_bytes(), np.uint8)
    assert raw.size == want.size
    same("a still through ffmpeg", raw.reshape(want.shape), want)
    calls = [json.loads(line) for line in log.read_text().splitlines()]
    reader = next(c for c in calls if c[c.index("-i") + 1] != "-")
    writer = next(c for c in calls if c[c.index("-i") + 1] == "-")
    assert reader[reader.index("-pix_fmt") + 1] == "bgr24" and writer[writer.index("-pix_fmt") + 1] == "bgr24"
    eng.close()
