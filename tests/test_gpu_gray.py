"""Gray frames on the GPU (Img2Img::renderGray / renderGrayResized / renderSequenceGray*).  The contract: for rep(g) the BGR frame with
B = G = R = g, render_gray(g) is the green channel of render(rep(g)) and render_gray_resized(g, size, f) the green channel of
render_resized(rep(g), size, f).  The reference is the engine's own render() / render_resized(), which the rest of the suite holds to the oracle, and every
comparison is equality on every byte: there is no tolerance.  Engines: the small synthetic graphs at tile 64."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_parity import make_engine, smooth_frame
from test_gpu_rgba import W2X, rgba_frame

pytestmark = pytest.mark.gpu

# name -> (model, scale, batch, tile, small, precision, load options)
CONFIGS = {
    "swin_x4_b2_blend": ("swin_unet/art", 4, 2, 64, True, None, dict(overlap=(0.0625, 0.0625))),
    "swin_x4_b2_tta": ("swin_unet/art", 4, 2, 64, True, None, dict(overlap=(0.0625, 0.0625), tta=True)),
    # (batch 3, not 2: the models are exported once per session and engine files lie next to them - test_gpu_parity.test_error_paths expects no fp16 engine
    #  beside the cunet x2 batch-2 model when it starts)
    "cunet_x2_b3_noblend_tta": ("cunet/art", 2, 3, 64, False, None, dict(overlap=(0.0, 0.0), tta=True)),
    "cunet_x1_b2_blend": ("cunet/art", 1, 2, 64, False, None, dict(overlap=(0.0625, 0.0625))),
    "cunet_x2_b1_fp32": ("cunet/art", 2, 1, 64, False, "FP32", dict(overlap=(0.0625, 0.0625))),
}


@pytest.fixture(scope="module")
def engines(pkg, onnx_model):
    made = {}

    def get(name):
        if name not in made:
            model, scale, batch, tile, small, precision, kw = CONFIGS[name]
            path = onnx_model(model, scale, batch, tile, small=small)
            if precision is None:
                eng = make_engine(pkg, path, batch, tile, scale, **kw)
            else:
                prec = getattr(pkg.Precision, precision)
                eng = pkg.Img2Img()
                assert eng.build(path, pkg.BuildConfig.fixed(batch, tile, precision=prec)), eng.last_error()
                assert eng.load(path, pkg.RenderConfig(precision=prec, batchSize=batch, height=tile, width=tile, scaling=scale, **kw)), eng.last_error()
            made[name] = (eng, scale)
        return made[name]
    yield get
    for eng, _ in made.values():
        eng.close()


def gray_frame(rows, cols, seed, kind="smooth", dtype=np.uint8):
    if kind == "smooth":
        g = smooth_frame(rows, cols, seed)[..., 1]
        return np.ascontiguousarray(g) if dtype == np.uint8 else (g.astype(np.uint16) * 257)
    return np.random.default_rng(seed).integers(0, np.iinfo(dtype).max + 1, (rows, cols), dtype=dtype)


def rep(g):
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2))


def same(tag, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    bad = got != want
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {bad.size} samples differ, first at {tuple(np.argwhere(bad)[0])}, max |d| {int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max())}"


# ---- 1. 8-bit frames against the green channel of render()
@pytest.mark.parametrize("name,rows,cols", [("swin_x4_b2_blend", 45, 57), ("swin_x4_b2_blend", 40, 141), ("cunet_x2_b3_noblend_tta", 61, 83),
                                            ("cunet_x1_b2_blend", 37, 541), ("cunet_x2_b1_fp32", 57, 70)])
def test_render_gray_is_the_green_channel_of_render(engines, name, rows, cols):
    eng, scale = engines(name)
    for seed, kind in ((1, "smooth"), (2, "noise")):
        g = gray_frame(rows, cols, seed, kind)
        out = eng.render_gray(g)
        assert out.shape == (rows * scale, cols * scale)
        same(f"{name} {rows}x{cols} {kind}", out, eng.render(rep(g))[..., 1])


# ---- 2. 16-bit frames
# (cunet_x1_b2_blend at 37 x 541: no TTA, blended, a ragged last group next to fast-path groups - a 16-bit frame on the four-pixel fast path)
@pytest.mark.parametrize("name,rows,cols", [("swin_x4_b2_blend", 45, 57), ("cunet_x2_b3_noblend_tta", 61, 83), ("cunet_x1_b2_blend", 37, 541)])
def test_render_gray_at_16_bits(engines, name, rows, cols):
    eng, scale = engines(name)
    g = gray_frame(rows, cols, 3, "noise", np.uint16)
    out = eng.render_gray(g)
    assert out.dtype == np.uint16
    same(f"{name} 16-bit", out, eng.render(rep(g))[..., 1])


# ---- 3. destination views: padded rows, and rows that start one byte into an aligned buffer.  (The caller's view is the target of the 2-D copy down; the kernels
#         write the engine's own aligned buffer, where only the ragged right end - 228 = 4 * 57 columns here has none, 131 below has - stores sample by sample.)
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_destination_views(engines, dtype):
    eng, scale = engines("swin_x4_b2_blend")
    g = gray_frame(45, 57, 4, "noise", dtype)
    want = eng.render_gray(g)
    H, W = want.shape
    wide = np.zeros((H, W + 13), dtype)
    assert eng.render_gray(g, dst=wide[:, :W]) is True
    same("padded rows", wide[:, :W], want)
    assert not wide[:, W:].any()
    raw = np.zeros((H, (W + 8) * np.dtype(dtype).itemsize), np.uint8)                  # one BYTE into the buffer: a 16-bit row is then not even 2-byte aligned
    if dtype == np.uint8:
        view = raw[:, 1:1 + W]
        assert eng.render_gray(g, dst=view) is True
        same("one byte in", view, want)
        assert not raw[:, 0].any() and not raw[:, 1 + W:].any()
    else:
        view = raw[:, 2:2 + 2 * W].view(np.uint16)                                      # one SAMPLE in: 2-byte aligned, never 8-byte aligned at the row start
        assert eng.render_gray(g, dst=view) is True
        same("one sample in", view, want)
        assert not raw[:, :2].any() and not raw[:, 2 + 2 * W:].any()
    src = np.zeros((45, 80), dtype); src[:, 3:60] = g                                   # a source view with padded rows
    same("padded source", eng.render_gray(src[:, 3:60]), want)
    # the resized call through the same views
    size = (101, 131)
    want = eng.render_gray_resized(g, size)
    wide = np.zeros((size[0], size[1] + 5), dtype)
    assert eng.render_gray_resized(g, size, dst=wide[:, 1:1 + size[1]]) is True
    same("resized, one sample in", wide[:, 1:1 + size[1]], want)
    assert not wide[:, 0].any() and not wide[:, 1 + size[1]:].any()


# ---- 4. resized
def targets(r, c):
    return [(3 * r, 3 * c), (2 * r, 2 * c), (r * 5 // 2, 4 * c), (2 * r + 1, 2 * c + 1), (r, c)]


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
def test_resized_is_the_green_channel_of_render_resized(engines, filt):
    eng, scale = engines("swin_x4_b2_blend")
    cases = [((50, 66), targets(50, 66)), ((45, 57), targets(45, 57)), ((40, 141), [(90, 530), (81, 333)])]
    for k, ((r, c), sizes) in enumerate(cases):
        g = gray_frame(r, c, 10 + k, "noise" if k % 2 else "smooth")
        bgr = rep(g)
        for size in sizes:
            out = eng.render_gray_resized(g, size, filt)
            assert out.shape == size
            same(f"{r}x{c} -> {size} {filt}", out, eng.render_resized(bgr, size, filt)[..., 1])
        same("scaled size", eng.render_gray_resized(g, (r * scale, c * scale), filt), eng.render_gray(g))


def test_resized_16_bit_and_fp32(engines):
    eng, _ = engines("swin_x4_b2_blend")
    g = gray_frame(45, 57, 20, "noise", np.uint16)
    same("16-bit resized", eng.render_gray_resized(g, (113, 150)), eng.render_resized(rep(g), (113, 150))[..., 1])
    eng, _ = engines("cunet_x2_b1_fp32")
    g = gray_frame(57, 70, 21)
    for size, filt in (((90, 113), "bilinear"), ((57, 139), "bicubic")):
        same(f"fp32 -> {size}", eng.render_gray_resized(g, size, filt), eng.render_resized(rep(g), size, filt)[..., 1])


# ---- 5. sequences
@pytest.mark.parametrize("pinned", [False, True])
def test_rolling_sequence_matches_single_frames(pkg, onnx_model, monkeypatch, pinned):
    """five 90 x 130 frames on swin x4 with TTA (48 slots of one pass: the sequence rolls, compose_planes_kernel at one plane - resized: the canvas compose and
    resample_planes_kernel - on the second group's stream): the bytes of the per-frame calls, with W2X_NO_ROLLING=1 and without, on a repeated call, pageable and
    page-locked, and with source rows wider than the frame"""
    path = onnx_model("swin_unet/art", 4, 2, 64, small=True)
    frames = [gray_frame(90, 130, 50 + k, "noise" if k % 2 else "smooth") for k in range(5)]
    size = (270, 391)
    monkeypatch.setenv("W2X_NO_ROLLING", "1")
    plain = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625), tta=True)
    unrolled = plain.render_sequence_gray(frames, pinned=pinned), plain.render_sequence_gray(frames, size=size, pinned=pinned)
    plain.close()
    monkeypatch.delenv("W2X_NO_ROLLING")
    eng = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625), tta=True)
    want = [eng.render_gray(f) for f in frames], [eng.render_gray_resized(f, size) for f in frames]
    same("frame 0 against render()", want[0][0], eng.render(rep(frames[0]))[..., 1])
    same("frame 0 against render_resized()", want[1][0], eng.render_resized(rep(frames[0]), size)[..., 1])
    for which, sz in enumerate((None, size)):
        for k in range(5):
            same(f"unrolled {sz} {k}", unrolled[which][k], want[which][k])
        for attempt in range(2):
            got = eng.render_sequence_gray(frames, size=sz, pinned=pinned)
            assert len(got) == 5
            for k in range(5):
                same(f"rolling {sz} attempt {attempt} frame {k}", got[k], want[which][k])
        wide = [np.pad(f, ((0, 0), (0, 24)))[:, :130] for f in frames[:3]]
        assert wide[0].strides[0] == 154
        for k, o in enumerate(eng.render_sequence_gray(wide, size=sz)):
            same(f"wide rows {sz} {k}", o, want[which][k])
    # short sequences
    for n in (1, 3):
        for which, sz in enumerate((None, size)):
            got = eng.render_sequence_gray(frames[:n], size=sz, filter="bicubic")
            assert len(got) == n
            for k in range(n):
                same(f"count {n} {sz} {k}", got[k], want[which][k])
    bil = eng.render_sequence_gray(frames[:2], size=size, filter="bilinear")
    for k in range(2):
        same(f"bilinear {k}", bil[k], eng.render_gray_resized(frames[k], size, "bilinear"))
    mine = [np.zeros(size, np.uint8) for _ in range(2)]
    assert eng.render_sequence_gray(frames[:2], size=size, outs=mine) is mine
    same("caller's buffers", mine[1], want[1][1])
    eng.close()


# ---- 6. kinds do not leak into each other: the captured passes of every kind on one engine and one frame size
def test_kinds_do_not_leak(engines):
    eng, scale = engines("swin_x4_b2_blend")
    r, c = 48, 64
    bgr = smooth_frame(r, c, 30)
    g = gray_frame(r, c, 31, "noise")
    g16 = gray_frame(r, c, 32, "noise", np.uint16)
    bgra = rgba_frame(r, c, 33)
    rng = np.random.default_rng(34)
    yuv = (rng.integers(16, 236, (r, c), dtype=np.uint8), rng.integers(16, 241, (r // 2, c // 2), dtype=np.uint8), rng.integers(16, 241, (r // 2, c // 2), dtype=np.uint8))
    first = None
    for rnd in range(3):
        got = [eng.render(bgr), eng.render_gray(g), eng.render_rgba(bgra), eng.render_yuv(*yuv), eng.render_gray(g16), eng.render(bgr)]
        flat = [np.concatenate([p.ravel() for p in x]) if isinstance(x, tuple) else x for x in got]
        if first is None:
            first = flat
        for k, (a, b) in enumerate(zip(flat, first)):
            same(f"round {rnd} call {k}", a, b)
    same("bgr twice", first[0], first[5])
    same("gray", first[1], eng.render(rep(g))[..., 1])
    same("gray 16", first[4], eng.render(rep(g16))[..., 1])
    same("rgba colour", first[2][..., :3], eng.render(np.ascontiguousarray(bgra[..., :3])))
    same("rgba alpha", first[2][..., 3], eng.render_gray(np.ascontiguousarray(bgra[..., 3])))


# ---- 7. refusals
def test_refusals_leave_the_engine_usable(engines, pkg):
    eng, scale = engines("swin_x4_b2_blend")
    err = int(pkg.Severity.error)
    g = gray_frame(40, 50, 40, "noise")
    bgr = smooth_frame(40, 50, 41)
    bgra = rgba_frame(40, 50, 42)
    before = (eng.render_gray(g), eng.render(bgr), eng.render_resized(bgr, (100, 150)), eng.render_rgba(bgra))
    L, h = eng._L, eng._h
    out = np.zeros((170, 210), np.uint16)                                   # larger than any destination below

    def plain(rows=40, cols=50, step=50, dstep=200, src=g, deep=False):
        fn = L.w2x_render_gray16 if deep else L.w2x_render_gray
        return fn(h, src.ctypes.data if src is not None else None, rows, cols, step, out.ctypes.data, dstep)

    def resized(orows=100, ocols=150, step=50, dstep=None, filt=0, src=g, rows=40, cols=50, deep=False):
        fn = L.w2x_render_gray16_resized if deep else L.w2x_render_gray_resized
        return fn(h, src.ctypes.data if src is not None else None, rows, cols, step, out.ctypes.data, orows, ocols, ocols if dstep is None else dstep, filt)

    two = (C.c_void_p * 2)(g.ctypes.data, g.ctypes.data)
    outs2 = (C.c_void_p * 2)(out.ctypes.data, out.ctypes.data)

    def seq(srcs=two, dsts=outs2, count=2, rows=40, cols=50, step=50, dstep=200):
        return L.w2x_render_sequence_gray(h, srcs, rows, cols, step, dsts, dstep, count)

    def seq_resized(srcs=two, dsts=outs2, count=2, orows=100, ocols=150, filt=0, step=50):
        return L.w2x_render_sequence_gray_resized(h, srcs, 40, 50, step, dsts, orows, ocols, ocols, count, filt)

    # refused by the engine, with a message
    cases = {
        "resized: one row too many": lambda: resized(orows=161), "resized: one column too many": lambda: resized(ocols=201),
        "resized: fewer rows than the input": lambda: resized(orows=39), "resized: fewer columns than the input": lambda: resized(ocols=49),
        "resized: no rows": lambda: resized(orows=0), "no rows": lambda: plain(rows=0), "no columns": lambda: plain(cols=0),
        "short source step": lambda: plain(step=49), "short destination step": lambda: plain(dstep=199),
        "16-bit: short source step": lambda: plain(step=99, deep=True), "16-bit: short destination step": lambda: plain(dstep=399, deep=True),
        "resized: short source step": lambda: resized(step=49), "resized: short destination step": lambda: resized(dstep=149),
        "null frame": lambda: plain(src=None), "resized: null frame": lambda: resized(src=None),
        "filter 2": lambda: resized(filt=2), "filter -1": lambda: resized(filt=-1), "16-bit: filter 2": lambda: resized(filt=2, deep=True),
        "sequence: short source step": lambda: seq(step=49), "sequence: short destination step": lambda: seq(dstep=199), "sequence: no rows": lambda: seq(rows=0),
        "sequence: too large": lambda: seq_resized(orows=161), "sequence: filter 2": lambda: seq_resized(filt=2), "sequence: filter -1": lambda: seq_resized(filt=-1),
        "sequence: a null frame": lambda: seq(srcs=(C.c_void_p * 2)(g.ctypes.data, None)),
    }
    for name, call in cases.items():
        n = len(eng.messages)
        assert call() == 0, name
        new = [m for s, m in eng.messages[n:] if s == err]
        assert new, name
    # the plain call's destination is sized by the entry (rows * scale x cols * scale): a wrong one is what the wrapper refuses, with the engine's message
    for shape in ((161, 200), (160, 201), (159, 200), (160, 199)):
        n = len(eng.messages)
        assert eng.render_gray(g, dst=np.zeros(shape, np.uint8)) is False
        assert "invalid size" in [m for s, m in eng.messages[n:] if s == err][-1]
    # the count and the arrays of the sequence entries: what the neighbouring entries (w2x_render_sequence*) answer - 0 for a negative count or a null array
    # of a non-empty sequence; an empty sequence is done, and touches nothing
    assert seq(count=-1) == 0 and seq(srcs=None) == 0 and seq(dsts=None) == 0
    assert seq_resized(count=-1) == 0 and seq_resized(srcs=None) == 0 and seq_resized(dsts=None) == 0
    assert seq(count=0, srcs=None, dsts=None) == L.w2x_render_sequence(h, None, 40, 50, 150, None, 600, 0) == 1
    assert seq(srcs=None) == L.w2x_render_sequence(h, None, 40, 50, 150, outs2, 600, 2) == 0
    # a sequence at 16 bits: the wrapper's ValueError (the C entries carry 8-bit frames only); frames that differ
    with pytest.raises(ValueError):
        eng.render_sequence_gray([g.astype(np.uint16)] * 2)
    with pytest.raises(ValueError):
        eng.render_sequence_gray([g, gray_frame(40, 51, 43)])
    with pytest.raises(ValueError):
        eng.render_gray_resized(g, (100, 150), filter="lanczos")
    fresh = pkg.Img2Img()
    assert fresh.render_gray(g, dst=np.zeros((160, 200), np.uint8)) is False and "before a successful load" in fresh.last_error()
    fresh.close()
    after = (eng.render_gray(g), eng.render(bgr), eng.render_resized(bgr, (100, 150)), eng.render_rgba(bgra))
    for k, (a, b) in enumerate(zip(after, before)):
        same(f"after the refusals, call {k}", a, b)
    same("a sequence after the refusals", eng.render_sequence_gray([g, g])[1], before[0])


# ---- 8. the command line
FAKE_FFPROBE = """#!/usr/bin/env python3
# stand-in for ffprobe on a raw gray clip: width,height,r_frame_rate,nb_read_packets like `-of csv=p=0`
import os, sys
w, h = int(os.environ["FAKE_W"]), int(os.environ["FAKE_H"])
print(f"{w},{h},30/1,{os.environ.get('FAKE_FRAMES') or os.path.getsize(sys.argv[-1]) // (w * h)}")
"""

FAKE_FFMPEG = """#!/usr/bin/env python3
# stand-in for ffmpeg: logs its argv; `-i FILE ... -` copies the raw clip to stdout, `-i - ... OUT` copies stdin to OUT
import json, os, shutil, sys
a = sys.argv[1:]
with open(os.environ["FAKE_LOG"], "a") as f: f.write(json.dumps(a) + "\\n")
src = a[a.index("-i") + 1]
if src == "-":
    with open(a[-1], "wb") as f: shutil.copyfileobj(sys.stdin.buffer, f)
else:
    with open(src, "rb") as f: shutil.copyfileobj(f, sys.stdout.buffer)
"""
TAG = "(swin_unet_art)(noise3)(scale4)"


def w2x_setup(pkg, tmp_path, env=None):
    """the small swin x4 model built through the command line, and an engine loaded from the same file"""
    import synth_models as sm
    path = sm.model_path(str(tmp_path), "swin_unet/art", 4, 3)
    sm.export_onnx(sm.make_model("swin_unet/art", 4, seed=5, small=True), path, 2, 64, dynamic=True)
    common = ["--models", str(tmp_path / "models"), "--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "2", "--tileSize", "64"]
    r = subprocess.run([W2X, *common, "build"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    eng = pkg.Img2Img()
    assert eng.load(path, pkg.RenderConfig(batchSize=2, height=64, width=64, scaling=4)), eng.last_error()
    return common, eng


def test_cli_gray_stills(pkg, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    common, eng = w2x_setup(pkg, tmp_path)
    g = gray_frame(45, 57, 70)
    g16 = gray_frame(45, 57, 71, "noise", np.uint16)
    bgr = smooth_frame(45, 57, 72)
    ga = np.stack([g, gray_frame(45, 57, 73, "noise")], axis=-1)
    Image.fromarray(g).save(tmp_path / "g.png")
    Image.fromarray(g16).save(tmp_path / "h.png")
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(tmp_path / "c.png")
    Image.fromarray(ga, "LA").save(tmp_path / "la.png")
    assert Image.open(tmp_path / "g.png").mode == "L" and Image.open(tmp_path / "h.png").mode.startswith("I;16") and Image.open(tmp_path / "la.png").mode == "LA"
    runs = []

    def run(name, *extra):
        out = tmp_path / f"o{len(runs)}"; out.mkdir(); runs.append(out)
        r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / name), "-o", str(out), *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        files = sorted(os.listdir(out))
        assert len(files) == 1, files
        return files[0], Image.open(out / files[0])

    name, im = run("g.png", "--gray")
    assert name == f"g{TAG}.png" and im.mode == "L"
    same("--gray", np.array(im), eng.render_gray(g))
    name, im = run("g.png", "--gray", "--outsize", "151x99")
    assert name == f"g{TAG}(151x99).png" and im.mode == "L"
    same("--gray --outsize", np.array(im), eng.render_gray_resized(g, (99, 151)))
    name, im = run("h.png", "--gray", "--deep")
    assert name == f"h{TAG}.png" and im.mode.startswith("I;16")
    same("--gray --deep", np.array(im).astype(np.uint16), eng.render_gray(g16))
    # without the flag, and with it on files that are not gray: the outputs of today
    name, im = run("g.png")
    assert name == f"g{TAG}.png" and im.mode == "RGB"
    same("a gray PNG without --gray", np.array(im), np.ascontiguousarray(eng.render(rep(g))[..., ::-1]))
    name, im = run("c.png", "--gray")
    assert im.mode == "RGB"
    same("a colour PNG with --gray", np.array(im), np.ascontiguousarray(eng.render(bgr)[..., ::-1]))
    want = eng.render_rgba(np.ascontiguousarray(np.concatenate([rep(ga[..., 0]), ga[..., 1:]], axis=2)))      # gray + alpha: the RGBA route of today
    for extra in ((), ("--gray",)):
        name, im = run("la.png", *extra)
        assert im.mode == "RGBA"
        same(f"gray + alpha {extra}", np.array(im), np.ascontiguousarray(want[..., [2, 1, 0, 3]]))
    eng.close()


def test_cli_deep_rgba_takes_the_gray_alpha_route(pkg, tmp_path):
    """a 16-bit RGBA PNG under --deep takes the two-call route, whose alpha call is now renderGray on the 8-bit alpha plane: colour is render() at 16 bits,
    alpha the green channel of render() of the replicated 8-bit alpha - what the route gave before"""
    import struct
    import zlib
    common, eng = w2x_setup(pkg, tmp_path)
    rng = np.random.default_rng(80)
    rgb16 = rng.integers(0, 65536, (41, 53, 3), dtype=np.uint16)
    a8 = rgba_frame(41, 53, 81)[..., 3].copy()
    rgba16 = np.concatenate([rgb16, (a8.astype(np.uint16) * 257)[..., None]], axis=2)

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))
    raw = b"".join(b"\x00" + row.astype(">u2").tobytes() for row in rgba16)
    (tmp_path / "d.png").write_bytes(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 53, 41, 16, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))
    out = tmp_path / "o"; out.mkdir()
    r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "d.png"), "-o", str(out), "--deep"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    # the 16-bit RGBA PNG back by hand (the writer uses filter 0 on every row)
    data = (out / f"d{TAG}.png").read_bytes()
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        n, t = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if t == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", data[pos + 8:pos + 8 + n])
        if t == b"IDAT":
            idat += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    assert hdr[:4] == (53 * 4, 41 * 4, 16, 6)
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(41 * 4, 1 + 53 * 4 * 8)
    assert not rows[:, 0].any()
    got = np.ascontiguousarray(rows[:, 1:]).view(">u2").reshape(41 * 4, 53 * 4, 4).astype(np.uint16)
    same("colour", got[..., :3], np.ascontiguousarray(eng.render(np.ascontiguousarray(rgb16[..., ::-1]))[..., ::-1]))
    same("alpha", got[..., 3], eng.render(rep(a8))[..., 1].astype(np.uint16) * 257)
    eng.close()


def test_cli_gray_video(pkg, tmp_path):
    """`w2x render --gray` on a clip read through ffmpeg (fake ffmpeg / ffprobe scripts stand in for the pipes and log their arguments): raw gray frames in,
    renderSequenceGray[Resized] in the chunks of the bgr24 loop (6 frames: a full chunk of 4 and a ragged one), raw gray frames out"""
    import json
    W, H, N = 100, 70, 6
    frames = [gray_frame(H, W, 90 + k, "noise" if k % 2 else "smooth") for k in range(N)]
    (tmp_path / "clip.mkv").write_bytes(b"".join(f.tobytes() for f in frames))
    bindir = tmp_path / "bin"; bindir.mkdir()
    for name, text in (("ffprobe", FAKE_FFPROBE), ("ffmpeg", FAKE_FFMPEG)):
        (bindir / name).write_text(text); (bindir / name).chmod(0o755)
    log = tmp_path / "argv.jsonl"
    env = dict(os.environ, PATH=f"{bindir}:{os.environ['PATH']}", FAKE_W=str(W), FAKE_H=str(H), FAKE_LOG=str(log))
    common, eng = w2x_setup(pkg, tmp_path, env)
    for k, (extra, size, tag) in enumerate((((), (4 * H, 4 * W), ""), (("--outsize", "250x175"), (175, 250), "(250x175)"))):
        log.write_text("")
        out = tmp_path / f"v{k}"; out.mkdir()
        r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "clip.mkv"), "-o", str(out), "--gray", *extra], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr
        raw = np.frombuffer((out / f"clip{TAG}{tag}.mp4").read_bytes(), np.uint8)
        assert raw.size == N * size[0] * size[1]
        got = raw.reshape(N, *size)
        for i, f in enumerate(frames):
            same(f"video frame {i} {extra}", got[i], eng.render_gray(f) if not extra else eng.render_gray_resized(f, size))
        calls = [json.loads(line) for line in log.read_text().splitlines()]
        reader = next(c for c in calls if c[c.index("-i") + 1] != "-")
        writer = next(c for c in calls if c[c.index("-i") + 1] == "-")
        assert reader[reader.index("-pix_fmt") + 1] == "gray" and reader[reader.index("-f") + 1] == "rawvideo"
        i = writer.index("-i")
        assert writer[writer.index("-f") + 1] == "rawvideo" and writer.index("-f") < i
        assert writer[writer.index("-pix_fmt") + 1] == "gray" and writer.index("-pix_fmt") < i
        assert writer[writer.index("-s") + 1] == f"{size[1]}x{size[0]}" and writer.index("-s") < i
        assert writer[i + 1:].count("-pix_fmt") == 1 and writer[i + 1:][writer[i + 1:].index("-pix_fmt") + 1] == "yuv420p"      # --pix_fmt stays the encoder's
    eng.close()


def test_cli_gray_leaves_a_colour_still_read_through_ffmpeg_alone(pkg, tmp_path):
    """a single frame read through ffmpeg (a still in a format the built-in codecs do not read) is a colour file like any other: under --gray the reader is
    still asked for bgr24 and the bytes are the ones written without the flag - render() of the frame"""
    import json
    W, H = 100, 70
    bgr = smooth_frame(H, W, 95)
    assert (bgr[..., 0] != bgr[..., 2]).any()
    (tmp_path / "cover.jpg").write_bytes(bgr.tobytes())
    bindir = tmp_path / "bin"; bindir.mkdir()
    for name, text in (("ffprobe", FAKE_FFPROBE), ("ffmpeg", FAKE_FFMPEG)):
        (bindir / name).write_text(text); (bindir / name).chmod(0o755)
    log = tmp_path / "argv.jsonl"
    env = dict(os.environ, PATH=f"{bindir}:{os.environ['PATH']}", FAKE_W=str(W), FAKE_H=str(H), FAKE_FRAMES="1", FAKE_LOG=str(log))
    common, eng = w2x_setup(pkg, tmp_path, env)
    want = eng.render(bgr)
    for k, extra in enumerate((("--gray",), ())):
        log.write_text("")
        out = tmp_path / f"s{k}"; out.mkdir()
        r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "cover.jpg"), "-o", str(out), *extra], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr
        raw = np.frombuffer((out / f"cover{TAG}.png").read_bytes(), np.uint8)
        assert raw.size == want.size
        same(f"a colour still through ffmpeg {extra}", raw.reshape(want.shape), want)
        calls = [json.loads(line) for line in log.read_text().splitlines()]
        reader = next(c for c in calls if c[c.index("-i") + 1] != "-")
        writer = next(c for c in calls if c[c.index("-i") + 1] == "-")
        assert reader[reader.index("-pix_fmt") + 1] == "bgr24" and writer[writer.index("-pix_fmt") + 1] == "bgr24"
    eng.close()
