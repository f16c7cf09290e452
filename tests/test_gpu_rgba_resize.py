"""Resized RGBA frames and RGBA sequences on the GPU (Img2Img::renderRgbaResized / renderSequenceRgba*).  Every comparison is equality on every
byte, and the expected values come from calls the project already had: colour == render_resized(bleed(BGR, A, R), size, filter), alpha == the green channel
of render_resized(gray(A), size, filter).  Engines: the 64-pixel-tile synthetic ones of tests/test_gpu_rgba.py."""
import subprocess

import numpy as np
import pytest

import rgba_ref
from test_gpu_rgba import CONFIGS, W2X, assert_rgba, rgba_frame, tile_count
from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu

NAMES = ["swin_x4_b2_blend", "cunet_x2_b2_noblend_tta"]
# targets for the 71 x 103 frame (rows, cols), per scale.  Widths cover outW % 4 = 3, 0, 1, 2 (the 16-byte store is decided per row from the address); heights
# that are no multiple of the 16-row tile; the first is the INPUT size (factor = scaling: the most taps, the largest rows_max, the whole four-plane LDS), the
# third stretches the two axes differently, the last keeps the scaled height.
TARGETS = {4: [(71, 103), (150, 200), (100, 301), (284, 410)], 2: [(71, 103), (100, 152), (75, 205), (142, 198)]}


@pytest.fixture(scope="module")
def engines(pkg, onnx_model):
    made = {}

    def get(name):
        if name not in made:
            model, scale, batch, tile, small, kw = CONFIGS[name]
            made[name] = (make_engine(pkg, onnx_model(model, scale, batch, tile, small=small), batch, tile, scale, **kw), scale, batch, tile, kw)
        return made[name]
    yield get
    for eng, *_ in made.values():
        eng.close()


def gray(bgra):
    return np.ascontiguousarray(np.repeat(bgra[..., 3:4], 3, axis=2))


def expected(eng, bgra, bleed, size, filt):
    """the two render_resized() calls renderRgbaResized replaces"""
    bgr = rgba_ref.bleed(np.ascontiguousarray(bgra[..., :3]), np.ascontiguousarray(bgra[..., 3]), bleed)
    return eng.render_resized(bgr, size, filt), eng.render_resized(gray(bgra), size, filt)[..., 1]


# ---- 1. the resized call against the two render_resized() calls
@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
@pytest.mark.parametrize("name", NAMES)
def test_resized_is_two_render_resized_calls(engines, pkg, name, filt):
    eng, scale, batch, tile, kw = engines(name)
    assert {c % 4 for _, c in TARGETS[scale]} == {0, 1, 2, 3} and any(r % 16 for r, _ in TARGETS[scale])
    assert tile_count(pkg, eng, 71, 103, scale, tile, kw) > 1
    bgra = rgba_frame(71, 103, 1)
    for bleed in (0, 5):
        for size in TARGETS[scale] if bleed == 0 else TARGETS[scale][:2]:
            colour, alpha = expected(eng, bgra, bleed, size, filt)
            assert_rgba(f"{name} 71x103 -> {size} {filt} bleed {bleed}", eng.render_rgba_resized(bgra, size, bleed=bleed, filter=filt), colour, alpha)
    # one tile: the largest square frame of one tile, and a frame whose targets are lower than one 16-row output tile
    one = next(n for n in range(tile, 0, -1) if tile_count(pkg, eng, n, n, scale, tile, kw) == 1)
    for (rows, cols), sizes in (((one, one), [(one, one), (one + 7, one * scale - 2)]), ((9, 13), [(9, 13), (11, 13 * scale - 1), (15, 21)])):
        assert tile_count(pkg, eng, rows, cols, scale, tile, kw) == 1
        bgra1 = rgba_frame(rows, cols, rows + cols, "noise")
        for size in sizes:
            for bleed in (0, 5):
                colour, alpha = expected(eng, bgra1, bleed, size, filt)
                assert_rgba(f"{name} {rows}x{cols} -> {size} {filt} bleed {bleed}", eng.render_rgba_resized(bgra1, size, bleed=bleed, filter=filt), colour, alpha)


# ---- 2. at the scaled size: renderRgba
@pytest.mark.parametrize("name", NAMES)
def test_the_scaled_size_is_render_rgba(engines, name):
    eng, scale, *_ = engines(name)
    bgra = rgba_frame(71, 103, 2)
    for filt in ("bicubic", "bilinear"):
        assert np.array_equal(eng.render_rgba_resized(bgra, (71 * scale, 103 * scale), bleed=3, filter=filt), eng.render_rgba(bgra, bleed=3))


# ---- 3. an fp32-storage engine
def test_fp32_storage_engine(pkg, onnx_model):
    path = onnx_model("cunet/art", 2, 1, 64, noise=1)
    eng = pkg.Img2Img()
    assert eng.build(path, pkg.BuildConfig.fixed(1, 64, precision=pkg.Precision.TF32)), eng.last_error()
    assert eng.load(path, pkg.RenderConfig(precision=pkg.Precision.TF32, batchSize=1, height=64, width=64, scaling=2, overlap=(0.0625, 0.0625))), eng.last_error()
    bgra = rgba_frame(57, 70, 3)
    for size, filt in (((57, 70), "bicubic"), ((90, 113), "bilinear")):
        colour, alpha = expected(eng, bgra, 4, size, filt)
        assert_rgba(f"tf32 57x70 -> {size} {filt}", eng.render_rgba_resized(bgra, size, bleed=4, filter=filt), colour, alpha)
    eng.close()


# ---- 4. skip_uniform_alpha
@pytest.mark.parametrize("name", NAMES)
def test_skip_uniform_alpha(engines, name):
    eng, scale, *_ = engines(name)
    bgra = rgba_frame(71, 103, 4)
    for size in TARGETS[scale][:3]:
        for v in (255, 37):
            flat = bgra.copy(); flat[..., 3] = v
            out = eng.render_rgba_resized(flat, size, skip_uniform_alpha=True)
            assert out.shape == size + (4,) and (out[..., 3] == v).all()
            assert np.array_equal(out[..., :3], eng.render_resized(np.ascontiguousarray(flat[..., :3]), size))
        assert np.array_equal(eng.render_rgba_resized(bgra, size, bleed=2, skip_uniform_alpha=True), eng.render_rgba_resized(bgra, size, bleed=2))


# ---- 5. padded steps on both sides
def test_padded_steps(engines):
    eng, scale, *_ = engines("swin_x4_b2_blend")
    bgra = rgba_frame(50, 90, 5)
    src = np.zeros((50, 101, 4), np.uint8); src[:, :90] = bgra
    for size in ((77, 123), (120, 200)):
        dst = np.zeros((size[0], size[1] + 13, 4), np.uint8)
        assert eng.render_rgba_resized(src[:, :90], size, dst=dst[:, :size[1]]) is True
        colour, alpha = expected(eng, bgra, 0, size, "bicubic")
        assert_rgba(f"padded -> {size}", dst[:, :size[1]], colour, alpha)
        assert not dst[:, size[1]:].any()                                                       # nothing written past cols' * 4 in a row


# ---- 6. sequences
@pytest.mark.parametrize("name", NAMES)
def test_sequences_are_the_single_frame_calls(engines, name):
    eng, scale, *_ = engines(name)
    frames = [rgba_frame(45, 67, 60 + k, "cutout" if k % 2 else "noise") for k in range(5)]
    bgr = np.ascontiguousarray(frames[0][..., :3])
    first = eng.render(bgr)
    first_seq = eng.render_sequence([np.ascontiguousarray(f[..., :3]) for f in frames])
    size = (45 * scale - 40, 67 * scale - 61)
    for pinned in (False, True):
        outs = eng.render_sequence_rgba(frames, bleed=3, pinned=pinned)
        assert len(outs) == 5
        for k, o in enumerate(outs):
            assert np.array_equal(o, eng.render_rgba(frames[k], bleed=3)), (name, "plain", pinned, k)
        outs = eng.render_sequence_rgba(frames, size=size, bleed=3, filter="bilinear", pinned=pinned)
        for k, o in enumerate(outs):
            assert o.shape == size + (4,) and np.array_equal(o, eng.render_rgba_resized(frames[k], size, bleed=3, filter="bilinear")), (name, "resized", pinned, k)
    # the first call matches the two-call statement too (not only the single-frame call)
    colour, alpha = expected(eng, frames[1], 3, size, "bilinear")
    assert_rgba(f"{name} sequence frame 1", outs[1], colour, alpha)
    # an opaque frame in the middle of a skip_uniform_alpha sequence: the 2N schedule, the N schedule, the 2N schedule again
    mixed = [f.copy() for f in frames]
    mixed[2][..., 3] = 255
    for sz in (None, size):
        outs = eng.render_sequence_rgba(mixed, size=sz, skip_uniform_alpha=True)
        for k, o in enumerate(outs):
            single = eng.render_rgba(mixed[k], skip_uniform_alpha=True) if sz is None else eng.render_rgba_resized(mixed[k], sz, skip_uniform_alpha=True)
            assert np.array_equal(o, single), (name, sz, k)
        assert (outs[2][..., 3] == 255).all()
        want = eng.render(np.ascontiguousarray(mixed[2][..., :3])) if sz is None else eng.render_resized(np.ascontiguousarray(mixed[2][..., :3]), sz)
        assert np.array_equal(outs[2][..., :3], want)
    # caller's output buffers
    mine = [np.zeros(size + (4,), np.uint8) for _ in range(5)]
    assert eng.render_sequence_rgba(frames, size=size, outs=mine) is mine
    assert np.array_equal(mine[4], eng.render_rgba_resized(frames[4], size))
    # the rgba / resize state is reset: render() and render_sequence() give their own bytes
    assert np.array_equal(eng.render(bgr), first)
    again = eng.render_sequence([np.ascontiguousarray(f[..., :3]) for f in frames])
    assert all(np.array_equal(a, b) for a, b in zip(again, first_seq))
    assert np.array_equal(eng.render_resized(bgr, size), expected(eng, frames[0], 0, size, "bicubic")[0])


# ---- 7. refusals
def test_refusals_leave_the_engine_usable(engines, pkg):
    eng, scale, batch, tile, kw = engines("cunet_x2_b2_noblend_tta")
    err = int(pkg.Severity.error)
    bgra = rgba_frame(40, 60, 41)
    L, h = eng._L, eng._h

    def refused(call, text):
        n = len(eng.messages)
        assert call() is False
        new = [m for s, m in eng.messages[n:] if s == err]
        assert new and text in new[-1], (text, new)

    def raises(call, text):
        n = len(eng.messages)
        with pytest.raises(pkg.W2xError):
            call()
        new = [m for s, m in eng.messages[n:] if s == err]
        assert new and text in new[-1], (text, new)

    def dst(rows, cols):
        return np.empty((rows, cols, 4), np.uint8)

    # one step beyond the allowed range in each direction
    for size in ((39, 60), (40, 59), (81, 120), (80, 121)):
        refused(lambda: eng.render_rgba_resized(bgra, size, dst=dst(*size)), "invalid size for a resize")
        raises(lambda: eng.render_sequence_rgba([bgra, bgra], size=size), "invalid size for a resize")
    good = dst(50, 70)
    refused(lambda: eng.render_rgba_resized(bgra.astype(np.uint16), (50, 70), dst=good), "8-bit")                  # depth 16
    refused(lambda: eng.render_rgba_resized(bgra, (50, 70), bleed=17, dst=good), "not in [0, 16]")
    raises(lambda: eng.render_sequence_rgba([bgra, bgra], bleed=17), "not in [0, 16]")
    raises(lambda: eng.render_sequence_rgba([bgra, bgra], size=(50, 70), bleed=17), "not in [0, 16]")
    # short steps, through the C functions
    refused(lambda: bool(L.w2x_render_rgba_resized(h, bgra.ctypes.data, 40, 60, 239, good.ctypes.data, 50, 70, 280, 0, 0, 0)), "invalid step")
    refused(lambda: bool(L.w2x_render_rgba_resized(h, bgra.ctypes.data, 40, 60, 240, good.ctypes.data, 50, 70, 279, 0, 0, 0)), "invalid size")
    refused(lambda: bool(L.w2x_render_rgba_resized(h, None, 40, 60, 240, good.ctypes.data, 50, 70, 280, 0, 0, 0)), "empty")
    refused(lambda: bool(L.w2x_render_rgba_resized(h, bgra.ctypes.data, 40, 60, 240, good.ctypes.data, 50, 70, 280, 0, 0, 7)), "filter")
    import ctypes as C
    two = (C.c_void_p * 2)(bgra.ctypes.data, bgra.ctypes.data)
    big = dst(80, 120)
    outs2 = (C.c_void_p * 2)(big.ctypes.data, big.ctypes.data)
    refused(lambda: bool(L.w2x_render_sequence_rgba(h, two, 40, 60, 239, outs2, 480, 2, 0, 0)), "invalid step")
    refused(lambda: bool(L.w2x_render_sequence_rgba(h, two, 40, 60, 240, outs2, 479, 2, 0, 0)), "invalid size")
    refused(lambda: bool(L.w2x_render_sequence_rgba_resized(h, two, 40, 60, 240, outs2, 80, 120, 479, 2, 0, 0, 0)), "invalid size")
    refused(lambda: bool(L.w2x_render_sequence_rgba(h, two, 0, 60, 240, outs2, 480, 2, 0, 0)), "empty")
    # frames of different sizes within a sequence
    raises(lambda: eng.render_sequence_rgba([bgra, rgba_frame(40, 61, 42)]), "one size")
    raises(lambda: eng.render_sequence_rgba([bgra, rgba_frame(41, 60, 42)], size=(50, 70)), "one size")
    with pytest.raises(ValueError):
        eng.render_sequence_rgba([bgra, bgra], size=(50, 70), outs=[good, dst(50, 71)])              # a dst of the wrong size
    with pytest.raises(ValueError):
        eng.render_rgba_resized(bgra, (50, 70), dst=dst(50, 71))
    fresh = pkg.Img2Img()
    assert fresh.render_rgba_resized(bgra, (50, 70), dst=good) is False and "before a successful load" in fresh.last_error()
    fresh.close()
    # correct calls afterwards succeed
    colour, alpha = expected(eng, bgra, 3, (50, 70), "bicubic")
    assert_rgba("after refusals", eng.render_rgba_resized(bgra, (50, 70), bleed=3), colour, alpha)
    outs = eng.render_sequence_rgba([bgra, bgra], size=(50, 70), bleed=3)
    assert_rgba("sequence after refusals", outs[1], colour, alpha)
    assert np.array_equal(eng.render_sequence_rgba([bgra])[0], eng.render_rgba(bgra))


# ---- 8. the command line
def test_cli_resized_stills_with_alpha(pkg, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import synth_models as sm
    path = sm.model_path(str(tmp_path), "swin_unet/art", 4, 3)
    sm.export_onnx(sm.make_model("swin_unet/art", 4, seed=5, small=True), path, 2, 64, dynamic=True)
    common = ["--models", str(tmp_path / "models"), "--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "2", "--tileSize", "64"]
    assert subprocess.run([W2X, *common, "build"], capture_output=True, text=True, timeout=300).returncode == 0
    bgra = rgba_frame(71, 103, 1)
    Image.fromarray(np.ascontiguousarray(bgra[..., [2, 1, 0, 3]])).save(tmp_path / "a.png")
    eng = pkg.Img2Img()
    assert eng.load(path, pkg.RenderConfig(batchSize=2, height=64, width=64, scaling=4)), eng.last_error()
    runs = ((["--outsize", "301x100"], "(301x100)", (100, 301), 0), (["--outscale", "3"], "(outscale3)", (213, 309), 0),
            (["--outsize", "200x150", "--alpha-bleed", "4"], "(200x150)", (150, 200), 4))
    for k, (extra, tag, size, bleed) in enumerate(runs):
        out = tmp_path / f"o{k}"; out.mkdir()
        r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "a.png"), "-o", str(out), *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = np.array(Image.open(out / f"a(swin_unet_art)(noise3)(scale4){tag}.png"))
        assert got.shape == size + (4,)
        colour, alpha = expected(eng, bgra, bleed, size, "bicubic")                                  # (bleed 4: render_resized of the host-bled frame)
        assert_rgba(f"w2x {' '.join(extra)}", np.ascontiguousarray(got[..., [2, 1, 0, 3]]), colour, alpha)
    assert not np.array_equal(expected(eng, bgra, 4, (150, 200), "bicubic")[0], expected(eng, bgra, 0, (150, 200), "bicubic")[0])
    eng.close()
