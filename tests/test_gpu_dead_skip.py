"""Dead-skip: the windows and row tiles of edge tiles that no kept output pixel depends on are not computed.  Every render with the skip
on must be the bytes of the same render with the debug switch no_dead_skip (every slot "all"; read where a frame's slot table is set up) - also with
W2X_POISON, which turns every stale activation into an fp16 NaN before each frame, so that a live window reading a dead row shows up as a difference
and not as luck.  swin_unet/art scale 4, tile 64 (token maps 48 / 24 / 12), batch 2.  No tolerance anywhere: equality."""
import numpy as np
import pytest

from parity_util import smooth_frame

pytestmark = pytest.mark.gpu

FRAMES = [(70, 100), (65, 65), (290, 380)]      # rows, cols (100 x 70, 65 x 65, 380 x 290)


def make_engine(pkg, path, **kw):
    eng = pkg.Img2Img()
    assert eng.build(path, pkg.BuildConfig.fixed(2, 64)), eng.last_error()
    assert eng.load(path, pkg.RenderConfig(batchSize=2, height=64, width=64, scaling=4, overlap=(0.0625, 0.0625), **kw)), eng.last_error()
    return eng


@pytest.fixture(scope="module")
def model(onnx_model):
    return onnx_model("swin_unet/art", 4, 2, 64, small=False)


def strips(eng, frame, like):
    out = np.full_like(like, 77)
    for part in range(2):
        assert eng.render_strip(frame, out, part, 2), eng.last_error()
    return out


@pytest.fixture(scope="module")
def reference(pkg, model):
    """frame -> the render with every slot "all" (no_dead_skip), computed once on an un-poisoned engine"""
    eng = make_engine(pkg, model)
    ref = {}
    with pkg.debug_switches(no_dead_skip=1):
        for shape in FRAMES:
            frame = smooth_frame(*shape, 7)
            ref[shape] = (frame, eng.render(frame))
            assert np.array_equal(strips(eng, frame, ref[shape][1]), ref[shape][1])
    yield eng, ref
    eng.close()


def test_the_tables_say_something_is_skipped(pkg, model):
    """(the comparison below would pass trivially if nothing were dead at these sizes)"""
    for rows, cols in FRAMES:
        n, _, rout = pkg.calculate_tiles(cols, rows, cols * 4, rows * 4, 64, 192, 4, (0.0625, 0.0625))
        ops = pkg.dead_skip_extents(model, 2, 64, cols, rows, 4, (0.0625, 0.0625), n - 1)
        assert any(e["live_units"] < e["total_units"] for e in ops if e["kind"] in (4, 5)), (rows, cols)


@pytest.mark.parametrize("shape", FRAMES)
def test_render_and_strips_equal_no_dead_skip(reference, shape):
    eng, ref = reference
    frame, want = ref[shape]
    assert np.array_equal(eng.render(frame), want)
    assert np.array_equal(strips(eng, frame, want), want)
    assert np.array_equal(eng.render(frame), want)          # (the replayed graphs)


@pytest.mark.parametrize("shape", FRAMES)
def test_poisoned_render_and_strips_equal_no_dead_skip(pkg, model, reference, monkeypatch, shape):
    _, ref = reference
    frame, want = ref[shape]
    monkeypatch.setenv("W2X_POISON", "1")
    eng = make_engine(pkg, model)
    try:
        assert np.array_equal(eng.render(frame), want)
        assert np.array_equal(strips(eng, frame, want), want)
        with pkg.debug_switches(no_dead_skip=1):
            assert np.array_equal(eng.render(frame), want)
        assert np.array_equal(eng.render(frame), want)
    finally:
        eng.close()


def test_tta(pkg, model, monkeypatch):
    """TTA slots are "all" (the kept rect would have to go through each slot's dihedral map): the switch changes nothing, poisoned or not"""
    frame = smooth_frame(70, 100, 9)
    monkeypatch.setenv("W2X_POISON", "1")
    eng = make_engine(pkg, model, tta=True)
    try:
        got = eng.render(frame)
        with pkg.debug_switches(no_dead_skip=1):
            want = eng.render(frame)
        assert np.array_equal(got, want)
    finally:
        eng.close()


def test_render16(pkg, model, reference, monkeypatch):
    frame = (smooth_frame(70, 100, 11).astype(np.uint16) * 257)
    eng, _ = reference
    with pkg.debug_switches(no_dead_skip=1):
        want = eng.render(frame)
    assert np.array_equal(eng.render(frame), want)
    monkeypatch.setenv("W2X_POISON", "1")
    eng2 = make_engine(pkg, model)
    try:
        assert np.array_equal(eng2.render(frame), want)
    finally:
        eng2.close()


def test_render_sequence_rolling(pkg, model):
    """three frames of 380 x 290 through the rolling path (both tile slabs)"""
    frames = [smooth_frame(290, 380, 20 + k) for k in range(3)]
    eng = make_engine(pkg, model)
    try:
        with pkg.debug_switches(no_dead_skip=1):
            want = [eng.render(f) for f in frames]
        got = eng.render_sequence(frames)
        assert len(got) == 3
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        got = eng.render_sequence(frames)                   # (captured passes of both slabs replayed)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    finally:
        eng.close()
