"""RGBA frames on the GPU (Img2Img::renderRgba): alpha_bleed_kernel against tests/rgba_ref.py, and renderRgba against the two render() calls it
replaces - colour == render(bleed(BGR, A, R)), alpha == the green channel of render(gray(A)) - byte for byte, every sample compared.  Engines for
swin_unet x4 and cunet x2 on synthetic graphs, as in the other GPU tests."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import rgba_ref
from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W2X = os.path.join(ROOT, "waifu2x-tensorrt_amd", "w2x")

# name -> (model, scale, batch, tile, small, load options)
CONFIGS = {
    "swin_x4_b2_blend": ("swin_unet/art", 4, 2, 64, True, dict(overlap=(0.0625, 0.0625))),
    "swin_x4_b2_tta": ("swin_unet/art", 4, 2, 64, True, dict(overlap=(0.0625, 0.0625), tta=True)),
    "cunet_x2_b2_noblend_tta": ("cunet/art", 2, 2, 64, False, dict(overlap=(0.0, 0.0), tta=True)),
    "cunet_x2_b2_blend_ttabug": ("cunet/art", 2, 2, 64, False, dict(overlap=(0.0625, 0.0625), tta=True, ttaBugCompat=True)),
    "cunet_x2_b4_blend": ("cunet/art", 2, 4, 64, False, dict(overlap=(0.0625, 0.0625))),
    "cunet_x2_b3_noblend_tta": ("cunet/art", 2, 3, 64, False, dict(overlap=(0.0, 0.0), tta=True)),
}


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


def rgba_frame(rows, cols, seed, kind="cutout"):
    """a BGRA frame: noise colours; alpha a soft-edged shape with fully transparent surroundings and holes, or noise"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
    if kind == "cutout":
        yy, xx = np.mgrid[0:rows, 0:cols]
        d = np.hypot((yy - rows / 2) / max(rows, 1), (xx - cols / 2) / max(cols, 1))
        a = np.clip((0.42 - d) * 1800, 0, 255)
        a[(yy // 7 + xx // 5) % 9 == 0] = 0                       # holes inside the shape
        f[..., 3] = a.astype(np.uint8)
    elif kind == "noise":
        f[..., 3] = f[..., 3] * (rng.random((rows, cols)) < 0.6)
    return f


def tile_count(pkg, eng, rows, cols, scale, tile, kw):
    n, _, _ = pkg.calculate_tiles(cols, rows, cols * scale, rows * scale, tile, eng.output_tile_size, scale, kw.get("overlap", (0.0625, 0.0625)))
    return n


def expected(eng, bgra, bleed):
    """the two render() calls renderRgba replaces"""
    bgr = rgba_ref.bleed(np.ascontiguousarray(bgra[..., :3]), np.ascontiguousarray(bgra[..., 3]), bleed)
    colour = eng.render(bgr)
    alpha = eng.render(np.ascontiguousarray(np.repeat(bgra[..., 3:4], 3, axis=2)))[..., 1]
    return colour, alpha


def assert_rgba(tag, out, colour, alpha):
    assert out.dtype == np.uint8 and out.shape == colour.shape[:2] + (4,), (tag, out.shape)
    dc = int((out[..., :3] != colour).sum()); da = int((out[..., 3] != alpha).sum())
    print(f"{tag}: {dc} colour bytes and {da} alpha bytes differ of {colour.size} / {alpha.size}")
    assert dc == 0 and da == 0, f"{tag}: {dc} colour bytes, {da} alpha bytes differ"


# ---- 1. the bleed kernel alone
def test_device_bleed_matches_the_reference(engines):
    eng = engines("cunet_x2_b2_noblend_tta")[0]
    cases = list(rgba_ref.cases())
    # several workgroup tiles (64 x 32 pixels) wide and high; holes that cross tile borders and touch every frame edge
    rng = np.random.default_rng(77)
    rows, cols = 150, 200
    bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    a = np.full((rows, cols), 255, np.uint8)
    a[20:75, 40:150] = 0            # crosses x = 64, 128 and y = 32, 64; wider than 2 * 16
    a[0:12, 90:140] = 0             # top edge, across x = 128
    a[120:150, 0:30] = 0            # bottom-left corner
    a[60:100, 185:200] = 0          # right edge, across y = 64, 96
    a[100:140, 60:70] = 0           # narrow, across y = 128 and x = 64
    cases.append(("tiled 150x200", bgr, a, (0, 1, 2, 5, 16)))
    sp = (rng.random((rows, cols)) < 0.01).astype(np.uint8) * 255
    cases.append(("tiled sparse 150x200", bgr, sp, (1, 5, 16)))
    for name, bgr, alpha, radii in cases:
        bgra = np.ascontiguousarray(np.dstack([bgr, alpha]))
        for r in radii:
            got = eng.alpha_bleed_device(bgra, r)
            ref = rgba_ref.bleed(bgr, alpha, r)
            assert got.shape == ref.shape and np.array_equal(got, ref), f"{name} at radius {r}: {int((got != ref).sum())} bytes differ"


def test_device_bleed_takes_padded_rows(engines):
    eng = engines("cunet_x2_b2_noblend_tta")[0]
    big = rgba_frame(70, 120, 5, "noise")
    view = big[:, :97]
    ref = rgba_ref.bleed(np.ascontiguousarray(view[..., :3]), np.ascontiguousarray(view[..., 3]), 6)
    assert np.array_equal(eng.alpha_bleed_device(view, 6), ref)


# ---- 2. / 3. renderRgba against the two render() calls
@pytest.mark.parametrize("name", ["swin_x4_b2_blend", "cunet_x2_b2_noblend_tta", "cunet_x2_b2_blend_ttabug", "cunet_x2_b4_blend"])
def test_bleed_zero_is_two_renders(engines, pkg, name):
    eng, scale, batch, tile, kw = engines(name)
    one = next(n for n in range(tile, 0, -1) if tile_count(pkg, eng, n, n, scale, tile, kw) == 1)      # the largest square frame of one tile
    assert tile_count(pkg, eng, 71, 103, scale, tile, kw) > 1 and tile_count(pkg, eng, max(one // 2, 1), max(one // 3, 1), scale, tile, kw) == 1
    for rows, cols, seed in ((71, 103, 1), (45, 67, 2), (one, one, 3), (max(one // 2, 1), max(one // 3, 1), 4)):      # odd sizes; the last two: one tile
        bgra = rgba_frame(rows, cols, seed, "cutout" if seed % 2 else "noise")
        colour, alpha = expected(eng, bgra, 0)
        assert np.array_equal(colour, eng.render(np.ascontiguousarray(bgra[..., :3])))       # (bleed 0 leaves the colours as stored)
        assert_rgba(f"{name} {rows}x{cols}", eng.render_rgba(bgra), colour, alpha)
    # padded row steps on both sides
    bgra = rgba_frame(50, 90, 9)
    src = np.zeros((50, 101, 4), np.uint8); src[:, :90] = bgra
    dst = np.zeros((50 * scale, 90 * scale + 13, 4), np.uint8)
    assert eng.render_rgba(src[:, :90], dst=dst[:, :90 * scale]) is True
    colour, alpha = expected(eng, bgra, 0)
    assert_rgba(f"{name} padded", dst[:, :90 * scale], colour, alpha)
    assert not dst[:, 90 * scale:].any()                                                        # nothing written past the rows


def test_a_pass_holds_tiles_of_both_kinds(engines, pkg):
    """3 tiles at batch 4: the first pass is 3 colour tiles and 1 alpha tile; 6 tiles in 2 batches where two calls take 2"""
    eng, scale, batch, tile, kw = engines("cunet_x2_b4_blend")
    cols = next(c for c in range(1, 400) if tile_count(pkg, eng, 20, c, scale, tile, kw) == 3)          # one row of three tiles
    bgra = rgba_frame(20, cols, 12)
    seen = []
    eng.setProgressCallback(lambda cur, total, speed: seen.append((cur, total)))
    out = eng.render_rgba(bgra)
    eng.setProgressCallback(None)
    assert seen == [(1, 2), (2, 2)], seen
    colour, alpha = expected(eng, bgra, 0)
    assert_rgba("3 tiles at batch 4", out, colour, alpha)


@pytest.mark.parametrize("name", ["swin_x4_b2_blend", "cunet_x2_b2_noblend_tta", "cunet_x2_b4_blend"])
@pytest.mark.parametrize("bleed", [1, 4, 16])
def test_bleed_radii(engines, name, bleed):
    eng = engines(name)[0]
    for rows, cols, seed, kind in ((71, 103, 21, "cutout"), (45, 67, 22, "noise")):
        bgra = rgba_frame(rows, cols, seed, kind)
        colour, alpha = expected(eng, bgra, bleed)
        assert_rgba(f"{name} {rows}x{cols} bleed {bleed}", eng.render_rgba(bgra, bleed=bleed), colour, alpha)
    # the bleed changed what the network saw
    bgra = rgba_frame(71, 103, 21)
    assert not np.array_equal(eng.render_rgba(bgra, bleed=bleed)[..., :3], eng.render_rgba(bgra)[..., :3])


def test_swin_tta(engines):
    eng = engines("swin_x4_b2_tta")[0]
    bgra = rgba_frame(45, 67, 31)
    colour, alpha = expected(eng, bgra, 4)
    assert_rgba("swin tta bleed 4", eng.render_rgba(bgra, bleed=4), colour, alpha)


# ---- 4. the schedule, as the progress callback shows it; the uniform shortcut
@pytest.mark.parametrize("name", ["swin_x4_b2_blend", "cunet_x2_b2_noblend_tta", "cunet_x2_b4_blend", "cunet_x2_b3_noblend_tta"])
def test_progress_totals_and_the_uniform_shortcut(engines, pkg, name):
    eng, scale, batch, tile, kw = engines(name)
    steps = 8 if kw.get("tta") else 1
    seen = []
    eng.setProgressCallback(lambda cur, total, speed: seen.append((cur, total)))
    try:
        for rows, cols in ((71, 103), (40, 150), (30, 30)):
            n = tile_count(pkg, eng, rows, cols, scale, tile, kw)
            both, colour_only = math.ceil(2 * n * steps / batch), math.ceil(n * steps / batch)
            bgra = rgba_frame(rows, cols, rows + cols)
            for skip in (False, True):                      # a plane that is not uniform: the whole schedule either way
                seen.clear()
                out = eng.render_rgba(bgra, skip_uniform_alpha=skip)
                assert seen == [(k + 1, both) for k in range(both)], (name, rows, cols, skip, seen)
                if skip:
                    assert np.array_equal(out, eng.render_rgba(bgra))
            for v in (0, 37, 255):
                flat = bgra.copy(); flat[..., 3] = v
                seen.clear()
                out = eng.render_rgba(flat, skip_uniform_alpha=True)
                assert seen == [(k + 1, colour_only) for k in range(colour_only)], (name, rows, cols, v, seen)
                assert (out[..., 3] == v).all()
                assert np.array_equal(out[..., :3], eng.render(np.ascontiguousarray(flat[..., :3])))
                # with the shortcut off the same frame gives the network's alpha
                seen.clear()
                out = eng.render_rgba(flat)
                assert seen == [(k + 1, both) for k in range(both)], (name, rows, cols, v, seen)
                colour, alpha = expected(eng, flat, 0)
                assert_rgba(f"{name} uniform {v} without the shortcut", out, colour, alpha)
            # the shortcut with a bleed: a uniform plane has nothing to spread
            flat = bgra.copy(); flat[..., 3] = 0
            assert np.array_equal(eng.render_rgba(flat, bleed=16, skip_uniform_alpha=True)[..., :3], eng.render(np.ascontiguousarray(flat[..., :3])))
            # one pixel off: not uniform
            flat[rows - 1, cols - 1, 3] = 1
            seen.clear()
            eng.render_rgba(flat, skip_uniform_alpha=True)
            assert seen and seen[-1] == (both, both)
    finally:
        eng.setProgressCallback(None)


# ---- 5. robustness
def test_refusals_leave_the_engine_usable(engines, pkg):
    eng, scale, batch, tile, kw = engines("cunet_x2_b2_noblend_tta")
    err = int(pkg.Severity.error)
    bgra = rgba_frame(40, 60, 41)
    good = np.empty((80, 120, 4), np.uint8)

    def refused(call, text):
        n = len(eng.messages)
        assert call() is False
        new = [m for s, m in eng.messages[n:] if s == err]
        assert new and text in new[-1], (text, new)

    L, h = eng._L, eng._h
    refused(lambda: eng.render_rgba(bgra, bleed=17, dst=good), "not in [0, 16]")
    refused(lambda: eng.render_rgba(bgra, bleed=-1, dst=good), "not in [0, 16]")
    refused(lambda: eng.render_rgba(bgra, dst=np.empty((80, 121, 4), np.uint8)), "invalid size")
    refused(lambda: eng.render_rgba(bgra, dst=np.empty((79, 120, 4), np.uint8)), "invalid size")
    refused(lambda: eng.render_rgba(bgra.astype(np.uint16), dst=good), "8-bit")
    refused(lambda: bool(L.w2x_render_rgba(h, None, 40, 60, 240, good.ctypes.data, 480, 0, 0)), "empty or has an invalid step")
    refused(lambda: bool(L.w2x_render_rgba(h, bgra.ctypes.data, 40, 60, 239, good.ctypes.data, 480, 0, 0)), "invalid step")
    refused(lambda: bool(L.w2x_render_rgba(h, bgra.ctypes.data, 40, 60, 240, None, 480, 0, 0)), "invalid size")
    refused(lambda: bool(L.w2x_render_rgba(h, bgra.ctypes.data, 40, 60, 240, good.ctypes.data, 479, 0, 0)), "invalid size")
    refused(lambda: bool(L.w2x_render_rgba(h, bgra.ctypes.data, 0, 60, 240, good.ctypes.data, 480, 0, 0)), "empty")
    out3 = np.empty((40, 60, 3), np.uint8)
    refused(lambda: bool(L.w2x_alpha_bleed_device(h, bgra.ctypes.data, 40, 60, 240, out3.ctypes.data, 180, 17)), "not in [0, 16]")
    refused(lambda: bool(L.w2x_alpha_bleed_device(h, bgra.ctypes.data, 40, 60, 100, out3.ctypes.data, 180, 2)), "invalid step")
    refused(lambda: bool(L.w2x_alpha_bleed_device(h, bgra.ctypes.data, 40, 60, 240, out3.ctypes.data, 179, 2)), "invalid size")
    fresh = pkg.Img2Img()
    n = len(fresh.messages)
    assert fresh.render_rgba(bgra, dst=good) is False and "before a successful load" in fresh.last_error() and len(fresh.messages) > n
    fresh.close()
    # the engine renders normally after the refusals
    colour, alpha = expected(eng, bgra, 3)
    assert_rgba("after refusals", eng.render_rgba(bgra, bleed=3), colour, alpha)
    assert np.array_equal(eng.render(np.ascontiguousarray(bgra[..., :3])), expected(eng, bgra, 0)[0])


def test_render_and_bench_resident_around_render_rgba(engines):
    eng = engines("cunet_x2_b4_blend")[0]
    bgra = rgba_frame(71, 103, 51)
    bgr = np.ascontiguousarray(bgra[..., :3])
    first = eng.render(bgr)
    out = eng.render_rgba(bgra, bleed=2)
    assert eng.bench_resident(2) < 0            # an RGBA frame is not replayed
    again = eng.render(bgr)
    assert np.array_equal(first, again)
    ms = eng.bench_resident(3)
    assert ms > 0
    res = np.empty_like(first)
    assert eng.resident_output(res) and np.array_equal(res, first)
    colour, alpha = expected(eng, bgra, 2)
    assert_rgba("before bench_resident", out, colour, alpha)
    assert_rgba("after bench_resident", eng.render_rgba(bgra, bleed=2), colour, alpha)
    # a 16-bit render() between RGBA frames
    deep = (bgr.astype(np.uint16) << 8) | bgr
    d1 = eng.render(deep)
    assert_rgba("after a 16-bit frame", eng.render_rgba(bgra, bleed=2), colour, alpha)
    assert np.array_equal(eng.render(deep), d1)


# ---- 7. determinism
def test_two_calls_give_equal_bytes(engines):
    for name in ("swin_x4_b2_blend", "cunet_x2_b2_noblend_tta"):
        eng = engines(name)[0]
        bgra = rgba_frame(71, 103, 61)
        a = eng.render_rgba(bgra, bleed=8)
        b = eng.render_rgba(bgra, bleed=8)
        c = eng.render_rgba(bgra, bleed=8, skip_uniform_alpha=True)
        assert np.array_equal(a, b) and np.array_equal(a, c)
        assert np.array_equal(eng.alpha_bleed_device(bgra, 8), eng.alpha_bleed_device(bgra, 8))


# ---- 6. the command line
def write_bmp32(path, bgra):
    rows, cols = bgra.shape[:2]
    img = bgra[::-1].tobytes()
    with open(path, "wb") as f:
        f.write(b"BM" + struct.pack("<IHHI", 54 + len(img), 0, 0, 54) + struct.pack("<IiiHHIIiiII", 40, cols, rows, 1, 32, 0, len(img), 2835, 2835, 0, 0) + img)


def read_bmp32(path):
    d = open(path, "rb").read()
    off, = struct.unpack_from("<I", d, 10)
    cols, rows, _, bits = struct.unpack_from("<iiHH", d, 18)
    assert bits == 32 and rows > 0
    return np.frombuffer(d, np.uint8, rows * cols * 4, off).reshape(rows, cols, 4)[::-1]


def test_cli_alpha_bleed_and_skip_uniform(pkg, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import synth_models as sm
    models = tmp_path / "models"
    path = sm.model_path(str(tmp_path), "cunet/art", 2, 1)
    sm.export_onnx(sm.make_model("cunet/art", 2, seed=6), path, 2, 64, dynamic=True)
    bgra = rgba_frame(80, 100, 71)
    Image.fromarray(np.ascontiguousarray(bgra[..., [2, 1, 0, 3]])).save(tmp_path / "in.png")
    write_bmp32(tmp_path / "sprite.bmp", bgra)
    opaque = bgra.copy(); opaque[..., 3] = 255
    Image.fromarray(np.ascontiguousarray(opaque[..., [2, 1, 0, 3]])).save(tmp_path / "opaque.png")
    common = ["--models", str(models), "--model", "cunet/art", "--scale", "2", "--noise", "1", "--batchSize", "2", "--tileSize", "64"]
    assert subprocess.run([W2X, *common, "build"], capture_output=True, text=True, timeout=300).returncode == 0
    out = tmp_path / "o"; out.mkdir()
    r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "in.png"), str(tmp_path / "sprite.bmp"), "-o", str(out), "--alpha-bleed", "4"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    eng = pkg.Img2Img()
    assert eng.load(path, pkg.RenderConfig(batchSize=2, height=64, width=64, scaling=2)), eng.last_error()
    want = eng.render_rgba(bgra, bleed=4)
    got = np.array(Image.open(out / "in(cunet_art)(noise1)(scale2).png"))
    assert got.shape == (160, 200, 4) and np.array_equal(got[..., [2, 1, 0, 3]], want)
    assert np.array_equal(read_bmp32(out / "sprite(cunet_art)(noise1)(scale2).bmp"), want)
    assert not np.array_equal(want[..., :3], eng.render_rgba(bgra)[..., :3])
    # an opaque export: alpha 255 throughout with --alpha-skip-uniform, and half the batches in the log
    r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "opaque.png"), "-o", str(out), "--alpha-skip-uniform"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.array(Image.open(out / "opaque(cunet_art)(noise1)(scale2).png"))
    assert got.shape == (160, 200, 4) and (got[..., 3] == 255).all()
    assert np.array_equal(got[..., 2::-1], eng.render(np.ascontiguousarray(opaque[..., :3])))
    n, _, _ = pkg.calculate_tiles(100, 80, 200, 160, 64, eng.output_tile_size, 2, (0.0625, 0.0625))
    assert n > 1 and f"batch {math.ceil(n / 2)}/{math.ceil(n / 2)} " in r.stderr and f"batch {n}/{n} " not in r.stderr
    eng.close()
