"""Resize in linear light on the GPU (Img2Img::setResizeLight): the canvas kernels decode, the resize kernels of every frame format encode.

The reference is tests/light_ref.py: clip -> decode -> torch F.interpolate(antialias=True) -> clip -> encode in float64; its float32 twin is the model of an
ideal fp32 implementation.

Bounds.  The device's L carries an fp32 error of about 2^-21, encode's slope is at most 12.92 and the hardware log2 / exp2 pair adds a few 2^-20 relative:
together about 1e-5, orders below half a 12-bit code (1.2e-4).  So up to 12 bits only rounding ties can move: at most 1 code from the float64 reference.  The
share of samples that are not exactly equal and the largest distance at 16 bits are measured per case on the float32 model; the device may mismatch in at most
twice the model's share plus 0.001 and, at 16 bits, be one code further off than the model's maximum (its log2 / exp2 are hardware approximations and its tap
order is not torch's).  Float outputs: the model's largest error plus 1e-5 (12.92 * 2^-21 = 6.2e-6 for the tap order, 4 * 2^-20 = 3.8e-6 for the pair).
Every figure is printed ("LIGHT ..." lines; profiles/resize_light/record.txt keeps them).

The tests can fail: every against-reference case also asserts that the references of the two neighbouring rules - gamma and the other curve - lie outside the
case's tolerance in at least 1 % of its samples (the smooth frame does not qualify and is kept for the accuracy figure alone)."""
import numpy as np
import pytest

import dither_ref
import light_ref as ref
import yuv_siting_ref as ysr
from test_gpu_parity import make_engine, smooth_frame
from test_gpu_resize import noisy_frame, oracle_canvas
from test_gpu_yuv_layouts import oracle_canvas as yuv_oracle_canvas, same

pytestmark = pytest.mark.gpu

CURVES = ("srgb", "bt709")
DTYPES = {8: np.uint8, 10: np.uint16, 12: np.uint16, 16: np.uint16}
FLOAT_EXTRA = 1e-5
FRESH_FRAME, FRESH_SIZE = (60, 44, 71), (150, 101)


def fresh_bytes(eng):
    """rendered before anybody has called set_resize_light on the engine: the bytes of an engine that never heard of the setting"""
    frame = noisy_frame(*FRESH_FRAME)
    return eng.render_resized(frame, FRESH_SIZE), eng.render_resized(frame, FRESH_SIZE, "bilinear")


@pytest.fixture(scope="module")
def swin(pkg, onnx_model):
    path = onnx_model("swin_unet/art", 4, 2, 64, small=True)
    eng = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625))
    eng.fresh = fresh_bytes(eng)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def cunet_tta(pkg, onnx_model):
    path = onnx_model("cunet/art", 2, 2, 64)
    eng = make_engine(pkg, path, 2, 64, 2, overlap=(0.0, 0.0), tta=True)
    yield eng
    eng.close()


@pytest.fixture(autouse=True)
def settings_back(request):
    """every test leaves the module's engines at the defaults"""
    yield
    for name in ("swin", "cunet_tta"):
        if name in request.fixturenames:
            eng = request.getfixturevalue(name)
            eng.set_resize_light("gamma")
            eng.set_dither("none")


def hook(eng, canvas, size, bits, filt, mode):
    """[H, W, 3] float32 canvas -> [h, w, 3] of `bits` through resize_planes under `mode`"""
    assert eng.set_resize_light(mode)
    planes = [np.ascontiguousarray(canvas[..., k], np.float32) for k in range(3)]
    return np.stack(eng.resize_planes(planes, size, bits, filt), -1)


def share_off(a, b, tol):
    return float((np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) > tol).mean())


def check_codes(tag, got, canvas, size, filt, mode, bits, neighbours=True):
    """integer output against the float64 reference under the bounds of the module docstring; returns (share, max) of the device"""
    want = ref.codes(ref.linear_resized(canvas, size, filt, mode), bits).astype(np.int64)
    model = ref.codes(ref.linear_resized(canvas, size, filt, mode, np.float32), bits).astype(np.int64)
    d, dm = np.abs(got.astype(np.int64) - want), np.abs(model - want)
    share, share_m, top, top_m = float((d != 0).mean()), float((dm != 0).mean()), int(d.max()), int(dm.max())
    tol = 1 if bits <= 12 else top_m + 1
    print(f"LIGHT {tag} {mode} {filt} -> {size[0]}x{size[1]} {bits} bits: device off {share:.6f} max {top}; fp32 model off {share_m:.6f} max {top_m}; bound max {tol}")
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert top <= tol, f"{tag}: {top} codes off, bound {tol}"
    assert share <= 2 * share_m + 0.001, f"{tag}: {share:.6f} of the samples differ, the model's {share_m:.6f}"
    if neighbours:
        for other in ref.other_modes(mode):
            far = share_off(ref.codes(ref.linear_resized(canvas, size, filt, other), bits), want, tol)
            print(f"LIGHT {tag} {mode} -> {size[0]}x{size[1]} {bits} bits: the reference of {other} is outside the bound in {far:.4f} of the samples")
            assert far >= 0.01, f"{tag}: the bound does not tell {mode} from {other} ({far:.4f})"
    return share, top


def check_float(tag, got, canvas, size, filt, mode):
    want = ref.linear_resized(canvas, size, filt, mode)
    model = ref.linear_resized(canvas, size, filt, mode, np.float32)
    err, err_m = float(np.abs(got.astype(np.float64) - want).max()), float(np.abs(model.astype(np.float64) - want).max())
    tol = err_m + FLOAT_EXTRA
    print(f"LIGHT {tag} {mode} {filt} -> {size[0]}x{size[1]} float: device max error {err:.3e}; fp32 model {err_m:.3e}; bound {tol:.3e}")
    assert got.dtype == np.float32 and got.min() >= 0.0 and got.max() <= 1.0
    assert err <= tol, f"{tag}: {err:.3e} > {tol:.3e}"
    for other in ref.other_modes(mode):
        far = share_off(ref.linear_resized(canvas, size, filt, other), want, tol)
        assert far >= 0.01, f"{tag}: the bound does not tell {mode} from {other} ({far:.4f})"


# ---- 1. the hook, known answers
def test_checkerboard_keeps_its_light(swin):
    """a one-pixel 0 / 1 checkerboard halved with the triangle filter: every interior sample averages to 0.5 - code 128 of the encoded values, but light 0.5 is
    code 188 in sRGB"""
    y, x = np.mgrid[0:64, 0:96]
    board = np.repeat(((x + y) & 1).astype(np.float32)[..., None], 3, -1)
    size = (32, 48)
    answers = {"gamma": 128, "srgb": 188, "bt709": int(ref.codes(ref.encode(0.5, "bt709"), 8))}
    assert answers["bt709"] not in (128, 188)
    for mode, code in answers.items():
        out = hook(swin, board, size, 8, "bilinear", mode)
        assert (out[1:-1, 1:-1] == code).all(), (mode, code, np.unique(out[1:-1, 1:-1]))
        want = ref.codes(ref.linear_resized(board, size, "bilinear", mode), 8)
        assert np.abs(out.astype(int) - want.astype(int)).max() <= 1, mode
        print(f"LIGHT checkerboard {mode}: interior code {code}")


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("mode", CURVES)
def test_constant_rows_come_back_as_their_code(swin, mode, bits):
    """row c of the canvas is the constant c / q in every plane; the width is halved, the height kept (its taps are the identity): row c comes back as code c"""
    q = (1 << bits) - 1
    canvas = np.repeat(np.repeat((np.arange(q + 1, dtype=np.float32) / np.float32(q))[:, None, None], 8, 1), 3, 2)
    for filt in ("bicubic", "bilinear"):
        assert (ref.codes(ref.linear_resized(canvas, (q + 1, 4), filt, mode), bits) == np.arange(q + 1)[:, None, None]).all()   # (the reference agrees)
        out = hook(swin, canvas, (q + 1, 4), bits, filt, mode)
        assert out.dtype == DTYPES[bits] and (out == np.arange(q + 1)[:, None, None]).all(), (mode, bits, filt)


def test_black_and_white_stay_exact(swin):
    for mode in CURVES:
        for bits in (8, 10, 12, 16):
            for value in (0.0, 1.0):
                out = hook(swin, np.full((40, 56, 3), value, np.float32), (17, 31), bits, "bicubic", mode)
                assert (out == (0 if value == 0.0 else (1 << bits) - 1)).all(), (mode, bits, value)
        # overshoot is clamped before the decode: still black and white
        out = hook(swin, np.stack([np.full((40, 56), -0.2, np.float32), np.full((40, 56), 1.3, np.float32), np.full((40, 56), 1.0, np.float32)], -1), (20, 28), 8, "bilinear", mode)
        assert (out[..., 0] == 0).all() and (out[..., 1] == 255).all() and (out[..., 2] == 255).all()


# ---- 2. the hook against float64
def overshoot_canvas(rows, cols, seed):
    return np.random.default_rng(seed).uniform(-0.05, 1.05, (rows, cols, 3)).astype(np.float32)


# Every target has at least 10 000 samples: the share bound grants 0.001 beyond the model's share, which a target of a few hundred samples cannot resolve (one
# sample of 741 is 0.00135).  Canvas 105 x 151 (odd both ways): x 3/4, x 1/2 and a mixed target that keeps the width; canvas 209 x 301: x 1/4 (the largest factor,
# rows_max at its top); canvas 70 x 300 -> 35 x 150.  Every target is wider than one 64-column tile and taller than one 16-row tile, none a multiple of either.
HOOK_CASES = [((105, 151, 81), [(79, 113), (53, 76), (60, 151)]), ((209, 301, 83), [(53, 76)]), ((70, 300, 82), [(35, 150)])]


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
@pytest.mark.parametrize("mode", CURVES)
def test_hook_against_float64(swin, mode, filt):
    for shape, sizes in HOOK_CASES:
        canvas = overshoot_canvas(*shape)
        for size in sizes:
            tag = f"hook {shape[0]}x{shape[1]}"
            for bits in (8, 10, 16):
                check_codes(tag, hook(swin, canvas, size, bits, filt, mode), canvas, size, filt, mode, bits)
            check_float(tag, hook(swin, canvas, size, 32, filt, mode), canvas, size, filt, mode)


def test_hook_under_gamma_is_the_plain_resize(swin):
    canvas = overshoot_canvas(52, 76, 81)
    out = hook(swin, canvas, (26, 38), 8, "bicubic", "gamma")
    want = ref.codes(ref.linear_resized(canvas, (26, 38), "bicubic", "gamma"), 8)
    assert np.abs(out.astype(int) - want.astype(int)).max() <= 1 and (out == want).mean() >= 0.999


# ---- 3. the engine against the oracle: the captured canvas of pipeline.render (test_gpu_resize.oracle_canvas), then light_ref
_canvases = {}


def canvas_of(key, eng, frame, monkeypatch, **kw):
    if key not in _canvases:
        _canvases[key] = oracle_canvas(eng, frame, monkeypatch, **kw)
    return _canvases[key]


SWIN = dict(batch=2, tile=64, scale=4, ov=0.0625)


@pytest.mark.parametrize("mode", CURVES)
def test_swin_render_resized_against_the_oracle(swin, monkeypatch, mode):
    """the noisy ragged frame to x3, x2 and x1 (the share that tells the rules apart grows as the target shrinks), the smooth one for the accuracy figure alone"""
    for kind, frame in (("noisy", noisy_frame(75, 53, 12)), ("smooth", smooth_frame(100, 140, 11))):
        canvas, full = canvas_of(("swin", kind), swin, frame, monkeypatch, **SWIN)
        r, c = frame.shape[:2]
        assert swin.set_resize_light(mode)
        for size, filt in (((3 * r, 3 * c), "bicubic"), ((2 * r, 2 * c), "bilinear"), ((r, c), "bicubic")):
            out = swin.render_resized(frame, size, filt)
            check_codes(f"swin {kind}", out[..., ::-1], canvas, size, filt, mode, 8, neighbours=kind == "noisy")
        assert np.array_equal(swin.render_resized(frame, (4 * r, 4 * c)), full)          # the scaled size: render()'s bytes, no round trip


@pytest.mark.parametrize("mode", CURVES)
def test_sixteen_bit_render_resized_against_the_oracle(swin, monkeypatch, mode):
    """the noisy ragged frame at 16 bits, code c as c * 257 - the same values c / 255.  (Noise in the low byte is left out: such a frame's plain render() is
    already up to 64 LSB16 away from the oracle, under gamma and without any resize - the network's fp16 input, not this path.)"""
    frame = noisy_frame(75, 53, 12).astype(np.uint16) * 257
    canvas, full = canvas_of(("swin", "noisy16"), swin, frame, monkeypatch, **SWIN)
    assert swin.set_resize_light(mode)
    for size in ((150, 106), (225, 130)):
        out = swin.render_resized(frame, size)
        assert out.dtype == np.uint16
        check_codes("swin 16-bit", out[..., ::-1], canvas, size, "bicubic", mode, 16)
    assert np.array_equal(swin.render_resized(frame, (300, 212)), full)


def test_cunet_tta_against_the_oracle(cunet_tta, monkeypatch):
    """cunet x2 with TTA and no overlap.  The mean over eight augmentations leaves this network's output little contrast (canvas 0.32 .. 0.50 on the noise frame,
    std 0.044): at 8 bits the three rules agree to 1 code, so the 8-bit case gives the accuracy figure alone and the 16-bit frame (c * 257) carries the
    neighbour assertions - at that depth the curvature of the curves over such a spread is tens of codes."""
    frame = noisy_frame(67, 45, 22)
    canvas, _ = canvas_of(("cunet", "noisy"), cunet_tta, frame, monkeypatch, batch=2, tile=64, scale=2, ov=0.0, tta=True)
    frame16 = frame.astype(np.uint16) * 257
    canvas16, _ = canvas_of(("cunet", "noisy16"), cunet_tta, frame16, monkeypatch, batch=2, tile=64, scale=2, ov=0.0, tta=True)
    for mode in CURVES:
        assert cunet_tta.set_resize_light(mode)
        for size, filt in (((100, 68), "bicubic"), ((67, 45), "bilinear")):
            check_codes("cunet tta", cunet_tta.render_resized(frame, size, filt)[..., ::-1], canvas, size, filt, mode, 8, neighbours=False)
            check_codes("cunet tta 16-bit", cunet_tta.render_resized(frame16, size, filt)[..., ::-1], canvas16, size, filt, mode, 16)


def test_fp32_engine_against_the_oracle(pkg, onnx_model, monkeypatch):
    """the fp32-storage engine: the float4v instantiation of the decoding canvas kernel"""
    path = onnx_model("cunet/art", 2, 1, 64)
    eng = pkg.Img2Img()
    assert eng.set_resize_light("srgb")                                                   # before load(): kept
    assert eng.build(path, pkg.BuildConfig.fixed(1, 64, precision=pkg.Precision.FP32)), eng.last_error()
    assert eng.load(path, pkg.RenderConfig(precision=pkg.Precision.FP32, batchSize=1, height=64, width=64, scaling=2, overlap=(0.0625, 0.0625))), eng.last_error()
    assert eng.resize_light() == "srgb"
    frame = noisy_frame(70, 50, 41)
    canvas, _ = oracle_canvas(eng, frame, monkeypatch, batch=1, tile=64, scale=2, ov=0.0625, fp16=False)
    check_codes("fp32 engine", eng.render_resized(frame, (105, 75))[..., ::-1], canvas, (105, 75), "bicubic", "srgb", 8)
    assert eng.set_resize_light("bt709")
    check_codes("fp32 engine", eng.render_resized(frame, (88, 61), "bilinear")[..., ::-1], canvas, (88, 61), "bilinear", "bt709", 8)
    eng.close()


# ---- 4. equalities under srgb (no oracle)
def test_planar_gray_and_float_equalities(swin):
    frame = noisy_frame(61, 45, 91)
    size = (140, 99)
    assert swin.set_resize_light("srgb")
    bgr = swin.render_resized(frame, size)
    rgb_planes = tuple(np.ascontiguousarray(frame[..., 2 - k]) for k in range(3))
    planes = swin.render_planar_resized(rgb_planes, size)
    assert all(np.array_equal(planes[k], bgr[..., 2 - k]) for k in range(3)), "planar 8 / 8 is render_resized's planes"
    frame16 = (frame.astype(np.uint16) * 257)
    bgr16 = swin.render_resized(frame16, size)
    planes16 = swin.render_planar_resized(tuple(np.ascontiguousarray(frame16[..., 2 - k]) for k in range(3)), size)
    assert all(np.array_equal(planes16[k], bgr16[..., 2 - k]) for k in range(3)), "planar 16 / 16 is render_resized's planes"
    # every integer depth is the quantisation of the float output
    V = swin.render_planar_resized(rgb_planes, size, out_bits=32)
    assert all(p.dtype == np.float32 for p in V)
    for bits in (8, 10, 12, 16):
        got = swin.render_planar_resized(rgb_planes, size, out_bits=bits)
        want = dither_ref.dither_planes(V, bits, "none")
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), f"{bits} bits is not the quantised float output"
    assert not np.array_equal(planes[1], planes_gamma(swin, rgb_planes, size)[1]), "srgb and gamma give the same bytes"
    assert swin.set_resize_light("srgb")
    # ordered dither under srgb: floor(V * maxcode + t) of the float output
    assert swin.set_dither("ordered", 3)
    for bits in (8, 10):
        got = swin.render_planar_resized(rgb_planes, size, out_bits=bits)
        want = dither_ref.dither_planes(V, bits, "ordered", 3)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), f"ordered dither at {bits} bits"
    assert same(swin.render_planar_resized(rgb_planes, size, out_bits=32), V), "float output is never dithered"
    assert swin.set_dither("none")
    # gray: the green channel of the replicated frame
    gray = np.ascontiguousarray(frame[..., 1])
    rep = np.repeat(gray[..., None], 3, -1)
    assert np.array_equal(swin.render_gray_resized(gray, size), swin.render_resized(rep, size)[..., 1])


def planes_gamma(eng, planes, size):
    eng.set_resize_light("gamma")
    return eng.render_planar_resized(planes, size)


def test_rgba_colour_is_encoded_and_alpha_is_not(swin, pkg):
    rng = np.random.default_rng(92)
    frame = noisy_frame(58, 47, 93)
    alpha = (rng.integers(0, 256, (58, 47)) * (rng.random((58, 47)) > 0.3)).astype(np.uint8)
    bgra = np.ascontiguousarray(np.dstack([frame, alpha]))
    size = (120, 111)
    outs = {}
    for mode in ("gamma", "srgb", "bt709"):
        assert swin.set_resize_light(mode)
        outs[mode] = swin.render_rgba_resized(bgra, size, bleed=3)
        bled = pkg.alpha_bleed(frame, alpha, 3)
        assert np.array_equal(outs[mode][..., :3], swin.render_resized(bled, size)), f"{mode}: the colour is render_resized of the bled colour"
        planes = tuple(np.ascontiguousarray(bgra[..., k]) for k in (2, 1, 0, 3))
        outs[mode + " planar"] = swin.render_planar_rgba_resized(planes, size, bleed=3)
        assert all(np.array_equal(outs[mode + " planar"][k], outs[mode][..., (2, 1, 0, 3)[k]]) for k in range(4)), mode
        opaque = np.ascontiguousarray(np.dstack([frame, np.full((58, 47), 200, np.uint8)]))
        outs[mode + " uniform"] = swin.render_rgba_resized(opaque, size, skip_uniform_alpha=True)
        assert (outs[mode + " uniform"][..., 3] == 200).all()
    for mode in CURVES:
        assert np.array_equal(outs[mode][..., 3], outs["gamma"][..., 3]), f"{mode}: alpha bytes depend on the setting"
        assert np.array_equal(outs[mode + " planar"][3], outs["gamma planar"][3])
        assert not np.array_equal(outs[mode][..., :3], outs["gamma"][..., :3])


def test_sequences_scaled_size_and_gamma(swin):
    frames = [noisy_frame(60, 44, 71 + k) for k in range(4)]
    for mode in CURVES:
        assert swin.set_resize_light(mode)
        want = [swin.render_resized(f, FRESH_SIZE) for f in frames]
        got = swin.render_sequence_resized(frames, FRESH_SIZE)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), f"{mode}: a sequence is its single calls"
        assert not np.array_equal(want[0], swin.fresh[0])
        planes = [tuple(np.ascontiguousarray(f[..., 2 - k]) for k in range(3)) for f in frames[:2]]
        seq = swin.render_sequence_planar(planes, FRESH_SIZE, out_bits=10)
        assert all(same(a, swin.render_planar_resized(p, FRESH_SIZE, out_bits=10)) for a, p in zip(seq, planes))
    full = {}
    for mode in ("gamma", "srgb", "bt709"):
        assert swin.set_resize_light(mode)
        full[mode] = swin.render_resized(frames[0], (240, 176))
        assert np.array_equal(full[mode], swin.render(frames[0])), f"{mode}: the scaled size is render()"
    assert np.array_equal(full["srgb"], full["gamma"]) and np.array_equal(full["bt709"], full["gamma"])
    # back to gamma: the bytes the engine gave before it was ever told about the setting
    assert swin.set_resize_light("gamma")
    assert np.array_equal(swin.render_resized(frames[0], FRESH_SIZE), swin.fresh[0])
    assert np.array_equal(swin.render_resized(frames[0], FRESH_SIZE, "bilinear"), swin.fresh[1])


# ---- 5. YUV: odd source and target sizes, every layout's kernel
YUV_OUTS = [("i420", "left", 8), ("i420", "center", 8), ("i420", "topleft", 8), ("i422", "left", 10), ("i444", "left", 8), ("nv12", "left", 8)]
YUV_SIZE = (101, 151)


@pytest.mark.parametrize("mode", CURVES)
def test_yuv_layouts_against_float64(swin, monkeypatch, mode):
    """the 45 x 67 noise frame (4:2:0, left) to 101 x 151 in every output layout and siting: within 1 code of clip -> decode -> resize -> clip -> encode -> the
    Y'CbCr matrix and the site filters on V, in every plane"""
    planes = ysr.gpu_noise(45, 67)
    key = ("yuv", 45, 67)
    if key not in _canvases:
        _canvases[key] = yuv_oracle_canvas(swin, ysr.decode(planes, "i420", "left"), monkeypatch, **SWIN)
    canvas = _canvases[key]
    V = {m: ref.linear_resized(canvas, YUV_SIZE, "bicubic", m) for m in ref.MODES}
    assert swin.set_resize_light(mode)
    outs = {}
    for layout, siting, bits in YUV_OUTS:
        out = swin.render_yuv_layout_resized(tuple(planes), YUV_SIZE, layout="i420", out_layout=layout, out_bits=bits, siting="left", out_siting=siting)
        outs[(layout, siting, bits)] = out
        want = ysr.encode(V[mode], layout, siting, bits=bits)
        far = {m: [] for m in ref.other_modes(mode)}
        for name, a, b, k in zip("YUV" if len(out) == 3 else ("Y", "UV"), out, want, range(3)):
            assert a.shape == b.shape and a.dtype == b.dtype
            d = np.abs(a.astype(np.int64) - b.astype(np.int64))
            print(f"LIGHT yuv {mode} -> {layout} {siting} {bits} bits {name}: max {int(d.max())} codes, exact {float((d == 0).mean()):.6f} of {d.size}")
            assert d.max() <= 1, (layout, siting, bits, name, int(d.max()))
            for m in far:
                far[m].append(np.abs(ysr.encode(V[m], layout, siting, bits=bits)[k].astype(np.int64) - b.astype(np.int64)).ravel() > 1)
        for m, parts in far.items():
            share = float(np.concatenate(parts).mean())
            print(f"LIGHT yuv {mode} -> {layout} {siting} {bits} bits: the reference of {m} is outside the bound in {share:.4f} of the samples")
            assert share >= 0.01, (layout, siting, bits, m, share)
    # the Y plane is one plane whatever the layout; NV12 holds the I420 samples
    y = outs[("i420", "left", 8)][0]
    for key8 in (("i420", "center", 8), ("i420", "topleft", 8), ("i444", "left", 8), ("nv12", "left", 8)):
        assert np.array_equal(outs[key8][0], y), key8
    y10 = swin.render_yuv_layout_resized(tuple(planes), YUV_SIZE, layout="i420", out_layout="i420", out_bits=10)[0]
    assert np.array_equal(outs[("i422", "left", 10)][0], y10)
    i420, nv12 = outs[("i420", "left", 8)], outs[("nv12", "left", 8)]
    assert np.array_equal(nv12[1][:, 0::2], i420[1]) and np.array_equal(nv12[1][:, 1::2], i420[2])
    # a sequence is its single calls, and the 4:2:0 entry is the layout entry
    seq = swin.render_sequence_yuv_layout_resized([tuple(planes)] * 2, YUV_SIZE, layout="i420", out_layout="nv12")
    assert all(same(s, nv12) for s in seq)
    assert same(swin.render_yuv_resized(*planes, YUV_SIZE), i420)
