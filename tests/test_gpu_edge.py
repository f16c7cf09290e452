"""Edge modes on the GPU (Img2Img::setEdge): what a tile, the colour bleed and the resize read beyond the frame edge - replicate (the default),
wrap, mirror.

Byte equality, no tolerance: eng.render(f) under each mode against the oracle pipeline (oracle/pipeline.py with the engine's own network, as
test_gpu_pipeline_bytes.py pins Replicate) with pipeline.pad_roi indexing through tests/edge_ref.py; the project's equalities between the frame formats
repeated under wrap and mirror; chains; the key of the captured passes.  Frames are noise, so opposite edges differ, and every oracle case asserts that its
three results differ from one another: without the feature the wrap and mirror cases fail.

The resize under a mode is checked against float64 (edge_ref.resized: np.pad in the mode, torch's antialiased resize to three times the target, the middle
third) under the bounds of DESIGN 9n: at most 1 code (at 16 bits: one code beyond the maximum of the float32 restatement of the same rule), a share of
unequal samples of at most twice that restatement's plus 0.001, and every case asserts that the Replicate reference lies outside the bound.  Float output: the
restatement's largest error plus 4e-6 - two passes of at most 17 taps summed in fp32 in another order than torch's: (17 + 1) * 2^-24 * sum|w v| per pass with
sum|w| <= 1.3 and |v| <= 1.05, the second pass carrying the first's error times 1.3: 18 * 6e-8 * 1.4 * 2.3 = 3.5e-6, and 2e-7 for the weights' own rounding.
Engines: the seeded synthetic graphs of tools/synth_models.py at tile 64, batch 2."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_ref as ref
import rgba_ref
from oracle import pipeline
from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W2X = os.path.join(ROOT, "waifu2x-tensorrt_amd", "w2x")
BLEND = (0.0625, 0.0625)
FLOAT_EXTRA = 4e-6
EDGED = ("wrap", "mirror")
# cunet x2, batch 2, tile 64 at noise level 0: a graph file of this module's own.  The suite's model directory is shared, load() takes any engine file it finds
# beside the graph, and tests/test_gpu_parity.py::test_error_paths asserts that none but a TF32 one lies beside the noise-3 graph of this shape.
CUNET = ("cunet/art", 2, 2, 64, 0)


def noise(rows, cols, seed, dtype=np.uint8, ch=3):
    return np.random.default_rng(seed).integers(0, np.iinfo(dtype).max + 1, (rows, cols, ch), dtype=dtype)


def same(tag, got, want):
    if isinstance(got, (tuple, list)):
        assert len(got) == len(want), tag
        for k in range(len(got)):
            same(f"{tag} plane {k}", got[k], want[k])
        return
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    bad = got != want
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {bad.size} samples differ, first at {tuple(np.argwhere(bad)[0])}"


def planes_of(bgr):
    return tuple(np.ascontiguousarray(bgr[..., k]) for k in (2, 1, 0))


def bgr_of(planes):
    return np.ascontiguousarray(np.stack([planes[2], planes[1], planes[0]], axis=-1))


def rep(g):
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2))


@pytest.fixture(scope="module")
def engines(pkg, onnx_model):
    made = {}

    def get(name):
        if name not in made:
            if name in ("cunet", "cunet_b"):
                made[name] = make_engine(pkg, onnx_model(*CUNET), 2, 64, 2, overlap=BLEND)
            elif name == "swin_tta":
                made[name] = make_engine(pkg, onnx_model("swin_unet/art", 4, 2, 64, small=True), 2, 64, 4, overlap=BLEND, tta=True)
            elif name == "swin":
                made[name] = make_engine(pkg, onnx_model("swin_unet/art", 4, 2, 64, small=True), 2, 64, 4, overlap=BLEND)
            elif name == "cunet_fp32":
                path = onnx_model(*CUNET)
                eng = pkg.Img2Img()
                assert eng.build(path, pkg.BuildConfig.fixed(2, 64, precision=pkg.Precision.FP32)), eng.last_error()
                assert eng.load(path, pkg.RenderConfig(precision=pkg.Precision.FP32, batchSize=2, height=64, width=64, scaling=2, overlap=BLEND)), eng.last_error()
                made[name] = eng
            else:
                raise KeyError(name)
        return made[name]
    yield get
    for eng in made.values():
        eng.close()


_USED = []


def use(engines, name):
    eng = engines(name)
    if not any(e is eng for e in _USED):
        _USED.append(eng)
    return eng


@pytest.fixture(autouse=True)
def settings_back():
    """every test leaves the module's engines at the default"""
    yield
    for eng in _USED:
        eng.set_edge("replicate")


def oracle(eng, frame, mode, monkeypatch, *, scale, tta=False, fp16=True):
    """oracle.pipeline.render with the engine's own network and pad_roi indexing through the rule of `mode`"""
    monkeypatch.setattr(pipeline, "pad_roi", ref.pad_roi(mode))
    out = pipeline.render(frame, eng.infer, batch=2, tile=64, scaling=scale, overlap=BLEND, tta=tta, net_dtype=np.float16 if fp16 else None, tile_out=eng.output_tile_size)
    monkeypatch.undo()
    return out


def smallest_side():
    """the smallest frame side a blend of 1/16 at tile 64 accepts: one more than the overlap (calculateTiles: nx = ceil((w - ov) / (stride - ov)))"""
    return pipeline.c_lround(64 * BLEND[0]) + 1


# ---- 1. byte equality against the oracle
ORACLE_CASES = [
    # name, engine, scale, tta, fp16, frame
    ("cunet x2 blend 70x90", "cunet", 2, False, True, lambda: noise(70, 90, 1)),                       # several tiles, seams on every side
    ("swin x4 tta 45x67", "swin_tta", 4, True, True, lambda: noise(45, 67, 2)),
    ("cunet x2 16-bit 70x90", "cunet", 2, False, True, lambda: noise(70, 90, 3).astype(np.uint16) * 257),   # (code c as c * 257, like the 16-bit cases of test_gpu_resize_light.py)
    ("cunet x2 fp32 57x70", "cunet_fp32", 2, False, False, lambda: noise(57, 70, 4)),
    ("cunet x2 7x6: smaller than the tile border", "cunet", 2, False, True, lambda: noise(7, 6, 5)),   # cunet's border is 18 pixels: the rule folds more than once
    ("cunet x2 smallest frame", "cunet", 2, False, True, lambda: noise(smallest_side(), smallest_side(), 6)),
]


@pytest.mark.parametrize("name,engine,scale,tta,fp16,make", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_render_under_each_mode_is_the_oracle_with_the_rule(engines, monkeypatch, name, engine, scale, tta, fp16, make):
    eng, frame = use(engines, engine), make()
    want = {mode: oracle(eng, frame, mode, monkeypatch, scale=scale, tta=tta, fp16=fp16) for mode in ref.MODES}
    for a, b in (("replicate", "wrap"), ("replicate", "mirror"), ("wrap", "mirror")):
        assert (want[a] != want[b]).any(), f"{name}: the oracle's {a} and {b} frames are the same"
    for mode in ("wrap", "mirror", "replicate"):
        assert eng.set_edge(mode) and eng.edge() == mode
        same(f"{name} {mode}", eng.render(frame), want[mode])
        same(f"{name} {mode}, again", eng.render(frame), want[mode])


def test_the_smallest_frame_is_the_smallest(engines):
    eng, n = use(engines, "cunet"), smallest_side()
    assert n >= 2
    for mode in ref.MODES:
        assert eng.set_edge(mode)
        with pytest.raises(Exception):
            eng.render(noise(n - 1, n - 1, 7))
        assert eng.render(noise(n, n, 7)).shape == (2 * n, 2 * n, 3)


# ---- 2. the project's equalities, under wrap and under mirror
def quantised(f, bits):
    m = (1 << bits) - 1
    return np.clip(np.rint(f * np.float32(m)), 0, m).astype(np.uint8 if bits == 8 else np.uint16)


def rgba_noise(rows, cols, seed):
    f = noise(rows, cols, seed, ch=4)
    f[..., 3] = f[..., 3] * (np.random.default_rng(seed + 1).random((rows, cols)) < 0.5)
    f[:, :3, 3] = 0                                               # a transparent band on the left edge: under wrap its colour comes from the right edge
    f[-2:, :, 3] = 0
    return f


@pytest.mark.parametrize("mode", EDGED)
def test_gray_and_planar_are_render(engines, mode):
    eng = use(engines, "cunet")
    f, f16 = noise(40, 52, 11), noise(40, 52, 12, np.uint16)
    assert eng.set_edge("replicate")
    plain = eng.render(f)
    assert eng.set_edge(mode)
    out, out16 = eng.render(f), eng.render(f16)
    assert (out != plain).any()
    g, g16 = np.ascontiguousarray(f[..., 1]), np.ascontiguousarray(f16[..., 1])
    same(f"{mode} gray", eng.render_gray(g), np.ascontiguousarray(eng.render(rep(g))[..., 1]))
    same(f"{mode} gray 16", eng.render_gray(g16), np.ascontiguousarray(eng.render(rep(g16))[..., 1]))
    same(f"{mode} planar 8 / 8", eng.render_planar(planes_of(f)), planes_of(out))
    same(f"{mode} planar 16 / 16", eng.render_planar(planes_of(f16)), planes_of(out16))
    fl = eng.render_planar(planes_of(f), out_bits=32)
    for bits in (8, 10, 16):
        same(f"{mode} planar out_bits {bits}", eng.render_planar(planes_of(f), out_bits=bits), tuple(quantised(p, bits) for p in fl))
    # resized: the same equalities on the resize under the mode
    size = (61, 79)
    bgr = eng.render_resized(f, size)
    same(f"{mode} planar resized", eng.render_planar_resized(planes_of(f), size), planes_of(bgr))
    same(f"{mode} gray resized", eng.render_gray_resized(g, size), np.ascontiguousarray(eng.render_resized(rep(g), size)[..., 1]))
    flr = eng.render_planar_resized(planes_of(f), size, out_bits=32)
    same(f"{mode} planar resized out_bits 16", eng.render_planar_resized(planes_of(f), size, out_bits=16), tuple(quantised(p, 16) for p in flr))
    same(f"{mode} the scaled size is the plain call", eng.render_resized(f, (80, 104)), out)


@pytest.mark.parametrize("mode", EDGED)
def test_rgba_is_the_bleed_under_the_mode_and_two_renders(engines, pkg, mode):
    eng = use(engines, "cunet")
    bgra = rgba_noise(40, 52, 21)
    bgr, a = np.ascontiguousarray(bgra[..., :3]), np.ascontiguousarray(bgra[..., 3])
    assert eng.set_edge(mode)
    alpha = np.ascontiguousarray(eng.render(rep(a))[..., 1])
    for radius in (0, 3):
        bled = pkg.alpha_bleed(bgr, a, radius, edge=mode)
        same(f"{mode} host bleed is the reference's", bled, ref.bleed(bgr, a, radius, mode))
        if radius:
            assert (bled != rgba_ref.bleed(bgr, a, radius)).any() == (mode == "wrap"), "wrap alone takes colour across the joint"
        out = eng.render_rgba(bgra, bleed=radius)
        same(f"{mode} bleed {radius} colour", np.ascontiguousarray(out[..., :3]), eng.render(bled))
        same(f"{mode} bleed {radius} alpha", np.ascontiguousarray(out[..., 3]), alpha)
        # planar RGBA likewise, at 8 and at 16 bits
        for bits, scale in ((8, 1), (16, 257)):
            dt = np.uint8 if bits == 8 else np.uint16
            planes = [np.ascontiguousarray(bgra[..., k]).astype(dt) * dt(scale) for k in (2, 1, 0, 3)]
            colour = pkg.alpha_bleed_planes(planes, radius, bits=bits, edge=mode)
            got = eng.render_planar_rgba(planes, bleed=radius)
            same(f"{mode} planar rgba {bits} bits bleed {radius} colour", tuple(got[:3]), eng.render_planar(colour))
            same(f"{mode} planar rgba {bits} bits bleed {radius} alpha", got[3], eng.render_planar((planes[3],) * 3)[1])
    size = (61, 79)
    out = eng.render_rgba_resized(bgra, size, bleed=3)
    same(f"{mode} rgba resized colour", np.ascontiguousarray(out[..., :3]), eng.render_resized(pkg.alpha_bleed(bgr, a, 3, edge=mode), size))
    same(f"{mode} rgba resized alpha", np.ascontiguousarray(out[..., 3]), np.ascontiguousarray(eng.render_resized(rep(a), size)[..., 1]))


@pytest.mark.parametrize("mode", EDGED)
def test_sequences_are_their_single_calls(engines, mode):
    eng = use(engines, "cunet")
    assert eng.set_edge(mode)
    frames = [noise(40, 52, 30 + k) for k in range(3)]
    for k, out in enumerate(eng.render_sequence(frames)):
        same(f"{mode} sequence frame {k}", out, eng.render(frames[k]))
    for k, out in enumerate(eng.render_sequence_resized(frames, (61, 79))):
        same(f"{mode} resized sequence frame {k}", out, eng.render_resized(frames[k], (61, 79)))
    grays = [np.ascontiguousarray(f[..., 0]) for f in frames]
    for k, out in enumerate(eng.render_sequence_gray(grays)):
        same(f"{mode} gray sequence frame {k}", out, eng.render_gray(grays[k]))
    rgbas = [rgba_noise(40, 52, 40 + k) for k in range(2)]
    for k, out in enumerate(eng.render_sequence_rgba(rgbas, bleed=2)):
        same(f"{mode} rgba sequence frame {k}", out, eng.render_rgba(rgbas[k], bleed=2))
    for k, out in enumerate(eng.render_sequence_planar([planes_of(f) for f in frames[:2]], out_bits=10)):
        same(f"{mode} planar sequence frame {k}", tuple(out), eng.render_planar(planes_of(frames[k]), out_bits=10))


def test_device_bleed_is_the_host_bleed(engines, pkg):
    """alpha_bleed_kernel and its planar twin under wrap: frames of a single pixel, a single row and a single column (the halo is many periods), one workgroup
    tile and several; under mirror they stay the plain bleed"""
    eng = use(engines, "cunet")
    cases = [c for c in rgba_ref.cases() if c[0].startswith(("random", "sparse", "corner"))]
    rng = np.random.default_rng(77)
    bgr = rng.integers(0, 256, (150, 200, 3), dtype=np.uint8)
    a = np.full((150, 200), 255, np.uint8)
    a[:, :20] = 0; a[:9, :] = 0; a[60:100, 185:200] = 0; a[20:75, 40:150] = 0          # holes on every frame edge and across the workgroup tiles (64 x 32)
    cases.append(("tiled 150x200", bgr, a, (1, 5, 16)))
    differs = 0
    for mode in ("wrap", "mirror"):
        assert eng.set_edge(mode)
        for name, bgr, alpha, radii in cases:
            bgra = np.ascontiguousarray(np.dstack([bgr, alpha]))
            for r in radii:
                want = pkg.alpha_bleed(bgr, alpha, r, edge=mode)
                got = eng.alpha_bleed_device(bgra, r)
                assert np.array_equal(got, want), f"{mode} {name} at radius {r}: {int((got != want).sum())} bytes differ"
                plain = rgba_ref.bleed(bgr, alpha, r)
                if mode == "wrap":
                    differs += not np.array_equal(want, plain)
                else:
                    assert np.array_equal(got, plain)
        # the planar kernel, 8 / 10 / 16 bits, a ragged frame of several tiles
        for bits in (8, 10, 16):
            dt = np.uint8 if bits == 8 else np.uint16
            prng = np.random.default_rng(bits)
            planes = [prng.integers(0, 1 << bits, (75, 141)).astype(dt) for _ in range(3)]
            planes.append((prng.integers(0, 1 << bits, (75, 141)) * (prng.random((75, 141)) < 0.05)).astype(dt))
            for r in (1, 7, 16):
                same(f"{mode} planar bleed {bits} bits radius {r}", tuple(eng.alpha_bleed_planes_device(planes, r, bits=bits)), tuple(pkg.alpha_bleed_planes(planes, r, bits=bits, edge=mode)))
    assert differs >= 10


# ---- 3. chains
@pytest.mark.parametrize("modes", [("wrap", "wrap"), ("mirror", "mirror"), ("wrap", "mirror"), ("replicate", "wrap")])
def test_chains_gather_under_their_own_engines_modes(engines, pkg, modes):
    a, b = use(engines, "cunet"), use(engines, "cunet_b")
    f = noise(40, 52, 51)
    assert a.set_edge("replicate") and b.set_edge("replicate")
    plain = pkg.render_chained([a, b], f)
    assert a.set_edge(modes[0]) and b.set_edge(modes[1])
    mid = a.render_planar(planes_of(f), out_bits=32)
    got = pkg.render_chained_planar([a, b], planes_of(f))
    same(f"{modes} unquantised chain is the float route", tuple(got), b.render_planar(mid, out_bits=8))
    same(f"{modes} interleaved", pkg.render_chained([a, b], f), bgr_of(got))
    assert (pkg.render_chained([a, b], f) != plain).any()
    same(f"{modes} quantised chain is two calls", pkg.render_chained([a, b], f, quantize=True), b.render(a.render(f)))
    # the last engine's mode governs the resize
    target = (121, 157)
    same(f"{modes} resized chain", pkg.render_chained_resized([a, b], f, target), bgr_of(b.render_planar_resized(mid, target, out_bits=8)))


# ---- 4. the key of the captured passes
def test_a_call_after_set_edge_does_not_replay_the_old_gather(engines, pkg, onnx_model):
    """One engine, one frame: replicate -> wrap -> mirror -> replicate, three calls each (a pass runs eagerly at first sight, is captured at the second and
    replayed from the third).  Each call gives its own mode's bytes, which are a fresh engine's."""
    eng = use(engines, "cunet")
    f = noise(70, 90, 61)
    fresh = {}
    for mode in ref.MODES:
        e = pkg.Img2Img()
        assert e.set_edge(mode)                                   # before load(): kept
        assert e.load(onnx_model(*CUNET), pkg.RenderConfig(batchSize=2, height=64, width=64, scaling=2, overlap=BLEND)), e.last_error()
        assert e.edge() == mode
        fresh[mode] = e.render(f)
        e.close()
    assert (fresh["replicate"] != fresh["wrap"]).any() and (fresh["replicate"] != fresh["mirror"]).any() and (fresh["wrap"] != fresh["mirror"]).any()
    for mode in ("replicate", "wrap", "mirror", "replicate", "mirror", "wrap"):
        assert eng.set_edge(mode)
        for k in range(3):
            same(f"{mode}, call {k}", eng.render(f), fresh[mode])
    # the other formats' passes carry the key too
    g = np.ascontiguousarray(f[..., 1])
    outs = {}
    for mode in ("replicate", "wrap", "replicate", "wrap"):
        assert eng.set_edge(mode)
        for k in range(3):
            out = eng.render_gray(g)
            same(f"gray {mode}, call {k}", out, outs.setdefault(mode, out))
    assert (outs["replicate"] != outs["wrap"]).any()


# ---- 5. the resize under a mode
def edged_canvas(rows, cols, seed):
    """noise with overshoot on a ramp along both axes: opposite edges differ strongly"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    ramp = 0.8 * (0.5 * x / (cols - 1) + 0.5 * y / (rows - 1))
    return (ramp[..., None] + rng.uniform(-0.05, 0.25, (rows, cols, 3))).astype(np.float32)


def replicate_resized(canvas, size, filt):
    x = torch.from_numpy(np.ascontiguousarray(canvas, np.float64)).permute(2, 0, 1)[None]
    return F.interpolate(x, size=tuple(size), mode=filt, antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()


# canvas 105 x 151 (odd both ways): x 3/4, x 1/2 and a mixed target that keeps the width; canvas 209 x 301: x 1/4 (the largest factor, rows_max at its top);
# canvas 70 x 300 -> x 1/2.  Every target is wider than one 64-column tile and taller than one 16-row tile, none a multiple of either.
HOOK_CASES = [((105, 151, 81), [(79, 113), (53, 76), (60, 151)]), ((209, 301, 83), [(53, 76)]), ((70, 300, 82), [(35, 150)])]
_REFS = {}


def references(shape, size, filt, mode):
    key = (shape, size, filt, mode)
    if key not in _REFS:
        canvas = edged_canvas(*shape)
        _REFS[key] = tuple(np.clip(v, 0, 1) for v in (ref.resized(canvas, size, filt, mode), ref.resized(canvas, size, filt, mode, np.float32).astype(np.float64),
                                                      replicate_resized(canvas, size, filt)))
        for v in _REFS[key]:
            v.setflags(write=False)
    return _REFS[key]


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
@pytest.mark.parametrize("mode", EDGED)
def test_resize_hook_against_float64(engines, mode, filt):
    eng = use(engines, "swin")
    assert eng.set_edge(mode)
    for shape, sizes in HOOK_CASES:
        canvas = edged_canvas(*shape)
        planes = [np.ascontiguousarray(canvas[..., k]) for k in range(3)]
        for size in sizes:
            want, model, plain = references(shape, size, filt, mode)
            tag = f"EDGE hook {shape[0]}x{shape[1]} -> {size[0]}x{size[1]} {mode} {filt}"
            for bits in (8, 16):
                got = np.stack(eng.resize_planes(planes, size, bits, filt), -1).astype(np.int64)
                w, m, p = (ref.codes(v, bits).astype(np.int64) for v in (want, model, plain))
                d, dm = np.abs(got - w), np.abs(m - w)
                share, share_m, top, top_m = float((d != 0).mean()), float((dm != 0).mean()), int(d.max()), int(dm.max())
                tol = 1 if bits == 8 else top_m + 1
                far = int((np.abs(p - w) > tol).sum())
                print(f"{tag} {bits} bits: device off {share:.6f} max {top}; fp32 model off {share_m:.6f} max {top_m}; bound max {tol}; replicate outside the bound in {far} samples")
                assert top <= tol, f"{tag} {bits} bits: {top} codes off, bound {tol}"
                assert share <= 2 * share_m + 0.001, f"{tag} {bits} bits: {share:.6f} of the samples differ, the model's {share_m:.6f}"
                assert far > 0, f"{tag} {bits} bits: the bound does not tell {mode} from replicate"
            got = np.stack(eng.resize_planes(planes, size, 32, filt), -1)
            err, err_m = float(np.abs(got.astype(np.float64) - want).max()), float(np.abs(model - want).max())
            print(f"{tag} float: device max error {err:.3e}; fp32 model {err_m:.3e}; bound {err_m + FLOAT_EXTRA:.3e}")
            assert got.dtype == np.float32 and got.min() >= 0.0 and got.max() <= 1.0
            assert err <= err_m + FLOAT_EXTRA, f"{tag} float: {err:.3e} > {err_m + FLOAT_EXTRA:.3e}"
            assert float(np.abs(plain - want).max()) > err_m + FLOAT_EXTRA


def test_resize_hook_under_replicate_is_untouched(engines):
    eng = use(engines, "swin")
    canvas = edged_canvas(105, 151, 81)
    planes = [np.ascontiguousarray(canvas[..., k]) for k in range(3)]
    assert eng.set_edge("replicate")
    before = eng.resize_planes(planes, (53, 76), 8)
    assert eng.set_edge("wrap")
    wrapped = eng.resize_planes(planes, (53, 76), 8)
    assert eng.set_edge("replicate")
    same("replicate after wrap", tuple(eng.resize_planes(planes, (53, 76), 8)), tuple(before))
    assert any((a != b).any() for a, b in zip(wrapped, before))
    # a tiny canvas: a tile needs the same input row more than once
    tiny = edged_canvas(3, 5, 9)
    assert eng.set_edge("wrap")
    got = np.stack(eng.resize_planes([np.ascontiguousarray(tiny[..., k]) for k in range(3)], (2, 3), 32), -1)
    want = np.clip(ref.resized_by_taps(tiny, (2, 3), "bicubic", "wrap"), 0, 1)
    assert np.abs(got - want).max() <= FLOAT_EXTRA


def test_render_resized_under_wrap_against_the_oracle(engines, monkeypatch):
    """the engine's whole path: the oracle's canvas (pad_roi through the rule, captured where pipeline.render quantises it) followed by the reference resize,
    within tests/test_gpu_resize.py's bound: at most 1 LSB and at least 99.9 % of the samples equal"""
    eng = use(engines, "swin")
    frame = noise(75, 53, 12)
    seen = {}
    orig = pipeline.to_u8
    monkeypatch.setattr(pipeline, "to_u8", lambda canvas: (seen.__setitem__("canvas", canvas.copy()), orig(canvas))[1])
    monkeypatch.setattr(pipeline, "pad_roi", ref.pad_roi("wrap"))
    full = pipeline.render(frame, eng.infer, batch=2, tile=64, scaling=4, overlap=BLEND, net_dtype=np.float16, tile_out=eng.output_tile_size)
    monkeypatch.undo()
    assert eng.set_edge("wrap")
    for size, filt in (((225, 159), "bicubic"), ((150, 106), "bilinear"), ((75, 212), "bicubic")):
        want = ref.codes(np.clip(ref.resized(seen["canvas"], size, filt, "wrap"), 0, 1), 8)[..., ::-1]
        out = eng.render_resized(frame, size, filt)
        d = np.abs(out.astype(np.int64) - want.astype(np.int64))
        exact = float((d == 0).mean())
        print(f"EDGE render_resized wrap {filt} -> {size}: max {int(d.max())} LSB, exact {exact:.6f}")
        assert out.shape == want.shape and d.max() <= 1 and exact >= 0.999
    same("the scaled size is render()", eng.render_resized(frame, (300, 212)), full)


# ---- 6. refusals
def test_yuv_strips_and_shards_are_refused_by_name(engines, pkg):
    eng, other = use(engines, "cunet"), use(engines, "cunet_b")
    L = pkg.lib()
    f = noise(40, 52, 71)
    before = eng.render(f)
    y, u = np.zeros((40, 52), np.uint8), np.zeros((20, 26), np.uint8)
    for mode in EDGED:
        assert eng.set_edge(mode)
        want = eng.render(f)
        dst = np.full((80, 104, 3), 9, np.uint8)
        outs = (np.full((80, 104), 9, np.uint8), np.full((40, 52), 9, np.uint8), np.full((40, 52), 9, np.uint8))
        handles = (C.c_void_p * 2)(eng._h, other._h)
        calls = {
            "renderStrip": lambda: eng.render_strip(f, dst, 0, 2),
            "renderYuv": lambda: eng.render_yuv(y, u, u, out=outs),
            "renderSharded": lambda: bool(L.w2x_render_sharded(handles, 2, f.ctypes.data, 40, 52, f.strides[0], dst.ctypes.data, dst.strides[0])),
            "shardCompute": lambda: eng.shard_compute(f, 0, 2),
        }
        for who, call in calls.items():
            del eng.messages[:]
            assert call() is False, who
            assert len(eng.messages) == 1 and eng.messages[0][1].startswith(f"[{who}@") and f"setEdge({mode})" in eng.messages[0][1], (who, eng.messages)
        assert (dst == 9).all() and all((p == 9).all() for p in outs)
        same(f"{mode}: the next valid call", eng.render(f), want)
    assert eng.set_edge("replicate")
    same("replicate again", eng.render(f), before)
    dst = np.zeros((80, 104, 3), np.uint8)
    assert eng.render_strip(f, dst, 0, 1)
    same("a strip of one is render()", dst, before)
    # an unknown mode leaves the setting
    assert eng.set_edge("wrap") and L.w2x_set_edge(eng._h, 7) == 0 and eng.edge() == "wrap"


# ---- 7. the command line
def test_cli_edge_on_a_still(pkg, tmp_path):
    """`w2x render --edge wrap` on a PPM still gives the library's bytes, plain and with --outsize"""
    import synth_models as sm
    from test_cli import _read_png_rows
    path = sm.model_path(str(tmp_path), "cunet/art", 2, 3)
    sm.export_onnx(sm.make_model("cunet/art", 2, seed=5), path, 2, 64, dynamic=True)
    common = ["--models", str(tmp_path / "models"), "--model", "cunet/art", "--scale", "2", "--noise", "3", "--batchSize", "2", "--tileSize", "64"]
    rgb = noise(45, 60, 81)
    (tmp_path / "tex.ppm").write_bytes(b"P6\n60 45\n255\n" + rgb.tobytes())
    out = tmp_path / "out"; out.mkdir()
    r = subprocess.run([W2X, *common, "build"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    eng = pkg.Img2Img()
    assert eng.load(path, pkg.RenderConfig(batchSize=2, height=64, width=64, scaling=2)), eng.last_error()
    bgr = np.ascontiguousarray(rgb[..., ::-1])
    plain = eng.render(bgr)
    assert eng.set_edge("wrap")
    for extra, name, want in (((), "tex(cunet_art)(noise3)(scale2).png", eng.render(bgr)),
                              (("--outsize", "100x70"), "tex(cunet_art)(noise3)(scale2)(100x70).png", eng.render_resized(bgr, (70, 100)))):
        r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "tex.ppm"), "-o", str(out), "--edge", "wrap", *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got, depth = _read_png_rows(out / name)
        assert depth == 8
        same(f"cli --edge wrap {extra}", np.ascontiguousarray(got[..., :3].astype(np.uint8)), np.ascontiguousarray(want[..., ::-1]))
    assert (eng.render(bgr) != plain).any()
    eng.close()
