"""Chained renders on the GPU (Img2Img::renderChained and its neighbours): one frame through two or three engines with the frame staying on the device
between them.  Every check is equality on every byte (float output: every bit) with what the single calls give one after the other; there is no tolerance.
  unquantised: render_chained_planar([a, b], f) == b.render_planar(a.render_planar(f, out_bits=32)) - the float frame between the two single calls is the
               clamped, unrounded canvas, which is what the chain keeps on the device in the consuming engine's tile type;
  quantised:   render_chained([a, b], f, quantize=True) == b.render(a.render(f)).
Engines: the seeded synthetic graphs of tools/synth_models.py at tile 64, batch 2, with the weights of their image head times HEAD_GAIN.  As they are seeded the
graphs keep their output inside (0.2, 0.9) - by design, synth_models._init - and no frame takes a first stage to 0 or 1; with the gain a black block comes out
as exactly 0.0 and a white one as exactly 1.0, and where two saturated tiles blend the canvas passes 1 (1.00000012 on the CPU oracle, oracle/pipeline.py with
onnx_exec at float16 on chain_frame(70, 90) and (40, 52): cunet x2 7314 / 39033 and 1993 / 13061 canvas samples <= 0 / >= 1, swin_unet x2 9440 / 14243 and
2937 / 5143), so the clamp in front of the hand-off has something to do.  The unquantised checks first assert that the float frame reaches both ends.
Frames: ragged, 70 x 90 - several tiles in stage 1 and, in stage 2 (140 x 180), a grid with seams on every side: a cunet tile of 64 keeps 28 source pixels."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import synth_models as sm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W2X = os.path.join(ROOT, "waifu2x-tensorrt_amd", "w2x")

HEAD_GAIN = 4.0
TILE, BATCH, BLEND = 64, 2, (0.0625, 0.0625)
# name -> (model, scale, precision, RenderConfig extras)
CONFIGS = {
    "cunet": ("cunet/art", 2, None, dict(overlap=BLEND)),
    "cunet_copy": ("cunet/art", 2, None, dict(overlap=BLEND)),
    "cunet_tta": ("cunet/art", 2, None, dict(overlap=BLEND, tta=True)),
    "cunet_noblend": ("cunet/art", 2, None, dict(overlap=(0.0, 0.0))),
    "cunet_tf32": ("cunet/art", 2, "TF32", dict(overlap=BLEND)),
    "swin2": ("swin_unet/art", 2, None, dict(overlap=BLEND)),
    "swin4": ("swin_unet/art", 4, None, dict(overlap=BLEND)),
}


def contrast_model(model, scale):
    net = sm.make_model(model, scale, seed=1235, small=model.startswith("swin"))
    with torch.no_grad():
        if model.startswith("cunet"):
            for u in (net.unet1, net.unet2):
                u.conv_bottom.weight.mul_(HEAD_GAIN)
        else:
            net.to_image.proj.weight.mul_(HEAD_GAIN)
    return net


@pytest.fixture(scope="module")
def engines(pkg, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("w2x_chain_models"))
    paths, built, made = {}, set(), {}

    def get(name):
        if name not in made:
            model, scale, precision, kw = CONFIGS[name]
            if (model, scale) not in paths:
                paths[model, scale] = sm.export_onnx(contrast_model(model, scale), sm.model_path(root, model, scale, 1), BATCH, TILE)
            path = paths[model, scale]
            prec = pkg.Precision.FP16 if precision is None else getattr(pkg.Precision, precision)
            eng = pkg.Img2Img()
            if (path, prec) not in built:
                assert eng.build(path, pkg.BuildConfig.fixed(BATCH, TILE, precision=prec)), eng.last_error()
                built.add((path, prec))
            assert eng.load(path, pkg.RenderConfig(precision=prec, batchSize=BATCH, height=TILE, width=TILE, scaling=scale, **kw)), eng.last_error()
            made[name] = eng
        return made[name]
    yield get
    for eng in made.values():
        eng.close()


def chain_frame(rows, cols, seed, dtype=np.uint8):
    """noise with a pure black and a pure white block of at least 24 x 24 pixels"""
    top = np.iinfo(dtype).max
    f = np.random.default_rng(seed).integers(0, top + 1, (rows, cols, 3), dtype=dtype)
    f[4:32, 6:36] = 0
    f[rows - 34:rows - 6, cols - 40:cols - 8] = top
    return f


def planes_of(bgr):
    return tuple(np.ascontiguousarray(bgr[..., k]) for k in (2, 1, 0))


def bgr_of(planes):
    return np.ascontiguousarray(np.stack([planes[2], planes[1], planes[0]], axis=-1))


def same(tag, got, want):
    if isinstance(got, tuple):
        assert len(got) == len(want) == 3, tag
        for k in range(3):
            same(f"{tag} plane {k}", got[k], want[k])
        return
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    bad = got != want
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {bad.size} samples differ, first at {tuple(np.argwhere(bad)[0])}"


_MID = {}


def float_mid(get, name, rows, cols, seed, dtype=np.uint8):
    """the float frame between the two single calls, computed once per (engine, frame) and left unchanged; asserted to reach exactly 0.0 and exactly 1.0"""
    key = (name, rows, cols, seed, np.dtype(dtype).name)
    if key not in _MID:
        mid = get(name).render_planar(planes_of(chain_frame(rows, cols, seed, dtype)), out_bits=32)
        lo, hi = min(float(p.min()) for p in mid), max(float(p.max()) for p in mid)
        print(f"float frame behind {name} {rows}x{cols}: min {lo!r} max {hi!r}, {sum(int((p == 0).sum()) for p in mid)} samples at 0, {sum(int((p == 1).sum()) for p in mid)} at 1")
        assert lo == 0.0 and hi == 1.0, (name, lo, hi)
        for p in mid:
            p.setflags(write=False)
        _MID[key] = mid
    return _MID[key]


# ---- 1. unquantised, planar: the chain is the two single calls through a float frame
@pytest.mark.parametrize("first,second,out_bits", [
    ("cunet", "cunet_copy", 8), ("cunet", "cunet_copy", 16), ("cunet", "cunet_copy", 32), ("swin2", "cunet", 8), ("swin2", "cunet", 32),
    ("cunet", "cunet_tta", 8), ("cunet", "cunet_noblend", 8), ("cunet_noblend", "cunet", 16), ("cunet", "cunet_tf32", 32), ("cunet", "cunet_tf32", 8),
    ("cunet_tf32", "cunet", 8)])
def test_planar_chain_is_the_float_route(pkg, engines, first, second, out_bits):
    a, b = engines(first), engines(second)
    src = planes_of(chain_frame(70, 90, 7))
    mid = float_mid(engines, first, 70, 90, 7)
    want = b.render_planar(mid, out_bits=out_bits)
    got = pkg.render_chained_planar([a, b], src, out_bits=out_bits)
    assert got[0].shape == (280, 360)
    same(f"{first} . {second} -> {out_bits} bits", got, want)


# ---- 2. unquantised, interleaved: the planes of (1) interleaved as BGR
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_interleaved_chain_is_the_planar_one(pkg, engines, dtype):
    a, b = engines("cunet"), engines("cunet_copy")
    f = chain_frame(70, 90, 7, dtype)
    bits = 8 * np.dtype(dtype).itemsize
    want = bgr_of(b.render_planar(float_mid(engines, "cunet", 70, 90, 7, dtype), out_bits=bits))
    same(f"interleaved {bits} bits", pkg.render_chained([a, b], f), want)
    same(f"interleaved {bits} bits / planar chain", pkg.render_chained([a, b], f), bgr_of(pkg.render_chained_planar([a, b], planes_of(f))))


def test_interleaved_chain_in_pipelined_parts(pkg, engines):
    """a larger frame: more of render()'s pipelined parts in the last stage of a plain interleaved call (a frame of 16 tiles and more runs in parts)"""
    a, b = engines("cunet"), engines("cunet_copy")
    f = chain_frame(100, 130, 11)
    want = bgr_of(b.render_planar(float_mid(engines, "cunet", 100, 130, 11), out_bits=8))
    same("pipelined last stage", pkg.render_chained([a, b], f), want)
    same("pipelined last stage, quantised", pkg.render_chained([a, b], f, quantize=True), b.render(a.render(f)))


# ---- 3. quantised: the bytes of the single calls one after the other
@pytest.mark.parametrize("first,second,dtype,rows,cols", [("cunet", "cunet_copy", np.uint8, 70, 90), ("cunet", "cunet_copy", np.uint16, 70, 90), ("swin4", "cunet", np.uint8, 40, 52)])
def test_quantised_chain_is_two_calls(pkg, engines, first, second, dtype, rows, cols):
    a, b = engines(first), engines(second)
    f = chain_frame(rows, cols, 7, dtype)
    got = pkg.render_chained([a, b], f, quantize=True)
    same(f"quantised {first} . {second}", got, b.render(a.render(f)))
    assert (got != pkg.render_chained([a, b], f)).any(), "quantize changes nothing"
    planes = planes_of(f)
    same("quantised planar", pkg.render_chained_planar([a, b], planes, quantize=True), b.render_planar(a.render_planar(planes)))


# ---- 4. the same engine twice
def test_the_same_engine_twice(pkg, engines):
    b, c = engines("cunet"), engines("cunet_copy")
    f = chain_frame(70, 90, 7)
    same("[b, b]", pkg.render_chained([b, b], f), pkg.render_chained([b, c], f))
    same("[b, b] quantised", pkg.render_chained([b, b], f, quantize=True), pkg.render_chained([b, c], f, quantize=True))
    same("[b, b] against the float route", pkg.render_chained_planar([b, b], planes_of(f)), b.render_planar(float_mid(engines, "cunet", 70, 90, 7), out_bits=8))


# ---- 5. three stages
def test_three_stages(pkg, engines):
    a, b, c = engines("cunet"), engines("swin2"), engines("cunet_copy")
    src = planes_of(chain_frame(40, 52, 7))
    mid = float_mid(engines, "cunet", 40, 52, 7)
    want = c.render_planar(b.render_planar(mid, out_bits=32), out_bits=8)
    got = pkg.render_chained_planar([a, b, c], src)
    assert got[0].shape == (320, 416)
    same("x8 from three x2 models", got, want)
    same("x8, one engine three times", pkg.render_chained_planar([a, a, a], src), a.render_planar(a.render_planar(mid, out_bits=32), out_bits=8))


# ---- 6. resized
@pytest.mark.parametrize("filter", ["bicubic", "bilinear"])
def test_resized_chain(pkg, engines, filter):
    a, b = engines("cunet"), engines("cunet_copy")
    f = chain_frame(70, 90, 7)
    mid = float_mid(engines, "cunet", 70, 90, 7)
    for target in ((210, 270), (157, 202), (280, 200), (141, 359)):           # x3, x2.25, two anisotropic ones
        want = bgr_of(b.render_planar_resized(mid, target, out_bits=8, filter=filter))
        same(f"resized to {target} {filter}", pkg.render_chained_resized([a, b], f, target, filter=filter), want)
        same(f"planar resized to {target} {filter}", pkg.render_chained_planar([a, b], planes_of(f), target, out_bits=16, filter=filter),
             b.render_planar_resized(mid, target, out_bits=16, filter=filter))
    same("the full size is the plain call", pkg.render_chained_resized([a, b], f, (280, 360), filter=filter), pkg.render_chained([a, b], f))


@pytest.mark.parametrize("filter", ["bicubic", "bilinear"])
def test_resized_chain_below_the_second_stage_frame(pkg, engines, filter):
    """Targets the single call refuses: x1 (70 x 90 from a second stage that reads 140 x 180) and one axis below.  The reference is the production resize of
    the second stage's canvas (resize_planes).  That canvas is only to be had clamped, as the float output of render_planar - so the second engine blends
    nothing here: without blend sums its canvas is the network's output, which the graph itself clips to [0, 1], and the clamp is the identity."""
    a, b = engines("cunet"), engines("cunet_noblend")
    f = chain_frame(70, 90, 7)
    canvas = b.render_planar(float_mid(engines, "cunet", 70, 90, 7), out_bits=32)
    for target in ((70, 90), (100, 300), (280, 95)):
        want = bgr_of(b.resize_planes(canvas, target, 8, filter=filter))
        same(f"resized to {target} {filter}", pkg.render_chained_resized([a, b], f, target, filter=filter), want)


def test_resized_chain_takes_the_last_engines_settings(pkg, engines):
    a, b = engines("cunet"), engines("cunet_copy")
    f = chain_frame(70, 90, 7)
    mid = float_mid(engines, "cunet", 70, 90, 7)
    plain = pkg.render_chained_resized([a, b], f, (157, 202))
    plain_q = pkg.render_chained([a, b], f, quantize=True)
    try:
        assert b.set_dither("ordered") and b.set_resize_light("srgb")
        want = bgr_of(b.render_planar_resized(mid, (157, 202), out_bits=8))
        got = pkg.render_chained_resized([a, b], f, (157, 202))
        same("dither and light of the last engine", got, want)
        assert (got != plain).any()
        assert a.set_dither("bluenoise") and a.set_resize_light("bt709")
        same("the first engine's settings do not count", pkg.render_chained_resized([a, b], f, (157, 202)), want)
        assert b.set_dither("none") and b.set_resize_light("gamma")
        same("undithered again, the first engine still dithering", pkg.render_chained_resized([a, b], f, (157, 202)), plain)
        same("a quantised frame between the stages is not dithered either", pkg.render_chained([a, b], f, quantize=True), plain_q)
    finally:
        for e in (a, b):
            e.set_dither("none")
            e.set_resize_light("gamma")


# ---- 7. sequences and progress
def test_sequence_outputs_are_the_single_calls(pkg, engines):
    a, b = engines("cunet"), engines("cunet_copy")
    frames = [a.alloc_host((70, 90, 3)) for _ in range(3)]
    try:
        for i, buf in enumerate(frames):
            buf[...] = chain_frame(70, 90, 20 + i)
        singles = [pkg.render_chained([a, b], np.array(fr)) for fr in frames]
        for i, out in enumerate(pkg.render_sequence_chained([a, b], frames, pinned=True)):
            same(f"sequence frame {i}", out, singles[i])
        for i, out in enumerate(pkg.render_sequence_chained([a, b], frames, quantize=True)):
            same(f"quantised sequence frame {i}", out, b.render(a.render(np.array(frames[i]))))
        resized = [pkg.render_chained_resized([a, b], np.array(fr), (157, 202)) for fr in frames]
        for i, out in enumerate(pkg.render_sequence_chained([a, b], frames, size=(157, 202), pinned=True)):
            same(f"resized sequence frame {i}", out, resized[i])
        for i, out in enumerate(pkg.render_sequence_chained([b, b], frames)):
            same(f"sequence through one engine twice, frame {i}", out, singles[i])
    finally:
        for buf in frames:
            a.free_host(buf)


def batches(pkg, eng, rows, cols, scale, tta=False):
    n = pkg.calculate_tiles(cols, rows, cols * scale, rows * scale, TILE, eng.output_tile_size, scale, BLEND)[0]
    return math.ceil(n * (8 if tta else 1) / BATCH)


def test_progress_counts_the_batches_of_every_stage(pkg, engines):
    a, b = engines("cunet"), engines("cunet_tta")
    seen, other = [], []
    a.setProgressCallback(lambda cur, total, rate: seen.append((cur, total)))
    b.setProgressCallback(lambda cur, total, rate: other.append((cur, total)))
    try:
        pkg.render_chained([a, b], chain_frame(70, 90, 7))
        total = batches(pkg, a, 70, 90, 2) + batches(pkg, b, 140, 180, 2, tta=True)
        assert [c for c, _ in seen] == list(range(1, total + 1)) and {t for _, t in seen} == {total}
        assert not other, "the callback of engines[0] alone hears of the chain"
        del seen[:]
        pkg.render_sequence_chained([a, b], [chain_frame(70, 90, 7)] * 2)
        assert not seen and not other, "sequences report nothing"
    finally:
        a.setProgressCallback(None)
        b.setProgressCallback(None)


# ---- 8. refusals: False with a message, nothing written, and the next valid call is right
def test_refusals(pkg, engines):
    a, b = engines("cunet"), engines("cunet_copy")
    f = chain_frame(70, 90, 7)
    want = pkg.render_chained([a, b], f)
    L = pkg.lib()
    import ctypes as C

    def refused(call, text):
        n = len(a.messages)
        dst = np.full((280, 360, 3), 0x5A, np.uint8)
        assert call(dst) in (False, 0)
        assert any(text in m for _, m in a.messages[n:]), (text, a.messages[n:])
        assert (dst == 0x5A).all(), "a refused call wrote"

    handles = lambda es: (C.c_void_p * len(es))(*[e._h for e in es])
    raw = lambda es, count, dst: L.w2x_render_chained(handles(es), count, f.ctypes.data, 70, 90, f.strides[0], dst.ctypes.data, dst.strides[0], 8, 0)
    refused(lambda d: raw([a], 1, d), "2 to 4 stages")
    refused(lambda d: raw([a, b, a, b, a], 5, d), "2 to 4 stages")
    fresh = pkg.Img2Img()
    refused(lambda d: raw([a, fresh], 2, d), "before a successful load (engine 1)")
    fresh.close()
    refused(lambda d: pkg.render_chained([a, b], f, dst=d[:279]), "invalid size")
    refused(lambda d: pkg.render_chained_resized([a, b], f, (69, 360), dst=np.ascontiguousarray(d[:69])), "invalid size")
    refused(lambda d: L.w2x_render_chained(handles([a, b]), 2, f.ctypes.data, 70, 90, 90 * 3 - 1, d.ctypes.data, d.strides[0], 8, 0), "invalid step")
    refused(lambda d: L.w2x_render_chained(handles([a, b]), 2, f.ctypes.data, 70, 90, f.strides[0], d.ctypes.data, d.strides[0], 12, 0), "8-bit or both 16-bit")
    refused(lambda d: L.w2x_render_chained_resized(handles([a, b]), 2, f.ctypes.data, 70, 90, f.strides[0], d.ctypes.data, 280, 360, d.strides[0], 8, 0, 7), "Unknown resize filter")
    fl = tuple(p.astype(np.float32) / 255 for p in planes_of(f))
    n = len(a.messages)
    with pytest.raises(pkg.W2xError):
        pkg.render_chained_planar([a, b], fl, quantize=True)
    assert any("integer samples" in m for _, m in a.messages[n:])
    with pytest.raises(pkg.W2xError):                                 # four x2 stages to the source size: the last canvas would shrink by 16
        pkg.render_chained_resized([a, b, a, b], f, (70, 90))
    assert "shrink by a factor of 4" in a.last_error()
    assert L.w2x_render_chained(None, 2, f.ctypes.data, 70, 90, f.strides[0], want.ctypes.data, want.strides[0], 8, 0) == 0
    assert L.w2x_render_chained((C.c_void_p * 2)(a._h, None), 2, f.ctypes.data, 70, 90, f.strides[0], want.ctypes.data, want.strides[0], 8, 0) == 0
    same("a valid call after the refusals", pkg.render_chained([a, b], f), want)
    same("and a single render", a.render(f), bgr_of(a.render_planar(planes_of(f))))


# ---- 9. the command line: --chain on a still, against the library
def test_cli_chain_still(pkg, tmp_path):
    """w2x build --chain 2 builds both stages' engine files; render --chain 2 is render_chained() of the stages the options name (the model at --noise, then the
    scale-only model), --outsize render_chained_resized(), --chain-quantize the quantised chain.  Stills travel as PPM in and through `w2x convert` back: no
    image library is needed."""
    paths = {}
    for noise in (1, -1):
        paths[noise] = sm.export_onnx(contrast_model("cunet/art", 2), sm.model_path(str(tmp_path), "cunet/art", 2, noise), BATCH, TILE, dynamic=True)
    common = ["--models", str(tmp_path / "models"), "--model", "cunet/art", "--scale", "2", "--noise", "1", "--batchSize", str(BATCH), "--tileSize", str(TILE), "--blend", "1/16"]
    r = subprocess.run([W2X, *common, "build", "--chain", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for noise in (1, -1):
        stem = os.path.splitext(os.path.basename(paths[noise]))[0]
        assert any(n.startswith(stem + "_") and n.endswith(".w2x") for n in os.listdir(os.path.dirname(paths[noise]))), (noise, os.listdir(os.path.dirname(paths[noise])))
    stages = []
    for noise in (1, -1):
        eng = pkg.Img2Img()
        assert eng.load(paths[noise], pkg.RenderConfig(batchSize=BATCH, height=TILE, width=TILE, scaling=2, overlap=BLEND)), eng.last_error()
        stages.append(eng)
    f = chain_frame(70, 90, 7)
    (tmp_path / "in.ppm").write_bytes(b"P6\n90 70\n255\n" + np.ascontiguousarray(f[..., ::-1]).tobytes())

    def run(tag, *extra):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "in.ppm"), "-o", str(out), "--chain", "2", *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        files = sorted(os.listdir(out))
        assert len(files) == 1 and "(chain2)" in files[0] and files[0].endswith(".png"), files
        ppm = tmp_path / (tag + ".ppm")
        r = subprocess.run([W2X, "convert", "-i", str(out / files[0]), "-o", str(ppm)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        raw = ppm.read_bytes()
        head = raw.split(b"\n", 3)
        assert head[0] == b"P6" and head[2] == b"255", head[:3]
        w, h = (int(v) for v in head[1].split())
        return np.ascontiguousarray(np.frombuffer(head[3], np.uint8).reshape(h, w, 3)[..., ::-1])
    try:
        same("w2x render --chain 2", run("plain"), pkg.render_chained(stages, f))
        same("w2x render --chain 2 --chain-quantize", run("quantised", "--chain-quantize"), pkg.render_chained(stages, f, quantize=True))
        same("w2x render --chain 2 --outsize", run("sized", "--outsize", "202x157"), pkg.render_chained_resized(stages, f, (157, 202)))
    finally:
        for eng in stages:
            eng.close()
