"""Resized YUV 4:2:0 output on the GPU (Img2Img::renderYuvResized / renderSequenceYuvResized, `w2x render --colorspace .. --outsize WxH`):
gather_yuv_kernel reads the planes, compose_canvas_kernel leaves the fp32 canvas unclamped, resample_yuv_kernel (k_resample.hip) resizes it and
encodes the result as Y, U and V planes.

The reference is yuv_ref.encode(interpolate_float64(canvas, (R, C), filter, antialias=True)): yuv_ref.decode's float RGB frame through pipeline.render
with the engine's own network (eng.infer), the canvas captured where render() would quantise it (as test_gpu_yuv.oracle_yuv does), torch-CPU
F.interpolate(antialias=True) in float64 (test_gpu_resize.oracle_resized without its quantisation), yuv_ref.encode.  One canvas per frame serves all of
its targets and both filters.

Bounds.  At most 1 code in every plane of every case (the bound of test_gpu_yuv.py and test_gpu_resize.py).  The share of codes exactly equal was
measured once per case on an MI355X against this reference (profiles/yuv_resize/gpu_exact.txt, the worst plane of each case in MEASURED below); a
case's floor is 1 - 2 (1 - measured): the kernels are deterministic, the margin absorbs a toolchain change, and an implementation off by a tap or a
site falls far below it.  (The fp32 engine matched every code, so its floor by that rule is 1.)"""
import ctypes as C
import os
import subprocess
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yuv_ref
from oracle import pipeline
from test_gpu_parity import make_engine, smooth_frame

pytestmark = pytest.mark.gpu

# the worst plane's share of exactly equal codes per case, as measured (profiles/yuv_resize/gpu_exact.txt)
MEASURED = {
    "swin bicubic frame0 50x66 -> 150x198": 0.989461,
    "swin bicubic frame0 50x66 -> 100x132": 0.993106,
    "swin bicubic frame0 50x66 -> 125x264": 0.987818,
    "swin bicubic frame0 50x66 -> 101x133": 0.992705,
    "swin bicubic frame0 50x66 -> 50x66": 0.996364,
    "swin bicubic frame1 45x57 -> 135x171": 0.986831,
    "swin bicubic frame1 45x57 -> 90x114": 0.992008,
    "swin bicubic frame1 45x57 -> 112x228": 0.983983,
    "swin bicubic frame1 45x57 -> 91x115": 0.991018,
    "swin bicubic frame1 45x57 -> 45x57": 0.995322,
    "swin bilinear frame0 50x66 -> 150x198": 0.991515,
    "swin bilinear frame0 50x66 -> 100x132": 0.994848,
    "swin bilinear frame0 50x66 -> 125x264": 0.988576,
    "swin bilinear frame0 50x66 -> 101x133": 0.995012,
    "swin bilinear frame0 50x66 -> 50x66": 0.995152,
    "swin bilinear frame1 45x57 -> 135x171": 0.989907,
    "swin bilinear frame1 45x57 -> 90x114": 0.993177,
    "swin bilinear frame1 45x57 -> 112x228": 0.985785,
    "swin bilinear frame1 45x57 -> 91x115": 0.991591,
    "swin bilinear frame1 45x57 -> 45x57": 0.996881,
    "8 -> 10 bits bicubic -> 156x228": 0.947734,
    "8 -> 10 bits bilinear -> 130x191": 0.962384,
    "cunet tta bt2020 pc bicubic frame0 -> 92x124": 0.994653,
    "cunet tta bt2020 pc bilinear frame0 -> 92x124": 0.996581,
    "cunet tta bt2020 pc bicubic frame1 -> 92x124": 0.995179,
    "cunet tta bt2020 pc bilinear frame1 -> 92x124": 0.995705,
    "fp32 engine bicubic -> 86x105": 1.000000,
    "fp32 engine bilinear -> 86x105": 1.000000,
    "wide bicubic -> 90x530 at 10 bits": 0.960671,
    "wide bicubic -> 81x333 at 8 bits": 0.991288,
    "wide bilinear -> 40x448 at 8 bits": 0.994141,
}


def oracle_canvas(eng, planes, *, matrix, full_range, in_bits, batch, tile, scale, ov, tta=False, fp16=True):
    """the float canvas (H x W x 3, RGB) pipeline.render would quantise for this YUV frame"""
    rgb = yuv_ref.decode(*planes, matrix=matrix, full_range=full_range, bits=in_bits)
    seen = {}
    orig_blob, orig_u16 = pipeline.blob_from_tiles, pipeline.to_u16

    def blob(tiles):                     # float tiles pass unscaled (blob_from_tiles scales non-u8 tiles by 1/65535)
        a = np.stack(tiles)
        if a.dtype == np.float32:
            return np.ascontiguousarray(a.transpose(0, 3, 1, 2))
        return orig_blob(tiles)

    def capture(canvas):
        seen["canvas"] = canvas.copy()
        return orig_u16(canvas)
    with mock.patch.object(pipeline, "blob_from_tiles", blob), mock.patch.object(pipeline, "to_u16", capture):
        pipeline.render(np.ascontiguousarray(rgb[..., ::-1].astype(np.float32)), eng.infer, batch=batch, tile=tile, scaling=scale, overlap=(ov, ov), tta=tta,
                        net_dtype=np.float16 if fp16 else None, tile_out=eng.output_tile_size)
    return seen["canvas"]


def reference(canvas, size, filt, *, matrix, full_range, out_bits):
    x = torch.from_numpy(np.ascontiguousarray(canvas, np.float64)).permute(2, 0, 1)[None]
    y = F.interpolate(x, size=tuple(size), mode=filt, antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()
    return yuv_ref.encode(y, matrix=matrix, full_range=full_range, bits=out_bits)


def compare(tag, out, ref, problems):
    """prints every plane's figures, then notes what misses the bounds (the caller asserts once all of its cases have been printed)"""
    worst = 1.0
    for name, a, b in zip("YUV", out, ref):
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, name, a.shape, b.shape, a.dtype, b.dtype)
        d = np.abs(a.astype(np.int64) - b.astype(np.int64))
        exact = float((d == 0).mean())
        worst = min(worst, exact)
        print(f"{tag} {name}: max {int(d.max())} codes, exact {exact:.6f} of {d.size}")
        if d.max() > 1:
            problems.append(f"{tag} {name}: max {int(d.max())} codes")
    if tag not in MEASURED:
        problems.append(f"{tag}: no measured share on record")
    elif worst < 1.0 - 2.0 * (1.0 - MEASURED[tag]):
        problems.append(f"{tag}: exact {worst:.6f} below the floor {1.0 - 2.0 * (1.0 - MEASURED[tag]):.6f}")


@pytest.fixture(scope="module")
def swin(pkg, onnx_model):
    path = onnx_model("swin_unet/art", 4, 2, 64, small=True)
    eng = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625))
    yield eng
    eng.close()


SWIN = dict(batch=2, tile=64, scale=4, ov=0.0625)
_canvases = {}


def swin_canvas(swin, key, planes, **fmt):
    if key not in _canvases:
        _canvases[key] = oracle_canvas(swin, planes, **fmt, **SWIN)
    return _canvases[key]


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
def test_swin_x4_bt709_against_the_reference(swin, filt):
    """swin_unet x4, blend 1/16, BT.709 limited 8 -> 8 bits on a smooth and a noise frame: x3, x2, x2.5 rows with x4 columns, odd x odd, and x1"""
    problems = []
    for k, planes in enumerate((yuv_ref.smooth_planes(50, 66, 8, 12), yuv_ref.random_planes(45, 57, 8, 11))):
        r, c = planes[0].shape
        canvas = swin_canvas(swin, ("bt709", k), planes, matrix="bt709", full_range=False, in_bits=8)
        for size in ((3 * r, 3 * c), (2 * r, 2 * c), (int(round(2.5 * r)), 4 * c), (2 * r + 1, 2 * c + 1), (r, c)):
            out = swin.render_yuv_resized(*planes, size, matrix="bt709", filter=filt)
            assert [p.shape for p in out] == yuv_ref.plane_shapes(*size) and out[0].dtype == np.uint8
            compare(f"swin {filt} frame{k} {r}x{c} -> {size[0]}x{size[1]}", out, reference(canvas, size, filt, matrix="bt709", full_range=False, out_bits=8), problems)
    assert not problems, "\n".join(problems)


def test_eight_bit_in_ten_bit_out(swin):
    """an 8-bit source to a 10-bit output (BT.601, limited), x3 and an odd width"""
    problems = []
    planes = yuv_ref.smooth_planes(52, 76, 8, 21, matrix="bt601")
    canvas = swin_canvas(swin, ("bt601", 0), planes, matrix="bt601", full_range=False, in_bits=8)
    for size, filt in (((156, 228), "bicubic"), ((130, 191), "bilinear")):
        out = swin.render_yuv_resized(*planes, size, matrix="bt601", out_bits=10, filter=filt)
        assert out[0].dtype == np.uint16 and int(out[0].max()) <= 1023
        compare(f"8 -> 10 bits {filt} -> {size[0]}x{size[1]}", out, reference(canvas, size, filt, matrix="bt601", full_range=False, out_bits=10), problems)
    assert not problems, "\n".join(problems)


def test_cunet_tta_bt2020_full_range_ten_bit(pkg, onnx_model):
    """cunet x2 with TTA and no blend, 10-bit full-range BT.2020 in and out, to x1.5"""
    path = onnx_model("cunet/art", 2, 2, 64)
    eng = make_engine(pkg, path, 2, 64, 2, overlap=(0.0, 0.0), tta=True)
    problems = []
    for k, planes in enumerate((yuv_ref.random_planes(61, 83, 10, 31, full_range=True), yuv_ref.smooth_planes(61, 83, 10, 32, "bt2020", True))):
        canvas = oracle_canvas(eng, planes, matrix="bt2020", full_range=True, in_bits=10, batch=2, tile=64, scale=2, ov=0.0, tta=True)
        for filt in ("bicubic", "bilinear"):
            out = eng.render_yuv_resized(*planes, (92, 124), matrix="bt2020", full_range=True, filter=filt)
            compare(f"cunet tta bt2020 pc {filt} frame{k} -> 92x124", out, reference(canvas, (92, 124), filt, matrix="bt2020", full_range=True, out_bits=10), problems)
    eng.close()
    assert not problems, "\n".join(problems)


def test_fp32_engine(pkg, onnx_model):
    """the fp32-storage engine (Precision.FP32): the float4v tiles of the gather and of the canvas compose"""
    path = onnx_model("cunet/art", 2, 1, 64)
    eng = pkg.Img2Img()
    assert eng.build(path, pkg.BuildConfig.fixed(1, 64, precision=pkg.Precision.FP32)), eng.last_error()
    assert eng.load(path, pkg.RenderConfig(precision=pkg.Precision.FP32, batchSize=1, height=64, width=64, scaling=2, overlap=(0.0625, 0.0625))), eng.last_error()
    planes = yuv_ref.smooth_planes(57, 70, 8, 41)
    canvas = oracle_canvas(eng, planes, matrix="bt709", full_range=False, in_bits=8, batch=1, tile=64, scale=2, ov=0.0625, fp16=False)
    problems = []
    for filt in ("bicubic", "bilinear"):
        out = eng.render_yuv_resized(*planes, (86, 105), filter=filt)
        compare(f"fp32 engine {filt} -> 86x105", out, reference(canvas, (86, 105), filt, matrix="bt709", full_range=False, out_bits=8), problems)
    eng.close()
    assert not problems, "\n".join(problems)


def test_wide_and_ragged_targets_plane_by_plane(swin):
    """targets of many column tiles: 530 columns (more than 512: eight whole tiles of 64 and a ragged one, every seam takes its halo column from the
    tile on its left) at 10 bits, and 333 columns (odd, five tiles and 13 columns: the sample-by-sample stores and the clamped last chroma column)"""
    problems = []
    planes = yuv_ref.smooth_planes(40, 141, 8, 71)
    canvas = swin_canvas(swin, ("wide", 0), planes, matrix="bt709", full_range=False, in_bits=8)
    for size, bits, filt in (((90, 530), 10, "bicubic"), ((81, 333), 8, "bicubic"), ((40, 448), 8, "bilinear")):
        out = swin.render_yuv_resized(*planes, size, out_bits=bits, filter=filt)
        compare(f"wide {filt} -> {size[0]}x{size[1]} at {bits} bits", out, reference(canvas, size, filt, matrix="bt709", full_range=False, out_bits=bits), problems)
    assert not problems, "\n".join(problems)


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def test_the_scaled_size_is_render_yuv(swin):
    planes = yuv_ref.random_planes(45, 57, 8, 11)
    for bits in (8, 10):
        want = swin.render_yuv(*planes, out_bits=bits)
        for filt in ("bicubic", "bilinear"):
            assert same(swin.render_yuv_resized(*planes, (180, 228), out_bits=bits, filter=filt), want), (bits, filt)
    seq = swin.render_sequence_yuv_resized([planes, planes], (180, 228))
    assert same(seq[0], swin.render_yuv(*planes)) and same(seq[1], seq[0])


@pytest.mark.parametrize("pinned", [False, True])
def test_rolling_sequence_matches_single_frames(pkg, onnx_model, monkeypatch, pinned):
    """renderSequenceYuvResized over frames that roll (with TTA a 90 x 130 frame on swin x4 fills 48 slots of its one pass: run_rolling_frame, the canvas
    compose and resample_yuv_kernel on the second group's stream): byte-identical to per-frame render_yuv_resized, to the same sequence with
    W2X_NO_ROLLING=1, on a repeated call, with pageable or page-locked outputs, and with plane steps wider than the rows"""
    path = onnx_model("swin_unet/art", 4, 2, 64, small=True)
    frames = [yuv_ref.random_planes(90, 130, 10, 50 + k) for k in range(5)]
    size = (270, 391)
    monkeypatch.setenv("W2X_NO_ROLLING", "1")
    plain = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625), tta=True)
    unrolled = plain.render_sequence_yuv_resized(frames, size, out_bits=10, pinned=pinned)
    plain.close()
    monkeypatch.delenv("W2X_NO_ROLLING")
    eng = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625), tta=True)
    want = [eng.render_yuv_resized(*f, size, out_bits=10) for f in frames]
    assert all(same(a, b) for a, b in zip(unrolled, want))
    for attempt in range(2):
        got = eng.render_sequence_yuv_resized(frames, size, out_bits=10, pinned=pinned)
        for k, (a, b) in enumerate(zip(got, want)):
            assert same(a, b), (attempt, k)
    wide = [tuple(np.pad(p, ((0, 0), (0, 24)))[:, :p.shape[1]] for p in f) for f in frames[:3]]
    assert all(same(a, b) for a, b in zip(eng.render_sequence_yuv_resized(wide, size, out_bits=10), want))
    bil = eng.render_sequence_yuv_resized(frames[:2], size, out_bits=8, filter="bilinear")
    assert all(same(a, eng.render_yuv_resized(*f, size, out_bits=8, filter="bilinear")) for a, f in zip(bil, frames))
    assert same(eng.render_yuv_resized(*frames[1], size, out_bits=10), want[1])
    eng.close()


def test_refused_calls_leave_the_engine_usable(swin, pkg):
    """each invalid call returns 0 with a message and launches nothing; afterwards every kind of render gives the bytes it gave before"""
    y, u, v = yuv_ref.random_planes(40, 50, 8, 61)
    bgr = smooth_frame(40, 50, 62)
    before = (swin.render_yuv_resized(y, u, v, (100, 150)), swin.render_yuv(y, u, v), swin.render(bgr), swin.render_resized(bgr, (100, 150)))
    L, h = swin._L, swin._h

    def call(planes=(y, u, v), steps=None, rows=40, cols=50, bits=8, orows=100, ocols=150, obits=8, osteps=None, matrix=1, rng=0, filt=0, seq=False):
        out = tuple(np.zeros(s, np.uint16) for s in yuv_ref.plane_shapes(max(orows, 1), max(ocols, 1)))
        sp = (C.c_void_p * 3)(*[p.ctypes.data if p is not None else None for p in planes])
        st = (C.c_size_t * 3)(*(steps if steps else [p.strides[0] for p in planes]))
        dp = (C.c_void_p * 3)(*[p.ctypes.data for p in out])
        ds = (C.c_size_t * 3)(*(osteps if osteps else [p.strides[0] for p in out]))
        if seq:
            return L.w2x_render_sequence_yuv_resized(h, sp, st, rows, cols, bits, dp, ds, orows, ocols, obits, 1, matrix, rng, filt)
        return L.w2x_render_yuv_resized(h, sp, st, rows, cols, bits, dp, ds, orows, ocols, obits, matrix, rng, filt)

    cases = {
        "one row too many": dict(orows=161), "one column too many": dict(ocols=201), "fewer rows than the input": dict(orows=39),
        "fewer columns than the input": dict(ocols=49), "no rows": dict(orows=0), "negative columns": dict(ocols=-4),
        "input bits 9": dict(bits=9), "output bits 16": dict(obits=16), "matrix 3": dict(matrix=3), "matrix -1": dict(matrix=-1), "range 2": dict(rng=2),
        "null U plane": dict(planes=(y, None, v), steps=[50, 25, 25]), "short Y step": dict(steps=[49, 25, 25]), "short V step": dict(steps=[50, 25, 24]),
        "short output step": dict(osteps=[149, 75, 75]), "filter 2": dict(filt=2), "filter -1": dict(filt=-1),
        "sequence: too large": dict(orows=161, seq=True), "sequence: filter 7": dict(filt=7, seq=True),
    }
    for name, kw in cases.items():
        count = len(swin.messages)
        assert call(**kw) == 0, name
        new = [m for sev, m in swin.messages[count:] if sev <= int(pkg.Severity.error)]
        assert new, f"{name}: no message"
        print(f"{name}: {new[-1]}")
    assert call() == 1 and call(seq=True) == 1                       # the helper's valid call is accepted
    dst = tuple(np.zeros(s, np.uint8) for s in yuv_ref.plane_shapes(161, 150))
    assert swin.render_yuv_resized(y, u, v, (161, 150), dst=dst) is False and "invalid size" in swin.last_error()
    with pytest.raises(pkg.W2xError):
        swin.render_yuv_resized(y, u, v, (100, 201))
    with pytest.raises(pkg.W2xError):
        swin.render_sequence_yuv_resized([(y, u, v)] * 2, (39, 150))
    with pytest.raises(ValueError):
        swin.render_yuv_resized(y, u, v, (100, 150), filter="lanczos")
    with pytest.raises(ValueError):                                   # frames of a sequence that differ in size
        swin.render_sequence_yuv_resized([(y, u, v), yuv_ref.random_planes(40, 52, 8, 63)], (100, 150))
    with pytest.raises(Exception):
        swin.render_yuv_resized(y, u, v, (100, 150), out_bits=12)
    # what the plain calls refuse, they still refuse
    assert swin.render_yuv(y, u, v, out=tuple(np.zeros(s, np.uint8) for s in yuv_ref.plane_shapes(160, 200))) is True
    with pytest.raises(ValueError):
        swin.render_yuv(y, u, v, out=tuple(np.zeros(s, np.uint8) for s in yuv_ref.plane_shapes(100, 150)))
    assert swin.render_resized(bgr, (161, 150), dst=np.zeros((161, 150, 3), np.uint8)) is False
    after = (swin.render_yuv_resized(y, u, v, (100, 150)), swin.render_yuv(y, u, v), swin.render(bgr), swin.render_resized(bgr, (100, 150)))
    assert same(after[0], before[0]) and same(after[1], before[1]) and np.array_equal(after[2], before[2]) and np.array_equal(after[3], before[3])


def test_cli_outsize_yuv_video_bgr_video_and_still(pkg, tmp_path):
    """`w2x render --outsize WxH`: with --colorspace a raw yuv420p10le clip (fake ffmpeg / ffprobe log their arguments) is render_yuv_resized frame by
    frame and the writer gets -s WxH, the raw format in front of -i and the colour tags; without it a bgr24 clip and an RGBA still are render_resized"""
    import json
    Image = pytest.importorskip("PIL.Image")
    import synth_models as sm
    from test_cli import FAKE_FFMPEG as BGR_FFMPEG, FAKE_FFPROBE as BGR_FFPROBE, W2X
    from test_gpu_yuv import FAKE_FFMPEG as YUV_FFMPEG, FAKE_FFPROBE as YUV_FFPROBE
    path = sm.model_path(str(tmp_path), "swin_unet/art", 4, 3)
    sm.export_onnx(sm.make_model("swin_unet/art", 4, seed=5, small=True), path, 2, 64, dynamic=True)
    common = ["--models", str(tmp_path / "models"), "--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "2", "--tileSize", "64"]
    W, H, N, OW, OH = 100, 70, 6, 250, 141                              # 6 frames: a full chunk of 4 and a ragged one; x2.5 columns, x2.01 rows (odd)
    envs = {}
    for kind, probe, mpeg in (("yuv", YUV_FFPROBE, YUV_FFMPEG), ("bgr", BGR_FFPROBE, BGR_FFMPEG)):
        bindir = tmp_path / f"bin_{kind}"; bindir.mkdir()
        for name, text in (("ffprobe", probe), ("ffmpeg", mpeg)):
            (bindir / name).write_text(text); (bindir / name).chmod(0o755)
        envs[kind] = dict(os.environ, PATH=f"{bindir}:{os.environ['PATH']}", FAKE_W=str(W), FAKE_H=str(H), FAKE_LOG=str(tmp_path / f"argv_{kind}.jsonl"))
    r = subprocess.run([W2X, *common, "build"], capture_output=True, text=True, env=envs["yuv"], timeout=300)
    assert r.returncode == 0, r.stderr
    out = tmp_path / "out"; out.mkdir()
    yuv_frames = [yuv_ref.random_planes(H, W, 10, 80 + k) for k in range(N)]
    (tmp_path / "clip.mkv").write_bytes(b"".join(p.tobytes() for f in yuv_frames for p in f))
    r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "clip.mkv"), "-o", str(out), "--colorspace", "bt709", "--pix_fmt", "yuv420p10le",
                        "--outsize", f"{OW}x{OH}"], capture_output=True, text=True, env=envs["yuv"], timeout=300)
    assert r.returncode == 0, r.stderr
    bgr_frames = np.stack([smooth_frame(H, W, 90 + k) for k in range(5)])
    (tmp_path / "plain.mp4").write_bytes(bgr_frames.tobytes())
    r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "plain.mp4"), "-o", str(out), "--outsize", f"{OW}x{OH}", "--resize-filter", "bilinear"],
                       capture_output=True, text=True, env=envs["bgr"], timeout=300)
    assert r.returncode == 0, r.stderr
    rgba = np.random.default_rng(71).integers(0, 256, (45, 60, 4), dtype=np.uint8)
    rgba[..., :3] = smooth_frame(45, 60, 72)
    Image.fromarray(rgba).save(tmp_path / "a.png")
    r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "a.png"), "-o", str(out), "--outsize", "151x99"], capture_output=True, text=True, env=envs["bgr"], timeout=300)
    assert r.returncode == 0, r.stderr
    # an input the size cannot be reached from stops the run with its size and the bounds
    r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "a.png"), "-o", str(out), "--outsize", "250x141"], capture_output=True, text=True, env=envs["bgr"], timeout=300)
    assert r.returncode != 0 and "60x45" in r.stderr and "240x180" in r.stderr and "--outsize" in r.stderr, r.stderr

    eng = pkg.Img2Img()
    assert eng.load(path, pkg.RenderConfig(batchSize=2, height=64, width=64, scaling=4)), eng.last_error()
    raw = np.frombuffer((out / f"clip(swin_unet_art)(noise3)(scale4)({OW}x{OH}).mp4").read_bytes(), np.uint16)
    shapes = yuv_ref.plane_shapes(OH, OW)
    per = sum(a * b for a, b in shapes)
    assert raw.size == N * per
    for k in range(N):
        want = eng.render_yuv_resized(*yuv_frames[k], (OH, OW), matrix="bt709")
        o = k * per
        for p, (a, b) in zip(want, shapes):
            assert np.array_equal(raw[o:o + a * b].reshape(a, b), p), k
            o += a * b
    vid = np.frombuffer((out / f"plain(swin_unet_art)(noise3)(scale4)({OW}x{OH}).mp4").read_bytes(), np.uint8).reshape(5, OH, OW, 3)
    for k in range(5):
        assert np.array_equal(vid[k], eng.render_resized(bgr_frames[k], (OH, OW), "bilinear")), k
    got = np.array(Image.open(out / "a(swin_unet_art)(noise3)(scale4)(151x99).png"))
    assert got.shape == (99, 151, 4)
    colour = eng.render_resized(np.ascontiguousarray(rgba[..., 2::-1]), (99, 151))
    alpha = eng.render_resized(np.ascontiguousarray(np.repeat(rgba[..., 3:4], 3, axis=2)), (99, 151))
    assert np.array_equal(got[..., :3], colour[..., ::-1]) and np.array_equal(got[..., 3], alpha[..., 1])
    eng.close()
    calls = [json.loads(line) for line in (tmp_path / "argv_yuv.jsonl").read_text().splitlines()]
    reader = next(c for c in calls if c[c.index("-i") + 1] != "-")
    writer = next(c for c in calls if c[c.index("-i") + 1] == "-")
    assert reader[reader.index("-pix_fmt") + 1] == "yuv420p10le" and reader[reader.index("-f") + 1] == "rawvideo"
    i = writer.index("-i")
    assert writer[writer.index("-f") + 1] == "rawvideo" and writer[writer.index("-pix_fmt") + 1] == "yuv420p10le" and writer.index("-pix_fmt") < i
    assert writer[writer.index("-s") + 1] == f"{OW}x{OH}" and writer.index("-s") < i
    tags = {k: writer[writer.index(k) + 1] for k in ("-colorspace", "-color_primaries", "-color_trc", "-color_range")}
    assert tags == {"-colorspace": "bt709", "-color_primaries": "bt709", "-color_trc": "bt709", "-color_range": "tv"}
