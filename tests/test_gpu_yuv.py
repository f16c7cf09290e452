"""YUV 4:2:0 frames on the GPU (Img2Img::renderYuv / renderSequenceYuv): gather_yuv_kernel converts the planes to RGB as it reads the
tiles, compose_yuv_kernel writes the canvas back as Y, U and V planes at 8 or 10 bits.

The reference: yuv_ref.decode's float RGB frame fed to pipeline.render with the engine's own network (eng.infer), its canvas captured (render()
looks to_u16 up by module name) and encoded by yuv_ref.encode.  pipeline.blob_from_tiles scales non-u8 tiles by 1/65535, so the test wraps it to
pass float tiles through unscaled.  The device converts in fp32 (the oracle in float64, rounded to fp32 / fp16 at the network's edge), so a code
may land on the other side of a rounding tie, and an fp16 engine's network sees inputs that differ from the oracle's by an fp16 rounding here and
there: at most 1 code everywhere, and per case at least a floor set below the fraction measured (profiles/yuv/gpu_yuv_exact.txt) exactly equal.
10-bit codes are four times finer than 8-bit ones, so the fp16 network's own rounding shows in more of them."""
import numpy as np
import pytest

import yuv_ref
from oracle import pipeline
from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu


def oracle_yuv(eng, planes, monkeypatch, *, matrix, full_range, in_bits, out_bits, batch, tile, scale, ov, tta=False, fp16=True):
    """(Y, U, V) the reference gives for this frame"""
    rgb = yuv_ref.decode(*planes, matrix=matrix, full_range=full_range, bits=in_bits)
    seen = {}
    orig_blob, orig_u16 = pipeline.blob_from_tiles, pipeline.to_u16

    def blob(tiles):
        a = np.stack(tiles)
        if a.dtype == np.float32:
            return np.ascontiguousarray(a.transpose(0, 3, 1, 2))
        return orig_blob(tiles)

    def capture(canvas):
        seen["canvas"] = canvas.copy()
        return orig_u16(canvas)
    monkeypatch.setattr(pipeline, "blob_from_tiles", blob)
    monkeypatch.setattr(pipeline, "to_u16", capture)
    pipeline.render(np.ascontiguousarray(rgb[..., ::-1].astype(np.float32)), eng.infer, batch=batch, tile=tile, scaling=scale, overlap=(ov, ov), tta=tta,
                    net_dtype=np.float16 if fp16 else None, tile_out=eng.output_tile_size)
    monkeypatch.undo()
    return yuv_ref.encode(seen["canvas"], matrix=matrix, full_range=full_range, bits=out_bits)


def pkg_error():
    import importlib
    return int(importlib.import_module("waifu2x-tensorrt_amd").Severity.error)


def assert_close(tag, out, ref, min_exact):
    worst = 1.0
    for name, a, b in zip("YUV", out, ref):
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, name, a.shape, b.shape, a.dtype, b.dtype)
        d = np.abs(a.astype(np.int64) - b.astype(np.int64))
        exact = float((d == 0).mean())
        worst = min(worst, exact)
        print(f"{tag} {name}: max {int(d.max())} codes, exact {exact:.6f} of {d.size}")
        assert d.max() <= 1 and exact >= min_exact, f"{tag} {name}: max {int(d.max())} codes, exact {exact:.6f}"
    return worst


@pytest.fixture(scope="module")
def swin(pkg, onnx_model):
    path = onnx_model("swin_unet/art", 4, 2, 64, small=True)
    eng = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625))
    yield eng
    eng.close()


@pytest.mark.parametrize("rows,cols", [(70, 102), (45, 67)])
def test_swin_x4_bt709_limited_against_the_reference(swin, monkeypatch, rows, cols):
    """swin_unet x4, blend 1/16, 8-bit limited BT.709 on a ragged even frame and an odd-sized one (noise and a smooth picture)"""
    for k, planes in enumerate((yuv_ref.random_planes(rows, cols, 8, 11), yuv_ref.smooth_planes(rows, cols, 8, 12))):
        ref = oracle_yuv(swin, planes, monkeypatch, matrix="bt709", full_range=False, in_bits=8, out_bits=8, batch=2, tile=64, scale=4, ov=0.0625)
        out = swin.render_yuv(*planes, matrix="bt709")
        assert [p.shape for p in out] == yuv_ref.plane_shapes(4 * rows, 4 * cols)
        assert_close(f"swin {rows}x{cols} frame{k}", out, ref, 0.97)


def test_eight_bit_in_ten_bit_out(swin, monkeypatch):
    """an 8-bit source rendered to a 10-bit output (BT.601, limited)"""
    planes = yuv_ref.smooth_planes(52, 76, 8, 21, matrix="bt601")
    ref = oracle_yuv(swin, planes, monkeypatch, matrix="bt601", full_range=False, in_bits=8, out_bits=10, batch=2, tile=64, scale=4, ov=0.0625)
    out = swin.render_yuv(*planes, matrix="bt601", out_bits=10)
    assert out[0].dtype == np.uint16 and int(out[0].max()) <= 1023
    assert_close("8 -> 10 bits", out, ref, 0.9)


def test_cunet_tta_bt2020_full_range_ten_bit(pkg, onnx_model, monkeypatch):
    """cunet x2 with TTA, 10-bit full-range BT.2020 in and out"""
    path = onnx_model("cunet/art", 2, 2, 64)
    eng = make_engine(pkg, path, 2, 64, 2, overlap=(0.0, 0.0), tta=True)
    for k, planes in enumerate((yuv_ref.random_planes(61, 83, 10, 31, full_range=True), yuv_ref.smooth_planes(61, 83, 10, 32, "bt2020", True))):
        ref = oracle_yuv(eng, planes, monkeypatch, matrix="bt2020", full_range=True, in_bits=10, out_bits=10, batch=2, tile=64, scale=2, ov=0.0, tta=True)
        out = eng.render_yuv(*planes, matrix="bt2020", full_range=True)
        assert_close(f"cunet tta bt2020 pc frame{k}", out, ref, 0.99)
    eng.close()


def test_fp32_engine(pkg, onnx_model, monkeypatch):
    """the fp32-storage engine (Precision.FP32): the float4v tiles of both kernels"""
    path = onnx_model("cunet/art", 2, 1, 64)
    eng = pkg.Img2Img()
    assert eng.build(path, pkg.BuildConfig.fixed(1, 64, precision=pkg.Precision.FP32)), eng.last_error()
    assert eng.load(path, pkg.RenderConfig(precision=pkg.Precision.FP32, batchSize=1, height=64, width=64, scaling=2, overlap=(0.0625, 0.0625))), eng.last_error()
    planes = yuv_ref.smooth_planes(57, 70, 8, 41)
    ref = oracle_yuv(eng, planes, monkeypatch, matrix="bt709", full_range=False, in_bits=8, out_bits=8, batch=1, tile=64, scale=2, ov=0.0625, fp16=False)
    assert_close("fp32 engine", eng.render_yuv(*planes), ref, 0.999)
    eng.close()


def test_wide_frames_cross_the_wave_seam(swin, pkg, onnx_model, monkeypatch):
    """outputs wider than one wave's 512 luma columns: lane 0 of the second wave computes the column left of its run from the tiles instead of
    taking it from a neighbouring lane.  swin x4 on 150 x 141 (564 columns out), and cunet x1 on an odd 541-column frame"""
    planes = yuv_ref.smooth_planes(150, 141, 8, 71)
    ref = oracle_yuv(swin, planes, monkeypatch, matrix="bt709", full_range=False, in_bits=8, out_bits=8, batch=2, tile=64, scale=4, ov=0.0625)
    assert_close("swin 150x141 -> 600x564", swin.render_yuv(*planes), ref, 0.97)
    path = onnx_model("cunet/art", 1, 2, 64)
    eng = make_engine(pkg, path, 2, 64, 1, overlap=(0.0625, 0.0625))
    for k, planes in enumerate((yuv_ref.smooth_planes(37, 541, 10, 72, "bt601"), yuv_ref.random_planes(37, 541, 10, 73))):
        ref = oracle_yuv(eng, planes, monkeypatch, matrix="bt601", full_range=False, in_bits=10, out_bits=8, batch=2, tile=64, scale=1, ov=0.0625)
        assert_close(f"cunet x1 37x541 frame{k}", eng.render_yuv(*planes, matrix="bt601", out_bits=8), ref, 0.97)
    eng.close()


@pytest.mark.parametrize("pinned", [False, True])
def test_rolling_sequence_matches_single_frames(pkg, onnx_model, monkeypatch, pinned):
    """renderSequenceYuv over frames that roll: with TTA a 90 x 130 frame on swin x4 (6 tiles) fills 48 slots of its one pass, so every pass splits
    into two tile groups and frame f is composed on the second group's stream while frame f + 1 runs (run_rolling_frame, two slabs).  The frames
    must be byte-identical to per-frame renderYuv, to the same sequence with W2X_NO_ROLLING=1, and on a repeated call; pageable or page-locked
    outputs; plane steps wider than the rows (an AVFrame's linesize) give the same bytes"""
    path = onnx_model("swin_unet/art", 4, 2, 64, small=True)
    frames = [yuv_ref.random_planes(90, 130, 10, 50 + k) for k in range(5)]
    monkeypatch.setenv("W2X_NO_ROLLING", "1")
    plain = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625), tta=True)
    unrolled = plain.render_sequence_yuv(frames, out_bits=10, pinned=pinned)
    plain.close()
    monkeypatch.delenv("W2X_NO_ROLLING")
    eng = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625), tta=True)
    want = [eng.render_yuv(*f, out_bits=10) for f in frames]
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    assert all(same(a, b) for a, b in zip(unrolled, want))
    for attempt in range(2):
        got = eng.render_sequence_yuv(frames, out_bits=10, pinned=pinned)
        for k, (a, b) in enumerate(zip(got, want)):
            assert same(a, b), (attempt, k)
    wide = [tuple(np.pad(p, ((0, 0), (0, 24)))[:, :p.shape[1]] for p in f) for f in frames[:3]]
    assert all(same(a, b) for a, b in zip(eng.render_sequence_yuv(wide, out_bits=10), want))
    assert same(eng.render_yuv(*frames[1], out_bits=10), want[1])
    eng.close()


def test_refused_calls(swin):
    """each invalid call returns False with a message and launches nothing; a valid call after them still succeeds"""
    y, u, v = yuv_ref.random_planes(40, 50, 8, 61)
    want = swin.render_yuv(y, u, v)
    L, h = swin._L, swin._h
    import ctypes as C

    def call(planes=(y, u, v), steps=None, rows=40, cols=50, bits=8, out=None, orows=160, ocols=200, obits=8, matrix=1, rng=0):
        out = out if out is not None else tuple(np.zeros(s, np.uint8) for s in yuv_ref.plane_shapes(160, 200))
        sp = (C.c_void_p * 3)(*[p.ctypes.data if p is not None else None for p in planes])
        st = (C.c_size_t * 3)(*(steps if steps else [p.strides[0] for p in planes]))
        dp = (C.c_void_p * 3)(*[p.ctypes.data for p in out])
        ds = (C.c_size_t * 3)(*[p.strides[0] for p in out])
        return L.w2x_render_yuv(h, sp, st, rows, cols, bits, dp, ds, orows, ocols, obits, matrix, rng)

    cases = {
        "input bits 9": dict(bits=9), "output bits 16": dict(obits=16), "matrix 3": dict(matrix=3), "matrix -1": dict(matrix=-1), "range 2": dict(rng=2),
        "null U plane": dict(planes=(y, None, v), steps=[50, 25, 25]), "short Y step": dict(steps=[49, 25, 25]), "short V step": dict(steps=[50, 25, 24]),
        "output too small": dict(orows=159), "output 3x": dict(orows=120, ocols=150),
    }
    for name, kw in cases.items():
        before = len(swin.messages)
        assert call(**kw) == 0, name
        new = [m for sev, m in swin.messages[before:] if sev <= pkg_error()]
        assert new, f"{name}: no message"
        print(f"{name}: {new[-1]}")
    got = swin.render_yuv(y, u, v)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(Exception):
        swin.render_yuv(y, u, v, out_bits=12)
    assert all(np.array_equal(a, b) for a, b in zip(swin.render_yuv(y, u, v), want))


FAKE_FFPROBE = """#!/usr/bin/env python3
# stand-in for ffprobe on a raw yuv420p10le clip: width,height,r_frame_rate,nb_read_packets like `-of csv=p=0`
import os, sys
w, h = int(os.environ["FAKE_W"]), int(os.environ["FAKE_H"])
print(f"{w},{h},30/1,{os.path.getsize(sys.argv[-1]) // ((w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)) * 2)}")
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


def test_cli_video_as_yuv_matches_the_library(pkg, tmp_path):
    """`w2x render --colorspace bt2020 --color_range pc --pix_fmt yuv420p10le`: the frames are read and written as raw yuv420p10le (fake ffmpeg /
    ffprobe scripts stand in for the pipes and log their arguments), rendered by renderSequenceYuv, equal to render_yuv's; the writer gets the raw
    input format and the colour tags"""
    import json
    import os
    import subprocess
    import synth_models as sm
    W2X = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "waifu2x-tensorrt_amd", "w2x")
    models = tmp_path / "models"
    path = sm.model_path(str(tmp_path), "swin_unet/art", 4, 3)
    sm.export_onnx(sm.make_model("swin_unet/art", 4, seed=5, small=True), path, 2, 64, dynamic=True)
    W, H, N = 100, 70, 6                                                # 6 frames: a full chunk of 4 and a ragged one
    frames = [yuv_ref.random_planes(H, W, 10, 80 + k, full_range=True) for k in range(N)]
    (tmp_path / "clip.mkv").write_bytes(b"".join(p.tobytes() for f in frames for p in f))
    bindir = tmp_path / "bin"; bindir.mkdir()
    for name, text in (("ffprobe", FAKE_FFPROBE), ("ffmpeg", FAKE_FFMPEG)):
        (bindir / name).write_text(text); (bindir / name).chmod(0o755)
    out = tmp_path / "out"; out.mkdir()
    log = tmp_path / "argv.jsonl"
    common = ["--models", str(models), "--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "2", "--tileSize", "64"]
    env = dict(os.environ, PATH=f"{bindir}:{os.environ['PATH']}", FAKE_W=str(W), FAKE_H=str(H), FAKE_LOG=str(log))
    r = subprocess.run([W2X, *common, "build"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "clip.mkv"), "-o", str(out), "--colorspace", "bt2020", "--color_range", "pc",
                        "--pix_fmt", "yuv420p10le"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = np.frombuffer((out / "clip(swin_unet_art)(noise3)(scale4).mp4").read_bytes(), np.uint16)
    shapes = yuv_ref.plane_shapes(4 * H, 4 * W)
    per = sum(a * b for a, b in shapes)
    assert raw.size == N * per
    eng = pkg.Img2Img()
    assert eng.load(path, pkg.RenderConfig(batchSize=2, height=64, width=64, scaling=4)), eng.last_error()
    for k in range(N):
        want = eng.render_yuv(*frames[k], matrix="bt2020", full_range=True)
        o = k * per
        for p, (a, b) in zip(want, shapes):
            assert np.array_equal(raw[o:o + a * b].reshape(a, b), p), k
            o += a * b
    eng.close()
    calls = [json.loads(line) for line in log.read_text().splitlines()]
    reader = next(c for c in calls if c[c.index("-i") + 1] != "-")
    writer = next(c for c in calls if c[c.index("-i") + 1] == "-")
    assert reader[reader.index("-pix_fmt") + 1] == "yuv420p10le" and reader[reader.index("-f") + 1] == "rawvideo"
    i = writer.index("-i")
    assert writer[writer.index("-f") + 1] == "rawvideo" and writer[writer.index("-pix_fmt") + 1] == "yuv420p10le" and writer.index("-pix_fmt") < i
    assert writer[writer.index("-s") + 1] == f"{4 * W}x{4 * H}"
    tags = {k: writer[writer.index(k) + 1] for k in ("-colorspace", "-color_primaries", "-color_trc", "-color_range")}
    assert tags == {"-colorspace": "bt2020nc", "-color_primaries": "bt2020", "-color_trc": "bt2020-10", "-color_range": "pc"}
    assert writer[writer.index("-pix_fmt", i) + 1] == "yuv420p10le"
