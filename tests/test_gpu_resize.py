"""Resized output on the GPU (Img2Img::renderResized / renderSequenceResized, `w2x render --outscale`): the fp32 canvas render() would quantise,
resized by an antialiased separable filter on the device (compose_canvas_kernel + k_resample.hip), quantised and stored as BGR.

The oracle: pipeline.render with the engine's own network (eng.infer) up to the canvas - captured by wrapping pipeline.to_u8 / to_u16, which
render() looks up by module name - then torch-CPU F.interpolate(antialias=True) in float64, rint(x * 255) saturated, RGB -> BGR.  The device
sums in fp32 with float tap weights, so a sample may land on the other side of a rounding tie: at most 1 LSB, and at least 99.9 % of the samples
exactly equal (the fraction each case reaches is printed).  Small frames and T = 64 keep the file under its share of the GPU suite's time."""
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pipeline
from test_gpu_parity import make_engine, smooth_frame

pytestmark = pytest.mark.gpu


def noisy_frame(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)


def oracle_canvas(eng, frame, monkeypatch, *, batch, tile, scale, ov, tta=False, fp16=True):
    """the fp32 RGB canvas pipeline.render quantises for this frame (HxWx3)"""
    seen = {}
    for name in ("to_u8", "to_u16"):
        orig = getattr(pipeline, name)
        def capture(canvas, _orig=orig):
            seen["canvas"] = canvas.copy()
            return _orig(canvas)
        monkeypatch.setattr(pipeline, name, capture)
    full = pipeline.render(frame, eng.infer, batch=batch, tile=tile, scaling=scale, overlap=(ov, ov), tta=tta,
                           net_dtype=np.float16 if fp16 else None, tile_out=eng.output_tile_size)
    monkeypatch.undo()
    return seen["canvas"], full


def oracle_resized(canvas, size, filt, dtype=np.uint8):
    x = torch.from_numpy(np.ascontiguousarray(canvas, np.float64)).permute(2, 0, 1)[None]
    y = F.interpolate(x, size=tuple(size), mode=filt, antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()
    q = 255.0 if dtype == np.uint8 else 65535.0
    return np.ascontiguousarray(np.clip(np.rint(y * q), 0, q).astype(dtype)[..., ::-1])


def assert_close(tag, out, ref, min_exact=0.999):
    assert out.shape == ref.shape, (tag, out.shape, ref.shape)
    d = np.abs(out.astype(np.int64) - ref.astype(np.int64))
    exact = float((d == 0).mean())
    print(f"{tag}: max {int(d.max())} LSB, exact {exact:.6f} of {d.size} samples")
    assert d.max() <= 1 and exact >= min_exact, f"{tag}: max {int(d.max())} LSB, exact {exact:.6f}"
    return exact


@pytest.fixture(scope="module")
def swin(pkg, onnx_model):
    path = onnx_model("swin_unet/art", 4, 2, 64, small=True)
    eng = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def cunet_tta(pkg, onnx_model):
    path = onnx_model("cunet/art", 2, 2, 64)
    eng = make_engine(pkg, path, 2, 64, 2, overlap=(0.0, 0.0), tta=True)
    yield eng
    eng.close()


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
def test_swin_x4_resized_against_the_oracle(swin, monkeypatch, filt):
    """swin_unet x4 to x3, x2 and a x4 width with a x2.5 height (that axis passed through exactly), on a smooth frame and a noisy ragged one"""
    for k, frame in enumerate((smooth_frame(100, 140, 11), noisy_frame(75, 53, 12))):
        canvas, full = oracle_canvas(swin, frame, monkeypatch, batch=2, tile=64, scale=4, ov=0.0625)
        r, c = frame.shape[:2]
        for size in ((3 * r, 3 * c), (2 * r, 2 * c), (int(round(2.5 * r)), 4 * c)):
            out = swin.render_resized(frame, size, filt)
            assert_close(f"swin x4 {filt} frame{k} -> {size}", out, oracle_resized(canvas, size, filt))
        # the target equal to the scaled size: render()'s bytes
        assert np.array_equal(swin.render_resized(frame, (4 * r, 4 * c), filt), full)
        assert np.array_equal(swin.render(frame), full)


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
def test_cunet_tta_resized_against_the_oracle(cunet_tta, monkeypatch, filt):
    """cunet x2 with TTA and no overlap to x1.5 and to x1 (the input size)"""
    for k, frame in enumerate((smooth_frame(90, 120, 21), noisy_frame(67, 45, 22))):
        canvas, _ = oracle_canvas(cunet_tta, frame, monkeypatch, batch=2, tile=64, scale=2, ov=0.0, tta=True)
        r, c = frame.shape[:2]
        for size in ((int(round(1.5 * r)), int(round(1.5 * c))), (r, c)):
            out = cunet_tta.render_resized(frame, size, filt)
            assert_close(f"cunet x2 tta {filt} frame{k} -> {size}", out, oracle_resized(canvas, size, filt))


def test_sixteen_bit_resized_against_the_oracle(swin, monkeypatch):
    """16-bit frames: the oracle's to_u16 path, within 1 LSB16.  A 16-bit step is 1/257 of an 8-bit one, so the fp32 sums of the device meet more
    rounding ties: about 0.2 % of the samples are 1 LSB16 off (measured 0.997917 exact at 240 x 288)"""
    rng = np.random.default_rng(31)
    frame = (smooth_frame(80, 96, 32).astype(np.uint16) * 257 + rng.integers(0, 257, (80, 96, 3))).astype(np.uint16)
    canvas, full = oracle_canvas(swin, frame, monkeypatch, batch=2, tile=64, scale=4, ov=0.0625)
    for size in ((240, 288), (200, 384)):
        out = swin.render_resized(frame, size)
        assert out.dtype == np.uint16
        assert_close(f"16-bit -> {size}", out, oracle_resized(canvas, size, "bicubic", np.uint16), min_exact=0.99)
    assert np.array_equal(swin.render_resized(frame, (320, 384)), full)


def test_fp32_engine_resized_against_the_oracle(pkg, onnx_model, monkeypatch):
    """the fp32-storage engine (Precision.FP32): the float4v canvas compose"""
    path = onnx_model("cunet/art", 2, 1, 64)
    eng = pkg.Img2Img()
    assert eng.build(path, pkg.BuildConfig.fixed(1, 64, precision=pkg.Precision.FP32)), eng.last_error()
    assert eng.load(path, pkg.RenderConfig(precision=pkg.Precision.FP32, batchSize=1, height=64, width=64, scaling=2, overlap=(0.0625, 0.0625))), eng.last_error()
    frame = smooth_frame(70, 90, 41)
    canvas, _ = oracle_canvas(eng, frame, monkeypatch, batch=1, tile=64, scale=2, ov=0.0625, fp16=False)
    for filt in ("bicubic", "bilinear"):
        assert_close(f"fp32 engine {filt}", eng.render_resized(frame, (105, 135), filt), oracle_resized(canvas, (105, 135), filt))
    eng.close()


def test_resized_sequence_matches_resized_renders(pkg, onnx_model):
    """render_sequence_resized over 6 frames, pageable and alloc_host buffers, equals render_resized frame by frame.  The engine ROLLS (run_rolling_frame,
    both tile slabs in turn): with TTA every tile is 8 slots, so the last pass of a frame carries >= 8 live slots, and batch 2 x the super-batch factor is even
    with the default two tile groups (Impl::can_roll)."""
    path = onnx_model("swin_unet/art", 4, 2, 64, small=True)
    eng = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625), tta=True)
    frames = [smooth_frame(60, 70, 50 + k) for k in range(6)]
    size = (150, 175)
    want = [eng.render_resized(f, size) for f in frames]
    got = eng.render_sequence_resized(frames, size)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), f"pageable frame {k}"
    host = [eng.alloc_host(f.shape) for f in frames]
    for h, f in zip(host, frames):
        h[...] = f
    got = eng.render_sequence_resized(host, size, pinned=True)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), f"page-locked frame {k}"
    ring = [eng.alloc_host((size[0], size[1], 3)) for _ in range(3)]
    eng.render_sequence_resized(host, size, outs=[ring[k % 3] for k in range(6)], filter="bicubic")
    for k in (3, 4, 5):
        assert np.array_equal(ring[k % 3], want[k]), f"ring frame {k}"
    # bilinear, and the scaled size is render_sequence()
    got = eng.render_sequence_resized(frames[:3], size, filter="bilinear")
    for k in range(3):
        assert np.array_equal(got[k], eng.render_resized(frames[k], size, "bilinear")), f"bilinear frame {k}"
    got = eng.render_sequence_resized(frames[:3], (240, 280))
    for k in range(3):
        assert np.array_equal(got[k], eng.render(frames[k])), f"scaled size frame {k}"
    eng.close()


def test_refused_sizes_leave_the_engine_usable(swin):
    frame = smooth_frame(50, 60, 61)
    before = swin.render(frame)
    for size in ((201, 240), (200, 241), (49, 60), (50, 59), (0, 60), (50, 0)):
        swin.messages.clear()
        dst = np.zeros((size[0], size[1], 3), np.uint8)
        assert swin.render_resized(frame, size, dst=dst) is False, size
        assert "invalid size" in swin.last_error(), (size, swin.last_error())
    swin.messages.clear()
    with pytest.raises(pkg_error(swin)):
        swin.render_sequence_resized([frame, frame], (201, 240))
    with pytest.raises(ValueError):
        swin.render_resized(frame, (100, 120), "lanczos")
    assert np.array_equal(swin.render(frame), before)
    assert swin.bench_resident(2) > 0                         # render() frames are still replayed


def pkg_error(eng):
    import importlib
    return importlib.import_module("waifu2x-tensorrt_amd").W2xError


def test_cli_outscale_still_with_alpha_and_video(pkg, tmp_path):
    """`w2x render --outscale`: an RGBA still at x3 is render_resized of the BGR image and of the gray alpha image; a video at x2 (fake ffmpeg /
    ffprobe from test_cli) is render_resized frame by frame."""
    Image = pytest.importorskip("PIL.Image")
    import synth_models as sm
    from test_cli import FAKE_FFMPEG, FAKE_FFPROBE, W2X
    path = sm.model_path(str(tmp_path), "swin_unet/art", 4, 3)
    sm.export_onnx(sm.make_model("swin_unet/art", 4, seed=5, small=True), path, 2, 64, dynamic=True)
    common = ["--models", str(tmp_path / "models"), "--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "2", "--tileSize", "64"]
    bindir = tmp_path / "bin"; bindir.mkdir()
    for name, text in (("ffprobe", FAKE_FFPROBE), ("ffmpeg", FAKE_FFMPEG)):
        (bindir / name).write_text(text); (bindir / name).chmod(0o755)
    W, H, N = 70, 50, 5
    env = dict(os.environ, PATH=f"{bindir}:{os.environ['PATH']}", FAKE_W=str(W), FAKE_H=str(H))
    r = subprocess.run([W2X, *common, "build"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(71)
    rgba = rng.integers(0, 256, (45, 60, 4), dtype=np.uint8)
    rgba[..., :3] = smooth_frame(45, 60, 72)
    Image.fromarray(rgba).save(tmp_path / "a.png")
    frames = np.stack([smooth_frame(H, W, 80 + k) for k in range(N)])
    (tmp_path / "clip.mp4").write_bytes(frames.tobytes())
    out = tmp_path / "out"; out.mkdir()
    r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "a.png"), "-o", str(out), "--outscale", "3"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "clip.mp4"), "-o", str(out), "--outscale", "2", "--resize-filter", "bilinear"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.array(Image.open(out / "a(swin_unet_art)(noise3)(scale4)(outscale3).png"))
    assert got.shape == (135, 180, 4)
    vid = np.frombuffer((out / "clip(swin_unet_art)(noise3)(scale4)(outscale2).mp4").read_bytes(), np.uint8).reshape(N, 2 * H, 2 * W, 3)
    eng = pkg.Img2Img()
    assert eng.load(path, pkg.RenderConfig(batchSize=2, height=64, width=64, scaling=4)), eng.last_error()
    colour = eng.render_resized(np.ascontiguousarray(rgba[..., 2::-1]), (135, 180))
    alpha = eng.render_resized(np.ascontiguousarray(np.repeat(rgba[..., 3:4], 3, axis=2)), (135, 180))
    assert np.array_equal(got[..., :3], colour[..., ::-1]) and np.array_equal(got[..., 3], alpha[..., 1])
    for k in range(N):
        assert np.array_equal(vid[k], eng.render_resized(frames[k], (2 * H, 2 * W), "bilinear")), k
    eng.close()
