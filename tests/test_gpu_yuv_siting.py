"""YUV chroma siting on the GPU (YuvImage::siting): centre and top-left sited 4:2:0 / 4:2:2 frames in and out, source and destination siting
independent - the sited instantiations of gather_yuv_kernel, compose_yuv_kernel (centre: no left column; top-left: bands of chroma rows with the luma row
above carried in registers) and the resample_yuv kernels (top-left: a row halo above each tile), through w2x_render_yuv_sited / w2x_render_sequence_yuv_sited.

Frames (tests/test_yuv_siting_host.py shows that their sitings can be told apart at 1 code): 45 x 67 - odd both ways, 90 chroma rows of output = 8 bands of 12
and 12 resample tiles of 16 rows at x4 - and 9 x 141, whose 564 output columns make a chroma row span two waves (lane 0 of the second wave computes its left
column, and the carried one, from the tiles).  Noise (yuv_layout_ref.random_planes) and a smooth picture.

1. Byte equalities that need no oracle.
2. The float64 reference of tests/yuv_siting_ref.py: decode by the source siting -> pipeline.render with the engine's own network -> the captured canvas
   (test_gpu_yuv_layouts.oracle_canvas), one oracle run per (frame, source layout, source siting), resized where the case is (torch F.interpolate in float64 as
   in test_gpu_yuv_resize_layouts.py) and encoded to every destination under test.
   Bound, derived as in test_gpu_yuv.py: the device converts in fp32, the reference in float64, so a code may land on the other side of one rounding tie, and
   an fp16 engine's network sees inputs that differ from the oracle's by an fp16 rounding here and there: at most 1 code in every plane.  The floors of the
   exactly equal fraction are the ones the existing tests hold for the same engine and depths at the left siting: 0.97 swin at 8 bits, 0.9 at 8 -> 10 bits,
   0.999 for the fp32 engine.  Every measured fraction is printed ("EXACT ..." lines; profiles/yuv_siting/gpu_exact.txt is this file's output).
   Cross-check: on the noise frame the device's centre / top-left output against the reference for "left" must MISS the bound.
3. Refusals: the engine's own wording for an unknown siting.
4. The command line: `w2x render --colorspace bt2020 --chroma-loc topleft` with the logging stand-ins for ffmpeg / ffprobe of test_gpu_yuv_layouts.py."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yuv_layout_ref as ylr
import yuv_siting_ref as ref
from test_gpu_parity import make_engine
from test_gpu_yuv_layouts import FAKE_FFMPEG, FAKE_FFPROBE, compare, oracle_canvas, pkg_error, same

pytestmark = pytest.mark.gpu

SITINGS = ref.SITINGS
SWIN = dict(batch=2, tile=64, scale=4, ov=0.0625)
FLOOR_8, FLOOR_10, FLOOR_FP32 = 0.97, 0.9, 0.999


@pytest.fixture(scope="module")
def swin(pkg, onnx_model):
    path = onnx_model("swin_unet/art", 4, 2, 64, small=True)
    eng = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625))
    yield eng
    eng.close()


noise, smooth = ref.gpu_noise, ref.gpu_smooth        # the frames tests/test_yuv_siting_host.py checks (yuv_siting_ref.GPU_FRAMES)
FRAMES = sorted(ref.GPU_FRAMES, reverse=True)


# ---- 1. equalities, no oracle
@pytest.mark.parametrize("bits", [8, 10])
def test_left_left_is_the_unsited_call(swin, bits):
    planes = noise(45, 67, bits=bits)
    base = swin.render_yuv(*planes)
    L, h = swin._L, swin._h
    # the new entry itself with both sitings left (the wrapper would not go there): the scaled size, and a resized target
    for size, want in (((180, 268), base), ((150, 198), swin.render_yuv_layout_resized(planes, (150, 198)))):
        out = tuple(np.zeros(s, planes[0].dtype) for s in ylr.plane_shapes(*size, "i420"))
        sp, dp = (C.c_void_p * 3)(*[p.ctypes.data for p in planes]), (C.c_void_p * 3)(*[p.ctypes.data for p in out])
        ss, ds = (C.c_size_t * 3)(*[p.strides[0] for p in planes]), (C.c_size_t * 3)(*[p.strides[0] for p in out])
        assert L.w2x_render_yuv_sited(h, sp, ss, 45, 67, bits, 0, 0, dp, ds, size[0], size[1], bits, 0, 0, 1, 0, 0) == 1, swin.messages[-1:]
        assert same(out, want), size
    assert same(swin.render_yuv(*planes, siting="left", out_siting="left"), base)


def test_layouts_without_the_axis_ignore_the_siting(swin):
    p420, p444, p422 = noise(45, 67), noise(45, 67, "i444"), noise(45, 67, "i422")
    # i444 on a side makes that side's siting irrelevant
    want = swin.render_yuv(p444, layout="i444", out_layout="i420", out_siting="center")
    for s in SITINGS:
        assert same(swin.render_yuv(p444, layout="i444", out_layout="i420", siting=s, out_siting="center"), want), s
    want = swin.render_yuv(p420, layout="i420", out_layout="i444", siting="topleft")
    for s in SITINGS:
        assert same(swin.render_yuv(p420, layout="i420", out_layout="i444", siting="topleft", out_siting=s), want), s
        assert same(swin.render_yuv_layout_resized(p420, (150, 198), out_layout="i444", siting="topleft", out_siting=s),
                    swin.render_yuv_layout_resized(p420, (150, 198), out_layout="i444", siting="topleft", out_siting="left")), s
    # i422: topleft is left, on either side, plain and resized
    assert same(swin.render_yuv(p422, layout="i422", siting="topleft"), swin.render_yuv(p422, layout="i422"))
    assert same(swin.render_yuv(p422, layout="i422", out_layout="i420", siting="topleft", out_siting="center"),
                swin.render_yuv(p422, layout="i422", out_layout="i420", siting="left", out_siting="center"))
    assert same(swin.render_yuv_layout_resized(p420, (150, 198), out_layout="i422", siting="center", out_siting="topleft"),
                swin.render_yuv_layout_resized(p420, (150, 198), out_layout="i422", siting="center", out_siting="left"))
    assert not same(swin.render_yuv(p422, layout="i422", siting="center"), swin.render_yuv(p422, layout="i422"))


@pytest.mark.parametrize("rows,cols", FRAMES)
def test_luma_and_nv12_equalities_per_siting(swin, rows, cols):
    planes = noise(rows, cols)
    nv = ylr.pack_nv12(*planes)
    base = swin.render_yuv(*planes)
    size = (3 * rows + 1, 3 * cols + 1)
    rbase = swin.render_yuv_layout_resized(planes, size)
    for s in SITINGS:
        out = swin.render_yuv(*planes, out_siting=s)
        # the Y plane does not depend on the destination siting or layout
        assert np.array_equal(out[0], base[0]), s
        for lay in ("i422", "i444"):
            assert np.array_equal(swin.render_yuv(planes, layout="i420", out_layout=lay, out_siting=s)[0], base[0]), (s, lay)
        # an NV12 destination is the I420 destination interleaved; an NV12 source gives what its samples give as I420
        assert same(swin.render_yuv(planes, layout="i420", out_layout="nv12", out_siting=s), ylr.pack_nv12(*out)), s
        assert same(swin.render_yuv(nv, layout="nv12", out_layout="i420", siting=s), swin.render_yuv(*planes, siting=s)), s
        # the same at a resized target
        r = swin.render_yuv_layout_resized(planes, size, out_siting=s)
        assert np.array_equal(r[0], rbase[0]), s
        assert same(swin.render_yuv_layout_resized(planes, size, out_layout="nv12", out_siting=s), ylr.pack_nv12(*r)), s
        assert same(swin.render_yuv_layout_resized(nv, size, layout="nv12", out_layout="i420", siting=s, out_siting=s),
                    swin.render_yuv_layout_resized(planes, size, siting=s, out_siting=s)), s
        # a resized call at the scaled size is the plain call
        assert same(swin.render_yuv_layout_resized(planes, (4 * rows, 4 * cols), siting=s), swin.render_yuv(*planes, siting=s)), s
    # ten bits out: P010 is << 6
    out10 = swin.render_yuv(*planes, out_bits=10, out_siting="topleft")
    assert same(swin.render_yuv(planes, layout="i420", out_layout="nv12", out_bits=10, out_siting="topleft"), ylr.pack_nv12(*out10))


def test_sequences_and_changing_sitings_on_one_engine(swin):
    frames = [ylr.random_planes(45, 67, 8, 70 + k, "i420") for k in range(3)]
    single = {(a, b): [swin.render_yuv(*f, siting=a, out_siting=b) for f in frames] for a, b in (("center", "left"), ("topleft", "topleft"), ("left", "left"))}
    # changing the siting between calls on one engine gives each call's own bytes (a captured pass keys on the source siting), in either order
    for key in (("left", "left"), ("topleft", "topleft"), ("center", "left"), ("topleft", "topleft")):
        assert same(swin.render_yuv(*frames[0], siting=key[0], out_siting=key[1]), single[key][0]), key
    assert not same(single[("center", "left")][0], single[("left", "left")][0]) and not same(single[("topleft", "topleft")][0], single[("left", "left")][0])
    for (a, b), want in single.items():
        got = swin.render_sequence_yuv(frames, siting=a, out_siting=b)
        assert all(same(x, y) for x, y in zip(got, want)), (a, b)
    size = (150, 198)
    want = [swin.render_yuv_layout_resized(f, size, siting="center", out_siting="topleft") for f in frames]
    got = swin.render_sequence_yuv_layout_resized(frames, size, siting="center", out_siting="topleft")
    assert all(same(x, y) for x, y in zip(got, want))


# ---- 2. against the float64 reference
def resized(canvas, size, filt):
    x = torch.from_numpy(np.ascontiguousarray(canvas, np.float64)).permute(2, 0, 1)[None]
    return F.interpolate(x, size=tuple(size), mode=filt, antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()


_canvases = {}


def canvas_of(eng, monkeypatch, key, planes, layout, siting, okw):
    """one oracle run per (engine, frame, source samples, source siting): an NV12 frame holds its I420 frame's samples"""
    if key not in _canvases:
        _canvases[key] = oracle_canvas(eng, ref.decode(planes, layout, siting), monkeypatch, **okw)
    return _canvases[key]


# source layout, destination layout, destination bits: the four combinations of the issue (the mixed-siting pair is added per siting below)
COMBOS = [("i420", "i420", 8), ("i420", "i420", 10), ("nv12", "i422", 8), ("i422", "i420", 8)]
TARGETS = [(None, "bicubic"), ((150, 198), "bicubic"), ((175, 250), "bicubic"), ((150, 198), "bilinear")]


def source(kind, rows, cols, layout, siting):
    return noise(rows, cols, layout) if kind == "noise" else smooth(rows, cols, layout, siting)


def check(tag, eng, monkeypatch, kind, rows, cols, siting, out_siting, combos, targets, okw=SWIN, floors=(FLOOR_8, FLOOR_10)):
    bad = []
    for layout, out_layout, ob in combos:
        planes = source(kind, rows, cols, layout, siting)
        canvas = canvas_of(eng, monkeypatch, (tag, kind, rows, cols, "i420" if layout == "nv12" else layout, ref.effective(layout, siting)), planes, layout, siting, okw)
        for size, filt in targets:
            rgb = canvas if size is None else resized(canvas, size, filt)
            want = ref.encode(rgb, out_layout, out_siting, bits=ob)
            if size is None:
                out = eng.render_yuv(tuple(planes), layout=layout, out_layout=out_layout, out_bits=ob, siting=siting, out_siting=out_siting)
            else:
                out = eng.render_yuv_layout_resized(tuple(planes), size, layout=layout, out_layout=out_layout, out_bits=ob, filter=filt, siting=siting, out_siting=out_siting)
            where = "plain" if size is None else f"{filt} -> {size[0]}x{size[1]}"
            bad += compare(f"{tag} {kind} {rows}x{cols} {siting} -> {out_siting} {layout} 8 -> {out_layout} {ob} {where}", out, want, floors[0] if ob == 8 else floors[1])
    return bad


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("siting", ["center", "topleft"])
def test_swin_45x67_against_the_reference(swin, monkeypatch, siting, kind):
    bad = check("swin", swin, monkeypatch, kind, 45, 67, siting, siting, COMBOS, TARGETS)
    bad += check("swin", swin, monkeypatch, kind, 45, 67, "center", "left", [("i420", "i420", 8)], TARGETS[:2]) if siting == "center" else []
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("siting", ["center", "topleft"])
def test_swin_9x141_against_the_reference(swin, monkeypatch, siting, kind):
    """564 output columns: a chroma row of 282 sites spans two waves of compose_yuv_kernel; the resized targets keep more than one wave (27 x 423) and nine
    64-column resample tiles with a ragged last one (20 x 563)"""
    targets = [(None, "bicubic"), ((27, 423), "bicubic"), ((20, 563), "bilinear")]
    bad = check("swin", swin, monkeypatch, kind, 9, 141, siting, siting, COMBOS, targets)
    bad += check("swin", swin, monkeypatch, kind, 9, 141, "center", "left", [("i420", "i420", 8)], targets[:2]) if siting == "center" else []
    assert not bad, "\n".join(bad)


def test_fp32_engine_against_the_reference(pkg, onnx_model, monkeypatch):
    """the fp32-storage engine (Precision.FP32): the float4v instantiations of the sited kernels; cunet x2, 45 x 67"""
    path = onnx_model("cunet/art", 2, 1, 64)
    eng = pkg.Img2Img()
    assert eng.build(path, pkg.BuildConfig.fixed(1, 64, precision=pkg.Precision.FP32)), eng.last_error()
    assert eng.load(path, pkg.RenderConfig(precision=pkg.Precision.FP32, batchSize=1, height=64, width=64, scaling=2, overlap=(0.0625, 0.0625))), eng.last_error()
    okw = dict(batch=1, tile=64, scale=2, ov=0.0625, fp16=False)
    bad = []
    for siting in ("center", "topleft"):
        bad += check("fp32", eng, monkeypatch, "smooth", 45, 67, siting, siting, [("i420", "i420", 8), ("nv12", "i422", 8)], [(None, "bicubic"), ((75, 101), "bicubic")],
                     okw=okw, floors=(FLOOR_FP32, FLOOR_FP32))
    eng.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("siting", ["center", "topleft"])
def test_the_bound_tells_a_siting_from_left(swin, monkeypatch, siting):
    """the cross-check: the device's output for `siting` against the reference for "left" misses 1 code, on the source side and on the destination side alone"""
    planes = noise(45, 67)
    canvas_left = canvas_of(swin, monkeypatch, ("swin", "noise", 45, 67, "i420", "left"), planes, "i420", "left", SWIN)
    canvas = canvas_of(swin, monkeypatch, ("swin", "noise", 45, 67, "i420", siting), planes, "i420", siting, SWIN)

    def worst(out, want):
        return max(int(np.abs(a.astype(int) - b.astype(int)).max()) for a, b in zip(out[1:], want[1:]))
    # a sited source read as left: the network sees other colours, Y included
    src_only = swin.render_yuv(*planes, siting=siting, out_siting="left")
    miss = max(int(np.abs(a.astype(int) - b.astype(int)).max()) for a, b in zip(src_only, ref.encode(canvas_left, "i420", "left")))
    print(f"EXACT cross-check {siting} source against the left reference: max {miss} codes")
    assert miss > 1
    assert not compare(f"cross-check {siting} source, own reference", src_only, ref.encode(canvas, "i420", "left"), FLOOR_8)
    # a sited destination against the left encode of the same canvas: chroma misses, plain and resized
    for size in (None, (150, 198)):
        rgb = canvas_left if size is None else resized(canvas_left, size, "bicubic")
        out = swin.render_yuv(*planes, out_siting=siting) if size is None else swin.render_yuv_layout_resized(planes, size, out_siting=siting)
        miss = worst(out, ref.encode(rgb, "i420", "left"))
        print(f"EXACT cross-check {siting} destination {'plain' if size is None else 'resized'} against the left reference: max {miss} codes")
        assert miss > 1
        assert not compare(f"cross-check {siting} destination {'plain' if size is None else 'resized'}, own reference", out, ref.encode(rgb, "i420", siting), FLOOR_8)


# ---- 3. refusals
def test_unknown_sitings_are_refused_and_the_engine_stays_usable(swin):
    planes = noise(45, 67)
    want = swin.render_yuv(*planes, siting="center", out_siting="topleft")
    L, h = swin._L, swin._h
    out = tuple(np.full(s, 0xAB, np.uint8) for s in ylr.plane_shapes(180, 268, "i420"))
    sp, dp = (C.c_void_p * 3)(*[p.ctypes.data for p in planes]), (C.c_void_p * 3)(*[p.ctypes.data for p in out])
    ss, ds = (C.c_size_t * 3)(*[p.strides[0] for p in planes]), (C.c_size_t * 3)(*[p.strides[0] for p in out])
    sps, dps = (C.c_void_p * 6)(*list(sp) * 2), (C.c_void_p * 6)(*list(dp) * 2)
    for src_s, dst_s in ((3, 0), (-1, 0), (0, 3), (0, -1), (1, 3), (-1, 2)):
        for seq in (False, True):
            before = len(swin.messages)
            if seq:
                ok = L.w2x_render_sequence_yuv_sited(h, sps, ss, 45, 67, 8, 0, src_s, dps, ds, 180, 268, 8, 0, dst_s, 2, 1, 0, 0)
            else:
                ok = L.w2x_render_yuv_sited(h, sp, ss, 45, 67, 8, 0, src_s, dp, ds, 180, 268, 8, 0, dst_s, 1, 0, 0)
            new = [m for sev, m in swin.messages[before:] if sev <= pkg_error()]
            assert ok == 0 and len(new) == 1, (src_s, dst_s, seq, new)
            bad = src_s if not 0 <= src_s <= 2 else dst_s
            # the engine's own refusal (yuv_check), worded [C++ method@line]
            assert re.fullmatch(rf"\[{'renderSequenceYuvResized' if seq else 'renderYuvResized'}@\d+\] Unknown YUV chroma siting {bad}\.", new[0]), new
            assert all(np.all(p == 0xAB) for p in out)                 # no launch wrote anything
    with pytest.raises(ValueError, match="siting must be one of"):
        swin.render_yuv(*planes, siting="bottom")
    assert L.w2x_render_yuv_sited(h, sp, ss, 45, 67, 8, 0, 1, dp, ds, 180, 268, 8, 0, 2, 1, 0, 0) == 1
    assert same(out, want)
    assert same(swin.render_yuv(*planes, siting="center", out_siting="topleft"), want)


# ---- 4. the command line
def test_cli_chroma_loc_topleft_sites_both_sides_and_tags_the_writer(pkg, tmp_path):
    """`w2x render --colorspace bt2020 --chroma-loc topleft` on a raw yuv420p clip: the frames are render_yuv(siting="topleft") - both sides sited, so neither
    the left-sited frames nor the ones sited on one side only - and the writer's argument list holds `-chroma_sample_location topleft` beside the colour tags;
    without the option the frames are the left-sited ones and the writer gets no such argument"""
    import synth_models as sm
    W2X = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "waifu2x-tensorrt_amd", "w2x")
    models = tmp_path / "models"
    path = sm.model_path(str(tmp_path), "swin_unet/art", 4, 3)
    sm.export_onnx(sm.make_model("swin_unet/art", 4, seed=5, small=True), path, 2, 64, dynamic=True)
    W, H, N = 66, 44, 3
    frames = [ylr.random_planes(H, W, 8, 90 + k, "i420") for k in range(N)]
    (tmp_path / "clip.mkv").write_bytes(b"".join(p.tobytes() for f in frames for p in f))
    bindir = tmp_path / "bin"; bindir.mkdir()
    for name, text in (("ffprobe", FAKE_FFPROBE), ("ffmpeg", FAKE_FFMPEG)):
        (bindir / name).write_text(text); (bindir / name).chmod(0o755)
    common = ["--models", str(models), "--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "2", "--tileSize", "64"]
    env = dict(os.environ, PATH=f"{bindir}:{os.environ['PATH']}", FAKE_W=str(W), FAKE_H=str(H))
    r = subprocess.run([W2X, *common, "build"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    eng = pkg.Img2Img()
    assert eng.load(path, pkg.RenderConfig(batchSize=2, height=64, width=64, scaling=4)), eng.last_error()
    per = 4 * H * 4 * W * 3 // 2
    for tag, extra, siting in (("sited", ["--chroma-loc", "topleft"], "topleft"), ("plain", [], "left")):
        out = tmp_path / f"out_{tag}"; out.mkdir()
        log = tmp_path / f"argv_{tag}.jsonl"
        r = subprocess.run([W2X, *common, "render", "-i", str(tmp_path / "clip.mkv"), "-o", str(out), "--colorspace", "bt2020", *extra], capture_output=True, text=True,
                           env=dict(env, FAKE_LOG=str(log)), timeout=300)
        assert r.returncode == 0, r.stderr
        raw = np.frombuffer((out / "clip(swin_unet_art)(noise3)(scale4).mp4").read_bytes(), np.uint8)
        assert raw.size == N * per
        for k in range(N):
            want = {(a, b): np.concatenate([p.ravel() for p in eng.render_yuv(*frames[k], matrix="bt2020", siting=a, out_siting=b)])
                    for a, b in ((siting, siting), ("left", "left"), ("topleft", "left"), ("left", "topleft"))}
            got = raw[k * per:(k + 1) * per]
            assert np.array_equal(got, want[(siting, siting)]), (tag, k)
            if siting != "left":
                assert all(not np.array_equal(got, want[key]) for key in want if key != (siting, siting)), (tag, k)
        calls = [json.loads(line) for line in log.read_text().splitlines()]
        writer = next(c for c in calls if c[c.index("-i") + 1] == "-")
        assert writer[writer.index("-colorspace") + 1] == "bt2020nc" and writer[writer.index("-color_range") + 1] == "tv"
        if siting == "left":
            assert "-chroma_sample_location" not in writer
        else:
            assert writer[writer.index("-chroma_sample_location") + 1] == "topleft" and writer.index("-chroma_sample_location") > writer.index("-i")
    eng.close()
