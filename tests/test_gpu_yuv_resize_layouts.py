"""Resized YUV output in 4:2:2, 4:4:4 and NV12 / P010 on the GPU (Img2Img::renderYuvResized / renderSequenceYuvResized with YuvImage::layout on either side,
w2x_render_yuv_layout_resized): gather_yuv_kernel reads the source layout, compose_canvas_kernel leaves the fp32 canvas unclamped, and the kernels of
k_resample_yuv.hip resize it and encode the destination layout.

Two kinds of checks.  Byte equalities that need no oracle: (a) the new entry with I420 both ways is render_yuv_resized; (b) an NV12 / P010 source gives what
its I420 samples give, for every output layout; (c) an NV12 / P010 output is the I420 output interleaved (<< 6 at 10 bits); (d) the Y plane is the same bytes
in all four output layouts; (e) at the scaled size the call is render_yuv(layout=, out_layout=); (f) a sequence is its single calls.  And the float64 reference
yuv_layout_ref.encode(interpolate_float64(canvas, (R, C), filter, antialias=True), layout): the source planes decoded by yuv_layout_ref.decode, pipeline.render
with the engine's own network, the canvas captured where render() would quantise it (test_gpu_yuv_layouts.oracle_canvas), torch-CPU F.interpolate in float64.
One canvas per input frame serves all of its targets, output layouts, depths and both filters.

Bounds.  At most 1 code in every plane of every case (the device works in fp32, the reference in float64, and an fp16 engine's network sees
inputs an fp16 rounding apart here and there).  The share of exactly equal codes has no number fixed in advance: in the same run the existing I420 path -
render_yuv_resized on the same picture as 4:2:0 planes, same target, filter and depth - is compared with the same reference model, and with s the exact share
of its worst plane, the worst plane of the new layout must reach 1 - 2 (1 - s): DESIGN 9c's rule, anchored on resample_yuv_kernel instead of on the code
under test.  Every plane's figures are printed ("EXACT ..." lines; profiles/yuv_resize_layouts/gpu_exact.txt is this file's output)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yuv_layout_ref as ref
import yuv_ref
from test_gpu_parity import make_engine
from test_gpu_yuv_layouts import oracle_canvas

pytestmark = pytest.mark.gpu

LAYOUTS = ref.LAYOUTS
SWIN = dict(batch=2, tile=64, scale=4, ov=0.0625)


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def swin(pkg, onnx_model):
    path = onnx_model("swin_unet/art", 4, 2, 64, small=True)
    eng = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625))
    yield eng
    eng.close()


def pictures():
    """the two frames of test_gpu_yuv_resize.py's swin cases, so that the I420 anchor is the case on record there: smooth 50 x 66 and YUV noise 45 x 57 (odd sizes,
    more than one 64-column and one 16-row tile at every target, ragged last tiles).  The noise frame is given as its 4:2:0 planes; as a picture it is what
    they decode to."""
    noise = yuv_ref.random_planes(45, 57, 8, 11)
    return [ref.smooth_rgb(50, 66, 12), (ref.decode(noise, "i420"), noise)]


def targets(r, c):
    """x3, x2, x2.5 rows with x4 columns, odd x odd, x1"""
    return [(3 * r, 3 * c), (2 * r, 2 * c), (int(round(2.5 * r)), 4 * c), (2 * r + 1, 2 * c + 1), (r, c)]


# ---- the reference
def resized(canvas, size, filt):
    x = torch.from_numpy(np.ascontiguousarray(canvas, np.float64)).permute(2, 0, 1)[None]
    return F.interpolate(x, size=tuple(size), mode=filt, antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()


def plane_names(planes):
    return "YUV" if len(planes) == 3 else ("Y", "UV")


def shares(tag, out, want, problems):
    """prints every plane's figures, notes the planes over 1 code, returns the exact share of the worst plane"""
    assert len(out) == len(want), (tag, len(out), len(want))
    worst = 1.0
    for name, a, b in zip(plane_names(out), out, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, name, a.shape, b.shape, a.dtype, b.dtype)
        d = np.abs(a.astype(np.int64) - b.astype(np.int64))
        exact = float((d == 0).mean())
        worst = min(worst, exact)
        print(f"EXACT {tag} {name}: max {int(d.max())} codes, exact {exact:.6f} of {d.size}")
        if d.max() > 1:
            problems.append(f"{tag} {name}: max {int(d.max())} codes")
    return worst


_canvases = {}


def canvas_of(eng, monkeypatch, key, planes, layout, fmt, okw):
    """one oracle run per (engine, picture, source samples): an NV12 frame holds its I420 frame's samples, so the two share theirs"""
    if key not in _canvases:
        bits = 8 if planes[0].dtype == np.uint8 else 10
        _canvases[key] = oracle_canvas(eng, ref.decode(planes, layout, bits=bits, **fmt), monkeypatch, **okw)
    return _canvases[key]


def check_picture(tag, eng, monkeypatch, pic, in_layout, in_bits, sizes, filters, outs, okw, problems, matrix="bt709", full_range=False):
    """every (target, filter, output layout, depth) of one input frame against the reference, each with the floor the I420 path sets in this run.
    pic: the picture as float RGB, or (RGB, its 4:2:0 planes); outs: {output depth: layouts}."""
    fmt = dict(matrix=matrix, full_range=full_range)
    pic, planes420 = pic if isinstance(pic, tuple) else (pic, ref.encode(pic, "i420", bits=in_bits, **fmt))
    planes = planes420 if in_layout == "i420" else ref.pack_nv12(*planes420) if in_layout == "nv12" else ref.encode(pic, in_layout, bits=in_bits, **fmt)
    base = "i420" if in_layout == "nv12" else in_layout
    canvas = canvas_of(eng, monkeypatch, (tag, base), planes, in_layout, fmt, okw)
    canvas420 = canvas_of(eng, monkeypatch, (tag, "i420"), planes420, "i420", fmt, okw)
    r, c = planes[0].shape
    for size in sizes:
        for filt in filters:
            want, want420 = resized(canvas, size, filt), resized(canvas420, size, filt)
            for ob, lays in outs.items():
                case = f"{tag} {filt} {r}x{c} -> {size[0]}x{size[1]}"
                anchor = eng.render_yuv_resized(*planes420, size, out_bits=ob, filter=filt, **fmt)
                s = shares(f"{case} anchor i420 {in_bits} -> i420 {ob}", anchor, ref.encode(want420, "i420", bits=ob, **fmt), problems)
                floor = 1.0 - 2.0 * (1.0 - s)
                for lay in lays:
                    out = eng.render_yuv_layout_resized(planes, size, layout=in_layout, out_layout=lay, out_bits=ob, filter=filt, **fmt)
                    assert [p.shape for p in out] == ref.plane_shapes(*size, lay) and out[0].dtype == (np.uint8 if ob == 8 else np.uint16)
                    worst = shares(f"{case} {in_layout} {in_bits} -> {lay} {ob}", out, ref.encode(want, lay, bits=ob, **fmt), problems)
                    print(f"FLOOR {case} {in_layout} {in_bits} -> {lay} {ob}: worst plane {worst:.6f}, floor {floor:.6f} (anchor {s:.6f})")
                    if worst < floor:
                        problems.append(f"{case} {in_layout} {in_bits} -> {lay} {ob}: exact {worst:.6f} below the floor {floor:.6f} (I420 path: {s:.6f})")


# ---- 1. byte equalities, no oracle
@pytest.mark.parametrize("bits", [8, 10])
def test_layouts_that_must_agree_to_the_byte(swin, bits):
    for rows, cols in ((45, 57), (50, 66)):
        y, u, v = yuv_ref.random_planes(rows, cols, bits, 200 + bits)
        Y, UV = ref.pack_nv12(y, u, v)
        for size, filt in (((2 * rows + 1, 2 * cols + 1), "bicubic"), ((int(round(2.5 * rows)), 4 * cols), "bilinear"), ((rows, cols), "bicubic")):
            for ob in (8, 10):
                kw = dict(out_bits=ob, filter=filt)
                base = swin.render_yuv_resized(y, u, v, size, **kw)
                # (a) the new entry with I420 both ways is render_yuv_resized
                assert same(swin.render_yuv_layout_resized((y, u, v), size, **kw), base), (size, ob)
                for lay in LAYOUTS:
                    out = swin.render_yuv_layout_resized((y, u, v), size, out_layout=lay, **kw)
                    assert [p.shape for p in out] == ref.plane_shapes(*size, lay), (size, lay)
                    # (b) an NV12 / P010 source gives the bytes of its I420 samples, for every output layout (the low six bits of P010 are ignored)
                    assert same(swin.render_yuv_layout_resized((Y, UV), size, layout="nv12", out_layout=lay, **kw), out), (size, ob, lay)
                    if bits == 10:
                        assert same(swin.render_yuv_layout_resized((Y | 0x2A, UV | 0x3F), size, layout="nv12", out_layout=lay, **kw), out), (size, ob, lay)
                    # (c) NV12 / P010 resized output is the I420 resized output interleaved, << 6 at 10 bits
                    if lay == "nv12":
                        assert same(out, ref.pack_nv12(*base)), (size, ob)
                    # (d) the Y plane is the same bytes in all four output layouts and equals render_yuv_resized's
                    else:
                        assert out[0].dtype == base[0].dtype and np.array_equal(out[0], base[0]), (size, ob, lay)
        # (e) at the scaled size the call is render_yuv(layout=, out_layout=)
        src = ref.random_planes(rows, cols, bits, 300 + bits, "i422")
        for lay in LAYOUTS:
            for filt in ("bicubic", "bilinear"):
                got = swin.render_yuv_layout_resized(src, (4 * rows, 4 * cols), layout="i422", out_layout=lay, out_bits=18 - bits, filter=filt)
                assert same(got, swin.render_yuv(src, layout="i422", out_layout=lay, out_bits=18 - bits)), (lay, filt)


def test_the_even_row_luma_is_one_expression_in_every_layout(swin):
    """(c) and (d) at the case that told the kernels apart before they shared their expressions (profiles/resample_family/ab_parent.txt): the smooth 50 x 66
    picture of tools/resample_digest.py to 175 x 250, bicubic, 10 bits out.  Y[36][7] lies on a rounding tie of Y' there - code 500 with kb B rounded on its
    own, as the I420 kernel forms Y' on even rows, 499 with kb B fused into the sum, which is what the compiler made of the layout kernels' statement of the
    same form.  No other target of this file or of that tool has such a sample."""
    import resample_digest as rd
    planes = rd.yuv_source(rd.picture(50, 66, 7 * 50 + 66), 8)
    kw = dict(out_bits=10, filter="bicubic")
    base = swin.render_yuv_resized(*planes, (175, 250), **kw)
    assert base[0][36, 7] == 500
    for lay in LAYOUTS:
        out = swin.render_yuv_layout_resized(planes, (175, 250), out_layout=lay, **kw)
        if lay == "nv12":
            assert same(out, ref.pack_nv12(*base))
        else:
            assert out[0].dtype == base[0].dtype and np.array_equal(out[0], base[0]), lay


@pytest.mark.parametrize("pinned", [False, True])
def test_rolling_sequence_matches_single_frames(pkg, onnx_model, pinned):
    """(f) renderSequenceYuvResized over five frames that roll (with TTA a 90 x 130 frame on swin x4 fills 48 slots of its one pass: run_rolling_frame, the
    canvas compose and the resample kernel on the second group's stream), NV12 in: byte-identical to the per-frame calls for I422 at 10 bits, I444 and P010
    out, on a repeated call, with pageable or page-locked outputs, and with plane steps wider than the rows"""
    path = onnx_model("swin_unet/art", 4, 2, 64, small=True)
    eng = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625), tta=True)
    frames = [ref.random_planes(90, 130, 8, 50 + k, "nv12") for k in range(5)]
    size = (270, 391)
    for lay, ob, filt in (("i422", 10, "bicubic"), ("i444", 8, "bilinear"), ("nv12", 10, "bicubic")):
        kw = dict(layout="nv12", out_layout=lay, out_bits=ob, filter=filt)
        want = [eng.render_yuv_layout_resized(f, size, **kw) for f in frames]
        assert [p.shape for p in want[0]] == ref.plane_shapes(*size, lay)
        for attempt in range(2 if lay == "i422" else 1):
            got = eng.render_sequence_yuv_layout_resized(frames, size, pinned=pinned, **kw)
            for k, (a, b) in enumerate(zip(got, want)):
                assert same(a, b), (lay, attempt, k)
        if lay != "i444":
            continue
        wide = [tuple(np.pad(p, ((0, 0), (0, 24)))[:, :p.shape[1]] for p in f) for f in frames[:3]]
        assert wide[0][1].strides[0] == 130 + 24
        assert all(same(a, b) for a, b in zip(eng.render_sequence_yuv_layout_resized(wide, size, pinned=pinned, **kw), want))
        assert same(eng.render_yuv_layout_resized(frames[1], size, **kw), want[1])
    eng.close()


# ---- 2. against the float64 reference
@pytest.mark.parametrize("in_layout", LAYOUTS)
def test_swin_x4_422_and_444_out_against_the_reference(swin, monkeypatch, in_layout):
    """swin_unet x4, blend 1/16, BT.709 limited, 8-bit sources of each layout, I422 and I444 out at 8 and 10 bits, both filters, five targets per frame"""
    problems = []
    for k, pic in enumerate(pictures()):
        rows, cols = (pic[0] if isinstance(pic, tuple) else pic).shape[:2]
        check_picture(f"swin frame{k}", swin, monkeypatch, pic, in_layout, 8, targets(rows, cols), ("bicubic", "bilinear"),
                      {8: ("i422", "i444"), 10: ("i422", "i444")}, SWIN, problems)
    assert not problems, "\n".join(problems)


def test_a_canvas_that_leaves_the_range_is_clamped_between_the_resize_and_the_coding(pkg, tmp_path, monkeypatch):
    """The synthetic networks end in a Clip and keep most of their output well inside (0, 1): after either filter their canvases stay inside [0, 1] and no
    clamp of the kernels cuts anything.  Here the image head of the small swin x4 has four times the gain: 40 % of the canvas sits at 0 or 1, the bicubic
    filter overshoots at those edges (1.2 % of the x3 target's samples leave [0, 1], by up to 0.1), and a kernel that codes chroma from an unclamped colour,
    or lets an unclamped neighbour into the chroma filter - at the tile seams, columns 64, 128 and 192, the halo column - is out by several codes.  The 60 %
    of the canvas inside the range keep the I420 anchor, and with it the floor, off 1.  8-bit output only: the bound of 1 code rests on the engine's and the
    oracle's fp16 tiles lying a few fp16 steps (4.9e-4 at 0.5 and above) apart, which the head's gain multiplies by four here - well inside an 8-bit code
    (1 / 219 = 4.6e-3), not inside a 10-bit one (1 / 876 = 1.1e-3), for the existing I420 path as for the new kernels."""
    import synth_models as sm
    net = sm.make_model("swin_unet/art", 4, seed=1237, small=True)
    with torch.no_grad():
        net.to_image.proj.weight.mul_(4.0)
    path = sm.model_path(str(tmp_path), "swin_unet/art", 4, 3)
    sm.export_onnx(net, path, 2, 64, dynamic=True)
    eng = make_engine(pkg, path, 2, 64, 4, overlap=(0.0625, 0.0625))
    problems = []
    check_picture("gain 4", eng, monkeypatch, ref.smooth_rgb(50, 66, 12), "i420", 8, [(150, 198), (175, 250)], ("bicubic",), {8: ("i422", "i444")}, SWIN, problems)
    eng.close()
    assert not problems, "\n".join(problems)


def test_wide_and_ragged_targets(swin, monkeypatch):
    """targets of many column tiles: 448 columns (seven whole tiles: every seam takes its halo column from the tile on its left) and 333 (odd, five tiles and
    13 columns: the sample-by-sample stores, the clamped last chroma column, the last lane pair cut), each for I422 and I444, at 8 and at 10 bits"""
    problems = []
    pic = ref.smooth_rgb(40, 141, 71)
    check_picture("wide", swin, monkeypatch, pic, "i420", 8, [(81, 333)], ("bicubic",), {8: ("i422", "i444"), 10: ("i422", "i444")}, SWIN, problems)
    check_picture("wide", swin, monkeypatch, pic, "i420", 8, [(40, 448)], ("bilinear",), {8: ("i422", "i444"), 10: ("i422",)}, SWIN, problems)
    assert not problems, "\n".join(problems)


def test_cunet_tta_bt2020_full_range_ten_bit(pkg, onnx_model, monkeypatch):
    """cunet x2 with TTA and no blend, 10-bit full-range BT.2020, a 4:2:2 source to x1.5 in I422 and I444"""
    path = onnx_model("cunet/art", 2, 2, 64)
    eng = make_engine(pkg, path, 2, 64, 2, overlap=(0.0, 0.0), tta=True)
    problems = []
    check_picture("cunet tta bt2020 pc", eng, monkeypatch, ref.smooth_rgb(61, 83, 32), "i422", 10, [(92, 124)], ("bicubic", "bilinear"), {10: ("i422", "i444")},
                  dict(batch=2, tile=64, scale=2, ov=0.0, tta=True), problems, matrix="bt2020", full_range=True)
    eng.close()
    assert not problems, "\n".join(problems)


def test_fp32_engine(pkg, onnx_model, monkeypatch):
    """the fp32-storage engine (Precision.FP32): the float4v tiles of the gather and of the canvas compose; an NV12 source, I444 at 8 and I422 at 10 bits"""
    path = onnx_model("cunet/art", 2, 1, 64)
    eng = pkg.Img2Img()
    assert eng.build(path, pkg.BuildConfig.fixed(1, 64, precision=pkg.Precision.FP32)), eng.last_error()
    assert eng.load(path, pkg.RenderConfig(precision=pkg.Precision.FP32, batchSize=1, height=64, width=64, scaling=2, overlap=(0.0625, 0.0625))), eng.last_error()
    problems = []
    check_picture("fp32 engine", eng, monkeypatch, ref.smooth_rgb(57, 70, 41), "nv12", 8, [(86, 105)], ("bicubic", "bilinear"), {8: ("i444",), 10: ("i422",)},
                  dict(batch=1, tile=64, scale=2, ov=0.0625, fp16=False), problems)
    eng.close()
    assert not problems, "\n".join(problems)


# ---- 3. refusals
def test_refused_calls_leave_the_engine_usable(swin, pkg):
    """each invalid call returns 0 with one message and launches nothing; afterwards a valid call gives the bytes it gave before.  (The C ABI carries one layout
    per side for a whole sequence, so a layout that changes inside a sequence can be asked for from Python only, where the documented error is raised before
    the library is called.)"""
    y, u, v = yuv_ref.random_planes(40, 50, 8, 61)
    Y, UV = ref.pack_nv12(y, u, v)
    kw = dict(layout="nv12", out_layout="i444", out_bits=10)
    before = (swin.render_yuv_layout_resized((Y, UV), (100, 150), **kw), swin.render_yuv_layout_resized((y, u, v), (100, 151), out_layout="i422"),
              swin.render_yuv_resized(y, u, v, (100, 150)))
    L, h = swin._L, swin._h
    error = int(pkg.Severity.error)

    def call(planes=(y, u, v), steps=None, layout=0, olayout=2, orows=100, ocols=150, oplanes=None, osteps=None, filt=0, seq=False):
        out = [np.zeros((orows if orows > 0 else 1, 160), np.uint8) for _ in range(3)]
        sp = (C.c_void_p * 3)(*[p.ctypes.data if p is not None else None for p in planes])
        st = (C.c_size_t * 3)(*(steps if steps else [p.strides[0] if p is not None else 0 for p in planes]))
        dp = (C.c_void_p * 3)(*[p.ctypes.data if keep else None for p, keep in zip(out, oplanes or (1, 1, 1))])
        ds = (C.c_size_t * 3)(*(osteps if osteps else [p.strides[0] for p in out]))
        if seq:
            return L.w2x_render_sequence_yuv_layout_resized(h, sp, st, 40, 50, 8, layout, dp, ds, orows, ocols, 8, olayout, 1, 1, 0, filt)
        return L.w2x_render_yuv_layout_resized(h, sp, st, 40, 50, 8, layout, dp, ds, orows, ocols, 8, olayout, 1, 0, filt)

    assert call() == 1 and call(seq=True) == 1                         # the helper's valid call is accepted
    cases = {
        "one row too many": dict(orows=161), "one column too many": dict(ocols=201), "fewer rows than the input": dict(orows=39),
        "fewer columns than the input": dict(ocols=49), "no rows": dict(orows=0), "sequence: too large": dict(orows=161, seq=True),
        "i444 destination with chroma steps of ceil(cols/2)": dict(osteps=[160, 75, 75]),
        "i422 destination with a short V step": dict(olayout=1, osteps=[160, 75, 74]),
        "nv12 source with a null UV plane": dict(planes=(Y, None, None), steps=[50, 50, 0], layout=3),
        "nv12 destination with a null UV plane": dict(olayout=3, oplanes=(1, 0, 0)),
        "nv12 destination with a UV step of ceil(cols/2)": dict(olayout=3, osteps=[160, 75, 0]),
        "source layout 4": dict(layout=4), "destination layout -1": dict(olayout=-1), "filter 2": dict(filt=2),
    }
    for name, ckw in cases.items():
        count = len(swin.messages)
        assert call(**ckw) == 0, name
        new = [m for sev, m in swin.messages[count:] if sev <= error]
        assert len(new) == 1, (name, new)
        print(f"{name}: {new[-1]}")
    assert call(planes=(Y, UV, None), steps=[50, 50, 0], layout=3, olayout=3, oplanes=(1, 1, 0)) == 1   # NV12 ignores the third plane and step, on both sides
    # a layout that changes inside a sequence; planes that are not the named layout's; names nobody knows
    count = len(swin.messages)
    with pytest.raises(ValueError, match="one size, depth and layout"):
        swin.render_sequence_yuv_layout_resized([(Y, UV), (y, u, v)], (100, 150), layout="nv12", out_layout="i444")
    with pytest.raises(ValueError):
        swin.render_yuv_layout_resized((y, u, v), (100, 150), layout="i444")
    with pytest.raises(ValueError):
        swin.render_yuv_layout_resized((Y, UV), (100, 150), layout="nv12", out_layout="yuv411p")
    assert len(swin.messages) == count
    with pytest.raises(pkg.W2xError):
        swin.render_yuv_layout_resized((Y, UV), (100, 201), **kw)
    with pytest.raises(pkg.W2xError):
        swin.render_sequence_yuv_layout_resized([(Y, UV)] * 2, (39, 150), **kw)
    dst = tuple(np.zeros(s, np.uint8) for s in ref.plane_shapes(161, 150, "i422"))
    assert swin.render_yuv_layout_resized((y, u, v), (161, 150), out_layout="i422", dst=dst) is False and "invalid size" in swin.last_error()
    after = (swin.render_yuv_layout_resized((Y, UV), (100, 150), **kw), swin.render_yuv_layout_resized((y, u, v), (100, 151), out_layout="i422"),
             swin.render_yuv_resized(y, u, v, (100, 150)))
    assert all(same(a, b) for a, b in zip(after, before))
