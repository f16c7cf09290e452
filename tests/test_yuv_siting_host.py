"""YUV chroma siting without a device (YuvImage::siting): the float64 reference of tests/yuv_siting_ref.py against yuv_layout_ref at "left", the
weights and offsets of the two 1-D rules on impulses and ramps, the distinguishability of the sitings on the very frames the GPU tests use, the two C entries
of include/w2x/c_api_yuv_siting.h on a null and a never-loaded engine, the wrapper's marshalling through the recording stub of
tests/golden/make_binding_calls.py, and the command line's --chroma-loc.

The command line: here the parse alone (the option's value in the printed configuration, its refusals, its place in --help); the render and the writer's
`-chroma_sample_location` run on the GPU, tests/test_gpu_yuv_siting.py, with the logging stand-ins for ffmpeg."""
import ctypes as C
import importlib
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import yuv_layout_ref as ylr
import yuv_ref
import yuv_siting_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8, u16 = np.uint8, np.uint16
SITINGS = ref.SITINGS
SIZES = [(8, 10), (7, 9)]


# ---- 1. "left" is yuv_layout_ref, to the bit
@pytest.mark.parametrize("rows,cols", SIZES)
@pytest.mark.parametrize("layout", ylr.LAYOUTS)
def test_left_is_the_layout_reference_to_the_bit(layout, rows, cols):
    for bits in (8, 10):
        planes = ylr.random_planes(rows, cols, bits, 5 + bits, layout)
        assert np.array_equal(ref.decode(planes, layout, "left"), ylr.decode(planes, layout))
        assert np.array_equal(ref.decode(planes, layout), ylr.decode(planes, layout))
        rgb = np.random.default_rng(3).random((rows, cols, 3))
        for a, b in zip(ref.encode(rgb, layout, "left", bits=bits), ylr.encode(rgb, layout, bits=bits)):
            assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("rows,cols", SIZES)
def test_layouts_without_the_axis_ignore_the_rule(rows, cols):
    rgb = np.random.default_rng(4).random((rows, cols, 3))
    p444, p422 = ylr.random_planes(rows, cols, 8, 6, "i444"), ylr.random_planes(rows, cols, 8, 7, "i422")
    for s in SITINGS:                                                   # i444: no subsampled axis
        assert np.array_equal(ref.decode(p444, "i444", s), ref.decode(p444, "i444", "left"))
        assert all(np.array_equal(a, b) for a, b in zip(ref.encode(rgb, "i444", s), ref.encode(rgb, "i444", "left")))
    assert np.array_equal(ref.decode(p422, "i422", "topleft"), ref.decode(p422, "i422", "left"))       # i422: the column rule alone
    assert all(np.array_equal(a, b) for a, b in zip(ref.encode(rgb, "i422", "topleft"), ref.encode(rgb, "i422", "left")))
    assert not np.array_equal(ref.decode(p422, "i422", "center"), ref.decode(p422, "i422", "left"))
    # nv12 is i420 interleaved, per siting
    for s in SITINGS:
        p420 = ylr.random_planes(rows, cols, 8, 8, "i420")
        assert np.array_equal(ref.decode(ylr.pack_nv12(*p420), "nv12", s), ref.decode(p420, "i420", s))
        assert all(np.array_equal(a, b) for a, b in zip(ref.encode(rgb, "nv12", s), ylr.pack_nv12(*ref.encode(rgb, "i420", s))))
    with pytest.raises(ValueError):
        ref.decode(p444, "i444", "bottom")


# ---- 2. impulses: the weights of the two rules, clamped edges included
def expected_spread(n, cn, k, centred):
    """what one raised chroma sample k of cn spreads onto n luma samples, by the rule as the issue states it"""
    out = np.zeros(n)
    for i in range(n):
        if centred:
            taps = [(max(i // 2 - 1, 0), 0.25), (i // 2, 0.75)] if i % 2 == 0 else [(i // 2, 0.75), (min(i // 2 + 1, cn - 1), 0.25)]
        else:
            taps = [(i // 2, 1.0)] if i % 2 == 0 else [((i - 1) // 2, 0.5), (min((i + 1) // 2, cn - 1), 0.5)]
        out[i] = sum(w for j, w in taps if j == k)
    return out


def expected_gather(n, i, centred):
    """what one raised luma sample i of n puts on the ceil(n / 2) sites"""
    out = np.zeros((n + 1) // 2)
    for j in range(len(out)):
        taps = [(2 * j, 0.5), (min(2 * j + 1, n - 1), 0.5)] if centred else [(max(2 * j - 1, 0), 0.25), (2 * j, 0.5), (min(2 * j + 1, n - 1), 0.25)]
        out[j] = sum(w for q, w in taps if q == i)
    return out


@pytest.mark.parametrize("rows,cols", SIZES)
@pytest.mark.parametrize("siting", SITINGS)
def test_upsampling_weights_on_impulses(siting, rows, cols):
    ch, cw = (rows + 1) // 2, (cols + 1) // 2
    for ki in sorted({0, 1, ch // 2, ch - 1}):
        for kj in sorted({0, 1, cw // 2, cw - 1}):
            c = np.zeros((ch, cw)); c[ki, kj] = 1.0
            got = ref.upsample(c, rows, cols, "i420", siting)
            want = np.outer(expected_spread(rows, ch, ki, ref.ROWS_CENTRED[siting]), expected_spread(cols, cw, kj, ref.COLS_CENTRED[siting]))
            assert np.array_equal(got, want), (siting, ki, kj)
            got422 = ref.upsample(np.pad(c, ((0, rows - ch), (0, 0))), rows, cols, "i422", siting)       # the column rule alone
            assert np.array_equal(got422[ki], expected_spread(cols, cw, kj, ref.COLS_CENTRED[siting]))
    # a flat plane stays flat: every luma sample's weights sum to one, edges included
    assert np.array_equal(ref.upsample(np.full((ch, cw), 3.0), rows, cols, "i420", siting), np.full((rows, cols), 3.0))


@pytest.mark.parametrize("rows,cols", SIZES)
@pytest.mark.parametrize("siting", SITINGS)
def test_downsampling_weights_on_impulses(siting, rows, cols):
    for y in sorted({0, 1, 2, rows // 2, rows - 2, rows - 1}):
        for x in sorted({0, 1, 2, cols // 2, cols - 2, cols - 1}):
            rgb = np.zeros((rows, cols, 3)); rgb[y, x] = 1.0
            got = ref.site_rgb(rgb, "i420", siting)[..., 0]
            want = np.outer(expected_gather(rows, y, ref.ROWS_CENTRED[siting]), expected_gather(cols, x, ref.COLS_CENTRED[siting]))
            assert np.array_equal(got, want), (siting, y, x)
            assert np.array_equal(ref.site_rgb(rgb, "i422", siting)[y, :, 0], expected_gather(cols, x, ref.COLS_CENTRED[siting]))
    assert np.array_equal(ref.site_rgb(np.full((rows, cols, 3), 0.25), "i420", siting), np.full(((rows + 1) // 2, (cols + 1) // 2, 3), 0.25))


# ---- 3. ramps: the sign and the size of the offsets
def ramp_frame(rows, cols, axis):
    """a frame whose Cb rises linearly along `axis` inside the cube: R = G = 1/4, B = 1/4 + 0.6 t, t = n / N.  B - Y' = 0.6 t (1 - Kb), so Cb' = 0.3 t whatever the
    matrix: at 10 bits limited 0.3 * 896 / N codes per luma sample"""
    t = np.arange(cols if axis == 1 else rows, dtype=np.float64) / (cols if axis == 1 else rows)
    t = np.broadcast_to(t[None, :] if axis == 1 else t[:, None], (rows, cols))
    base = 0.25
    return np.stack([np.full((rows, cols), base), np.full((rows, cols), base), base + 0.6 * t], -1)


@pytest.mark.parametrize("siting", SITINGS)
def test_a_chroma_ramp_survives_its_own_siting_only(siting):
    rows, cols, bits = 24, 32, 10
    for axis in (0, 1):
        rgb = ramp_frame(rows, cols, axis)
        planes = ref.encode(rgb, "i420", siting, bits=bits)
        want = ref.encode(rgb, "i444", bits=bits)                       # the ramp's own codes per pixel
        inner = (slice(4, rows - 4), slice(4, cols - 4))
        for other in SITINGS:
            back = ref.encode(ref.decode(planes, "i420", other, bits=bits), "i444", bits=bits)
            d = np.abs(back[1].astype(int) - want[1].astype(int))[inner]
            centred = (ref.COLS_CENTRED if axis == 1 else ref.ROWS_CENTRED)
            if centred[other] == centred[siting]:
                assert d.max() <= 1, (siting, other, axis, int(d.max()))
            else:
                # the rules differ along this axis: half a luma sample of offset at the ramp's slope, 0.5 * 0.3 * 896 / N codes (4.2 along the columns, 5.6 along
                # the rows), everywhere; each side of the difference carries up to 1.5 codes of rounding (the plane's, the decoded pixel's, the ramp's own)
                n = cols if axis == 1 else rows
                shift = 0.5 * 0.3 * 896 / n
                assert shift > 4.0
                signed = (back[1].astype(int) - want[1].astype(int))[inner]
                sign = 1 if centred[siting] else -1                     # centred samples read as co-sited land half a sample late: the decoded ramp runs ahead
                assert np.all(np.abs(signed - sign * shift) <= 1.5), (siting, other, axis, signed.min(), signed.max(), shift)
                assert d.min() > 1


# ---- 4. the frames of the GPU tests tell the sitings apart
def test_gpu_frames_distinguish_the_sitings():
    """On the frames tests/test_gpu_yuv_siting.py uses (yuv_siting_ref.GPU_FRAMES through gpu_noise / gpu_smooth, the helpers that file calls): the references of
    any two sitings differ by more than 1 code in at least 1 % of the chroma samples, so its 1-code bound can tell a siting from its neighbour.  Source side: the
    frame decoded by either siting, re-coded at 4:4:4.  Destination side (noise frames; the canvas itself exists on the GPU only): the decoded frame at twice
    the size, encoded by either siting.  i422 tells left from center only."""
    def share(a, b):
        return float((np.abs(a.astype(int) - b.astype(int)) > 1).mean())
    pairs = {"i420": [("left", "center"), ("left", "topleft"), ("center", "topleft")], "i422": [("left", "center")]}
    for rows, cols in ref.GPU_FRAMES:
        for layout, pp in pairs.items():
            for a, b in pp:
                src = ref.gpu_noise(rows, cols, layout)
                da, db = (ref.encode(ref.decode(src, layout, s), "i444") for s in (a, b))
                s_dec = min(share(da[1], db[1]), share(da[2], db[2]))
                rgb = np.kron(ref.decode(src, layout, a), np.ones((2, 2, 1)))
                ea, eb = (ref.encode(rgb, layout, s) for s in (a, b))
                s_enc = min(share(ea[1], eb[1]), share(ea[2], eb[2]))
                print(f"DISTINCT noise {rows}x{cols} {layout} {a} / {b}: decode {s_dec:.4f}, encode {s_enc:.4f}")
                assert s_dec >= 0.01 and s_enc >= 0.01, (rows, cols, layout, a, b, s_dec, s_enc)
                for own in (a, b):                                      # the smooth picture as the GPU tests encode it for its own siting, read by the other
                    src = ref.gpu_smooth(rows, cols, layout, own)
                    da, db = (ref.encode(ref.decode(src, layout, s), "i444") for s in (a, b))
                    s_dec = min(share(da[1], db[1]), share(da[2], db[2]))
                    print(f"DISTINCT smooth {rows}x{cols} {layout} sited {own}, {a} / {b}: decode {s_dec:.4f}")
                    assert s_dec >= 0.01, (rows, cols, layout, own, a, b, s_dec)


# ---- 5. the C entries
ENTRIES = {"w2x_render_yuv_sited", "w2x_render_sequence_yuv_sited"}


def declared(header):
    hdr = open(os.path.join(ROOT, "include", "w2x", header)).read()
    return set(re.findall(r"\b(w2x_[a-z0-9_]+)\s*\(", hdr[hdr.index('extern "C"'):]))


@pytest.fixture(scope="module")
def engine_module(pkg):
    return importlib.import_module("waifu2x-tensorrt_amd.engine")


def test_header_library_and_table_agree(pkg, engine_module):
    names = declared("c_api_yuv_siting.h")
    assert names == ENTRIES == set(engine_module.YUV_SITED_SYMBOLS) == set(pkg.YUV_SITED_SYMBOLS)
    raw = C.CDLL(pkg.lib_path)
    for n in names:
        assert hasattr(raw, n), f"libw2x.so does not export {n}"
    for other in ("c_api.h", "c_api_gray.h", "c_api_planar.h", "c_api_rgbap.h", "c_api_yuv_resized.h"):
        assert not names & declared(other), other
    for table in ("SYMBOLS", "EXPORTED_SYMBOLS", "GRAY_SYMBOLS", "PLANAR_SYMBOLS", "RGBAP_SYMBOLS", "YUV_RESIZED_SYMBOLS"):
        assert not names & set(getattr(engine_module, table)), table
    L = pkg.lib()
    for n, (restype, argtypes) in engine_module.YUV_SITED_SYMBOLS.items():
        assert getattr(L, n).restype is restype and list(getattr(L, n).argtypes) == argtypes, n
    # the argument lists: those of the _yuv_layout_resized entries with a siting behind each layout
    for n, plain in (("w2x_render_yuv_sited", "w2x_render_yuv_layout_resized"), ("w2x_render_sequence_yuv_sited", "w2x_render_sequence_yuv_layout_resized")):
        a = list(engine_module.YUV_RESIZED_SYMBOLS[plain][1])
        assert engine_module.YUV_SITED_SYMBOLS[n] == (C.c_int, a[:7] + [C.c_int] + a[7:13] + [C.c_int] + a[13:])
    hdr = open(os.path.join(ROOT, "include", "w2x", "c_api_yuv_siting.h")).read()
    assert [int(re.search(rf"#define W2X_YUV_SITING_{k} (\d)", hdr).group(1)) for k in ("LEFT", "CENTER", "TOPLEFT")] == [0, 1, 2]
    assert engine_module.YUV_SITINGS == {"left": 0, "center": 1, "topleft": 2}


ROWS, COLS = 4, 6
LAYOUT_AT, SITING_AT = (5, 12), (6, 13)


class Args:
    """an nv12 source of 4 x 6 and an i444 destination of 7 x 9 at 10 bits"""

    def __init__(self):
        self.src = [np.zeros((ROWS, COLS), u8), np.zeros((ROWS // 2, COLS), u8)]
        self.dst = np.zeros((3, 7, 9), u16)
        self.sp = (C.c_void_p * 3)(self.src[0].ctypes.data, self.src[1].ctypes.data, None)
        self.dp = (C.c_void_p * 3)(*[p.ctypes.data for p in self.dst])
        self.ss, self.ds = (C.c_size_t * 3)(COLS, COLS, 0), (C.c_size_t * 3)(18, 18, 18)
        self.sps, self.dps = (C.c_void_p * 6)(*list(self.sp) * 2), (C.c_void_p * 6)(*list(self.dp) * 2)


def entries(a):
    one = (a.sp, a.ss, ROWS, COLS, 8, 3, 1, a.dp, a.ds, 7, 9, 10, 2, 2)
    two = (a.sps, a.ss, ROWS, COLS, 8, 3, 1, a.dps, a.ds, 7, 9, 10, 2, 2)
    return {
        "w2x_render_yuv_sited": ("renderYuvResized", one + (1, 0, 0), None),
        "w2x_render_sequence_yuv_sited": ("renderSequenceYuvResized", two + (2, 1, 0, 1), 14),
    }


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_c_entry_without_a_device(pkg, name):
    L, eng, a = pkg.lib(), pkg.Img2Img(), Args()
    method, args, count_at = entries(a)[name]
    fn = getattr(L, name)
    assert fn(None, *args) == 0 and eng.messages == []                       # a null engine
    assert fn(eng._h, *args) == 0                                             # never loaded: the engine's own refusal, one message that names the C++ method
    assert len(eng.messages) == 1 and eng.messages[0][0] == 1 and eng.messages[0][1].startswith(f"[{method}@"), eng.messages
    assert "before a successful load" in eng.messages[0][1]
    for bad in (2, -1, 99):                                                   # an unknown filter
        del eng.messages[:]
        assert fn(None, *args[:-1], bad) == 0 and eng.messages == []
        assert fn(eng._h, *args[:-1], bad) == 0
        assert eng.messages == [(1, f"[{name}@0] Unknown resize filter {bad}.")]
    for at in LAYOUT_AT:                                                      # layouts -1 and 4, on either side
        for bad in (-1, 4):
            del eng.messages[:]
            wrong = args[:at] + (bad,) + args[at + 1:]
            assert fn(None, *wrong) == 0 and eng.messages == []
            assert fn(eng._h, *wrong) == 0
            assert eng.messages == [(1, f"[{name}@0] Unknown YUV layout {bad}.")]
    for at in SITING_AT:                                                      # sitings -1 and 3: the engine's to refuse (yuv_check; its wording is pinned on a
        for bad in (-1, 3):                                                   # loaded engine by tests/test_gpu_yuv_siting.py) - here the missing load comes first
            del eng.messages[:]
            wrong = args[:at] + (bad,) + args[at + 1:]
            assert fn(None, *wrong) == 0 and eng.messages == []
            assert fn(eng._h, *wrong) == 0
            assert len(eng.messages) == 1 and eng.messages[0][1].startswith(f"[{method}@") and "before a successful load" in eng.messages[0][1], eng.messages
    if count_at is not None:
        del eng.messages[:]
        neg = args[:count_at] + (-1,) + args[count_at + 1:]                   # a negative count and null arrays: 0, no message
        assert fn(eng._h, *neg) == 0 and eng.messages == []
        for at in (0, 7):                                                     # the two arrays of plane pointers
            assert isinstance(args[at], C.Array) and args[at]._type_ is C.c_void_p
            null = args[:at] + (None,) + args[at + 1:]
            assert fn(eng._h, *null) == 0 and eng.messages == []
    eng.close()


# ---- 6. the wrapper
@pytest.fixture(scope="module")
def generator(pkg):
    spec = importlib.util.spec_from_file_location("make_binding_calls", os.path.join(ROOT, "tests", "golden", "make_binding_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_wrapper_left_is_the_call_without_the_keyword(generator):
    nvs = lambda c, n: [c.yuv(f"frame{k}", 4, 6, layout="nv12") for k in range(n)]
    calls = {
        "render_yuv": lambda c, **k: c.e.render_yuv(*c.yuv("src", 4, 6), **k),
        "render_yuv/layout": lambda c, **k: c.e.render_yuv(c.yuv("src", 4, 6, layout="nv12"), layout="nv12", out_layout="i444", out_bits=10, **k),
        "render_sequence_yuv": lambda c, **k: c.e.render_sequence_yuv([c.yuv(f"frame{i}", 4, 6) for i in range(2)], **k),
        "render_sequence_yuv/layout": lambda c, **k: c.e.render_sequence_yuv(nvs(c, 2), layout="nv12", **k),
        "render_yuv_layout_resized": lambda c, **k: c.e.render_yuv_layout_resized(c.yuv("src", 4, 6), (7, 9), out_layout="i422", filter="bilinear", **k),
        "render_sequence_yuv_layout_resized": lambda c, **k: c.e.render_sequence_yuv_layout_resized(nvs(c, 2), (7, 9), layout="nv12", **k),
    }
    cases = []
    for name, fn in calls.items():
        cases.append((name + "|plain", True, 1, lambda c, fn=fn: fn(c)))
        cases.append((name + "|left", True, 1, lambda c, fn=fn: fn(c, siting="left")))
        cases.append((name + "|left,left", True, 1, lambda c, fn=fn: fn(c, siting="left", out_siting="left")))
    logs = generator.generate(scenarios=cases)["scenarios"]
    for name in calls:
        plain = logs[name + "|plain"]
        assert plain["calls"] and not plain["raised"], plain
        assert all("sited" not in c[0] for c in plain["calls"])
        assert logs[name + "|left"] == plain and logs[name + "|left,left"] == plain, name


def test_wrapper_other_sitings_reach_the_sited_entries(generator):
    nvs = lambda c, n: [c.yuv(f"frame{k}", 4, 6, layout="nv12") for k in range(n)]
    cases = [
        ("one/center", True, 1, lambda c: c.e.render_yuv(*c.yuv("src", 4, 6), siting="center")),
        ("one/center_to_left_layouts", True, 1, lambda c: c.e.render_yuv(c.yuv("src", 4, 6, layout="nv12"), layout="nv12", out_layout="i444", out_bits=10,
                                                                         siting="center", out_siting="left", matrix="bt2020", full_range=True)),
        ("one/out_only", True, 1, lambda c: c.e.render_yuv(*c.yuv("src", 4, 6), out_siting="topleft")),
        ("resized/topleft", True, 1, lambda c: c.e.render_yuv_layout_resized(c.yuv("src", 4, 6), (7, 9), out_layout="i422", filter="bilinear", siting="topleft")),
        ("seq/center", True, 1, lambda c: c.e.render_sequence_yuv(nvs(c, 2), layout="nv12", siting="center")),
        ("seq_resized/left_to_topleft", True, 1, lambda c: c.e.render_sequence_yuv_layout_resized(nvs(c, 2), (7, 9), layout="nv12", out_layout="i420", filter="bilinear",
                                                                                                  out_siting="topleft")),
    ]
    logs = generator.generate(scenarios=cases)["scenarios"]

    def only_call(name):
        assert len(logs[name]["calls"]) == 1 and not logs[name]["raised"], logs[name]
        return logs[name]["calls"][0]

    def at(prefix, names="yuv"):
        got = [[f"{prefix}.{n}", 0] for n in names]
        return got + [None] * (3 - len(got))

    allocs = lambda *ks: [[f"alloc{k}", 0] for k in ks] + [None] * (3 - len(ks))
    NV = ("y", "uv")
    # engine, planes, steps, rows, cols, bits, layout, siting, destination planes, steps, rows, cols, bits, layout, siting, matrix, range, filter
    assert only_call("one/center") == ["w2x_render_yuv_sited", ["engine0", at("src"), [6, 3, 3], 4, 6, 8, 0, 1, allocs(0, 1, 2), [12, 6, 6], 8, 12, 8, 0, 1, 1, 0, 0]]
    assert only_call("one/center_to_left_layouts") == ["w2x_render_yuv_sited", ["engine0", at("src", NV), [6, 6, 0], 4, 6, 8, 3, 1, allocs(0, 1, 2), [24, 24, 24], 8, 12, 10, 2, 0,
                                                                                2, 1, 0]]
    assert only_call("one/out_only")[1][6:8] == [0, 0] and only_call("one/out_only")[1][13:15] == [0, 2]
    assert only_call("resized/topleft") == ["w2x_render_yuv_sited", ["engine0", at("src"), [6, 3, 3], 4, 6, 8, 0, 2, allocs(0, 1, 2), [9, 5, 5], 7, 9, 8, 1, 2, 1, 0, 1]]
    # engine, planes of every frame, steps, rows, cols, bits, layout, siting, destination planes, steps, rows, cols, bits, layout, siting, count, matrix, range, filter
    assert only_call("seq/center") == ["w2x_render_sequence_yuv_sited", ["engine0", at("frame0", NV) + at("frame1", NV), [6, 6, 0], 4, 6, 8, 3, 1,
                                                                         allocs(0, 1) + allocs(2, 3), [12, 12, 0], 8, 12, 8, 3, 1, 2, 1, 0, 0]]
    assert only_call("seq_resized/left_to_topleft") == ["w2x_render_sequence_yuv_sited", ["engine0", at("frame0", NV) + at("frame1", NV), [6, 6, 0], 4, 6, 8, 3, 0,
                                                                                          allocs(0, 1, 2) + allocs(3, 4, 5), [9, 5, 5], 7, 9, 8, 0, 2, 2, 1, 0, 1]]


def test_wrapper_unknown_sitings_raise_before_any_call(generator):
    cases = [
        ("one", True, 1, lambda c: c.e.render_yuv(*c.yuv("src", 4, 6), siting="bottom")),
        ("one_out", True, 1, lambda c: c.e.render_yuv(*c.yuv("src", 4, 6), out_siting="centre")),
        ("seq", True, 1, lambda c: c.e.render_sequence_yuv([c.yuv("frame0", 4, 6)], siting=1)),
        ("resized", True, 1, lambda c: c.e.render_yuv_layout_resized(c.yuv("src", 4, 6), (7, 9), siting="top-left")),
        ("seq_resized", True, 1, lambda c: c.e.render_sequence_yuv_layout_resized([c.yuv("frame0", 4, 6)], (7, 9), out_siting="LEFT")),
    ]
    logs = generator.generate(scenarios=cases)["scenarios"]
    for name, log in logs.items():
        assert log["raised"] and log["raised"][0] == "ValueError" and "siting must be one of" in log["raised"][1], (name, log)
        assert log["calls"] == [] and log["host_buffers"] == {"handed_out": 0, "all_freed": True}, (name, log)


# ---- 7. the command line (the parse only: see the module's docstring)
W2X = os.path.join(ROOT, "waifu2x-tensorrt_amd", "w2x")
BASE = ["--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "2", "--tileSize", "64"]


def w2x(*args):
    return subprocess.run([W2X, *args], capture_output=True, text=True)


def test_cli_chroma_loc(pkg, tmp_path):
    clip = tmp_path / "clip.mkv"
    clip.write_bytes(b"")
    r = w2x(*BASE, "render", "-i", str(clip), "--colorspace", "bt2020", "--print-config")
    assert r.returncode == 0 and json.loads(r.stdout)["chroma_loc"] is None
    for name in ("left", "center", "topleft"):
        r = w2x(*BASE, "render", "-i", str(clip), "--colorspace", "bt2020", "--chroma-loc", name.upper(), "--print-config")
        assert r.returncode == 0, r.stderr
        assert json.loads(r.stdout)["chroma_loc"] == name
    r = w2x(*BASE, "render", "-i", str(clip), "--chroma-loc", "topleft", "--print-config")
    assert r.returncode != 0 and "--chroma-loc: needs --colorspace" in r.stderr
    r = w2x(*BASE, "render", "-i", str(clip), "--colorspace", "bt709", "--chroma-loc", "bottom", "--print-config")
    assert r.returncode != 0 and "--chroma-loc" in r.stderr
    r = w2x(*BASE, "build", "--chroma-loc", "center", "--print-config")
    assert r.returncode != 0 and "--chroma-loc: only with render" in r.stderr
    r = w2x("--help")
    assert r.returncode == 0 and "--chroma-loc" in r.stdout and "topleft" in r.stdout
