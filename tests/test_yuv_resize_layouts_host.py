"""Resized YUV frames of every layout without a device: the two C entries of include/w2x/c_api_yuv_resized.h against libw2x.so and engine.YUV_RESIZED_SYMBOLS,
their refusals on a null and on a never-loaded engine (the pattern of tests/test_planar_host.py), the wrapper's own refusals and its marshalling through the
recording stub of tests/golden/make_binding_calls.py."""
import ctypes as C
import importlib
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8, u16 = np.uint8, np.uint16
ENTRIES = {"w2x_render_yuv_layout_resized", "w2x_render_sequence_yuv_layout_resized"}


def declared(header):
    hdr = open(os.path.join(ROOT, "include", "w2x", header)).read()
    return set(re.findall(r"\b(w2x_[a-z0-9_]+)\s*\(", hdr[hdr.index('extern "C"'):]))


@pytest.fixture(scope="module")
def engine_module(pkg):
    return importlib.import_module("waifu2x-tensorrt_amd.engine")


# ---- the header, the library and the wrapper's table name the same two entries, and neither is one of c_api.h's
def test_header_library_and_table_agree(pkg, engine_module):
    names = declared("c_api_yuv_resized.h")
    assert names == ENTRIES == set(engine_module.YUV_RESIZED_SYMBOLS) == set(pkg.YUV_RESIZED_SYMBOLS)
    raw = C.CDLL(pkg.lib_path)                                      # a handle of its own: what the file exports, not what lib() declared
    for n in names:
        assert hasattr(raw, n), f"libw2x.so does not export {n}"
    exported = subprocess.run(["nm", "-D", "--defined-only", pkg.lib_path], capture_output=True, text=True) if shutil.which("nm") else None
    if exported is not None and exported.returncode == 0:          # the other way round, where binutils is there: no such entry the header does not declare
        assert {s for s in re.findall(r"\bT (w2x_[a-z0-9_]+)", exported.stdout) if s.endswith("yuv_layout_resized")} == names
    for other in ("c_api.h", "c_api_gray.h", "c_api_planar.h", "c_api_rgbap.h"):
        assert not names & declared(other), other
    for table in ("SYMBOLS", "EXPORTED_SYMBOLS", "GRAY_SYMBOLS", "PLANAR_SYMBOLS", "RGBAP_SYMBOLS"):
        assert not names & set(getattr(engine_module, table)), table
    L = pkg.lib()
    for n, (restype, argtypes) in engine_module.YUV_RESIZED_SYMBOLS.items():
        assert getattr(L, n).restype is restype and list(getattr(L, n).argtypes) == argtypes, n
    hdr = open(os.path.join(ROOT, "include", "w2x", "c_api_yuv_resized.h")).read()
    assert '#include "c_api.h"' in hdr
    # the argument lists: those of the _yuv_layout entries and one int more, the filter
    for n in names:
        plain = engine_module.SYMBOLS[n[:-len("_resized")]]
        assert engine_module.YUV_RESIZED_SYMBOLS[n] == (plain[0], plain[1] + [C.c_int])
    for method in ("render_yuv_layout_resized", "render_sequence_yuv_layout_resized"):
        assert callable(getattr(pkg.Img2Img, method))


# ---- the C entries.  name -> (C++ method named in the engine's refusal, arguments after the engine, index of `count` or None)
ROWS, COLS = 4, 6
LAYOUT_AT = (5, 11)                                                  # src_layout, dst_layout


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
    one = (a.sp, a.ss, ROWS, COLS, 8, 3, a.dp, a.ds, 7, 9, 10, 2)
    two = (a.sps, a.ss, ROWS, COLS, 8, 3, a.dps, a.ds, 7, 9, 10, 2)
    return {
        "w2x_render_yuv_layout_resized": ("renderYuvResized", one + (1, 0, 0), None),
        "w2x_render_sequence_yuv_layout_resized": ("renderSequenceYuvResized", two + (2, 1, 0, 1), 12),
    }


ENTRY_NAMES = sorted(entries(Args()))


def test_the_table_holds_every_entry_of_the_header():
    assert set(ENTRY_NAMES) == declared("c_api_yuv_resized.h") == ENTRIES


@pytest.mark.parametrize("name", ENTRY_NAMES)
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
    if count_at is not None:
        del eng.messages[:]
        neg = args[:count_at] + (-1,) + args[count_at + 1:]                   # a negative count and null arrays: 0, no message
        assert fn(eng._h, *neg) == 0 and eng.messages == []
        for at in (0, 6):                                                     # the two arrays of plane pointers
            assert isinstance(args[at], C.Array) and args[at]._type_ is C.c_void_p
            null = args[:at] + (None,) + args[at + 1:]
            assert fn(eng._h, *null) == 0 and eng.messages == []
        none = args[:count_at] + (0,) + args[count_at + 1:]                   # an empty sequence: refused on this engine as the neighbouring entry refuses it
        assert fn(eng._h, None, *none[1:6], None, *none[7:]) == 0
        assert L.w2x_render_sequence_yuv_layout(eng._h, None, *none[1:6], None, *none[7:-1]) == 0
        assert len(eng.messages) == 2 and eng.messages[0][1].split("] ")[1] == eng.messages[1][1].split("] ")[1]
        del eng.messages[:]
        assert fn(eng._h, *neg[:-1], 7) == 0 and eng.messages == []           # the count and the arrays are looked at before the filter
    eng.close()


# ---- the wrapper: refusals that reach no entry, and what the accepted calls hand to the C ABI
@pytest.fixture(scope="module")
def generator(pkg):
    spec = importlib.util.spec_from_file_location("make_binding_calls", os.path.join(ROOT, "tests", "golden", "make_binding_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_wrapper_refusals_reach_no_entry(generator):
    z = np.zeros
    one = lambda c, *a, **k: c.e.render_yuv_layout_resized(*a, **k)
    seq = lambda c, *a, **k: c.e.render_sequence_yuv_layout_resized(*a, **k)
    cases = [
        ("i420_planes_as_i444", True, 1, lambda c: one(c, c.yuv("src", 4, 6), (7, 9), layout="i444")),
        ("i444_planes_as_i422", True, 1, lambda c: one(c, c.yuv("src", 4, 6, layout="i444"), (7, 9), layout="i422")),
        ("i422_planes_as_i420", True, 1, lambda c: one(c, c.yuv("src", 4, 6, layout="i422"), (7, 9))),
        ("nv12_planes_as_i420", True, 1, lambda c: one(c, c.yuv("src", 4, 6, layout="nv12"), (7, 9), layout="i420")),
        ("three_planes_as_nv12", True, 1, lambda c: one(c, c.yuv("src", 4, 6), (7, 9), layout="nv12")),
        ("nv12_odd_width_uv_short", True, 1, lambda c: one(c, (z((4, 7), u8), z((2, 7), u8)), (7, 9), layout="nv12")),
        ("positional_plane", True, 1, lambda c: one(c, z((4, 6), u8), (7, 9))),
        ("float_planes", True, 1, lambda c: one(c, (z((4, 6), np.float32),) * 3, (7, 9), layout="i444")),
        ("mixed_types", True, 1, lambda c: one(c, (z((4, 6), u8), z((4, 6), u16), z((4, 6), u8)), (7, 9), layout="i444")),
        ("unknown_layout", True, 1, lambda c: one(c, c.yuv("src", 4, 6), (7, 9), layout="yuv411p")),
        ("unknown_out_layout", True, 1, lambda c: one(c, c.yuv("src", 4, 6), (7, 9), out_layout="p016")),
        ("filter", True, 1, lambda c: one(c, c.yuv("src", 4, 6), (7, 9), filter="lanczos")),
        ("matrix", True, 1, lambda c: one(c, c.yuv("src", 4, 6), (7, 9), matrix="smpte240m")),
        ("dst_of_another_layout", True, 1, lambda c: one(c, c.yuv("src", 4, 6), (7, 9), out_layout="i444", dst=c.yuv("dst", 7, 9, layout="i422", out=True))),
        ("dst_dtype", True, 1, lambda c: one(c, c.yuv("src", 4, 6), (7, 9), out_bits=10, dst=c.yuv("dst", 7, 9, out=True))),
        ("dst_size", True, 1, lambda c: one(c, c.yuv("src", 4, 6), (7, 9), dst=c.yuv("dst", 7, 10, out=True))),
        ("seq_unknown_layout", True, 1, lambda c: seq(c, [c.yuv("frame0", 4, 6)], (7, 9), layout="i411")),
        ("seq_layouts_differ", True, 1, lambda c: seq(c, [c.yuv("frame0", 4, 6, layout="nv12"), c.yuv("frame1", 4, 6)], (7, 9), layout="nv12")),
        ("seq_first_frame_of_another_layout", True, 1, lambda c: seq(c, [c.yuv("frame0", 4, 6)] * 2, (7, 9), layout="i422")),
        ("seq_sizes_differ", True, 1, lambda c: seq(c, [c.yuv("frame0", 4, 6, layout="i444"), c.yuv("frame1", 4, 8, layout="i444")], (7, 9), layout="i444")),
        ("seq_filter", True, 1, lambda c: seq(c, [c.yuv("frame0", 4, 6)], (7, 9), filter="nearest")),
    ]
    logs = generator.generate(scenarios=cases)["scenarios"]
    for name, log in logs.items():
        assert log["raised"] and log["raised"][0] == "ValueError", (name, log)
        assert log["calls"] == [] and log["host_buffers"] == {"handed_out": 0, "all_freed": True}, (name, log)


def test_wrapper_marshalling(generator):
    one = lambda c, *a, **k: c.e.render_yuv_layout_resized(*a, **k)
    seq = lambda c, *a, **k: c.e.render_sequence_yuv_layout_resized(*a, **k)
    nvs = lambda c, n: [c.yuv(f"frame{k}", 4, 6, layout="nv12") for k in range(n)]
    cases = [
        ("one/defaults", True, 1, lambda c: one(c, c.yuv("src", 4, 6), (7, 9))),
        ("one/nv12_to_i444_10", True, 1, lambda c: one(c, c.yuv("src", 4, 6, layout="nv12"), (7, 9), layout="nv12", out_layout="i444", out_bits=10, matrix="bt2020",
                                                     full_range=True, filter="bilinear")),
        ("one/i422_10_padded_to_nv12", True, 1, lambda c: one(c, c.yuv("src", 4, 6, u16, "i422", pad=3), (7, 9), layout="i422", out_layout="nv12")),
        ("one/dst_nv12", True, 1, lambda c: one(c, c.yuv("src", 4, 6, layout="i444"), (7, 9), layout="i444", out_layout="nv12", matrix="bt601",
                                              dst=c.yuv("dst", 7, 9, layout="nv12", out=True))),
        ("one/fail", True, 1, lambda c: (c.fail("w2x_render_yuv_layout_resized", say=b"[renderYuvResized@7] scripted refusal."), one(c, c.yuv("src", 4, 6), (7, 9)))[1]),
        ("one/never_loaded", False, 1, lambda c: one(c, c.yuv("src", 4, 6), (7, 9), dst=c.yuv("dst", 7, 9, out=True))),
        ("one/empty_target", True, 1, lambda c: one(c, c.yuv("src", 4, 6), (0, 9), out_layout="i444")),
        ("seq/empty", True, 1, lambda c: seq(c, [], (7, 9), layout="nv12")),
        ("seq/nv12_to_i422", True, 1, lambda c: seq(c, nvs(c, 2), (7, 9), layout="nv12", out_layout="i422", out_bits=10, filter="bilinear")),
        ("seq/i444_to_nv12", True, 1, lambda c: seq(c, [c.yuv(f"frame{k}", 4, 6, layout="i444") for k in range(2)], (7, 9), layout="i444", out_layout="nv12")),
        ("seq/pinned", True, 1, lambda c: seq(c, nvs(c, 4), (7, 9), layout="nv12", pinned=True)),
        ("seq/fail_pinned_second_piece", True, 1, lambda c: (c.fail("w2x_render_sequence_yuv_layout_resized", 2), seq(c, nvs(c, 4), (7, 9), layout="nv12", pinned=True))[1]),
    ]
    logs = generator.generate(scenarios=cases)["scenarios"]
    assert all(log["host_buffers"]["all_freed"] for log in logs.values())

    def only_call(name):
        assert len(logs[name]["calls"]) == 1, logs[name]
        return logs[name]["calls"][0]

    def at(prefix, names="yuv", off=0):
        got = [[f"{prefix}.{n}", off] for n in names]
        return got + [None] * (3 - len(got))

    allocs = lambda *ks: [[f"alloc{k}", 0] for k in ks] + [None] * (3 - len(ks))
    NV = ("y", "uv")
    # engine, planes, steps, rows, cols, bits, layout, destination planes, steps, rows, cols, bits, layout, matrix, range, filter
    assert only_call("one/defaults") == ["w2x_render_yuv_layout_resized", ["engine0", at("src"), [6, 3, 3], 4, 6, 8, 0, allocs(0, 1, 2), [9, 5, 5], 7, 9, 8, 0, 1, 0, 0]]
    assert logs["one/defaults"]["allocated"] == [[[7, 9], "uint8"], [[4, 5], "uint8"], [[4, 5], "uint8"]]
    assert [p["shape"] for p in logs["one/defaults"]["result"]] == [[7, 9], [4, 5], [4, 5]]
    assert only_call("one/nv12_to_i444_10") == ["w2x_render_yuv_layout_resized", ["engine0", at("src", NV), [6, 6, 0], 4, 6, 8, 3, allocs(0, 1, 2), [18, 18, 18], 7, 9, 10, 2, 2, 1, 1]]
    assert logs["one/nv12_to_i444_10"]["allocated"] == [[[7, 9], "uint16"]] * 3
    # an NV12 destination: the third plane null with step 0
    assert only_call("one/i422_10_padded_to_nv12") == ["w2x_render_yuv_layout_resized", ["engine0", at("src"), [18, 12, 12], 4, 6, 10, 1, allocs(0, 1), [18, 20, 0], 7, 9, 10, 3, 1, 0, 0]]
    assert logs["one/i422_10_padded_to_nv12"]["allocated"] == [[[7, 9], "uint16"], [[4, 10], "uint16"]]
    assert only_call("one/dst_nv12") == ["w2x_render_yuv_layout_resized", ["engine0", at("src"), [6, 6, 6], 4, 6, 8, 2, at("dst", NV), [9, 10, 0], 7, 9, 8, 3, 0, 0, 0]]
    assert logs["one/dst_nv12"]["result"] is True
    assert logs["one/fail"]["raised"] == ["W2xError", "[renderYuvResized@7] scripted refusal."]
    assert only_call("one/never_loaded")[0] == "w2x_render_yuv_layout_resized"          # goes to the library, which refuses the call
    empty = only_call("one/empty_target")                                               # (an empty target: null destination planes, refused by the library)
    assert empty[0] == "w2x_render_yuv_layout_resized" and empty[1][7] == [None, None, None] and empty[1][9:] == [0, 9, 8, 2, 1, 0, 0]
    assert logs["seq/empty"]["calls"] == [] and logs["seq/empty"]["result"] == []
    # engine, planes of every frame, steps, rows, cols, bits, layout, destination planes of every frame, steps, rows, cols, bits, layout, count, matrix, range, filter
    assert only_call("seq/nv12_to_i422") == ["w2x_render_sequence_yuv_layout_resized", ["engine0", at("frame0", NV) + at("frame1", NV), [6, 6, 0], 4, 6, 8, 3,
                                                                                        allocs(0, 1, 2) + allocs(3, 4, 5), [18, 10, 10], 7, 9, 10, 1, 2, 1, 0, 1]]
    assert only_call("seq/i444_to_nv12") == ["w2x_render_sequence_yuv_layout_resized", ["engine0", at("frame0") + at("frame1"), [6, 6, 6], 4, 6, 8, 2,
                                                                                        allocs(0, 1) + allocs(2, 3), [9, 10, 0], 7, 9, 8, 3, 2, 1, 0, 0]]
    # a pinned sequence of four: a ring of three page-locked blocks (Y and UV of 7 x 9: 63 + 40 bytes), two pieces (3 + 1), copies returned, every block given back
    calls = logs["seq/pinned"]["calls"]
    assert [c[0] for c in calls] == ["w2x_alloc_host"] * 3 + ["w2x_render_sequence_yuv_layout_resized"] * 2 + ["w2x_free_host"] * 3
    assert [c[1][1] for c in calls[:3]] == [103] * 3
    assert calls[3][1][7] == [x for k in range(3) for x in ([f"host{k}", 0], [f"host{k}", 63], None)] and calls[3][1][8:] == [[9, 10, 0], 7, 9, 8, 3, 3, 1, 0, 0]
    assert calls[4][1][1] == at("frame3", NV) and calls[4][1][7] == [["host0", 0], ["host0", 63], None] and calls[4][1][13] == 1
    assert logs["seq/pinned"]["host_buffers"] == {"handed_out": 3, "all_freed": True} and len(logs["seq/pinned"]["result"]) == 4
    log = logs["seq/fail_pinned_second_piece"]
    assert log["raised"] == ["W2xError", "render_sequence_yuv_layout_resized failed"] and log["host_buffers"] == {"handed_out": 3, "all_freed": True}
