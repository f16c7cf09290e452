"""The two binding layers every caller goes through, without a device.
1. engine.py: the log of what each frame-taking wrapper method passes to the C ABI (tests/golden/make_binding_calls.py: a recording stub in place of the
   library) equals tests/golden/binding_calls.json.
2. c_api.cpp: every frame entry of include/w2x/c_api.h through raw ctypes - a null engine, a never-loaded engine (the message names the C++ method the
   entry calls), unknown filters, and the sequence entries' count / array checks; w2x_yuv_plane_sizes is the I420 case of w2x_yuv_layout_plane_sizes."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def header_entries(pattern):
    hdr = open(os.path.join(ROOT, "include", "w2x", "c_api.h")).read()
    return {n for n in re.findall(r"\b(w2x_[a-z0-9_]+)\s*\(", hdr[hdr.index('extern "C"'):]) if re.fullmatch(pattern, n)}


@pytest.fixture(scope="module")
def generator(pkg):
    spec = importlib.util.spec_from_file_location("make_binding_calls", os.path.join(GOLDEN, "make_binding_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_wrapper_call_log_is_the_recorded_one(pkg, generator):
    import json
    text = open(os.path.join(GOLDEN, "binding_calls.json")).read()
    want, got = json.loads(text), json.loads(generator.dumps(generator.generate()))
    assert got["exported"] == want["exported"]
    for name in want["symbols"]:
        assert got["symbols"].get(name) == want["symbols"][name], name
    assert sorted(got["scenarios"]) == sorted(want["scenarios"])
    for name in want["scenarios"]:
        assert got["scenarios"][name] == want["scenarios"][name], name
    assert generator.dumps(generator.generate()) == text           # and byte for byte, as the generator writes it


def test_call_log_covers_every_frame_entry_of_the_header(generator):
    import json
    log = json.load(open(os.path.join(GOLDEN, "binding_calls.json")))
    called = {c[0] for s in log["scenarios"].values() for c in s["calls"]}
    needed = header_entries(r"w2x_render.*|w2x_shard_compute|w2x_shard_finish|w2x_alpha_bleed.*")
    assert needed and needed <= called, sorted(needed - called)
    # the refusals the wrapper makes itself reach no entry (a pinned YUV sequence looks at its matrix late: its ring is taken and given back)
    refused = [s for n, s in log["scenarios"].items() if "/refuse_" in n]
    assert len(refused) >= 60 and all(s["result"] in (None, False) and {c[0] for c in s["calls"]} <= {"w2x_alloc_host", "w2x_free_host"} for s in refused)
    # every scripted failure on a pinned path gave its page-locked buffers back
    assert all(s["host_buffers"]["all_freed"] for s in log["scenarios"].values())
    assert sum(s["host_buffers"]["handed_out"] > 0 and s["raised"] is not None for s in log["scenarios"].values()) >= 6


def test_a_ring_that_cannot_be_completed_is_given_back(generator):
    """a pinned sequence whose second w2x_alloc_host fails frees the buffer it already took (asserted here, not a scenario of the log)"""
    def second_alloc_fails(method, args, **kw):
        def fn(c):
            c.fail("w2x_alloc_host", 2)
            return getattr(c.e, method)(*args(c), pinned=True, **kw)
        return fn
    cases = [("bgr", True, 1, second_alloc_fails("render_sequence", lambda c: (generator.frames(c, 4),))),
             ("resized", True, 1, second_alloc_fails("render_sequence_resized", lambda c: (generator.frames(c, 4), (7, 9)))),
             ("rgba", True, 1, second_alloc_fails("render_sequence_rgba", lambda c: (generator.frames(c, 4, 4),))),
             ("yuv", True, 1, second_alloc_fails("render_sequence_yuv", lambda c: (generator.yframes(c, 4),)))]
    logs = generator.generate(scenarios=cases)["scenarios"]
    assert sorted(logs) == ["bgr", "resized", "rgba", "yuv"]
    for name, log in logs.items():
        assert log["raised"] == ["W2xError", "w2x_alloc_host failed"], name
        assert [c[0] for c in log["calls"]] == ["w2x_alloc_host", "w2x_alloc_host", "w2x_free_host"], name
        assert log["host_buffers"] == {"handed_out": 1, "all_freed": True}, name


# ---- the C entries.  name -> (C++ method named in the engine's refusal, arguments after the engine, index of `count` or None, takes a filter last)
ROWS, COLS = 4, 6


class Args:
    def __init__(self):
        self.src = np.zeros((ROWS, COLS, 4), np.uint16)
        self.dst = np.zeros((2 * ROWS, 2 * COLS, 4), np.uint16)
        s, d = self.src.ctypes.data, self.dst.ctypes.data
        self.s, self.d = s, d
        self.srcs, self.dsts = (C.c_void_p * 2)(s, s), (C.c_void_p * 2)(d, d)
        self.sp, self.dp = (C.c_void_p * 6)(*[s] * 6), (C.c_void_p * 6)(*[d] * 6)
        self.ss, self.ds = (C.c_size_t * 3)(COLS, COLS // 2, COLS // 2), (C.c_size_t * 3)(2 * COLS, COLS, COLS)
        self.slabs = (C.c_void_p * 2)()


def entries(a):
    r, c, s, d = ROWS, COLS, a.s, a.d
    yuv = (a.sp, a.ss, r, c, 8, a.dp, a.ds, 2 * r, 2 * c, 8)
    yuvl = (a.sp, a.ss, r, c, 8, 0, a.dp, a.ds, 2 * r, 2 * c, 8, 0)
    return {
        "w2x_render": ("render", (s, r, c, c * 3, d, c * 6), None, False),
        "w2x_render16": ("render", (s, r, c, c * 6, d, c * 12), None, False),
        "w2x_render_resized": ("renderResized", (s, r, c, c * 3, d, 7, 9, 27, 0), None, True),
        "w2x_render16_resized": ("renderResized", (s, r, c, c * 6, d, 7, 9, 54, 1), None, True),
        "w2x_render_strip": ("renderStrip", (s, r, c, c * 3, d, c * 6, 0, 2), None, False),
        "w2x_shard_compute": ("shardCompute", (s, r, c, c * 3, 0, 2), None, False),
        "w2x_shard_finish": ("shardFinish", (d, 2 * r, 2 * c, c * 6, 0, 2, a.slabs, None), None, False),
        "w2x_render_sequence": ("renderSequence", (a.srcs, r, c, c * 3, a.dsts, c * 6, 2), 6, False),
        "w2x_render_sequence_resized": ("renderSequenceResized", (a.srcs, r, c, c * 3, a.dsts, 7, 9, 27, 2, 0), 8, True),
        "w2x_render_yuv": ("renderYuv", yuv + (1, 0), None, False),
        "w2x_render_sequence_yuv": ("renderSequenceYuv", yuv + (2, 1, 0), 10, False),
        "w2x_render_yuv_layout": ("renderYuv", yuvl + (1, 0), None, False),
        "w2x_render_sequence_yuv_layout": ("renderSequenceYuv", yuvl + (2, 1, 0), 12, False),
        "w2x_render_yuv_resized": ("renderYuvResized", yuv[:7] + (7, 9, 8, 1, 0, 1), None, True),
        "w2x_render_sequence_yuv_resized": ("renderSequenceYuvResized", yuv[:7] + (7, 9, 8, 2, 1, 0, 0), 10, True),
        "w2x_render_rgba": ("renderRgba", (s, r, c, c * 4, d, c * 8, 0, 0), None, False),
        "w2x_render_rgba_resized": ("renderRgbaResized", (s, r, c, c * 4, d, 7, 9, 36, 2, 1, 0), None, True),
        "w2x_render_sequence_rgba": ("renderSequenceRgba", (a.srcs, r, c, c * 4, a.dsts, c * 8, 2, 0, 0), 6, False),
        "w2x_render_sequence_rgba_resized": ("renderSequenceRgbaResized", (a.srcs, r, c, c * 4, a.dsts, 7, 9, 36, 2, 0, 0, 1), 8, True),
        "w2x_alpha_bleed_device": ("alphaBleed", (s, r, c, c * 4, d, c * 3, 2), None, False),
    }


ENTRY_NAMES = sorted(entries(Args()))


@pytest.fixture()
def raw(pkg):
    """(library, never-loaded engine, arguments); the engine's messages are in eng.messages"""
    eng = pkg.Img2Img()
    yield pkg.lib(), eng, Args()
    eng.close()


def test_the_table_holds_every_engine_frame_entry_of_the_header():
    # w2x_render_sharded takes an array of engines (below); w2x_alpha_bleed is host arithmetic without an engine (tests/test_rgba_host.py)
    assert set(ENTRY_NAMES) | {"w2x_render_sharded", "w2x_alpha_bleed"} == header_entries(r"w2x_render.*|w2x_shard_compute|w2x_shard_finish|w2x_alpha_bleed.*")


@pytest.mark.parametrize("name", ENTRY_NAMES)
def test_c_entry_without_a_device(raw, name):
    L, eng, a = raw
    method, args, count_at, resized = entries(a)[name]
    fn = getattr(L, name)
    assert fn(None, *args) == 0 and eng.messages == []                       # a null engine
    assert fn(eng._h, *args) == 0                                             # never loaded: the engine's own refusal, one message
    assert len(eng.messages) == 1 and eng.messages[0][0] == 1 and eng.messages[0][1].startswith(f"[{method}@"), eng.messages
    if resized:
        for bad in (2, -1, 99):
            del eng.messages[:]
            assert fn(None, *args[:-1], bad) == 0 and eng.messages == []      # the engine comes first: nothing of a null one is looked at
            assert fn(eng._h, *args[:-1], bad) == 0
            assert eng.messages == [(1, f"[{name}@0] Unknown resize filter {bad}.")]
    if count_at is not None:
        # (count == 0 is left out: a loaded engine makes its device current before it looks at the count, which is no clean refusal on a machine without one)
        del eng.messages[:]
        neg = args[:count_at] + (-1,) + args[count_at + 1:]
        assert fn(eng._h, *neg) == 0 and eng.messages == []
        arrays = [i for i, x in enumerate(args) if isinstance(x, C.Array) and x._type_ is C.c_void_p]     # srcs and dsts, or src_planes and dst_planes
        assert len(arrays) == 2
        for at in arrays:
            null = args[:at] + (None,) + args[at + 1:]
            assert fn(eng._h, *null) == 0 and eng.messages == []
        if resized:                                                           # the count and the arrays are looked at before the filter
            assert fn(eng._h, *neg[:-1], 7) == 0 and eng.messages == []


def test_render_sharded_without_a_device(raw, pkg):
    L, eng, a = raw
    other = pkg.Img2Img()
    args = (a.s, ROWS, COLS, COLS * 3, a.d, COLS * 6)
    assert L.w2x_render_sharded(None, 2, *args) == 0
    assert L.w2x_render_sharded((C.c_void_p * 2)(eng._h, other._h), 0, *args) == 0
    assert L.w2x_render_sharded((C.c_void_p * 2)(eng._h, other._h), -1, *args) == 0
    assert L.w2x_render_sharded((C.c_void_p * 2)(eng._h, None), 2, *args) == 0
    assert eng.messages == [] and other.messages == []
    assert L.w2x_render_sharded((C.c_void_p * 2)(eng._h, other._h), 2, *args) == 0
    assert len(eng.messages) == 1 and eng.messages[0][1].startswith("[renderSharded@") and other.messages == []
    other.close()


def test_yuv_plane_sizes_is_the_i420_case_of_the_layout_one(pkg):
    L = pkg.lib()

    def three(rows, cols, bits):
        pr, pc, pb = (C.c_int * 3)(-1, -1, -1), (C.c_int * 3)(-1, -1, -1), (C.c_size_t * 3)(7, 7, 7)
        return L.w2x_yuv_plane_sizes(rows, cols, bits, pr, pc, pb), list(pr), list(pc), list(pb)

    def layout(rows, cols, bits, lay=0):
        n, pr, pc, pb = C.c_int(-1), (C.c_int * 3)(-1, -1, -1), (C.c_int * 3)(-1, -1, -1), (C.c_size_t * 3)(7, 7, 7)
        return L.w2x_yuv_layout_plane_sizes(rows, cols, bits, lay, C.byref(n), pr, pc, pb), list(pr), list(pc), list(pb), n.value

    for rows in (1, 2, 5, 8, 1081):
        for cols in (1, 3, 6, 1920):
            for bits in (8, 10):
                got, want = three(rows, cols, bits), layout(rows, cols, bits)
                assert got == want[:4] and got[0] == 1 and want[4] == 3
                h, w, b = (rows + 1) // 2, (cols + 1) // 2, 1 if bits == 8 else 2
                assert got[1:] == ([rows, h, h], [cols, w, w], [rows * cols * b, h * w * b, h * w * b])
    for bad in ((0, 4, 8), (4, 0, 8), (-1, 4, 8), (4, 4, 9), (4, 4, 16), (4, 4, 0)):      # both refuse, nothing written
        assert three(*bad) == (0, [-1] * 3, [-1] * 3, [7] * 3)
        assert layout(*bad) == (0, [-1] * 3, [-1] * 3, [7] * 3, -1)
    assert L.w2x_yuv_plane_sizes(4, 6, 8, None, None, None) == 1            # any output pointer may be NULL
    pb = (C.c_size_t * 3)()
    assert L.w2x_yuv_plane_sizes(5, 7, 10, None, None, pb) == 1 and list(pb) == [70, 24, 24]
