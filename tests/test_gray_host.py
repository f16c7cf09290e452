"""Gray frames without a device: the C entries of include/w2x/c_api_gray.h against libw2x.so and engine.GRAY_SYMBOLS, their refusals on a null and on a
never-loaded engine (the pattern of tests/test_binding_calls.py part 2), the wrapper's own refusals and its marshalling through the recording stub of
tests/golden/make_binding_calls.py, and --gray on the command line (--print-config stops after parsing)."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W2X = os.path.join(ROOT, "waifu2x-tensorrt_amd", "w2x")
BASE = ["--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "2", "--tileSize", "64"]
u8, u16 = np.uint8, np.uint16


def declared(header):
    hdr = open(os.path.join(ROOT, "include", "w2x", header)).read()
    return set(re.findall(r"\b(w2x_[a-z0-9_]+)\s*\(", hdr[hdr.index('extern "C"'):]))


@pytest.fixture(scope="module")
def engine_module(pkg):
    import importlib
    return importlib.import_module("waifu2x-tensorrt_amd.engine")


# ---- the header, the library and the wrapper's table name the same entries, and none of them is one of c_api.h's
def test_header_library_and_table_agree(pkg, engine_module):
    names = declared("c_api_gray.h")
    assert names == {"w2x_render_gray", "w2x_render_gray16", "w2x_render_gray_resized", "w2x_render_gray16_resized", "w2x_render_sequence_gray",
                     "w2x_render_sequence_gray_resized"}
    assert names == set(engine_module.GRAY_SYMBOLS)
    raw = C.CDLL(pkg.lib_path)                                      # a handle of its own: what the file exports, not what lib() declared
    for n in names:
        assert hasattr(raw, n), f"libw2x.so does not export {n}"
    import shutil
    exported = subprocess.run(["nm", "-D", "--defined-only", pkg.lib_path], capture_output=True, text=True) if shutil.which("nm") else None
    if exported is not None and exported.returncode == 0:          # the other way round, where binutils is there: no gray entry the header does not declare
        assert {s for s in re.findall(r"\bT (w2x_[a-z0-9_]+)", exported.stdout) if "gray" in s} == names
    assert not names & declared("c_api.h") and not names & set(engine_module.EXPORTED_SYMBOLS) and not names & set(engine_module.SYMBOLS)
    L = pkg.lib()
    for n, (restype, argtypes) in engine_module.GRAY_SYMBOLS.items():
        assert getattr(L, n).restype is restype and list(getattr(L, n).argtypes) == argtypes, n
    hdr = open(os.path.join(ROOT, "include", "w2x", "c_api_gray.h")).read()
    assert '#include "c_api.h"' in hdr


# ---- the C entries.  name -> (C++ method named in the engine's refusal, arguments after the engine, index of `count` or None, takes a filter last)
ROWS, COLS = 4, 6


class Args:
    def __init__(self):
        self.src = np.zeros((ROWS, COLS), u16)
        self.dst = np.zeros((2 * ROWS, 2 * COLS), u16)
        self.s, self.d = self.src.ctypes.data, self.dst.ctypes.data
        self.srcs, self.dsts = (C.c_void_p * 2)(self.s, self.s), (C.c_void_p * 2)(self.d, self.d)


def entries(a):
    r, c, s, d = ROWS, COLS, a.s, a.d
    return {
        "w2x_render_gray": ("renderGray", (s, r, c, c, d, 2 * c), None, False),
        "w2x_render_gray16": ("renderGray", (s, r, c, 2 * c, d, 4 * c), None, False),
        "w2x_render_gray_resized": ("renderGrayResized", (s, r, c, c, d, 7, 9, 9, 0), None, True),
        "w2x_render_gray16_resized": ("renderGrayResized", (s, r, c, 2 * c, d, 7, 9, 18, 1), None, True),
        "w2x_render_sequence_gray": ("renderSequenceGray", (a.srcs, r, c, c, a.dsts, 2 * c, 2), 6, False),
        "w2x_render_sequence_gray_resized": ("renderSequenceGrayResized", (a.srcs, r, c, c, a.dsts, 7, 9, 9, 2, 0), 8, True),
    }


ENTRY_NAMES = sorted(entries(Args()))


def test_the_table_holds_every_entry_of_the_header():
    assert set(ENTRY_NAMES) == declared("c_api_gray.h")


@pytest.mark.parametrize("name", ENTRY_NAMES)
def test_c_entry_without_a_device(pkg, name):
    L, eng, a = pkg.lib(), pkg.Img2Img(), Args()
    method, args, count_at, resized = entries(a)[name]
    fn = getattr(L, name)
    assert fn(None, *args) == 0 and eng.messages == []                       # a null engine
    assert fn(eng._h, *args) == 0                                             # never loaded: the engine's own refusal, one message
    assert len(eng.messages) == 1 and eng.messages[0][0] == 1 and eng.messages[0][1].startswith(f"[{method}@"), eng.messages
    assert "before a successful load" in eng.messages[0][1]
    if resized:
        for bad in (2, -1, 99):
            del eng.messages[:]
            assert fn(None, *args[:-1], bad) == 0 and eng.messages == []
            assert fn(eng._h, *args[:-1], bad) == 0
            assert eng.messages == [(1, f"[{name}@0] Unknown resize filter {bad}.")]
    if count_at is not None:
        del eng.messages[:]
        neg = args[:count_at] + (-1,) + args[count_at + 1:]
        assert fn(eng._h, *neg) == 0 and eng.messages == []
        arrays = [i for i, x in enumerate(args) if isinstance(x, C.Array) and x._type_ is C.c_void_p]
        assert len(arrays) == 2
        for at in arrays:
            null = args[:at] + (None,) + args[at + 1:]
            assert fn(eng._h, *null) == 0 and eng.messages == []
        if resized:                                                           # the count and the arrays are looked at before the filter
            assert fn(eng._h, *neg[:-1], 7) == 0 and eng.messages == []
    eng.close()


# ---- the wrapper: refusals that reach no entry, and what the accepted calls hand to the C ABI
@pytest.fixture(scope="module")
def generator(pkg):
    spec = importlib.util.spec_from_file_location("make_binding_calls", os.path.join(ROOT, "tests", "golden", "make_binding_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def plane(c, name="src", r=4, cc=6, dtype=u8, pad=0, out=False):
    return c.arr(name, (r, cc), dtype, pad, out)


def planes(c, n, r=4, cc=6, dtype=u8, pad=0):
    return [plane(c, f"frame{k}", r, cc, dtype, pad) for k in range(n)]


def test_wrapper_refusals_reach_no_entry(generator):
    cases = [
        ("3d", True, 1, lambda c: c.e.render_gray(np.zeros((4, 6, 1), u8))),
        ("3d_resized", True, 1, lambda c: c.e.render_gray_resized(np.zeros((4, 6, 3), u8), (7, 9))),
        ("float", True, 1, lambda c: c.e.render_gray(np.zeros((4, 6), np.float32))),
        ("float_resized", True, 1, lambda c: c.e.render_gray_resized(np.zeros((4, 6), np.float32), (7, 9))),
        ("unpacked", True, 1, lambda c: c.e.render_gray(np.zeros((4, 12), u8)[:, ::2])),
        ("filter", True, 1, lambda c: c.e.render_gray_resized(plane(c), (7, 9), filter="lanczos")),
        ("dst_dtype", True, 1, lambda c: c.e.render_gray(plane(c), plane(c, "dst", 8, 12, u16, out=True))),
        ("dst_size_resized", True, 1, lambda c: c.e.render_gray_resized(plane(c), (7, 9), dst=plane(c, "dst", 7, 10, out=True))),
        ("seq_3d", True, 1, lambda c: c.e.render_sequence_gray([np.zeros((4, 6, 3), u8)] * 2)),
        ("seq_float", True, 1, lambda c: c.e.render_sequence_gray([np.zeros((4, 6), np.float32)] * 2)),
        ("seq_shapes_differ", True, 1, lambda c: c.e.render_sequence_gray([plane(c, "frame0"), plane(c, "frame1", 4, 7)])),
        ("seq_strides_differ", True, 1, lambda c: c.e.render_sequence_gray([plane(c, "frame0"), plane(c, "frame1", pad=2)])),
        ("seq_16bit", True, 1, lambda c: c.e.render_sequence_gray(planes(c, 2, dtype=u16))),
        ("seq_16bit_pinned", True, 1, lambda c: c.e.render_sequence_gray(planes(c, 2, dtype=u16), pinned=True)),
        ("seq_filter", True, 1, lambda c: c.e.render_sequence_gray(planes(c, 2), size=(7, 9), filter="lanczos")),
        ("seq_filter_pinned", True, 1, lambda c: c.e.render_sequence_gray(planes(c, 2), size=(7, 9), filter="lanczos", pinned=True)),
        ("seq_outs_size", True, 1, lambda c: c.e.render_sequence_gray(planes(c, 2), outs=[plane(c, f"out{k}", 8, 11, out=True) for k in range(2)])),
    ]
    logs = generator.generate(scenarios=cases)["scenarios"]
    for name, log in logs.items():
        assert log["raised"] and log["raised"][0] == "ValueError", (name, log)
        assert log["calls"] == [] and log["host_buffers"] == {"handed_out": 0, "all_freed": True}, (name, log)
    # a destination of the wrong size for the plain call: refused with the engine's message, False, no entry
    log = generator.generate(scenarios=[("dst_size", True, 1, lambda c: c.e.render_gray(plane(c), plane(c, "dst", 8, 11, out=True)))])["scenarios"]["dst_size"]
    assert log["result"] is False and log["calls"] == [] and log["messages"] == [[[1, "[renderGray@0] Output image has invalid size: expected 12x8."]]]


def test_wrapper_marshalling(generator):
    cases = [
        ("gray/alloc", True, 1, lambda c: c.e.render_gray(plane(c))),
        ("gray/alloc16_padded", True, 1, lambda c: c.e.render_gray(plane(c, dtype=u16, pad=3))),
        ("gray/dst_padded", True, 1, lambda c: c.e.render_gray(plane(c, pad=2), plane(c, "dst", 8, 12, pad=5, out=True))),
        ("gray/fail_alloc", True, 1, lambda c: (c.fail("w2x_render_gray", say=b"[renderGray@7] scripted refusal."), c.e.render_gray(plane(c)))[1]),
        ("gray/never_loaded", False, 1, lambda c: c.e.render_gray(plane(c), plane(c, "dst", 5, 5, out=True))),
        ("resized/alloc_bilinear", True, 1, lambda c: c.e.render_gray_resized(plane(c, pad=1), (7, 9), "bilinear")),
        ("resized/dst16", True, 1, lambda c: c.e.render_gray_resized(plane(c, dtype=u16), (7, 9), dst=plane(c, "dst", 7, 9, u16, pad=2, out=True))),
        ("resized/empty_target", True, 1, lambda c: c.e.render_gray_resized(plane(c), (0, 9))),
        ("seq/empty", True, 1, lambda c: c.e.render_sequence_gray([])),
        ("seq/alloc", True, 1, lambda c: c.e.render_sequence_gray(planes(c, 3))),
        ("seq/padded_size", True, 1, lambda c: c.e.render_sequence_gray(planes(c, 2, pad=4), size=(7, 9), filter="bilinear")),
        ("seq/outs", True, 1, lambda c: c.e.render_sequence_gray(planes(c, 2), outs=[plane(c, f"out{k}", 8, 12, out=True) for k in range(2)])),
        ("seq/pinned", True, 1, lambda c: c.e.render_sequence_gray(planes(c, 4), pinned=True)),
        ("seq/pinned_size", True, 1, lambda c: c.e.render_sequence_gray(planes(c, 4), size=(7, 9), pinned=True)),
        ("seq/fail_pinned_second_piece", True, 1, lambda c: (c.fail("w2x_render_sequence_gray", 2), c.e.render_sequence_gray(planes(c, 4), pinned=True))[1]),
        ("seq/second_alloc_fails", True, 1, lambda c: (c.fail("w2x_alloc_host", 2), c.e.render_sequence_gray(planes(c, 4), pinned=True))[1]),
    ]
    logs = generator.generate(scenarios=cases)["scenarios"]
    assert all(log["host_buffers"]["all_freed"] for log in logs.values())

    def only_call(name):
        assert len(logs[name]["calls"]) == 1, logs[name]
        return logs[name]["calls"][0]

    # engine, frame, rows, cols, step, dst, dst step
    assert only_call("gray/alloc") == ["w2x_render_gray", ["engine0", ["src", 0], 4, 6, 6, ["alloc0", 0], 12]]
    assert logs["gray/alloc"]["allocated"] == [[[8, 12], "uint8"]] and logs["gray/alloc"]["result"]["shape"] == [8, 12]
    assert only_call("gray/alloc16_padded") == ["w2x_render_gray16", ["engine0", ["src", 0], 4, 6, 18, ["alloc0", 0], 24]]
    assert logs["gray/alloc16_padded"]["result"]["dtype"] == "uint16"
    assert only_call("gray/dst_padded") == ["w2x_render_gray", ["engine0", ["src", 0], 4, 6, 8, ["dst", 0], 17]] and logs["gray/dst_padded"]["result"] is True
    assert logs["gray/fail_alloc"]["raised"] == ["W2xError", "[renderGray@7] scripted refusal."]
    assert only_call("gray/never_loaded")[0] == "w2x_render_gray"           # a dst of any size goes to the library, which refuses the call
    # ..., dst, dst rows, dst cols, dst step, filter
    assert only_call("resized/alloc_bilinear") == ["w2x_render_gray_resized", ["engine0", ["src", 0], 4, 6, 7, ["alloc0", 0], 7, 9, 9, 1]]
    assert only_call("resized/dst16") == ["w2x_render_gray16_resized", ["engine0", ["src", 0], 4, 6, 12, ["dst", 0], 7, 9, 22, 0]]
    empty = only_call("resized/empty_target")                                # (an empty target: a null destination, refused by the library; its step is numpy's)
    assert empty[0] == "w2x_render_gray_resized" and empty[1][:8] == ["engine0", ["src", 0], 4, 6, 6, None, 0, 9] and empty[1][9] == 0
    assert logs["seq/empty"]["calls"] == [] and logs["seq/empty"]["result"] == []
    # engine, frames, rows, cols, step, dsts, dst step, count
    assert only_call("seq/alloc") == ["w2x_render_sequence_gray", ["engine0", [["frame0", 0], ["frame1", 0], ["frame2", 0]], 4, 6, 6, [["alloc0", 0], ["alloc1", 0], ["alloc2", 0]], 12, 3]]
    assert only_call("seq/padded_size") == ["w2x_render_sequence_gray_resized", ["engine0", [["frame0", 0], ["frame1", 0]], 4, 6, 10, [["alloc0", 0], ["alloc1", 0]], 7, 9, 9, 2, 1]]
    assert only_call("seq/outs") == ["w2x_render_sequence_gray", ["engine0", [["frame0", 0], ["frame1", 0]], 4, 6, 6, [["out0", 0], ["out1", 0]], 12, 2]]
    # a pinned sequence of four: a ring of three page-locked buffers, two pieces (3 + 1), copies returned, every buffer given back
    calls = logs["seq/pinned"]["calls"]
    assert [c[0] for c in calls] == ["w2x_alloc_host"] * 3 + ["w2x_render_sequence_gray"] * 2 + ["w2x_free_host"] * 3
    assert [c[1][1] for c in calls[:3]] == [96, 96, 96]
    assert calls[3][1] == ["engine0", [["frame0", 0], ["frame1", 0], ["frame2", 0]], 4, 6, 6, [["host0", 0], ["host1", 0], ["host2", 0]], 12, 3]
    assert calls[4][1] == ["engine0", [["frame3", 0]], 4, 6, 6, [["host0", 0]], 12, 1]
    assert logs["seq/pinned"]["host_buffers"] == {"handed_out": 3, "all_freed": True} and len(logs["seq/pinned"]["result"]) == 4
    assert [c[1][1] for c in logs["seq/pinned_size"]["calls"][:3]] == [63, 63, 63]
    assert logs["seq/pinned_size"]["calls"][3][1][5:] == [[["host0", 0], ["host1", 0], ["host2", 0]], 7, 9, 9, 3, 0]
    log = logs["seq/fail_pinned_second_piece"]
    assert log["raised"] == ["W2xError", "render_sequence_gray failed"] and log["host_buffers"] == {"handed_out": 3, "all_freed": True}
    log = logs["seq/second_alloc_fails"]
    assert log["raised"] == ["W2xError", "w2x_alloc_host failed"]
    assert [c[0] for c in log["calls"]] == ["w2x_alloc_host", "w2x_alloc_host", "w2x_free_host"] and log["host_buffers"] == {"handed_out": 1, "all_freed": True}


# ---- the command line
def w2x(*args):
    return subprocess.run([W2X, *args], capture_output=True, text=True)


def test_gray_option_is_parsed_and_printed(tmp_path):
    png = tmp_path / "page.png"
    png.write_bytes(b"")                                                    # --print-config stops after parsing: the file only has to exist
    r = w2x(*BASE, "render", "-i", str(png), "--gray", "--print-config")
    assert r.returncode == 0, r.stderr
    with_gray = json.loads(r.stdout)
    assert with_gray["gray"] is True
    r = w2x(*BASE, "render", "-i", str(png), "--print-config")
    assert r.returncode == 0, r.stderr
    without = json.loads(r.stdout)
    assert without["gray"] is False
    assert with_gray["outputs"] == without["outputs"] == [str(tmp_path / "page(swin_unet_art)(noise3)(scale4).png")] and with_gray["suffix"] == without["suffix"]
    r = w2x(*BASE, "render", "-i", str(png), "--gray", "--outsize", "300x200", "--deep", "--print-config")
    assert r.returncode == 0 and json.loads(r.stdout)["gray"] is True
    assert json.loads(w2x(*BASE, "build", "--print-config").stdout)["gray"] is False


@pytest.mark.parametrize("extra,command", [((), "build"), (("--colorspace", "bt709"), "render"), (("--devices", "2"), "render")])
def test_gray_parse_errors_name_the_option(tmp_path, extra, command):
    png = tmp_path / "page.png"
    png.write_bytes(b"")
    args = [*BASE, command] + (["-i", str(png)] if command == "render" else []) + ["--gray", *extra, "--print-config"]
    r = w2x(*args)
    assert r.returncode != 0 and r.stderr.startswith("--gray:"), (r.returncode, r.stderr)
    assert r.stdout == ""


def test_help_lists_the_option():
    r = w2x("--help")
    assert r.returncode == 0 and "--gray" in r.stdout
    text = r.stdout[r.stdout.index("--gray"):]
    assert "colour type 4" in text and "RGBA" in text                       # gray + alpha files are said to stay RGBA
