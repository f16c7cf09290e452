"""Planar RGB frames without a device: the C entries of include/w2x/c_api_planar.h against libw2x.so and engine.PLANAR_SYMBOLS, their refusals on a null and
on a never-loaded engine (the pattern of tests/test_gray_host.py), the wrapper's own refusals and its marshalling through the recording stub of
tests/golden/make_binding_calls.py, and --rgb-in / --rgb-out on the command line (--print-config stops after parsing)."""
import ctypes as C
import importlib.util
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W2X = os.path.join(ROOT, "waifu2x-tensorrt_amd", "w2x")
BASE = ["--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "2", "--tileSize", "64"]
FORMATS = ["gbrp", "gbrp10le", "gbrp12le", "gbrp16le", "gbrpf32le"]
u8, u16, f32 = np.uint8, np.uint16, np.float32
RENDER_ENTRIES = {"w2x_render_planar", "w2x_render_planar_resized", "w2x_render_sequence_planar", "w2x_render_sequence_planar_resized"}


def declared(header):
    hdr = open(os.path.join(ROOT, "include", "w2x", header)).read()
    return set(re.findall(r"\b(w2x_[a-z0-9_]+)\s*\(", hdr[hdr.index('extern "C"'):]))


@pytest.fixture(scope="module")
def engine_module(pkg):
    import importlib
    return importlib.import_module("waifu2x-tensorrt_amd.engine")


# ---- the header, the library and the wrapper's table name the same entries, and none of them is one of c_api.h's
def test_header_library_and_table_agree(pkg, engine_module):
    names = declared("c_api_planar.h")
    assert names == RENDER_ENTRIES | {"w2x_planar_plane_bytes"}
    assert names == set(engine_module.PLANAR_SYMBOLS)
    assert not any("gray" in n for n in names)
    raw = C.CDLL(pkg.lib_path)                                      # a handle of its own: what the file exports, not what lib() declared
    for n in names:
        assert hasattr(raw, n), f"libw2x.so does not export {n}"
    exported = subprocess.run(["nm", "-D", "--defined-only", pkg.lib_path], capture_output=True, text=True) if shutil.which("nm") else None
    if exported is not None and exported.returncode == 0:          # the other way round, where binutils is there: no planar entry the header does not declare
        assert {s for s in re.findall(r"\bT (w2x_[a-z0-9_]+)", exported.stdout) if "planar" in s} == names
    assert not names & declared("c_api.h") and not names & declared("c_api_gray.h")
    assert not names & set(engine_module.EXPORTED_SYMBOLS) and not names & set(engine_module.SYMBOLS) and not names & set(engine_module.GRAY_SYMBOLS)
    L = pkg.lib()
    for n, (restype, argtypes) in engine_module.PLANAR_SYMBOLS.items():
        assert getattr(L, n).restype is restype and list(getattr(L, n).argtypes) == argtypes, n
    hdr = open(os.path.join(ROOT, "include", "w2x", "c_api_planar.h")).read()
    assert '#include "c_api.h"' in hdr


def test_plane_bytes(pkg, engine_module):
    L = pkg.lib()
    for bits, bps in ((8, 1), (10, 2), (12, 2), (16, 2), (32, 4)):
        assert L.w2x_planar_plane_bytes(7, 9, bits) == engine_module.planar_plane_bytes(7, 9, bits) == 63 * bps
    for bad in ((7, 9, 9), (7, 9, 0), (7, 9, 24), (7, 9, -8), (0, 9, 8), (7, 0, 8), (-1, 9, 16)):
        assert L.w2x_planar_plane_bytes(*bad) == 0, bad
    assert L.w2x_planar_plane_bytes(40000, 40000, 32) == 6400000000           # a size_t: no 32-bit product


# ---- the C entries.  name -> (C++ method named in the engine's refusal, arguments after the engine, index of `count` or None, takes a filter last)
ROWS, COLS = 4, 6


class Args:
    def __init__(self):
        self.src = np.zeros((3, ROWS, COLS), u16)
        self.dst = np.zeros((3, 2 * ROWS, 2 * COLS), f32)
        self.sp, self.dp = (C.c_void_p * 3)(*[p.ctypes.data for p in self.src]), (C.c_void_p * 3)(*[p.ctypes.data for p in self.dst])
        self.ss, self.ds = (C.c_size_t * 3)(*[2 * COLS] * 3), (C.c_size_t * 3)(*[8 * COLS] * 3)
        self.sps, self.dps = (C.c_void_p * 6)(*list(self.sp) * 2), (C.c_void_p * 6)(*list(self.dp) * 2)


def entries(a):
    r, c = ROWS, COLS
    one = (a.sp, a.ss, r, c, 10, a.dp, a.ds, 2 * r, 2 * c, 32)
    two = (a.sps, a.ss, r, c, 10, a.dps, a.ds, 2 * r, 2 * c, 32)
    return {
        "w2x_render_planar": ("renderPlanar", one, None, False),
        "w2x_render_planar_resized": ("renderPlanarResized", one + (0,), None, True),
        "w2x_render_sequence_planar": ("renderSequencePlanar", two + (2,), 10, False),
        "w2x_render_sequence_planar_resized": ("renderSequencePlanarResized", two + (2, 1), 10, True),
    }


ENTRY_NAMES = sorted(entries(Args()))


def test_the_table_holds_every_render_entry_of_the_header():
    assert set(ENTRY_NAMES) == declared("c_api_planar.h") - {"w2x_planar_plane_bytes"} == RENDER_ENTRIES


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
        for at in (0, 5):                                                     # the two arrays of plane pointers
            assert isinstance(args[at], C.Array) and args[at]._type_ is C.c_void_p
            null = args[:at] + (None,) + args[at + 1:]
            assert fn(eng._h, *null) == 0 and eng.messages == []
        none = args[:count_at] + (0,) + args[count_at + 1:]                   # an empty sequence: what the neighbouring entry answers on this engine
        assert fn(eng._h, None, *none[1:5], None, *none[6:]) == L.w2x_render_sequence(eng._h, None, ROWS, COLS, 3 * COLS, None, 6 * COLS, 0)
        assert [m.split("] ")[1] for _, m in eng.messages[:1]] == [m.split("] ")[1] for _, m in eng.messages[1:]]
        del eng.messages[:]
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


def frame(c, name="src", r=4, cc=6, dtype=u8, pad=0, out=False):
    return tuple(c.arr(f"{name}.{ch}", (r, cc), dtype, pad, out) for ch in "rgb")


def frames(c, n, r=4, cc=6, dtype=u8, pad=0):
    return [frame(c, f"frame{k}", r, cc, dtype, pad) for k in range(n)]


def test_wrapper_refusals_reach_no_entry(generator):
    z = np.zeros
    cases = [
        ("two_planes", True, 1, lambda c: c.e.render_planar((z((4, 6), u8),) * 2)),
        ("interleaved", True, 1, lambda c: c.e.render_planar(z((4, 6, 3), u8))),
        ("3d_planes", True, 1, lambda c: c.e.render_planar((z((4, 6, 1), u8),) * 3)),
        ("float64", True, 1, lambda c: c.e.render_planar((z((4, 6), np.float64),) * 3)),
        ("mixed_types", True, 1, lambda c: c.e.render_planar((z((4, 6), u8), z((4, 6), u16), z((4, 6), u8)))),
        ("mixed_shapes", True, 1, lambda c: c.e.render_planar((z((4, 6), u8), z((4, 7), u8), z((4, 6), u8)))),
        ("unpacked", True, 1, lambda c: c.e.render_planar((z((4, 12), u8)[:, ::2],) * 3)),
        ("bits_10_on_u8", True, 1, lambda c: c.e.render_planar(frame(c), bits=10)),
        ("bits_8_on_u16", True, 1, lambda c: c.e.render_planar(frame(c, dtype=u16), bits=8)),
        ("bits_16_on_float", True, 1, lambda c: c.e.render_planar(frame(c, dtype=f32), bits=16)),
        ("bits_14", True, 1, lambda c: c.e.render_planar(frame(c, dtype=u16), bits=14)),
        ("out_bits_9", True, 1, lambda c: c.e.render_planar(frame(c), out_bits=9)),
        ("order", True, 1, lambda c: c.e.render_planar(frame(c), order="bgra")),
        ("order_twice", True, 1, lambda c: c.e.render_planar(frame(c), order="rrg")),
        ("filter", True, 1, lambda c: c.e.render_planar_resized(frame(c), (7, 9), filter="lanczos")),
        ("dst_dtype", True, 1, lambda c: c.e.render_planar(frame(c), out_bits=10, dst=frame(c, "dst", 8, 12, u8, out=True))),
        ("dst_two", True, 1, lambda c: c.e.render_planar(frame(c), dst=frame(c, "dst", 8, 12, out=True)[:2])),
        ("dst_size_resized", True, 1, lambda c: c.e.render_planar_resized(frame(c), (7, 9), dst=frame(c, "dst", 7, 10, out=True))),
        ("seq_interleaved", True, 1, lambda c: c.e.render_sequence_planar([z((4, 6, 3), u8)] * 2)),
        ("seq_shapes_differ", True, 1, lambda c: c.e.render_sequence_planar([frame(c, "frame0"), frame(c, "frame1", 4, 7)])),
        ("seq_strides_differ", True, 1, lambda c: c.e.render_sequence_planar([frame(c, "frame0"), frame(c, "frame1", pad=2)])),
        ("seq_depths_differ", True, 1, lambda c: c.e.render_sequence_planar([frame(c, "frame0"), frame(c, "frame1", dtype=u16)])),
        ("seq_bits", True, 1, lambda c: c.e.render_sequence_planar(frames(c, 2), bits=12)),
        ("seq_filter_pinned", True, 1, lambda c: c.e.render_sequence_planar(frames(c, 2), (7, 9), filter="lanczos", pinned=True)),
        ("seq_out_bits_pinned", True, 1, lambda c: c.e.render_sequence_planar(frames(c, 2), out_bits=11, pinned=True)),
        ("seq_outs_size", True, 1, lambda c: c.e.render_sequence_planar(frames(c, 2), outs=[frame(c, f"out{k}", 8, 11, out=True) for k in range(2)])),
        ("seq_outs_dtype", True, 1, lambda c: c.e.render_sequence_planar(frames(c, 2), out_bits=32, outs=[frame(c, f"out{k}", 8, 12, u16, out=True) for k in range(2)])),
        ("seq_outs_strides", True, 1, lambda c: c.e.render_sequence_planar(frames(c, 2), outs=[frame(c, "out0", 8, 12, out=True), frame(c, "out1", 8, 12, pad=3, out=True)])),
    ]
    logs = generator.generate(scenarios=cases)["scenarios"]
    for name, log in logs.items():
        assert log["raised"] and log["raised"][0] == "ValueError", (name, log)
        assert log["calls"] == [] and log["host_buffers"] == {"handed_out": 0, "all_freed": True}, (name, log)
    # a destination of the wrong size for the plain call: refused with the engine's message, False, no entry
    log = generator.generate(scenarios=[("dst_size", True, 1, lambda c: c.e.render_planar(frame(c), dst=frame(c, "dst", 8, 11, out=True)))])["scenarios"]["dst_size"]
    assert log["result"] is False and log["calls"] == [] and log["messages"] == [[[1, "[renderPlanar@0] Output image has invalid size: expected 12x8."]]]


def test_wrapper_marshalling(generator):
    cases = [
        ("planar/alloc", True, 1, lambda c: c.e.render_planar(frame(c))),
        ("planar/10_to_float_padded", True, 1, lambda c: c.e.render_planar(frame(c, dtype=u16, pad=3), bits=10, out_bits=32)),
        ("planar/float_to_12", True, 1, lambda c: c.e.render_planar(frame(c, dtype=f32), out_bits=12)),
        ("planar/gbr_dst_padded", True, 1, lambda c: c.e.render_planar(frame(c, pad=2), order="gbr", dst=frame(c, "dst", 8, 12, pad=5, out=True))),
        ("planar/fail_alloc", True, 1, lambda c: (c.fail("w2x_render_planar", say=b"[renderPlanar@7] scripted refusal."), c.e.render_planar(frame(c)))[1]),
        ("planar/never_loaded", False, 1, lambda c: c.e.render_planar(frame(c), dst=frame(c, "dst", 5, 5, out=True))),
        ("resized/alloc_bilinear", True, 1, lambda c: c.e.render_planar_resized(frame(c, pad=1), (7, 9), filter="bilinear")),
        ("resized/dst16", True, 1, lambda c: c.e.render_planar_resized(frame(c, dtype=u16), (7, 9), dst=frame(c, "dst", 7, 9, u16, pad=2, out=True))),
        ("resized/empty_target", True, 1, lambda c: c.e.render_planar_resized(frame(c), (0, 9))),
        ("seq/empty", True, 1, lambda c: c.e.render_sequence_planar([])),
        ("seq/alloc", True, 1, lambda c: c.e.render_sequence_planar(frames(c, 2), out_bits=10)),
        ("seq/gbr_padded_size", True, 1, lambda c: c.e.render_sequence_planar(frames(c, 2, pad=4), (7, 9), order="gbr", filter="bilinear")),
        ("seq/outs", True, 1, lambda c: c.e.render_sequence_planar(frames(c, 2), outs=[frame(c, f"out{k}", 8, 12, pad=1, out=True) for k in range(2)])),
        ("seq/pinned", True, 1, lambda c: c.e.render_sequence_planar(frames(c, 4), out_bits=32, pinned=True)),
        ("seq/fail_pinned_second_piece", True, 1, lambda c: (c.fail("w2x_render_sequence_planar", 2), c.e.render_sequence_planar(frames(c, 4), pinned=True))[1]),
        ("seq/second_alloc_fails", True, 1, lambda c: (c.fail("w2x_alloc_host", 2), c.e.render_sequence_planar(frames(c, 4), pinned=True))[1]),
    ]
    logs = generator.generate(scenarios=cases)["scenarios"]
    assert all(log["host_buffers"]["all_freed"] for log in logs.values())

    def only_call(name):
        assert len(logs[name]["calls"]) == 1, logs[name]
        return logs[name]["calls"][0]

    def at(prefix, order="rgb", off=0):
        return [[f"{prefix}.{ch}", off] for ch in order]

    # engine, planes (R, G, B), steps, rows, cols, bits, destination planes, steps, rows, cols, bits
    assert only_call("planar/alloc") == ["w2x_render_planar", ["engine0", at("src"), [6, 6, 6], 4, 6, 8, [["alloc0", 0], ["alloc1", 0], ["alloc2", 0]], [12, 12, 12], 8, 12, 8]]
    assert logs["planar/alloc"]["allocated"] == [[[8, 12], "uint8"]] * 3 and [p["shape"] for p in logs["planar/alloc"]["result"]] == [[8, 12]] * 3
    assert only_call("planar/10_to_float_padded")[1][2:] == [[18, 18, 18], 4, 6, 10, [["alloc0", 0], ["alloc1", 0], ["alloc2", 0]], [48, 48, 48], 8, 12, 32]
    assert [p["dtype"] for p in logs["planar/10_to_float_padded"]["result"]] == ["float32"] * 3
    assert only_call("planar/float_to_12")[1][2:6] == [[24, 24, 24], 4, 6, 32] and only_call("planar/float_to_12")[1][7:] == [[24, 24, 24], 8, 12, 12]
    assert logs["planar/float_to_12"]["allocated"] == [[[8, 12], "uint16"]] * 3
    # order="gbr": the caller's planes are G, B, R - the entry receives R, G, B on both sides
    assert only_call("planar/gbr_dst_padded") == ["w2x_render_planar", ["engine0", at("src", "brg"), [8, 8, 8], 4, 6, 8, at("dst", "brg"), [17, 17, 17], 8, 12, 8]]
    assert logs["planar/gbr_dst_padded"]["result"] is True
    assert logs["planar/fail_alloc"]["raised"] == ["W2xError", "[renderPlanar@7] scripted refusal."]
    assert only_call("planar/never_loaded")[0] == "w2x_render_planar"        # a dst of any size goes to the library, which refuses the call
    assert only_call("resized/alloc_bilinear") == ["w2x_render_planar_resized", ["engine0", at("src"), [7, 7, 7], 4, 6, 8, [["alloc0", 0], ["alloc1", 0], ["alloc2", 0]], [9, 9, 9], 7, 9, 8, 1]]
    assert only_call("resized/dst16") == ["w2x_render_planar_resized", ["engine0", at("src"), [12, 12, 12], 4, 6, 16, at("dst"), [22, 22, 22], 7, 9, 16, 0]]
    empty = only_call("resized/empty_target")                                # (an empty target: null destination planes, refused by the library)
    assert empty[0] == "w2x_render_planar_resized" and empty[1][6] == [None, None, None] and empty[1][8:] == [0, 9, 8, 0]
    assert logs["seq/empty"]["calls"] == [] and logs["seq/empty"]["result"] == []
    # engine, planes of every frame, steps, rows, cols, bits, destination planes of every frame, steps, rows, cols, bits, count
    assert only_call("seq/alloc") == ["w2x_render_sequence_planar", ["engine0", at("frame0") + at("frame1"), [6, 6, 6], 4, 6, 8, [[f"alloc{k}", 0] for k in range(6)], [24, 24, 24], 8, 12, 10, 2]]
    assert only_call("seq/gbr_padded_size") == ["w2x_render_sequence_planar_resized", ["engine0", at("frame0", "brg") + at("frame1", "brg"), [10, 10, 10], 4, 6, 8,
                                                                                        [[f"alloc{k}", 0] for k in (2, 0, 1, 5, 3, 4)], [9, 9, 9], 7, 9, 8, 2, 1]]
    assert only_call("seq/outs") == ["w2x_render_sequence_planar", ["engine0", at("frame0") + at("frame1"), [6, 6, 6], 4, 6, 8, at("out0") + at("out1"), [13, 13, 13], 8, 12, 8, 2]]
    # a pinned sequence of four: a ring of three page-locked blocks (three float planes each), two pieces (3 + 1), copies returned, every block given back
    calls = logs["seq/pinned"]["calls"]
    assert [c[0] for c in calls] == ["w2x_alloc_host"] * 3 + ["w2x_render_sequence_planar"] * 2 + ["w2x_free_host"] * 3
    assert [c[1][1] for c in calls[:3]] == [3 * 96 * 4] * 3
    assert calls[3][1][6] == [[f"host{k}", o] for k in range(3) for o in (0, 384, 768)] and calls[3][1][7:] == [[48, 48, 48], 8, 12, 32, 3]
    assert calls[4][1][1] == at("frame3") and calls[4][1][6] == [["host0", 0], ["host0", 384], ["host0", 768]] and calls[4][1][-1] == 1
    assert logs["seq/pinned"]["host_buffers"] == {"handed_out": 3, "all_freed": True} and len(logs["seq/pinned"]["result"]) == 4
    log = logs["seq/fail_pinned_second_piece"]
    assert log["raised"] == ["W2xError", "render_sequence_planar failed"] and log["host_buffers"] == {"handed_out": 3, "all_freed": True}
    log = logs["seq/second_alloc_fails"]
    assert log["raised"] == ["W2xError", "w2x_alloc_host failed"]
    assert [c[0] for c in log["calls"]] == ["w2x_alloc_host", "w2x_alloc_host", "w2x_free_host"] and log["host_buffers"] == {"handed_out": 1, "all_freed": True}


# ---- the command line
def w2x(*args):
    return subprocess.run([W2X, *args], capture_output=True, text=True)


@pytest.fixture()
def clip(tmp_path):
    f = tmp_path / "clip.mkv"
    f.write_bytes(b"")                                                      # --print-config stops after parsing: the file only has to exist
    return str(f)


def test_formats_round_trip_through_print_config(clip):
    r = w2x(*BASE, "render", "-i", clip, "--print-config")
    assert r.returncode == 0, r.stderr
    without = json.loads(r.stdout)
    assert without["rgb_in"] is None and without["rgb_out"] is None and without["pix_fmt"] == "yuv420p"
    for k, fmt in enumerate(FORMATS):
        other = FORMATS[(k + 2) % 5]
        r = w2x(*BASE, "render", "-i", clip, "--rgb-in", fmt, "--rgb-out", other, "--print-config")
        assert r.returncode == 0, r.stderr
        cfg = json.loads(r.stdout)
        assert (cfg["rgb_in"], cfg["rgb_out"], cfg["pix_fmt"]) == (fmt, other, other)          # the encoder's format defaults to --rgb-out
        assert cfg["outputs"] == without["outputs"] and cfg["suffix"] == without["suffix"]
        cfg = json.loads(w2x(*BASE, "render", "-i", clip, f"--rgb-out={fmt}", "--print-config").stdout)
        assert (cfg["rgb_in"], cfg["rgb_out"], cfg["pix_fmt"]) == (None, fmt, fmt)
    # --rgb-in alone leaves the encoder's format; a --pix_fmt given stays the encoder's alone, on either side of --rgb-out
    cfg = json.loads(w2x(*BASE, "render", "-i", clip, "--rgb-in", "gbrp12le", "--print-config").stdout)
    assert (cfg["rgb_in"], cfg["rgb_out"], cfg["pix_fmt"]) == ("gbrp12le", None, "yuv420p")
    for args in (("--pix_fmt", "yuv444p10le", "--rgb-out", "gbrp16le"), ("--rgb-out", "gbrp16le", "--pix_fmt", "yuv444p10le")):
        cfg = json.loads(w2x(*BASE, "render", "-i", clip, *args, "--print-config").stdout)
        assert (cfg["rgb_out"], cfg["pix_fmt"]) == ("gbrp16le", "yuv444p10le")
    # with a target size, and over several devices (the chunks of a video go to the engines like bgr24 chunks)
    r = w2x(*BASE, "render", "-i", clip, "--rgb-in", "gbrp10le", "--rgb-out", "gbrpf32le", "--outsize", "300x200", "--devices", "2", "--print-config")
    assert r.returncode == 0 and json.loads(r.stdout)["rgb_out"] == "gbrpf32le"
    r = w2x(*BASE, "render", "-i", clip, "--rgb-out", "gbrp10le", "--outscale", "2.5", "--print-config")
    assert r.returncode == 0 and json.loads(r.stdout)["rgb_out"] == "gbrp10le"
    cfg = json.loads(w2x(*BASE, "build", "--print-config").stdout)
    assert cfg["rgb_in"] is None and cfg["rgb_out"] is None


@pytest.mark.parametrize("opt", ["--rgb-in", "--rgb-out"])
@pytest.mark.parametrize("extra,command,says", [
    (("rgb48le",), "render", "not in {gbrp,gbrp10le,gbrp12le,gbrp16le,gbrpf32le}"), (("GBRP",), "render", "not in {"), (("gbrp14le",), "render", "not in {"),
    (("gbrp",), "build", "only with render"), (("gbrp10le", "--colorspace", "bt709"), "render", "--colorspace"), (("gbrp16le", "--gray"), "render", "--gray")])
def test_parse_errors_name_the_option(clip, opt, extra, command, says):
    args = [*BASE, command] + (["-i", clip] if command == "render" else []) + [opt, *extra, "--print-config"]
    r = w2x(*args)
    assert r.returncode != 0 and r.stderr.startswith(f"{opt}:") and says in r.stderr, (r.returncode, r.stderr)
    assert r.stdout == ""


def test_help_lists_the_options_and_the_formats():
    r = w2x("--help")
    assert r.returncode == 0 and "--rgb-in" in r.stdout and "--rgb-out" in r.stdout
    text = r.stdout[r.stdout.index("--rgb-in"):]
    for fmt in FORMATS:
        assert fmt in text, fmt
    assert "--pix_fmt" in text and "--colorspace" in text and "--gray" in text
