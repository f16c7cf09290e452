"""Planar RGBA frames without a device: the C entries of include/w2x/c_api_rgbap.h against libw2x.so and engine.RGBAP_SYMBOLS, the host statement of the colour
bleed on codes of any integer depth (w2x_alpha_bleed_rgbap) against alpha_bleed at 8 bits and the numpy restatement of tests/planar_rgba_ref.py above, the
entries' refusals on a null and on a never-loaded engine, the wrapper's own refusals and its marshalling through the recording stub of
tests/golden/make_binding_calls.py, --rgba-in / --rgba-out on the command line (--print-config stops after parsing), and the bleed mode of the stand-alone
sanitizer program (make asan)."""
import ctypes as C
import importlib
import importlib.util
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import planar_rgba_ref as ref
import rgba_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "waifu2x-tensorrt_amd")
W2X = os.path.join(PKG_DIR, "w2x")
BASE = ["--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "2", "--tileSize", "64"]
FORMATS = ["gbrap", "gbrap10le", "gbrap12le", "gbrap16le", "gbrapf32le"]
u8, u16, f32 = np.uint8, np.uint16, np.float32
RENDER_ENTRIES = {"w2x_render_rgbap", "w2x_render_rgbap_resized", "w2x_render_sequence_rgbap", "w2x_render_sequence_rgbap_resized"}
BLEED_ENTRIES = {"w2x_alpha_bleed_rgbap", "w2x_alpha_bleed_rgbap_device"}


def declared(header):
    hdr = open(os.path.join(ROOT, "include", "w2x", header)).read()
    return set(re.findall(r"\b(w2x_[a-z0-9_]+)\s*\(", hdr[hdr.index('extern "C"'):]))


@pytest.fixture(scope="module")
def engine_module(pkg):
    return importlib.import_module("waifu2x-tensorrt_amd.engine")


# ---- the header, the library and the wrapper's table name the same entries, and none of them belongs to another header or table
def test_header_library_and_table_agree(pkg, engine_module):
    names = declared("c_api_rgbap.h")
    assert names == RENDER_ENTRIES | BLEED_ENTRIES
    assert names == set(engine_module.RGBAP_SYMBOLS)
    assert not any("planar" in n or "gray" in n for n in names)
    raw = C.CDLL(pkg.lib_path)                                      # a handle of its own: what the file exports, not what lib() declared
    for n in names:
        assert hasattr(raw, n), f"libw2x.so does not export {n}"
    exported = subprocess.run(["nm", "-D", "--defined-only", pkg.lib_path], capture_output=True, text=True) if shutil.which("nm") else None
    if exported is not None and exported.returncode == 0:          # the other way round, where binutils is there: no rgbap entry the header does not declare
        assert {s for s in re.findall(r"\bT (w2x_[a-z0-9_]+)", exported.stdout) if "rgbap" in s} == names
    for other in ("c_api.h", "c_api_gray.h", "c_api_planar.h"):
        assert not names & declared(other), other
    for table in (engine_module.EXPORTED_SYMBOLS, engine_module.SYMBOLS, engine_module.GRAY_SYMBOLS, engine_module.PLANAR_SYMBOLS):
        assert not names & set(table)
    L = pkg.lib()
    for n, (restype, argtypes) in engine_module.RGBAP_SYMBOLS.items():
        assert getattr(L, n).restype is restype and list(getattr(L, n).argtypes) == argtypes, n
    hdr = open(os.path.join(ROOT, "include", "w2x", "c_api_rgbap.h")).read()
    assert '#include "c_api.h"' in hdr


# ---- the host bleed
def same_planes(tag, got, want):
    assert len(got) == len(want) == 3, tag
    for k in range(3):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (tag, k)
        bad = got[k] != want[k]
        assert not bad.any(), f"{tag} plane {k}: {int(bad.sum())} samples differ, first at {tuple(np.argwhere(bad)[0])}"


def rgb_planes(bgr):
    """the R, G, B planes of an interleaved frame, each a fresh packed array (a 1 x 1 slice keeps the strides of its frame otherwise)"""
    return tuple(np.array(bgr[..., k], order="C", copy=True) for k in (2, 1, 0))


def test_host_bleed_at_8_bits_is_alpha_bleed(pkg):
    for name, bgr, alpha, radii in rgba_ref.cases():
        planes = rgb_planes(bgr) + (alpha,)
        for radius in radii:
            same_planes(f"{name} radius {radius}", pkg.alpha_bleed_planes(planes, radius), rgb_planes(pkg.alpha_bleed(bgr, alpha, radius)))
    # ffmpeg's order, and planes padded each its own way
    name, bgr, alpha, _ = rgba_ref.cases()[12]
    planes = rgb_planes(bgr) + (alpha,)
    want = pkg.alpha_bleed_planes(planes, 5)
    same_planes("order gbra", pkg.alpha_bleed_planes((planes[1], planes[2], planes[0], planes[3]), 5, order="gbra"), want)
    same_planes("padded planes", pkg.alpha_bleed_planes(ref.padded(planes), 5), want)


@pytest.mark.parametrize("bits", [10, 12, 16])
def test_host_bleed_at_deeper_codes_is_the_numpy_statement(pkg, bits):
    m = (1 << bits) - 1
    for rows, cols in ((1, 1), (1, 17), (17, 1), (33, 65), (70, 150)):
        for pattern in ("random", "sparse", "zero", "opaque", "corner"):
            planes = ref.frame(rows, cols, bits, pattern, 3 * rows + cols)
            for radius in (0, 1, 2, 5, 16):
                got = pkg.alpha_bleed_planes(ref.padded(planes), radius, bits=bits)
                same_planes(f"{bits} bits {rows}x{cols} {pattern} radius {radius}", got, ref.bleed_planes(planes, m, radius))
                known = planes[3] > 0
                for k in range(3):                                  # a known pixel never changes
                    assert np.array_equal(got[k][known], planes[k][known])
                if radius == 0 or pattern in ("zero", "opaque"):    # the identity
                    same_planes(f"{bits} bits {pattern} radius {radius} is the identity", got, planes[:3])


@pytest.mark.parametrize("bits", [10, 12])
def test_codes_above_the_depth_act_as_its_largest(pkg, bits):
    m = (1 << bits) - 1
    wild = ref.frame(40, 70, 16, "random", 5)
    assert all((p > m).any() for p in wild) and ((wild[3] > 0) & (wild[3] <= m)).any()
    tame = tuple(np.minimum(p, m) for p in wild)
    for radius in (0, 3, 16):
        got = pkg.alpha_bleed_planes(wild, radius, bits=bits)
        same_planes(f"radius {radius}", got, pkg.alpha_bleed_planes(tame, radius, bits=bits))
        same_planes(f"radius {radius}, numpy", got, ref.bleed_planes(wild, m, radius))
        assert all(int(p.max()) <= m for p in got)


def test_the_sums_of_eight_16_bit_codes_do_not_overflow(pkg):
    """an unknown pixel whose eight neighbours are all 65535: the mean is 65535 (a 16-bit sum would wrap, a sum + n / 2 in 19 bits does not)"""
    planes = tuple(np.full((5, 5), 65535, u16) for _ in range(4))
    for p in planes:
        p[2, 2] = 0
    got = pkg.alpha_bleed_planes(planes, 1)
    assert all((p == 65535).all() for p in got)
    got = pkg.alpha_bleed_planes(tuple(np.full((3, 40), 65535, u16) for _ in range(3)) + (np.pad(np.full((3, 1), 7, u16), ((0, 0), (0, 39))),), 16)
    assert all((p == 65535).all() for p in got)


def test_the_codes_that_round_two_ways_to_a_half():
    """what the frames of tests/test_gpu_planar_rgba.py plant (and, in B and A of its integer-against-float equality, leave out): found by enumeration"""
    assert {b: ref.rounding_codes(b) for b in (8, 10, 12, 16)} == {8: (), 10: (), **ref.ROUNDING_CODES}


def test_host_bleed_refusals(pkg):
    L = pkg.lib()
    planes = tuple(np.zeros((4, 6), u16) for _ in range(4))
    out = tuple(np.zeros((4, 6), u16) for _ in range(3))
    sp, ss = (C.c_void_p * 4)(*[p.ctypes.data for p in planes]), (C.c_size_t * 4)(12, 12, 12, 12)
    dp, ds = (C.c_void_p * 3)(*[p.ctypes.data for p in out]), (C.c_size_t * 3)(12, 12, 12)
    assert L.w2x_alpha_bleed_rgbap(sp, ss, 4, 6, 16, 2, dp, ds) == 1
    for bad in ((None, ss, 4, 6, 16, 2, dp, ds), (sp, None, 4, 6, 16, 2, dp, ds), (sp, ss, 4, 6, 16, 2, None, ds), (sp, ss, 0, 6, 16, 2, dp, ds), (sp, ss, 4, 0, 16, 2, dp, ds),
                (sp, ss, 4, 6, 32, 0, dp, ds), (sp, ss, 4, 6, 9, 2, dp, ds), (sp, ss, 4, 6, 16, 17, dp, ds), (sp, ss, 4, 6, 16, -1, dp, ds),
                (sp, (C.c_size_t * 4)(12, 12, 12, 11), 4, 6, 16, 2, dp, ds), (sp, (C.c_size_t * 4)(12, 13, 12, 12), 4, 6, 16, 2, dp, ds), (sp, ss, 4, 6, 16, 2, dp, (C.c_size_t * 3)(12, 10, 12)),
                ((C.c_void_p * 4)(planes[0].ctypes.data, None, planes[2].ctypes.data, planes[3].ctypes.data), ss, 4, 6, 16, 2, dp, ds),
                ((C.c_void_p * 4)(*[p.ctypes.data + (k == 3) for k, p in enumerate(planes)]), ss, 4, 6, 16, 2, dp, ds)):
        assert L.w2x_alpha_bleed_rgbap(*bad) == 0, bad[2:6]
    with pytest.raises(ValueError, match="integer samples"):
        pkg.alpha_bleed_planes(tuple(np.zeros((4, 6), f32) for _ in range(4)), 1)
    with pytest.raises(ValueError):
        pkg.alpha_bleed_planes(planes[:3], 1)
    with pytest.raises(ValueError):
        pkg.alpha_bleed_planes(planes, 17)


# ---- the C entries.  name -> (C++ method named in the engine's refusal, arguments after the engine, index of `count` or None, takes a filter last)
ROWS, COLS = 4, 6


class Args:
    def __init__(self):
        self.src = np.zeros((4, ROWS, COLS), u16)
        self.dst = np.zeros((4, 2 * ROWS, 2 * COLS), f32)
        self.sp, self.dp = (C.c_void_p * 4)(*[p.ctypes.data for p in self.src]), (C.c_void_p * 4)(*[p.ctypes.data for p in self.dst])
        self.ss, self.ds = (C.c_size_t * 4)(*[2 * COLS] * 4), (C.c_size_t * 4)(*[8 * COLS] * 4)
        self.sps, self.dps = (C.c_void_p * 8)(*list(self.sp) * 2), (C.c_void_p * 8)(*list(self.dp) * 2)


def entries(a):
    r, c = ROWS, COLS
    one = (a.sp, a.ss, r, c, 10, a.dp, a.ds, 2 * r, 2 * c, 32)
    two = (a.sps, a.ss, r, c, 10, a.dps, a.ds, 2 * r, 2 * c, 32)
    return {
        "w2x_render_rgbap": ("renderPlanarRgba", one + (3, 1), None, False),
        "w2x_render_rgbap_resized": ("renderPlanarRgbaResized", one + (3, 1, 0), None, True),
        "w2x_render_sequence_rgbap": ("renderSequencePlanarRgba", two + (2, 3, 1), 10, False),
        "w2x_render_sequence_rgbap_resized": ("renderSequencePlanarRgbaResized", two + (2, 3, 1, 1), 10, True),
    }


ENTRY_NAMES = sorted(entries(Args()))


def test_the_table_holds_every_render_entry_of_the_header():
    assert set(ENTRY_NAMES) == declared("c_api_rgbap.h") - BLEED_ENTRIES == RENDER_ENTRIES


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


def test_the_device_bleed_entry_without_a_device(pkg):
    L, eng, a = pkg.lib(), pkg.Img2Img(), Args()
    out = np.zeros((3, ROWS, COLS), u16)
    args = (a.sp, a.ss, ROWS, COLS, 10, 2, (C.c_void_p * 3)(*[p.ctypes.data for p in out]), (C.c_size_t * 3)(*[2 * COLS] * 3), None)
    assert L.w2x_alpha_bleed_rgbap_device(None, *args) == 0 and eng.messages == []
    assert L.w2x_alpha_bleed_rgbap_device(eng._h, *args) == 0
    assert len(eng.messages) == 1 and eng.messages[0][1].startswith("[alphaBleedPlanes@") and "before a successful load" in eng.messages[0][1]
    eng.close()


# ---- the wrapper: refusals that reach no entry, and what the accepted calls hand to the C ABI
@pytest.fixture(scope="module")
def generator(pkg):
    spec = importlib.util.spec_from_file_location("make_binding_calls", os.path.join(ROOT, "tests", "golden", "make_binding_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def frame(c, name="src", r=4, cc=6, dtype=u8, pad=0, out=False):
    return tuple(c.arr(f"{name}.{ch}", (r, cc), dtype, pad, out) for ch in "rgba")


def frames(c, n, r=4, cc=6, dtype=u8, pad=0):
    return [frame(c, f"frame{k}", r, cc, dtype, pad) for k in range(n)]


def test_wrapper_refusals_reach_no_entry(generator):
    z = np.zeros
    cases = [
        ("three_planes", True, 1, lambda c: c.e.render_planar_rgba((z((4, 6), u8),) * 3)),
        ("interleaved", True, 1, lambda c: c.e.render_planar_rgba(z((4, 6, 4), u8))),
        ("float64", True, 1, lambda c: c.e.render_planar_rgba((z((4, 6), np.float64),) * 4)),
        ("mixed_types", True, 1, lambda c: c.e.render_planar_rgba((z((4, 6), u8), z((4, 6), u8), z((4, 6), u8), z((4, 6), u16)))),
        ("mixed_shapes", True, 1, lambda c: c.e.render_planar_rgba((z((4, 6), u8), z((4, 6), u8), z((4, 6), u8), z((4, 7), u8)))),
        ("unpacked", True, 1, lambda c: c.e.render_planar_rgba((z((4, 12), u8)[:, ::2],) * 4)),
        ("bits_10_on_u8", True, 1, lambda c: c.e.render_planar_rgba(frame(c), bits=10)),
        ("bits_16_on_float", True, 1, lambda c: c.e.render_planar_rgba(frame(c, dtype=f32), bits=16)),
        ("bits_14", True, 1, lambda c: c.e.render_planar_rgba(frame(c, dtype=u16), bits=14)),
        ("out_bits_9", True, 1, lambda c: c.e.render_planar_rgba(frame(c), out_bits=9)),
        ("order_rgb", True, 1, lambda c: c.e.render_planar_rgba(frame(c), order="rgb")),
        ("order_twice", True, 1, lambda c: c.e.render_planar_rgba(frame(c), order="rrga")),
        ("filter", True, 1, lambda c: c.e.render_planar_rgba_resized(frame(c), (7, 9), filter="lanczos")),
        ("dst_dtype", True, 1, lambda c: c.e.render_planar_rgba(frame(c), out_bits=10, dst=frame(c, "dst", 8, 12, u8, out=True))),
        ("dst_three", True, 1, lambda c: c.e.render_planar_rgba(frame(c), dst=frame(c, "dst", 8, 12, out=True)[:3])),
        ("dst_size_resized", True, 1, lambda c: c.e.render_planar_rgba_resized(frame(c), (7, 9), dst=frame(c, "dst", 7, 10, out=True))),
        ("seq_interleaved", True, 1, lambda c: c.e.render_sequence_planar_rgba([z((4, 6, 4), u8)] * 2)),
        ("seq_three_planes", True, 1, lambda c: c.e.render_sequence_planar_rgba([frame(c, "frame0"), frame(c, "frame1")[:3]])),
        ("seq_shapes_differ", True, 1, lambda c: c.e.render_sequence_planar_rgba([frame(c, "frame0"), frame(c, "frame1", 4, 7)])),
        ("seq_strides_differ", True, 1, lambda c: c.e.render_sequence_planar_rgba([frame(c, "frame0"), frame(c, "frame1", pad=2)])),
        ("seq_depths_differ", True, 1, lambda c: c.e.render_sequence_planar_rgba([frame(c, "frame0"), frame(c, "frame1", dtype=u16)])),
        ("seq_filter_pinned", True, 1, lambda c: c.e.render_sequence_planar_rgba(frames(c, 2), (7, 9), filter="lanczos", pinned=True)),
        ("seq_out_bits_pinned", True, 1, lambda c: c.e.render_sequence_planar_rgba(frames(c, 2), out_bits=11, pinned=True)),
        ("seq_outs_size", True, 1, lambda c: c.e.render_sequence_planar_rgba(frames(c, 2), outs=[frame(c, f"out{k}", 8, 11, out=True) for k in range(2)])),
        ("seq_outs_strides", True, 1, lambda c: c.e.render_sequence_planar_rgba(frames(c, 2), outs=[frame(c, "out0", 8, 12, out=True), frame(c, "out1", 8, 12, pad=3, out=True)])),
    ]
    logs = generator.generate(scenarios=cases)["scenarios"]
    for name, log in logs.items():
        assert log["raised"] and log["raised"][0] == "ValueError", (name, log)
        assert log["calls"] == [] and log["host_buffers"] == {"handed_out": 0, "all_freed": True}, (name, log)
    # a destination of the wrong size for the plain call: refused with the engine's message, False, no entry
    log = generator.generate(scenarios=[("dst_size", True, 1, lambda c: c.e.render_planar_rgba(frame(c), dst=frame(c, "dst", 8, 11, out=True)))])["scenarios"]["dst_size"]
    assert log["result"] is False and log["calls"] == [] and log["messages"] == [[[1, "[renderPlanarRgba@0] Output image has invalid size: expected 12x8."]]]


def test_wrapper_marshalling(generator):
    cases = [
        ("one/alloc", True, 1, lambda c: c.e.render_planar_rgba(frame(c))),
        ("one/10_to_float_padded_options", True, 1, lambda c: c.e.render_planar_rgba(frame(c, dtype=u16, pad=3), bits=10, out_bits=32, bleed=5, skip_uniform_alpha=True)),
        ("one/gbra_dst_padded", True, 1, lambda c: c.e.render_planar_rgba(frame(c, pad=2), order="gbra", bleed=16, dst=frame(c, "dst", 8, 12, pad=5, out=True))),
        ("one/fail_alloc", True, 1, lambda c: (c.fail("w2x_render_rgbap", say=b"[renderPlanarRgba@7] scripted refusal."), c.e.render_planar_rgba(frame(c)))[1]),
        ("one/never_loaded", False, 1, lambda c: c.e.render_planar_rgba(frame(c), dst=frame(c, "dst", 5, 5, out=True))),
        ("resized/alloc_bilinear", True, 1, lambda c: c.e.render_planar_rgba_resized(frame(c, pad=1), (7, 9), bleed=2, filter="bilinear")),
        ("resized/dst16", True, 1, lambda c: c.e.render_planar_rgba_resized(frame(c, dtype=u16), (7, 9), skip_uniform_alpha=True, dst=frame(c, "dst", 7, 9, u16, pad=2, out=True))),
        ("seq/empty", True, 1, lambda c: c.e.render_sequence_planar_rgba([])),
        ("seq/alloc", True, 1, lambda c: c.e.render_sequence_planar_rgba(frames(c, 2), out_bits=10, bleed=4)),
        ("seq/gbra_padded_size", True, 1, lambda c: c.e.render_sequence_planar_rgba(frames(c, 2, pad=4), (7, 9), order="gbra", skip_uniform_alpha=True, filter="bilinear")),
        ("seq/outs", True, 1, lambda c: c.e.render_sequence_planar_rgba(frames(c, 2), outs=[frame(c, f"out{k}", 8, 12, pad=1, out=True) for k in range(2)])),
        ("seq/pinned", True, 1, lambda c: c.e.render_sequence_planar_rgba(frames(c, 4), out_bits=32, pinned=True)),
        ("seq/fail_pinned_second_piece", True, 1, lambda c: (c.fail("w2x_render_sequence_rgbap", 2), c.e.render_sequence_planar_rgba(frames(c, 4), pinned=True))[1]),
        ("seq/second_alloc_fails", True, 1, lambda c: (c.fail("w2x_alloc_host", 2), c.e.render_sequence_planar_rgba(frames(c, 4), pinned=True))[1]),
        ("bleed/device", True, 1, lambda c: c.e.alpha_bleed_planes_device(frame(c, dtype=u16, pad=1), 7, bits=12, order="gbra")),
    ]
    logs = generator.generate(scenarios=cases)["scenarios"]
    assert all(log["host_buffers"]["all_freed"] for log in logs.values())

    def only_call(name):
        assert len(logs[name]["calls"]) == 1, logs[name]
        return logs[name]["calls"][0]

    def at(prefix, order="rgba", off=0):
        return [[f"{prefix}.{ch}", off] for ch in order]

    allocs = [[f"alloc{k}", 0] for k in range(4)]
    # engine, planes (R, G, B, A), steps, rows, cols, bits, destination planes, steps, rows, cols, bits, bleed, skip_uniform_alpha
    assert only_call("one/alloc") == ["w2x_render_rgbap", ["engine0", at("src"), [6] * 4, 4, 6, 8, allocs, [12] * 4, 8, 12, 8, 0, 0]]
    assert logs["one/alloc"]["allocated"] == [[[8, 12], "uint8"]] * 4 and [p["shape"] for p in logs["one/alloc"]["result"]] == [[8, 12]] * 4
    assert only_call("one/10_to_float_padded_options")[1][2:] == [[18] * 4, 4, 6, 10, allocs, [48] * 4, 8, 12, 32, 5, 1]
    assert [p["dtype"] for p in logs["one/10_to_float_padded_options"]["result"]] == ["float32"] * 4
    # order="gbra": the caller's planes are G, B, R, A - the entry receives R, G, B, A on both sides
    assert only_call("one/gbra_dst_padded") == ["w2x_render_rgbap", ["engine0", at("src", "brga"), [8] * 4, 4, 6, 8, at("dst", "brga"), [17] * 4, 8, 12, 8, 16, 0]]
    assert logs["one/gbra_dst_padded"]["result"] is True
    assert logs["one/fail_alloc"]["raised"] == ["W2xError", "[renderPlanarRgba@7] scripted refusal."]
    assert only_call("one/never_loaded")[0] == "w2x_render_rgbap"            # a dst of any size goes to the library, which refuses the call
    assert only_call("resized/alloc_bilinear") == ["w2x_render_rgbap_resized", ["engine0", at("src"), [7] * 4, 4, 6, 8, allocs, [9] * 4, 7, 9, 8, 2, 0, 1]]
    assert only_call("resized/dst16") == ["w2x_render_rgbap_resized", ["engine0", at("src"), [12] * 4, 4, 6, 16, at("dst"), [22] * 4, 7, 9, 16, 0, 1, 0]]
    assert logs["seq/empty"]["calls"] == [] and logs["seq/empty"]["result"] == []
    # engine, planes of every frame, steps, rows, cols, bits, destination planes of every frame, steps, rows, cols, bits, count, bleed, skip_uniform_alpha
    assert only_call("seq/alloc") == ["w2x_render_sequence_rgbap", ["engine0", at("frame0") + at("frame1"), [6] * 4, 4, 6, 8, [[f"alloc{k}", 0] for k in range(8)], [24] * 4, 8, 12, 10, 2, 4, 0]]
    assert only_call("seq/gbra_padded_size") == ["w2x_render_sequence_rgbap_resized", ["engine0", at("frame0", "brga") + at("frame1", "brga"), [10] * 4, 4, 6, 8,
                                                                                       [[f"alloc{k}", 0] for k in (2, 0, 1, 3, 6, 4, 5, 7)], [9] * 4, 7, 9, 8, 2, 0, 1, 1]]
    assert only_call("seq/outs") == ["w2x_render_sequence_rgbap", ["engine0", at("frame0") + at("frame1"), [6] * 4, 4, 6, 8, at("out0") + at("out1"), [13] * 4, 8, 12, 8, 2, 0, 0]]
    # a pinned sequence of four: a ring of three page-locked blocks (four float planes each), two pieces (3 + 1), copies returned, every block given back
    calls = logs["seq/pinned"]["calls"]
    assert [c[0] for c in calls] == ["w2x_alloc_host"] * 3 + ["w2x_render_sequence_rgbap"] * 2 + ["w2x_free_host"] * 3
    assert [c[1][1] for c in calls[:3]] == [4 * 96 * 4] * 3
    assert calls[3][1][6] == [[f"host{k}", o] for k in range(3) for o in (0, 384, 768, 1152)] and calls[3][1][7:] == [[48] * 4, 8, 12, 32, 3, 0, 0]
    assert calls[4][1][1] == at("frame3") and calls[4][1][6] == [["host0", o] for o in (0, 384, 768, 1152)] and calls[4][1][11] == 1
    assert logs["seq/pinned"]["host_buffers"] == {"handed_out": 3, "all_freed": True} and len(logs["seq/pinned"]["result"]) == 4
    log = logs["seq/fail_pinned_second_piece"]                               # a ring that cannot be completed is given back
    assert log["raised"] == ["W2xError", "render_sequence_planar_rgba failed"] and log["host_buffers"] == {"handed_out": 3, "all_freed": True}
    log = logs["seq/second_alloc_fails"]
    assert log["raised"] == ["W2xError", "w2x_alloc_host failed"]
    assert [c[0] for c in log["calls"]] == ["w2x_alloc_host", "w2x_alloc_host", "w2x_free_host"] and log["host_buffers"] == {"handed_out": 1, "all_freed": True}
    # the bleed hook: planes R, G, B, A of the caller's G, B, R, A; radius; three planes out; the two words
    call = only_call("bleed/device")
    assert call[0] == "w2x_alpha_bleed_rgbap_device" and call[1][:7] == ["engine0", at("src", "brga"), [14] * 4, 4, 6, 12, 7] and call[1][7] == allocs[:3] and call[1][8] == [12] * 3


# ---- the command line
def w2x(*args):
    return subprocess.run([W2X, *args], capture_output=True, text=True)


@pytest.fixture()
def clip(tmp_path):
    f = tmp_path / "clip.webm"
    f.write_bytes(b"")                                                      # --print-config stops after parsing: the file only has to exist
    return str(f)


def test_formats_round_trip_through_print_config(clip):
    r = w2x(*BASE, "render", "-i", clip, "--print-config")
    assert r.returncode == 0, r.stderr
    without = json.loads(r.stdout)
    assert without["rgba_in"] is None and without["rgba_out"] is None and without["pix_fmt"] == "yuv420p"
    for k, fmt in enumerate(FORMATS):
        other = FORMATS[(k + 2) % 5]
        r = w2x(*BASE, "render", "-i", clip, "--rgba-in", fmt, "--rgba-out", other, "--print-config")
        assert r.returncode == 0, r.stderr
        cfg = json.loads(r.stdout)
        assert (cfg["rgba_in"], cfg["rgba_out"], cfg["pix_fmt"]) == (fmt, other, other)        # the encoder's format defaults to --rgba-out
        assert cfg["outputs"] == without["outputs"] and cfg["suffix"] == without["suffix"] and cfg["rgb_in"] is None and cfg["rgb_out"] is None
        cfg = json.loads(w2x(*BASE, "render", "-i", clip, f"--rgba-out={fmt}", "--print-config").stdout)
        assert (cfg["rgba_in"], cfg["rgba_out"], cfg["pix_fmt"]) == (None, fmt, fmt)
    cfg = json.loads(w2x(*BASE, "render", "-i", clip, "--rgba-in", "gbrap12le", "--print-config").stdout)
    assert (cfg["rgba_in"], cfg["rgba_out"], cfg["pix_fmt"]) == ("gbrap12le", None, "yuv420p")
    for args in (("--pix_fmt", "yuva444p10le", "--rgba-out", "gbrap16le"), ("--rgba-out", "gbrap16le", "--pix_fmt", "yuva444p10le")):
        cfg = json.loads(w2x(*BASE, "render", "-i", clip, *args, "--print-config").stdout)
        assert (cfg["rgba_out"], cfg["pix_fmt"]) == ("gbrap16le", "yuva444p10le")
    # with a target size, over several devices, with the bleed and the shortcut
    r = w2x(*BASE, "render", "-i", clip, "--rgba-in", "gbrap10le", "--rgba-out", "gbrapf32le", "--outsize", "300x200", "--devices", "2", "--alpha-bleed", "16", "--alpha-skip-uniform", "--print-config")
    assert r.returncode == 0, r.stderr
    cfg = json.loads(r.stdout)
    assert (cfg["rgba_out"], cfg["alpha_bleed"], cfg["alpha_skip_uniform"], cfg["devices"]) == ("gbrapf32le", 16, True, 2)
    r = w2x(*BASE, "render", "-i", clip, "--rgba-out", "gbrap10le", "--outscale", "2.5", "--print-config")
    assert r.returncode == 0 and json.loads(r.stdout)["rgba_out"] == "gbrap10le"
    r = w2x(*BASE, "render", "-i", clip, "--rgba-in", "gbrapf32le", "--alpha-bleed", "0", "--print-config")
    assert r.returncode == 0, r.stderr
    cfg = json.loads(w2x(*BASE, "build", "--print-config").stdout)
    assert cfg["rgba_in"] is None and cfg["rgba_out"] is None


@pytest.mark.parametrize("opt", ["--rgba-in", "--rgba-out"])
@pytest.mark.parametrize("extra,command,says", [
    (("rgba64le",), "render", "not in {gbrap,gbrap10le,gbrap12le,gbrap16le,gbrapf32le}"), (("GBRAP",), "render", "not in {"), (("gbrap14le",), "render", "not in {"),
    (("gbrp",), "render", "not in {"), (("gbrap",), "build", "only with render"), (("gbrap10le", "--colorspace", "bt709"), "render", "--colorspace"),
    (("gbrap16le", "--gray"), "render", "--gray"), (("gbrap", "--rgb-in", "gbrp"), "render", "--rgb-in"), (("gbrap", "--rgb-out", "gbrp10le"), "render", "--rgb-out")])
def test_parse_errors_name_the_option(clip, opt, extra, command, says):
    args = [*BASE, command] + (["-i", clip] if command == "render" else []) + [opt, *extra, "--print-config"]
    r = w2x(*args)
    assert r.returncode != 0 and r.stderr.startswith(f"{opt}:") and says in r.stderr, (r.returncode, r.stderr)
    assert r.stdout == ""


def test_the_bleed_on_float_frames_is_a_parse_error(clip):
    for args in (("--rgba-in", "gbrapf32le", "--alpha-bleed", "4"), ("--alpha-bleed", "1", "--rgba-in=gbrapf32le", "--rgba-out", "gbrap")):
        r = w2x(*BASE, "render", "-i", clip, *args, "--print-config")
        assert r.returncode != 0 and r.stderr.startswith("--alpha-bleed:") and "gbrapf32le" in r.stderr and r.stdout == "", r.stderr
    r = w2x(*BASE, "render", "-i", clip, "--rgba-in", "gbrap", "--rgba-out", "gbrapf32le", "--alpha-bleed", "4", "--print-config")      # float out is fine
    assert r.returncode == 0, r.stderr
    r = w2x(*BASE, "render", "-i", clip, "--rgba-in", "gbrap16le", "--alpha-bleed", "17", "--print-config")
    assert r.returncode != 0 and r.stderr.startswith("--alpha-bleed:")


def test_help_lists_the_options_and_the_formats():
    r = w2x("--help")
    assert r.returncode == 0 and "--rgba-in" in r.stdout and "--rgba-out" in r.stdout
    text = r.stdout[r.stdout.index("--rgba-in"):]
    for fmt in FORMATS:
        assert fmt in text, fmt
    assert "--alpha-bleed" in text and "--colorspace" in text and "--gray" in text and "--rgb-in" in text


# ---- the stand-alone sanitizer program (make asan): its planes mode runs alpha_bleed_planes on seeded frames and prints a digest of the planes
def test_the_sanitizer_program_bleeds_planes(tmp_path):
    r = subprocess.run(["make", "-C", PKG_DIR, "asan"], capture_output=True, text=True)
    exe = os.path.join(PKG_DIR, "w2x_parse_check")
    assert r.returncode == 0 and os.path.exists(exe), r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="exitcode=97:detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    for bits, rows, cols, radius, seed in ((8, 33, 65, 16, 1), (10, 40, 70, 5, 2), (12, 17, 1, 2, 3), (16, 70, 150, 16, 4), (16, 1, 1, 0, 5)):
        out = tmp_path / f"planes_{bits}_{seed}.bin"
        r = subprocess.run([exe, "planes", str(bits), str(rows), str(cols), str(radius), str(seed), str(out)], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.startswith("ok:") and r.stderr == "", (r.returncode, r.stdout, r.stderr[-2000:])      # (a sanitizer report exits 97)
        dt = u8 if bits == 8 else u16
        raw = np.frombuffer(out.read_bytes(), dt).reshape(7, rows, cols)          # the four planes it made, then the three it got
        src = tuple(raw[k] for k in range(4))
        assert (src[3] == 0).any() or rows * cols == 1
        want = ref.bleed_planes(src, (1 << bits) - 1, radius)
        for k in range(3):
            assert np.array_equal(raw[4 + k], want[k]), (bits, rows, cols, radius, k)
    for bad in (("planes", "9", "4", "4", "1", "1", str(tmp_path / "x")), ("planes", "8", "0", "4", "1", "1", str(tmp_path / "x")), ("planes", "8", "4", "4", "17", "1", str(tmp_path / "x")), ("planes", "8", "4")):
        r = subprocess.run([exe, *bad], capture_output=True, text=True, env=env)
        assert r.returncode == 2 and r.stderr.startswith("rejected:"), (bad, r.returncode, r.stderr[-500:])
