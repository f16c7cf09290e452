"""The refusals of the BGR, YUV, gray and sharded entry points (engine.cpp) that the C entries can reach, pinned word for word, and one interleaving of the frame
formats on one engine.

Every entry point checks its arguments in a fixed order and logs one "[who@line] text" error through the message callback; the table below holds, per
(call, bad argument), the exact text and `who`, and per family cases with two things wrong at once, which pin the order.  The calls go through the C entries
(the Python binding checks shapes itself and would get there first).  RGBA refusals are asserted in test_gpu_rgba.py and test_gpu_rgba_resize.py; here
only the order of the RGBA checks is pinned (two_wrong), next to the order of the gray ones.
Not reachable through the C ABI, which fills both images of a call from one set of arguments and refuses null frame lists itself, and so not in the table:
a depth that differs between input and output, "... takes 8-bit frames", "No frames given.", the frames of a sequence differing in size, depth or layout, a
resized YUV frame of another layout than I420; the two tile-grid refusals need a model whose scaling differs from the load's.  Of the gray calls
(include/w2x/c_api_gray.h) the same holds: "Input and output images must both be 8-bit or both 16-bit." (one entry per depth fills both images),
"... takes 8-bit frames (16-bit images go through renderGray()).", "No frames given.", "Input images must be of one size." and the two tile-grid refusals
are out of the ABI's reach, and so is the engine's "Unknown resize filter.": the C entry refuses an unknown filter under its own name before the engine is asked.

The small Swin graph: batch 2, tile 64, scale 2, 40 x 60 frames (one tile)."""
import ctypes as C
import re

import numpy as np
import pytest

from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu

ROWS, COLS, S = 40, 60, 2
OUT = f"{COLS * S}x{ROWS * S}"
EMPTY = "Input image is empty or has an invalid step."
OUT_SIZE = f"Output image has invalid size: expected {OUT}."
NOT_LOADED = "Render called before a successful load."


def resize_msg(rows, cols):
    return f"Output image has invalid size for a resize: {cols}x{rows} is not between {COLS}x{ROWS} and {COLS * S}x{ROWS * S}."


@pytest.fixture(scope="module")
def eng(pkg, onnx_model):
    e = make_engine(pkg, onnx_model("swin_unet/art", S, 2, 64, small=True), 2, 64, S, overlap=(0.0625, 0.0625))
    yield e
    e.close()


class Calls:
    """the C entries on one engine, every argument overridable by name"""

    def __init__(self, eng):
        self.eng, self.L, self.h = eng, eng._L, eng._h
        rng = np.random.default_rng(7)
        self.bgr = rng.integers(0, 256, (ROWS, COLS, 3), dtype=np.uint8)
        self.bgr16 = self.bgr.astype(np.uint16) * 257
        self.out = np.empty((ROWS * S, COLS * S, 3), np.uint8)
        self.out16 = np.empty((ROWS * S, COLS * S, 3), np.uint16)
        self.yuv = (rng.integers(16, 236, (ROWS, COLS), dtype=np.uint8), rng.integers(16, 241, (ROWS // 2, COLS // 2), dtype=np.uint8),
                    rng.integers(16, 241, (ROWS // 2, COLS // 2), dtype=np.uint8))
        self.yuv_out = (np.empty((ROWS * S, COLS * S), np.uint8), np.empty((ROWS, COLS), np.uint8), np.empty((ROWS, COLS), np.uint8))
        self.gray8 = np.ascontiguousarray(self.bgr[:, :, 1])
        self.gray_16 = self.gray8.astype(np.uint16) * 257
        self.gray_out = np.empty((ROWS * S, COLS * S), np.uint8)
        self.gray_out16 = np.empty((ROWS * S, COLS * S), np.uint16)
        self.bgra = rng.integers(0, 256, (ROWS, COLS, 4), dtype=np.uint8)
        self.bgra_out = np.empty((ROWS * S, COLS * S, 4), np.uint8)

    def render(self, fn="w2x_render", **k):
        a = dict(src=self.bgr.ctypes.data, rows=ROWS, cols=COLS, sstep=COLS * 3, dst=self.out.ctypes.data, dstep=COLS * S * 3); a.update(k)
        return bool(getattr(self.L, fn)(self.h, a["src"], a["rows"], a["cols"], a["sstep"], a["dst"], a["dstep"]))

    def render16(self, **k):
        a = dict(src=self.bgr16.ctypes.data, sstep=COLS * 6, dst=self.out16.ctypes.data, dstep=COLS * S * 6); a.update(k)
        return self.render("w2x_render16", **a)

    def strip(self, part, parts, **k):
        a = dict(src=self.bgr.ctypes.data, rows=ROWS, cols=COLS, sstep=COLS * 3, dst=self.out.ctypes.data, dstep=COLS * S * 3); a.update(k)
        return bool(self.L.w2x_render_strip(self.h, a["src"], a["rows"], a["cols"], a["sstep"], a["dst"], a["dstep"], part, parts))

    def resized(self, fn="w2x_render_resized", **k):
        a = dict(src=self.bgr.ctypes.data, rows=ROWS, cols=COLS, sstep=COLS * 3, dst=self.out.ctypes.data, drows=50, dcols=70, dstep=70 * 3, filter=0); a.update(k)
        return bool(getattr(self.L, fn)(self.h, a["src"], a["rows"], a["cols"], a["sstep"], a["dst"], a["drows"], a["dcols"], a["dstep"], a["filter"]))

    def resized16(self, **k):
        a = dict(src=self.bgr16.ctypes.data, sstep=COLS * 6, dst=self.out16.ctypes.data, dstep=70 * 6); a.update(k)
        return self.resized("w2x_render16_resized", **a)

    def sequence(self, srcs=None, dsts=None, **k):
        a = dict(rows=ROWS, cols=COLS, sstep=COLS * 3, dstep=COLS * S * 3); a.update(k)
        srcs = [self.bgr.ctypes.data] * 2 if srcs is None else srcs
        dsts = [self.out.ctypes.data] * 2 if dsts is None else dsts
        return bool(self.L.w2x_render_sequence(self.h, (C.c_void_p * len(srcs))(*srcs), a["rows"], a["cols"], a["sstep"], (C.c_void_p * len(dsts))(*dsts), a["dstep"], len(srcs)))

    def sequence_resized(self, srcs=None, dsts=None, **k):
        a = dict(rows=ROWS, cols=COLS, sstep=COLS * 3, drows=50, dcols=70, dstep=70 * 3, filter=1); a.update(k)
        srcs = [self.bgr.ctypes.data] * 2 if srcs is None else srcs
        dsts = [self.out.ctypes.data] * 2 if dsts is None else dsts
        return bool(self.L.w2x_render_sequence_resized(self.h, (C.c_void_p * len(srcs))(*srcs), a["rows"], a["cols"], a["sstep"], (C.c_void_p * len(dsts))(*dsts),
                                                       a["drows"], a["dcols"], a["dstep"], len(srcs), a["filter"]))

    def _yuv_args(self, k, count):
        a = dict(sp=[p.ctypes.data for p in self.yuv] * count, ss=[p.strides[0] for p in self.yuv], rows=ROWS, cols=COLS, sbits=8,
                 dp=[p.ctypes.data for p in self.yuv_out] * count, ds=[p.strides[0] for p in self.yuv_out], drows=ROWS * S, dcols=COLS * S, dbits=8, matrix=1, range=0)
        a.update(k)
        a["sp"] = (C.c_void_p * len(a["sp"]))(*a["sp"]); a["dp"] = (C.c_void_p * len(a["dp"]))(*a["dp"])
        a["ss"] = (C.c_size_t * 3)(*a["ss"]); a["ds"] = (C.c_size_t * 3)(*a["ds"])
        return a

    def yuv_call(self, **k):
        a = self._yuv_args(k, 1)
        return bool(self.L.w2x_render_yuv(self.h, a["sp"], a["ss"], a["rows"], a["cols"], a["sbits"], a["dp"], a["ds"], a["drows"], a["dcols"], a["dbits"], a["matrix"], a["range"]))

    def yuv_layout(self, slayout=0, dlayout=0, **k):
        a = self._yuv_args(k, 1)
        return bool(self.L.w2x_render_yuv_layout(self.h, a["sp"], a["ss"], a["rows"], a["cols"], a["sbits"], slayout, a["dp"], a["ds"], a["drows"], a["dcols"], a["dbits"], dlayout,
                                                 a["matrix"], a["range"]))

    def yuv_resized(self, **k):
        k = dict(dict(drows=50, dcols=70, ds=[70, 35, 35], filter=0), **k)
        a = self._yuv_args(k, 1)
        return bool(self.L.w2x_render_yuv_resized(self.h, a["sp"], a["ss"], a["rows"], a["cols"], a["sbits"], a["dp"], a["ds"], a["drows"], a["dcols"], a["dbits"], a["matrix"], a["range"],
                                                  a["filter"]))

    def yuv_sequence(self, **k):
        a = self._yuv_args(k, 2)
        return bool(self.L.w2x_render_sequence_yuv(self.h, a["sp"], a["ss"], a["rows"], a["cols"], a["sbits"], a["dp"], a["ds"], a["drows"], a["dcols"], a["dbits"], 2, a["matrix"], a["range"]))

    def yuv_sequence_layout(self, slayout=0, dlayout=0, **k):
        a = self._yuv_args(k, 2)
        return bool(self.L.w2x_render_sequence_yuv_layout(self.h, a["sp"], a["ss"], a["rows"], a["cols"], a["sbits"], slayout, a["dp"], a["ds"], a["drows"], a["dcols"], a["dbits"], dlayout, 2,
                                                          a["matrix"], a["range"]))

    def yuv_sequence_resized(self, **k):
        k = dict(dict(drows=50, dcols=70, ds=[70, 35, 35], filter=1), **k)
        a = self._yuv_args(k, 2)
        return bool(self.L.w2x_render_sequence_yuv_resized(self.h, a["sp"], a["ss"], a["rows"], a["cols"], a["sbits"], a["dp"], a["ds"], a["drows"], a["dcols"], a["dbits"], 2,
                                                           a["matrix"], a["range"], a["filter"]))

    # gray frames (c_api_gray.h): the green plane of the BGR frame, 8 and 16 bits
    def gray(self, fn="w2x_render_gray", **k):
        a = dict(src=self.gray8.ctypes.data, rows=ROWS, cols=COLS, sstep=COLS, dst=self.gray_out.ctypes.data, dstep=COLS * S); a.update(k)
        return bool(getattr(self.L, fn)(self.h, a["src"], a["rows"], a["cols"], a["sstep"], a["dst"], a["dstep"]))

    def gray16(self, **k):
        a = dict(src=self.gray_16.ctypes.data, sstep=COLS * 2, dst=self.gray_out16.ctypes.data, dstep=COLS * S * 2); a.update(k)
        return self.gray("w2x_render_gray16", **a)

    def gray_resized(self, fn="w2x_render_gray_resized", **k):
        a = dict(src=self.gray8.ctypes.data, rows=ROWS, cols=COLS, sstep=COLS, dst=self.gray_out.ctypes.data, drows=50, dcols=70, dstep=70, filter=0); a.update(k)
        return bool(getattr(self.L, fn)(self.h, a["src"], a["rows"], a["cols"], a["sstep"], a["dst"], a["drows"], a["dcols"], a["dstep"], a["filter"]))

    def gray16_resized(self, **k):
        a = dict(src=self.gray_16.ctypes.data, sstep=COLS * 2, dst=self.gray_out16.ctypes.data, dstep=70 * 2); a.update(k)
        return self.gray_resized("w2x_render_gray16_resized", **a)

    def gray_sequence(self, srcs=None, dsts=None, **k):
        a = dict(rows=ROWS, cols=COLS, sstep=COLS, dstep=COLS * S); a.update(k)
        srcs = [self.gray8.ctypes.data] * 2 if srcs is None else srcs
        dsts = [self.gray_out.ctypes.data] * 2 if dsts is None else dsts
        return bool(self.L.w2x_render_sequence_gray(self.h, (C.c_void_p * len(srcs))(*srcs), a["rows"], a["cols"], a["sstep"], (C.c_void_p * len(dsts))(*dsts), a["dstep"], len(srcs)))

    def gray_sequence_resized(self, srcs=None, dsts=None, **k):
        a = dict(rows=ROWS, cols=COLS, sstep=COLS, drows=50, dcols=70, dstep=70, filter=1); a.update(k)
        srcs = [self.gray8.ctypes.data] * 2 if srcs is None else srcs
        dsts = [self.gray_out.ctypes.data] * 2 if dsts is None else dsts
        return bool(self.L.w2x_render_sequence_gray_resized(self.h, (C.c_void_p * len(srcs))(*srcs), a["rows"], a["cols"], a["sstep"], (C.c_void_p * len(dsts))(*dsts),
                                                            a["drows"], a["dcols"], a["dstep"], len(srcs), a["filter"]))

    # RGBA frames: only the order of their checks is pinned here (two_wrong)
    def rgba(self, **k):
        a = dict(src=self.bgra.ctypes.data, rows=ROWS, cols=COLS, sstep=COLS * 4, dst=self.bgra_out.ctypes.data, dstep=COLS * S * 4, bleed=2, skip=0); a.update(k)
        return bool(self.L.w2x_render_rgba(self.h, a["src"], a["rows"], a["cols"], a["sstep"], a["dst"], a["dstep"], a["bleed"], a["skip"]))

    def rgba_resized(self, **k):
        a = dict(src=self.bgra.ctypes.data, rows=ROWS, cols=COLS, sstep=COLS * 4, dst=self.bgra_out.ctypes.data, drows=50, dcols=70, dstep=70 * 4, bleed=2, skip=0, filter=0); a.update(k)
        return bool(self.L.w2x_render_rgba_resized(self.h, a["src"], a["rows"], a["cols"], a["sstep"], a["dst"], a["drows"], a["dcols"], a["dstep"], a["bleed"], a["skip"], a["filter"]))

    def rgba_sequence(self, srcs=None, dsts=None, **k):
        a = dict(rows=ROWS, cols=COLS, sstep=COLS * 4, dstep=COLS * S * 4, bleed=2, skip=0); a.update(k)
        srcs = [self.bgra.ctypes.data] * 2 if srcs is None else srcs
        dsts = [self.bgra_out.ctypes.data] * 2 if dsts is None else dsts
        return bool(self.L.w2x_render_sequence_rgba(self.h, (C.c_void_p * len(srcs))(*srcs), a["rows"], a["cols"], a["sstep"], (C.c_void_p * len(dsts))(*dsts), a["dstep"], len(srcs),
                                                    a["bleed"], a["skip"]))

    def rgba_sequence_resized(self, srcs=None, dsts=None, **k):
        a = dict(rows=ROWS, cols=COLS, sstep=COLS * 4, drows=50, dcols=70, dstep=70 * 4, bleed=2, skip=0, filter=1); a.update(k)
        srcs = [self.bgra.ctypes.data] * 2 if srcs is None else srcs
        dsts = [self.bgra_out.ctypes.data] * 2 if dsts is None else dsts
        return bool(self.L.w2x_render_sequence_rgba_resized(self.h, (C.c_void_p * len(srcs))(*srcs), a["rows"], a["cols"], a["sstep"], (C.c_void_p * len(dsts))(*dsts),
                                                            a["drows"], a["dcols"], a["dstep"], len(srcs), a["bleed"], a["skip"], a["filter"]))

    def sharded(self, handles=None, **k):
        a = dict(src=self.bgr.ctypes.data, rows=ROWS, cols=COLS, sstep=COLS * 3, dst=self.out.ctypes.data, dstep=COLS * S * 3); a.update(k)
        handles = [self.h] if handles is None else handles
        return bool(self.L.w2x_render_sharded((C.c_void_p * len(handles))(*handles), len(handles), a["src"], a["rows"], a["cols"], a["sstep"], a["dst"], a["dstep"]))

    def shard_compute(self, part=0, parts=1, **k):
        a = dict(src=self.bgr.ctypes.data, rows=ROWS, cols=COLS, sstep=COLS * 3); a.update(k)
        return bool(self.L.w2x_shard_compute(self.h, a["src"], a["rows"], a["cols"], a["sstep"], part, parts))

    def shard_finish(self, part=0, parts=1, slabs=True, **k):
        a = dict(dst=self.out.ctypes.data, rows=ROWS * S, cols=COLS * S, dstep=COLS * S * 3); a.update(k)
        arr = (C.c_void_p * max(parts, 1))() if slabs else None
        return bool(self.L.w2x_shard_finish(self.h, a["dst"], a["rows"], a["cols"], a["dstep"], part, parts, arr, None))


def check(pkg, eng, who, call, text):
    """call() is refused with exactly one new error, "[who@line] text" """
    n = len(eng.messages)
    assert call() is False, (who, text)
    new = [m for s, m in eng.messages[n:] if s == int(pkg.Severity.error)]
    assert len(new) == 1, (who, text, new)
    m = re.fullmatch(r"\[(\w+)@(\d+)\] (.*)", new[0], re.S)
    assert m and m.group(1) == who and m.group(3) == text, (who, text, new[0])


def table(c):
    """(who, call, exact text): one bad argument each"""
    short, short16 = COLS * 3 - 1, COLS * 6 - 1
    t = [
        # ---- render / render16 / renderStrip (renderPart)
        ("render", lambda: c.render(src=None), EMPTY),
        ("render", lambda: c.render(rows=0), EMPTY),
        ("render", lambda: c.render(cols=-1), EMPTY),
        ("render", lambda: c.render(sstep=short), EMPTY),
        ("render", lambda: c.render16(sstep=short16), EMPTY),
        ("render", lambda: c.render(dst=None), OUT_SIZE),
        ("render", lambda: c.render(dstep=COLS * S * 3 - 1), OUT_SIZE),
        ("render", lambda: c.render16(dstep=COLS * S * 6 - 1), OUT_SIZE),
        ("renderStrip", lambda: c.strip(0, 0), "Invalid strip index."),
        ("renderStrip", lambda: c.strip(2, 2), "Invalid strip index."),
        ("renderStrip", lambda: c.strip(-1, 2), "Invalid strip index."),
        ("renderStrip", lambda: c.strip(0, 2, src=None), EMPTY),
        ("renderStrip", lambda: c.strip(1, 2, dst=None), OUT_SIZE),
        # ---- renderResized
        ("renderResized", lambda: c.resized(src=None), EMPTY),
        ("renderResized", lambda: c.resized(sstep=short), EMPTY),
        ("renderResized", lambda: c.resized(drows=39, dcols=60), resize_msg(39, 60)),
        ("renderResized", lambda: c.resized(drows=80, dcols=121), resize_msg(80, 121)),
        ("renderResized", lambda: c.resized(drows=0, dcols=0, dst=None), resize_msg(0, 0)),
        ("renderResized", lambda: c.resized16(drows=81, dcols=120), resize_msg(81, 120)),
        ("renderResized", lambda: c.resized(dst=None), "Output image is empty or has an invalid step."),
        ("renderResized", lambda: c.resized(dstep=70 * 3 - 1), "Output image is empty or has an invalid step."),
        ("renderResized", lambda: c.resized16(dstep=70 * 6 - 1), "Output image is empty or has an invalid step."),
        ("renderResized", lambda: c.resized(drows=ROWS * S, dcols=COLS * S, dstep=COLS * S * 3 - 1), OUT_SIZE),      # at the scaled size it is render()
        # ---- renderSequence
        ("renderSequence", lambda: c.sequence(srcs=[c.bgr.ctypes.data, None]), "Input images must be non-empty and of one size."),
        ("renderSequence", lambda: c.sequence(sstep=short), "Input images must be non-empty and of one size."),
        ("renderSequence", lambda: c.sequence(rows=0), "Input images must be non-empty and of one size."),
        ("renderSequence", lambda: c.sequence(dsts=[c.out.ctypes.data, None]), OUT_SIZE),
        ("renderSequence", lambda: c.sequence(dstep=COLS * S * 3 - 1), OUT_SIZE),
        # ---- renderSequenceResized
        ("renderSequenceResized", lambda: c.sequence_resized(drows=39, dcols=70), resize_msg(39, 70)),
        ("renderSequenceResized", lambda: c.sequence_resized(drows=50, dcols=121), resize_msg(50, 121)),
        ("renderSequenceResized", lambda: c.sequence_resized(srcs=[None, c.bgr.ctypes.data]), "Input images must be non-empty and of one size."),
        ("renderSequenceResized", lambda: c.sequence_resized(dsts=[c.out.ctypes.data, None]), "Output image has invalid size: expected 70x50."),
        ("renderSequenceResized", lambda: c.sequence_resized(dstep=70 * 3 - 1), "Output image has invalid size: expected 70x50."),
    ]
    # ---- the YUV calls: one check list (runSequenceYuv), every entry under its own name
    y, u, v = (p.ctypes.data for p in c.yuv)
    oy, ou, ov = (p.ctypes.data for p in c.yuv_out)
    plain = [("renderYuv", c.yuv_call, 1), ("renderYuv", c.yuv_layout, 1), ("renderSequenceYuv", c.yuv_sequence, 2), ("renderSequenceYuv", c.yuv_sequence_layout, 2)]
    sized = [("renderYuvResized", c.yuv_resized, 1), ("renderSequenceYuvResized", c.yuv_sequence_resized, 2)]
    for who, f, n in plain + sized:
        t += [
            (who, lambda f=f: f(matrix=3), "Unknown YUV matrix 3."),
            (who, lambda f=f: f(matrix=-1), "Unknown YUV matrix -1."),
            (who, lambda f=f: f(range=2), "Unknown YUV range 2."),
            (who, lambda f=f: f(sbits=9), "YUV frames must have 8 or 10 bits."),
            (who, lambda f=f: f(dbits=12), "YUV frames must have 8 or 10 bits."),
            (who, lambda f=f: f(rows=0), "Input image is empty."),
            (who, lambda f=f: f(cols=0), "Input image is empty."),
            (who, lambda f=f, n=n: f(sp=[y, u, v] * (n - 1) + [y, None, v]), "Input image has a missing plane or an invalid step."),
            (who, lambda f=f: f(ss=[COLS, COLS // 2 - 1, COLS // 2]), "Input image has a missing plane or an invalid step."),
            (who, lambda f=f, n=n: f(dp=[oy, ou, ov] * (n - 1) + [None, ou, ov]), "Output image has a missing plane or an invalid step."),
        ]
    for who, f, n in plain:
        t += [
            (who, lambda f=f: f(drows=ROWS * S + 1), OUT_SIZE),
            (who, lambda f=f: f(dcols=COLS), OUT_SIZE),
            (who, lambda f=f: f(ds=[COLS * S - 1, COLS, COLS]), "Output image has a missing plane or an invalid step."),
        ]
    for who, f in (("renderYuv", c.yuv_layout), ("renderSequenceYuv", c.yuv_sequence_layout)):
        t += [
            (who, lambda f=f: f(slayout=4), "Unknown YUV layout 4."),
            (who, lambda f=f: f(dlayout=-1), "Unknown YUV layout -1."),
            (who, lambda f=f: f(slayout=3, sp=[y, None, None] * 2), "Input image has a missing plane or an invalid step."),      # NV12: Y and UV
        ]
    for who, f, n in sized:
        t += [
            (who, lambda f=f: f(drows=39, dcols=60), resize_msg(39, 60)),
            (who, lambda f=f: f(drows=50, dcols=121), resize_msg(50, 121)),
            (who, lambda f=f: f(ds=[69, 35, 35]), "Output image has a missing plane or an invalid step."),
        ]
    # ---- the gray calls: one check list (runGray), every entry under its own name
    OUT_70x50 = "Output image has invalid size: expected 70x50."
    g = c.gray8.ctypes.data
    t += [
        ("renderGray", lambda: c.gray(rows=0), EMPTY),
        ("renderGray", lambda: c.gray(cols=-1), EMPTY),
        ("renderGray", lambda: c.gray(src=None), EMPTY),
        ("renderGray", lambda: c.gray(sstep=COLS - 1), EMPTY),
        ("renderGray", lambda: c.gray16(sstep=COLS * 2 - 1), EMPTY),
        ("renderGray", lambda: c.gray(dst=None), OUT_SIZE),
        ("renderGray", lambda: c.gray(dstep=COLS * S - 1), OUT_SIZE),
        ("renderGray", lambda: c.gray16(dstep=COLS * S * 2 - 1), OUT_SIZE),
        ("renderGrayResized", lambda: c.gray_resized(rows=0), EMPTY),
        ("renderGrayResized", lambda: c.gray_resized(src=None), EMPTY),
        ("renderGrayResized", lambda: c.gray_resized(sstep=COLS - 1), EMPTY),
        ("renderGrayResized", lambda: c.gray16_resized(sstep=COLS * 2 - 1), EMPTY),
        ("renderGrayResized", lambda: c.gray_resized(drows=39, dcols=60), resize_msg(39, 60)),
        ("renderGrayResized", lambda: c.gray_resized(drows=80, dcols=121), resize_msg(80, 121)),
        ("renderGrayResized", lambda: c.gray_resized(drows=0, dcols=0), resize_msg(0, 0)),
        ("renderGrayResized", lambda: c.gray16_resized(drows=81, dcols=120), resize_msg(81, 120)),
        ("renderGrayResized", lambda: c.gray_resized(dst=None), OUT_70x50),
        ("renderGrayResized", lambda: c.gray_resized(dstep=69), OUT_70x50),
        ("renderGrayResized", lambda: c.gray16_resized(dstep=70 * 2 - 1), OUT_70x50),
        ("renderGrayResized", lambda: c.gray_resized(drows=ROWS * S, dcols=COLS * S, dstep=COLS * S - 1), OUT_SIZE),      # at the scaled size it is renderGray()
        ("renderSequenceGray", lambda: c.gray_sequence(rows=0), EMPTY),
        ("renderSequenceGray", lambda: c.gray_sequence(srcs=[g, None]), EMPTY),
        ("renderSequenceGray", lambda: c.gray_sequence(sstep=COLS - 1), EMPTY),
        ("renderSequenceGray", lambda: c.gray_sequence(dsts=[c.gray_out.ctypes.data, None]), OUT_SIZE),
        ("renderSequenceGray", lambda: c.gray_sequence(dstep=COLS * S - 1), OUT_SIZE),
        ("renderSequenceGrayResized", lambda: c.gray_sequence_resized(cols=0), EMPTY),
        ("renderSequenceGrayResized", lambda: c.gray_sequence_resized(drows=39, dcols=70), resize_msg(39, 70)),
        ("renderSequenceGrayResized", lambda: c.gray_sequence_resized(drows=50, dcols=121), resize_msg(50, 121)),
        ("renderSequenceGrayResized", lambda: c.gray_sequence_resized(srcs=[None, g]), EMPTY),
        ("renderSequenceGrayResized", lambda: c.gray_sequence_resized(dsts=[c.gray_out.ctypes.data, None]), OUT_70x50),
        ("renderSequenceGrayResized", lambda: c.gray_sequence_resized(dstep=69), OUT_70x50),
    ]
    # ---- the sharded entries' frame checks
    t += [
        ("renderSharded", lambda: c.sharded(src=None), EMPTY),
        ("renderSharded", lambda: c.sharded(sstep=short), EMPTY),
        ("renderSharded", lambda: c.sharded(rows=0), EMPTY),
        ("renderSharded", lambda: c.sharded(dst=None), OUT_SIZE),
        ("renderSharded", lambda: c.sharded(dstep=COLS * S * 3 - 1), OUT_SIZE),
        ("renderSharded", lambda: c.sharded(handles=[c.h, c.h]), "renderSharded: the same engine twice."),
        ("shardCompute", lambda: c.shard_compute(0, 0), "Invalid part index."),
        ("shardCompute", lambda: c.shard_compute(2, 2), "Invalid part index."),
        ("shardCompute", lambda: c.shard_compute(src=None), EMPTY),
        ("shardCompute", lambda: c.shard_compute(sstep=short), EMPTY),
    ]
    return t


def two_wrong(c):
    """(who, call, the refusal that wins): two bad arguments each, at least two cases per family"""
    y, u, v = (p.ctypes.data for p in c.yuv)
    return [
        ("render", lambda: c.render(src=None, dst=None), EMPTY),
        ("renderStrip", lambda: c.strip(3, 2, src=None), "Invalid strip index."),
        ("renderResized", lambda: c.resized(src=None, drows=39, dcols=60), EMPTY),
        ("renderResized", lambda: c.resized(drows=39, dcols=60, dst=None), resize_msg(39, 60)),
        ("renderSequence", lambda: c.sequence(srcs=[None, None], dsts=[None, None]), "Input images must be non-empty and of one size."),
        ("renderSequence", lambda: c.sequence(srcs=[c.bgr.ctypes.data, None], dsts=[None, c.out.ctypes.data]), OUT_SIZE),      # frame 0's output before frame 1's input
        ("renderSequenceResized", lambda: c.sequence_resized(srcs=[None, None], drows=39, dcols=70), resize_msg(39, 70)),
        ("renderSequenceResized", lambda: c.sequence_resized(sstep=1, dstep=1), "Input images must be non-empty and of one size."),
        ("renderYuv", lambda: c.yuv_call(matrix=3, range=2), "Unknown YUV matrix 3."),
        ("renderYuv", lambda: c.yuv_call(sbits=9, rows=0), "YUV frames must have 8 or 10 bits."),
        ("renderYuv", lambda: c.yuv_layout(range=2, slayout=7), "Unknown YUV range 2."),
        ("renderYuv", lambda: c.yuv_layout(dlayout=5, sp=[y, None, v]), "Unknown YUV layout 5."),
        ("renderSequenceYuv", lambda: c.yuv_sequence(rows=0, drows=1), "Input image is empty."),
        ("renderSequenceYuv", lambda: c.yuv_sequence(sp=[y, u, v, y, u, None], drows=ROWS * S + 2), "Output image has invalid size: expected " + OUT + "."),      # frame 0's output before frame 1's input
        ("renderYuvResized", lambda: c.yuv_resized(drows=39, dcols=60, sp=[y, None, v]), resize_msg(39, 60)),
        ("renderYuvResized", lambda: c.yuv_resized(dbits=9, drows=39, dcols=60), "YUV frames must have 8 or 10 bits."),
        ("renderSequenceYuvResized", lambda: c.yuv_sequence_resized(matrix=5, drows=39, dcols=60), "Unknown YUV matrix 5."),
        ("renderSequenceYuvResized", lambda: c.yuv_sequence_resized(drows=81, dcols=60, ss=[1, 1, 1]), resize_msg(81, 60)),
        # gray and RGBA, one order: depth, the first frame's size, the target, per frame its size, its pointers and steps (input before output), the bleed
        # radius (RGBA), the grid
        ("renderGray", lambda: c.gray(rows=0, dst=None), EMPTY),
        ("renderGray", lambda: c.gray(src=None, dst=None), EMPTY),
        ("renderGray", lambda: c.gray16(sstep=1, dstep=1), EMPTY),
        ("renderGrayResized", lambda: c.gray_resized(cols=0, drows=39, dcols=60), EMPTY),                                     # the first frame's size before the target
        ("renderGrayResized", lambda: c.gray_resized(drows=81, dcols=60, dst=None), resize_msg(81, 60)),                      # a null destination with an out-of-range target: the target
        ("renderGrayResized", lambda: c.gray_resized(src=None, drows=39, dcols=60), resize_msg(39, 60)),
        ("renderGrayResized", lambda: c.gray16_resized(src=None, dstep=1), EMPTY),
        ("renderSequenceGray", lambda: c.gray_sequence(srcs=[None, None], dsts=[None, None]), EMPTY),
        ("renderSequenceGray", lambda: c.gray_sequence(srcs=[c.gray8.ctypes.data, None], dsts=[None, c.gray_out.ctypes.data]), OUT_SIZE),      # frame 0's output before frame 1's input
        ("renderSequenceGrayResized", lambda: c.gray_sequence_resized(srcs=[None, None], drows=39, dcols=70), resize_msg(39, 70)),
        ("renderSequenceGrayResized", lambda: c.gray_sequence_resized(rows=-1, drows=39, dcols=70), EMPTY),
        ("renderSequenceGrayResized", lambda: c.gray_sequence_resized(sstep=1, dstep=1), EMPTY),
        ("renderRgba", lambda: c.rgba(rows=0, bleed=17), EMPTY),
        ("renderRgba", lambda: c.rgba(src=None, dst=None), EMPTY),
        ("renderRgba", lambda: c.rgba(dst=None, bleed=17), OUT_SIZE),                                                         # pointers and steps before the bleed radius
        ("renderRgbaResized", lambda: c.rgba_resized(cols=0, drows=39, dcols=60), EMPTY),
        ("renderRgbaResized", lambda: c.rgba_resized(drows=81, dcols=60, dst=None), resize_msg(81, 60)),
        ("renderRgbaResized", lambda: c.rgba_resized(drows=39, dcols=60, bleed=-1), resize_msg(39, 60)),
        ("renderRgbaResized", lambda: c.rgba_resized(dstep=70 * 4 - 1, bleed=17), "Output image has invalid size: expected 70x50."),
        ("renderSequenceRgba", lambda: c.rgba_sequence(srcs=[c.bgra.ctypes.data, None], dsts=[None, c.bgra_out.ctypes.data]), OUT_SIZE),      # frame 0's output before frame 1's input
        ("renderSequenceRgba", lambda: c.rgba_sequence(srcs=[c.bgra.ctypes.data, None], bleed=17), EMPTY),
        ("renderSequenceRgbaResized", lambda: c.rgba_sequence_resized(srcs=[None, None], drows=39, dcols=70), resize_msg(39, 70)),
        ("renderSequenceRgbaResized", lambda: c.rgba_sequence_resized(sstep=1, bleed=17), EMPTY),
        ("renderSharded", lambda: c.sharded(handles=[c.h, c.h], src=None), "renderSharded: the same engine twice."),
        ("renderSharded", lambda: c.sharded(src=None, dst=None), EMPTY),
        ("shardCompute", lambda: c.shard_compute(0, 0, src=None), "Invalid part index."),
        ("shardCompute", lambda: c.shard_compute(1, 1, sstep=1), "Invalid part index."),
    ]


def test_every_refusal_word_for_word(pkg, onnx_model):
    # an engine of its own: the first check needs one that has not computed a shard, and the last ones leave one that has
    eng = make_engine(pkg, onnx_model("swin_unet/art", S, 2, 64, small=True), 2, 64, S, overlap=(0.0625, 0.0625))
    c = Calls(eng)
    check(pkg, eng, "shardFinish", lambda: c.shard_finish(), "shardFinish without a shardCompute.")
    for who, call, text in table(c):
        check(pkg, eng, who, call, text)
    # an empty sequence is no refusal
    n = len(eng.messages)
    assert c.sequence(srcs=[], dsts=[]) is True and len(eng.messages) == n
    # shardFinish's own checks, behind a shardCompute of the whole frame
    assert c.shard_compute(0, 1)
    check(pkg, eng, "shardFinish", lambda: c.shard_finish(0, 0), "Invalid part index.")
    check(pkg, eng, "shardFinish", lambda: c.shard_finish(1, 1), "Invalid part index.")
    check(pkg, eng, "shardFinish", lambda: c.shard_finish(slabs=False), "Invalid part index.")
    check(pkg, eng, "shardFinish", lambda: c.shard_finish(dst=None), OUT_SIZE)
    check(pkg, eng, "shardFinish", lambda: c.shard_finish(rows=ROWS * S - 1), OUT_SIZE)
    check(pkg, eng, "shardFinish", lambda: c.shard_finish(dstep=COLS * S * 3 - 1), OUT_SIZE)
    check(pkg, eng, "shardFinish", lambda: c.shard_finish(0, 0, dst=None), "Invalid part index.")                    # two wrong: the part index first
    check(pkg, eng, "shardFinish", lambda: c.shard_finish(slabs=False, dstep=1), "Invalid part index.")
    assert c.shard_finish() and np.array_equal(c.out, eng.render(c.bgr))                                           # and the engine is usable
    eng.close()


def test_sharded_refusals_that_need_a_second_configuration(pkg, eng, onnx_model):
    """blend bands as wide as the tile stride (overlap 1/2) leave shard_plan() nothing to hand out; engines of two configurations do not shard one frame"""
    wide = make_engine(pkg, onnx_model("swin_unet/art", S, 2, 64, small=True), 2, 64, S, overlap=(0.5, 0.5))
    try:
        c = Calls(wide)
        check(pkg, wide, "renderSharded", c.sharded, "renderSharded: the blend bands are wider than the tile stride; use render or renderStrip.")
        check(pkg, wide, "shardCompute", c.shard_compute, "the blend bands are wider than the tile stride; use render or renderStrip.")
        check(pkg, wide, "shardCompute", lambda: c.shard_compute(src=None), EMPTY)                                   # the frame before the plan
        check(pkg, eng, "renderSharded", lambda: Calls(eng).sharded(handles=[eng._h, wide._h]), "renderSharded: engine 1 was loaded with another model or configuration.")
        check(pkg, eng, "renderSharded", lambda: Calls(eng).sharded(handles=[eng._h, wide._h], src=None), "renderSharded: engine 1 was loaded with another model or configuration.")
    finally:
        wide.close()


def test_resident_replay_of_a_frame_rendered_in_parts(pkg, eng):
    """render() of 30 tiles runs in parts, each with its own slot table; bench_resident() rebuilds the table of the frame as one part (one_part_slots) and
    replays it: the resident output is the bytes render() returned"""
    rows, cols = 200, 260
    assert pkg.calculate_tiles(cols, rows, cols * S, rows * S, 64, eng.output_tile_size, S, (0.0625, 0.0625))[0] >= 16
    frame = np.random.default_rng(23).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    out = eng.render(frame)
    assert eng.bench_resident(2) > 0
    res = np.empty_like(out)
    assert eng.resident_output(res) and np.array_equal(res, out)
    assert np.array_equal(eng.render(frame), out)


def test_two_things_wrong_the_first_check_wins(pkg, eng):
    c = Calls(eng)
    for who, call, text in two_wrong(c):
        check(pkg, eng, who, call, text)


def test_every_entry_refuses_an_engine_that_is_not_loaded(pkg, eng):
    fresh = pkg.Img2Img()
    try:
        c = Calls(fresh)
        for who, call in [("render", c.render), ("render", c.render16), ("renderStrip", lambda: c.strip(0, 1)), ("renderResized", c.resized), ("renderSequence", c.sequence),
                          ("renderSequenceResized", c.sequence_resized), ("renderYuv", c.yuv_call), ("renderYuv", c.yuv_layout), ("renderSequenceYuv", c.yuv_sequence),
                          ("renderSequenceYuv", c.yuv_sequence_layout), ("renderYuvResized", c.yuv_resized), ("renderSequenceYuvResized", c.yuv_sequence_resized),
                          ("renderGray", c.gray), ("renderGray", c.gray16), ("renderGrayResized", c.gray_resized), ("renderGrayResized", c.gray16_resized),
                          ("renderSequenceGray", c.gray_sequence), ("renderSequenceGrayResized", c.gray_sequence_resized), ("shardCompute", c.shard_compute)]:
            check(pkg, fresh, who, call, NOT_LOADED)
        check(pkg, fresh, "render", lambda: c.render(src=None), NOT_LOADED)                                         # before any argument check
        check(pkg, fresh, "shardCompute", lambda: c.shard_compute(0, 0), NOT_LOADED)
        check(pkg, fresh, "renderYuv", lambda: c.yuv_call(matrix=3), NOT_LOADED)
        check(pkg, fresh, "shardFinish", c.shard_finish, "shardFinish without a shardCompute.")
        check(pkg, fresh, "renderSharded", c.sharded, "Render called before a successful load (engine 0).")
        check(pkg, eng, "renderSharded", lambda: Calls(eng).sharded(handles=[eng._h, fresh._h]), "Render called before a successful load (engine 1).")
    finally:
        fresh.close()


def test_formats_interleaved_on_one_engine(pkg, eng):
    """the frame format of a call does not outlive it: BGR, YUV, RGBA, gray, resized and sequence calls between two equal render() calls.  The successful calls
    are what tests the reset of the job; the two refused ones are turned away before any job is set and only show that a refusal leaves the engine usable."""
    c = Calls(eng)
    rng = np.random.default_rng(11)
    bgra = rng.integers(0, 256, (ROWS, COLS, 4), dtype=np.uint8)
    first = eng.render(c.bgr)                                                                     # 1
    check(pkg, eng, "renderYuv", lambda: c.yuv_call(range=2), "Unknown YUV range 2.")             # 2
    yuv = eng.render_yuv(*c.yuv)                                                                  # 3
    rgba = eng.render_rgba_resized(bgra, (50, 70), bleed=2)                                       # 4
    with pytest.raises(pkg.W2xError, match=r"Alpha bleed radius 17 is not in \[0, 16\]\."):       # 5
        eng.render_sequence_rgba([bgra, bgra], bleed=17)
    small = eng.render_resized(c.bgr, (50, 70))                                                   # 6
    seq = eng.render_sequence([c.bgr, c.bgr[::-1].copy()])                                        # 7
    gray_frames = [c.gray8, c.gray8[::-1].copy()]
    gray = eng.render_gray(c.gray8)                                                               # 8
    gray_small = eng.render_gray_resized(c.gray8, (50, 70))                                       # 9
    gray_seq = eng.render_sequence_gray(gray_frames)                                              # 10
    last = eng.render(c.bgr)                                                                      # 11
    assert np.array_equal(first, last)
    assert np.array_equal(seq[0], first) and not np.array_equal(seq[1], first)
    assert eng.bench_resident(2) > 0
    res = np.empty_like(first)
    assert eng.resident_output(res) and np.array_equal(res, first)
    # and the calls in between gave what they give alone
    assert all(np.array_equal(a, b) for a, b in zip(yuv, eng.render_yuv(*c.yuv)))
    assert np.array_equal(rgba, eng.render_rgba_resized(bgra, (50, 70), bleed=2))
    assert np.array_equal(small, eng.render_resized(c.bgr, (50, 70)))
    assert np.array_equal(gray, eng.render_gray(c.gray8))
    assert np.array_equal(gray_small, eng.render_gray_resized(c.gray8, (50, 70)))
    alone = eng.render_sequence_gray(gray_frames)
    assert len(gray_seq) == 2 and all(np.array_equal(a, b) for a, b in zip(gray_seq, alone))
    assert np.array_equal(gray_seq[0], gray) and not np.array_equal(gray_seq[1], gray)
