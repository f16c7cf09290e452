"""Writes tests/golden/binding_calls.json: what the Python wrapper (waifu2x-tensorrt_amd/engine.py) passes to the C ABI, call by call, for every frame-taking
method of Img2Img and for render_sharded() and alpha_bleed() - with the declared restype / argtypes of every symbol as lib() leaves them.  No GPU: a real
Img2Img object gets a recording stub for its `_L`, whose w2x_* attributes log (entry, arguments) and return a scripted value; w2x_alloc_host hands out ctypes
buffers the stub keeps alive.  Pointers are logged as [buffer, byte offset] - a scenario's own array by name, "alloc<k>" the k-th array the wrapper allocated
(np.empty / np.zeros), "host<k>" the k-th w2x_alloc_host buffer - so the log carries no addresses.  After every scripted call the stub fills the output buffers
with the number of that call, which shows in "first" which call a returned array's bytes come from (the pinned rings return copies).

The file pins the wrapper's behaviour: argument values, C entry chosen, exception types and texts, messages, and that every page-locked buffer is given
back.  tests/test_binding_calls.py regenerates the log from the working tree and compares.  Re-run only when that behaviour changes on purpose:
python tests/golden/make_binding_calls.py [--engine-file other/engine.py]   (--engine-file: log another engine.py, bound to the package's library)"""
import ctypes as C
import importlib
import importlib.util
import json
import os
import sys

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "binding_calls.json")
u8, u16 = numpy.uint8, numpy.uint16
SCALING, BATCH, TILE, TILE_OUT = 2, 1, 64, 56


def load_engine(path=None):
    """the package's engine module, or another engine.py bound to the package's library"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    mod = importlib.import_module("waifu2x-tensorrt_amd.engine")
    if path is None:
        return mod
    spec = importlib.util.spec_from_file_location("w2x_engine_compared", path)
    other = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = other
    spec.loader.exec_module(other)
    other.lib_path = mod.lib_path
    return other


def type_name(t):
    if t is None:
        return None
    if hasattr(t, "_argtypes_") and hasattr(t, "_restype_"):      # a CFUNCTYPE
        return "CFUNCTYPE(" + ", ".join(str(type_name(a)) for a in (t._restype_,) + tuple(t._argtypes_)) + ")"
    return t.__name__


def declarations(mod):
    L = mod.lib()
    table = {}
    for name in sorted(mod.EXPORTED_SYMBOLS):
        fn = getattr(L, name)
        table[name] = [type_name(fn.restype), None if fn.argtypes is None else [type_name(t) for t in fn.argtypes]]
    return table


class Recorder:
    """the log of one scenario, and the buffers its pointers are named after"""

    def __init__(self, real):
        self.real = real
        self.reset()

    def reset(self):
        self.buffers, self.outputs, self.handles = [], [], []    # (name, address, bytes); arrays to fill; engine handles
        self.calls, self.allocs, self.hosts, self.freed = [], [], [], []
        self.fail, self.say, self.returns, self.count, self.renders = {}, None, {"w2x_output_tile_size": TILE_OUT}, {}, 0

    def register(self, name, array, output):
        self.buffers.append((name, array.ctypes.data, array.nbytes))
        if output:
            self.outputs.append(array)

    def allocated(self, array):
        array.fill(0xEE)
        self.allocs.append([list(array.shape), str(array.dtype)])
        self.register(f"alloc{len(self.allocs) - 1}", array, True)

    def where(self, address):
        if not address:
            return None
        for k, h in enumerate(self.handles):
            if address == h:
                return f"engine{k}"
        for name, base, n in self.buffers:
            if base <= address < base + max(n, 1):
                return [name, address - base]
        return "elsewhere"

    def norm(self, t, a):
        if isinstance(a, C.Array):
            return [self.where(v) for v in a] if a._type_ is C.c_void_p else [int(v) for v in a]
        if t is C.c_void_p:
            return self.where(a.value if isinstance(a, C.c_void_p) else a)
        return a.decode() if isinstance(a, bytes) else a

    def call(self, name, args):
        types = getattr(self.real, name).argtypes
        assert types is not None and len(types) == len(args), f"{name}: {len(args)} arguments for {types}"
        for t, a in zip(types, args):
            t.from_param(a)                                        # what ctypes itself would refuse
        self.calls.append([name, [self.norm(t, a) for t, a in zip(types, args)]])
        k = self.count[name] = self.count.get(name, 0) + 1
        failing = self.fail.get(name) in (True, k)
        if name == "w2x_alloc_host":
            if failing:
                return None
            buf = numpy.zeros(args[1], u8)
            self.hosts.append(buf.ctypes.data)
            self.register(f"host{len(self.hosts) - 1}", buf, True)
            return buf.ctypes.data
        if name == "w2x_free_host":
            self.freed.append(args[1])
            return None
        self.renders += 1
        for o in self.outputs:
            o.fill(self.renders)
        if failing:
            if self.say:
                self.say[0]._on_msg(1, self.say[1], None)
            return 0
        return self.returns.get(name, 1)

    def describe(self, v):
        if isinstance(v, numpy.ndarray):
            return {"shape": list(v.shape), "dtype": str(v.dtype), "strides": list(v.strides) if v.size else None, "in": self.where(v.ctypes.data) if v.size else None,
                    "first": int(v.flat[0]) if v.size else None}
        if isinstance(v, (list, tuple)):
            return [self.describe(x) for x in v]
        return v


class Stub:
    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        if not name.startswith("w2x_"):
            raise AttributeError(name)
        return lambda *args: self._rec.call(name, args)


class NumpyProxy:
    """numpy for the wrapper, with the arrays it allocates made known to the recorder"""

    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        return getattr(numpy, name)

    def empty(self, shape, dtype=float):
        a = numpy.empty(shape, dtype)
        self._rec.allocated(a)
        return a

    def zeros(self, shape, dtype=float):
        a = numpy.zeros(shape, dtype)
        self._rec.allocated(a)
        return a


class Ctx:
    """what a scenario works with: the module `m`, engines `e` / `e2`, named arrays, the stub's script"""

    def __init__(self, mod, rec, engines):
        self.m, self.rec, self.engines = mod, rec, engines
        self.e = engines[0]
        self.e2 = engines[-1]

    def arr(self, name, shape, dtype=u8, pad=0, out=False):
        """a zeroed array `name`; pad > 0: a view of rows that are `pad` elements of axis 1 longer"""
        shape = tuple(shape)
        base = numpy.zeros((shape[0], shape[1] + pad) + shape[2:], dtype)
        self.rec.register(name, base, out)
        return base[:, :shape[1]] if pad else base

    def bgr(self, name="src", r=4, c=6, dtype=u8, pad=0, ch=3, out=False):
        return self.arr(name, (r, c, ch), dtype, pad, out)

    def yuv(self, prefix, r, c, dtype=u8, layout="i420", pad=0, out=False):
        cr = (r + 1) // 2 if layout in ("i420", "nv12") else r
        cc = c if layout == "i444" else (c + 1) // 2
        shapes = [(r, c), (cr, 2 * cc)] if layout == "nv12" else [(r, c), (cr, cc), (cr, cc)]
        return tuple(self.arr(f"{prefix}.{'yuv'[k] if len(shapes) == 3 else ('y', 'uv')[k]}", s, dtype, pad, out) for k, s in enumerate(shapes))

    def fail(self, entry, which=True, say=None):
        self.rec.fail[entry] = which
        if say:
            self.rec.say = (self.e, say)


SCENARIOS = []


def S(name, fn, loaded=True, engines=1):
    SCENARIOS.append((name, loaded, engines, fn))


# ---- render / render16
S("render/alloc", lambda c: c.e.render(c.bgr()))
S("render/alloc16", lambda c: c.e.render(c.bgr(dtype=u16)))
S("render/padded_src", lambda c: c.e.render(c.bgr(pad=2)))
S("render/dst", lambda c: c.e.render(c.bgr(), c.bgr("dst", 8, 12, out=True)))
S("render/dst16_padded", lambda c: c.e.render(c.bgr(dtype=u16, pad=1), c.bgr("dst", 8, 12, u16, pad=3, out=True)))
S("render/fail_alloc", lambda c: (c.fail("w2x_render"), c.e.render(c.bgr()))[1])
S("render/fail_alloc_message", lambda c: (c.fail("w2x_render", say=b"[render@7] scripted refusal."), c.e.render(c.bgr()))[1])
S("render/fail_dst", lambda c: (c.fail("w2x_render16"), c.e.render(c.bgr(dtype=u16), c.bgr("dst", 8, 12, u16, out=True)))[1])
S("render/refuse_float", lambda c: c.e.render(numpy.zeros((4, 6, 3), numpy.float32)))
S("render/refuse_2d", lambda c: c.e.render(numpy.zeros((4, 6), u8)))
S("render/refuse_4ch", lambda c: c.e.render(numpy.zeros((4, 6, 4), u8)))
S("render/refuse_unpacked", lambda c: c.e.render(numpy.zeros((4, 6, 4), u8)[..., :3]))
S("render/refuse_dst_size", lambda c: c.e.render(c.bgr(), c.bgr("dst", 8, 11, out=True)))
S("render/refuse_dst_dtype", lambda c: c.e.render(c.bgr(), c.bgr("dst", 8, 12, u16, out=True)))
S("render/refuse_dst_unpacked", lambda c: c.e.render(c.bgr(), numpy.zeros((8, 12, 4), u8)[..., :3]))
S("render/empty", lambda c: c.e.render(numpy.zeros((0, 6, 3), u8)))
S("render/never_loaded_alloc", lambda c: c.e.render(c.bgr()), loaded=False)
S("render/never_loaded_dst_of_any_size", lambda c: c.e.render(c.bgr(), c.bgr("dst", 5, 5, out=True)), loaded=False)

# ---- render_rgba / render_rgba_resized / alpha_bleed_device
S("render_rgba/alloc", lambda c: c.e.render_rgba(c.bgr(ch=4)))
S("render_rgba/options_padded", lambda c: c.e.render_rgba(c.bgr(ch=4, pad=2), bleed=5, skip_uniform_alpha=True))
S("render_rgba/dst", lambda c: c.e.render_rgba(c.bgr(ch=4), dst=c.bgr("dst", 8, 12, ch=4, pad=1, out=True)))
S("render_rgba/empty", lambda c: c.e.render_rgba(numpy.zeros((0, 6, 4), u8)))
S("render_rgba/fail_alloc", lambda c: (c.fail("w2x_render_rgba"), c.e.render_rgba(c.bgr(ch=4)))[1])
S("render_rgba/fail_dst", lambda c: (c.fail("w2x_render_rgba"), c.e.render_rgba(c.bgr(ch=4), dst=c.bgr("dst", 8, 12, ch=4, out=True)))[1])
S("render_rgba/refuse_16bit_alloc", lambda c: c.e.render_rgba(c.bgr(ch=4, dtype=u16)))
S("render_rgba/refuse_16bit_dst", lambda c: c.e.render_rgba(c.bgr(ch=4, dtype=u16), dst=c.bgr("dst", 8, 12, ch=4, out=True)))
S("render_rgba/refuse_3ch", lambda c: c.e.render_rgba(c.bgr()))
S("render_rgba/refuse_list", lambda c: c.e.render_rgba([[0, 0, 0, 0]]))
S("render_rgba/refuse_unpacked", lambda c: c.e.render_rgba(numpy.zeros((4, 6, 5), u8)[..., :4]))
S("render_rgba/refuse_dst_size", lambda c: c.e.render_rgba(c.bgr(ch=4), dst=c.bgr("dst", 9, 12, ch=4, out=True)))
S("render_rgba/refuse_dst_3ch", lambda c: c.e.render_rgba(c.bgr(ch=4), dst=c.bgr("dst", 8, 12, out=True)))
S("render_rgba/never_loaded_alloc", lambda c: c.e.render_rgba(c.bgr(ch=4)), loaded=False)
S("render_rgba/never_loaded_dst_of_any_size", lambda c: c.e.render_rgba(c.bgr(ch=4), dst=c.bgr("dst", 5, 5, ch=4, out=True)), loaded=False)
S("render_rgba_resized/alloc", lambda c: c.e.render_rgba_resized(c.bgr(ch=4), (7, 9)))
S("render_rgba_resized/options", lambda c: c.e.render_rgba_resized(c.bgr(ch=4, pad=3), (7, 9), bleed=16, skip_uniform_alpha=True, filter="bilinear"))
S("render_rgba_resized/dst", lambda c: c.e.render_rgba_resized(c.bgr(ch=4), (7, 9), dst=c.bgr("dst", 7, 9, ch=4, pad=2, out=True)))
S("render_rgba_resized/empty_target", lambda c: c.e.render_rgba_resized(c.bgr(ch=4), (0, 9)))
S("render_rgba_resized/fail_alloc", lambda c: (c.fail("w2x_render_rgba_resized"), c.e.render_rgba_resized(c.bgr(ch=4), (7, 9)))[1])
S("render_rgba_resized/fail_dst", lambda c: (c.fail("w2x_render_rgba_resized"), c.e.render_rgba_resized(c.bgr(ch=4), (7, 9), dst=c.bgr("dst", 7, 9, ch=4, out=True)))[1])
S("render_rgba_resized/refuse_16bit_alloc", lambda c: c.e.render_rgba_resized(c.bgr(ch=4, dtype=u16), (7, 9)))
S("render_rgba_resized/refuse_16bit_dst", lambda c: c.e.render_rgba_resized(c.bgr(ch=4, dtype=u16), (7, 9), dst=c.bgr("dst", 7, 9, ch=4, out=True)))
S("render_rgba_resized/refuse_3ch", lambda c: c.e.render_rgba_resized(c.bgr(), (7, 9)))
S("render_rgba_resized/refuse_filter", lambda c: c.e.render_rgba_resized(c.bgr(ch=4), (7, 9), filter="lanczos"))
S("render_rgba_resized/refuse_negative_size", lambda c: c.e.render_rgba_resized(c.bgr(ch=4), (-1, 9)))
S("render_rgba_resized/refuse_dst_size", lambda c: c.e.render_rgba_resized(c.bgr(ch=4), (7, 9), dst=c.bgr("dst", 8, 9, ch=4, out=True)))
S("alpha_bleed_device/ok", lambda c: c.e.alpha_bleed_device(c.bgr(ch=4, pad=1), 3))
S("alpha_bleed_device/empty", lambda c: c.e.alpha_bleed_device(numpy.zeros((4, 0, 4), u8), 3))
S("alpha_bleed_device/fail", lambda c: (c.fail("w2x_alpha_bleed_device"), c.e.alpha_bleed_device(c.bgr(ch=4), 17))[1])
S("alpha_bleed_device/refuse_3ch", lambda c: c.e.alpha_bleed_device(c.bgr(), 3))
S("alpha_bleed_device/refuse_16bit", lambda c: c.e.alpha_bleed_device(c.bgr(ch=4, dtype=u16), 3))


def frames(c, n=4, ch=3, r=4, cc=6, dtype=u8):
    return [c.bgr(f"frame{k}", r, cc, dtype, ch=ch) for k in range(n)]


def outs(c, n, r, cc, ch=3, dtype=u8):
    return [c.bgr(f"out{k}", r, cc, dtype, ch=ch, out=True) for k in range(n)]


# ---- render_sequence_rgba
S("render_sequence_rgba/empty", lambda c: c.e.render_sequence_rgba([]))
S("render_sequence_rgba/alloc", lambda c: c.e.render_sequence_rgba(frames(c, 4, 4)))
S("render_sequence_rgba/options", lambda c: c.e.render_sequence_rgba(frames(c, 2, 4), bleed=2, skip_uniform_alpha=True))
S("render_sequence_rgba/size", lambda c: c.e.render_sequence_rgba(frames(c, 2, 4), size=(7, 9), bleed=1, filter="bilinear"))
S("render_sequence_rgba/outs", lambda c: c.e.render_sequence_rgba(frames(c, 2, 4), outs=outs(c, 2, 8, 12, 4)))
S("render_sequence_rgba/outs_size", lambda c: c.e.render_sequence_rgba(frames(c, 2, 4), size=(7, 9), outs=outs(c, 2, 7, 9, 4)))
S("render_sequence_rgba/outs_short_leaves_null", lambda c: c.e.render_sequence_rgba(frames(c, 3, 4), outs=outs(c, 2, 8, 12, 4)))
S("render_sequence_rgba/outs_long", lambda c: c.e.render_sequence_rgba(frames(c, 2, 4), size=(7, 9), outs=outs(c, 3, 7, 9, 4)))
S("render_sequence_rgba/outs_and_pinned", lambda c: c.e.render_sequence_rgba(frames(c, 2, 4), outs=outs(c, 2, 8, 12, 4), pinned=True))
S("render_sequence_rgba/pinned", lambda c: c.e.render_sequence_rgba(frames(c, 4, 4), pinned=True))
S("render_sequence_rgba/pinned_two", lambda c: c.e.render_sequence_rgba(frames(c, 2, 4), pinned=True))
S("render_sequence_rgba/pinned_size", lambda c: c.e.render_sequence_rgba(frames(c, 4, 4), size=(7, 9), pinned=True))
S("render_sequence_rgba/fail", lambda c: (c.fail("w2x_render_sequence_rgba"), c.e.render_sequence_rgba(frames(c, 2, 4)))[1])
S("render_sequence_rgba/fail_size_message", lambda c: (c.fail("w2x_render_sequence_rgba_resized", say=b"[renderSequenceRgbaResized@3] scripted refusal."),
                                                        c.e.render_sequence_rgba(frames(c, 2, 4), size=(7, 9)))[1])
S("render_sequence_rgba/fail_pinned_second_piece", lambda c: (c.fail("w2x_render_sequence_rgba", 2), c.e.render_sequence_rgba(frames(c, 4, 4), pinned=True))[1])
S("render_sequence_rgba/fail_alloc_host", lambda c: (c.fail("w2x_alloc_host", 1), c.e.render_sequence_rgba(frames(c, 4, 4), pinned=True))[1])
S("render_sequence_rgba/refuse_3ch", lambda c: c.e.render_sequence_rgba(frames(c, 2, 3)))
S("render_sequence_rgba/refuse_16bit", lambda c: c.e.render_sequence_rgba(frames(c, 2, 4, dtype=u16)))
S("render_sequence_rgba/refuse_padded", lambda c: c.e.render_sequence_rgba([c.bgr("frame0", ch=4), c.bgr("frame1", ch=4, pad=1)]))
S("render_sequence_rgba/refuse_sizes_differ", lambda c: c.e.render_sequence_rgba([c.bgr("frame0", ch=4), c.bgr("frame1", 4, 7, ch=4)]))
S("render_sequence_rgba/refuse_filter", lambda c: c.e.render_sequence_rgba(frames(c, 2, 4), size=(7, 9), filter="lanczos"))
S("render_sequence_rgba/refuse_outs_size", lambda c: c.e.render_sequence_rgba(frames(c, 2, 4), outs=outs(c, 2, 8, 11, 4)))
S("render_sequence_rgba/empty_target", lambda c: c.e.render_sequence_rgba(frames(c, 2, 4), size=(0, 9)))
S("render_sequence_rgba/never_loaded", lambda c: c.e.render_sequence_rgba(frames(c, 2, 4)), loaded=False)

# ---- render_resized / render_sequence_resized
S("render_resized/alloc", lambda c: c.e.render_resized(c.bgr(), (7, 9)))
S("render_resized/alloc16_bilinear", lambda c: c.e.render_resized(c.bgr(dtype=u16, pad=1), (7, 9), "bilinear"))
S("render_resized/dst", lambda c: c.e.render_resized(c.bgr(), (7, 9), dst=c.bgr("dst", 7, 9, pad=2, out=True)))
S("render_resized/dst16", lambda c: c.e.render_resized(c.bgr(dtype=u16), (7, 9), dst=c.bgr("dst", 7, 9, u16, out=True)))
S("render_resized/empty_target", lambda c: c.e.render_resized(c.bgr(), (7, 0)))
S("render_resized/fail_alloc", lambda c: (c.fail("w2x_render_resized"), c.e.render_resized(c.bgr(), (7, 9)))[1])
S("render_resized/fail_dst", lambda c: (c.fail("w2x_render16_resized"), c.e.render_resized(c.bgr(dtype=u16), (7, 9), dst=c.bgr("dst", 7, 9, u16, out=True)))[1])
S("render_resized/refuse_4ch", lambda c: c.e.render_resized(c.bgr(ch=4), (7, 9)))
S("render_resized/refuse_filter", lambda c: c.e.render_resized(c.bgr(), (7, 9), "lanczos"))
S("render_resized/refuse_negative_size", lambda c: c.e.render_resized(c.bgr(), (7, -2)))
S("render_resized/refuse_dst_size", lambda c: c.e.render_resized(c.bgr(), (7, 9), dst=c.bgr("dst", 7, 10, out=True)))
S("render_resized/refuse_dst_dtype", lambda c: c.e.render_resized(c.bgr(), (7, 9), dst=c.bgr("dst", 7, 9, u16, out=True)))
S("render_sequence_resized/empty", lambda c: c.e.render_sequence_resized([], (7, 9)))
S("render_sequence_resized/alloc", lambda c: c.e.render_sequence_resized(frames(c, 4), (7, 9)))
S("render_sequence_resized/bilinear", lambda c: c.e.render_sequence_resized(frames(c, 2), (7, 9), filter="bilinear"))
S("render_sequence_resized/outs", lambda c: c.e.render_sequence_resized(frames(c, 2), (7, 9), outs(c, 2, 7, 9)))
S("render_sequence_resized/outs_short_leaves_null", lambda c: c.e.render_sequence_resized(frames(c, 3), (7, 9), outs(c, 2, 7, 9)))
S("render_sequence_resized/outs_long", lambda c: c.e.render_sequence_resized(frames(c, 2), (7, 9), outs(c, 3, 7, 9)))
S("render_sequence_resized/outs_and_pinned", lambda c: c.e.render_sequence_resized(frames(c, 2), (7, 9), outs(c, 2, 7, 9), True))
S("render_sequence_resized/pinned", lambda c: c.e.render_sequence_resized(frames(c, 4), (7, 9), pinned=True))
S("render_sequence_resized/fail", lambda c: (c.fail("w2x_render_sequence_resized"), c.e.render_sequence_resized(frames(c, 2), (7, 9)))[1])
S("render_sequence_resized/fail_pinned_second_piece", lambda c: (c.fail("w2x_render_sequence_resized", 2), c.e.render_sequence_resized(frames(c, 4), (7, 9), pinned=True))[1])
S("render_sequence_resized/empty_target", lambda c: c.e.render_sequence_resized(frames(c, 2), (7, 0)))
S("render_sequence_resized/never_loaded", lambda c: c.e.render_sequence_resized(frames(c, 2), (7, 9)), loaded=False)
S("render_sequence_resized/refuse_16bit", lambda c: c.e.render_sequence_resized(frames(c, 2, dtype=u16), (7, 9)))
S("render_sequence_resized/refuse_sizes_differ", lambda c: c.e.render_sequence_resized([c.bgr("frame0"), c.bgr("frame1", 5, 6)], (7, 9)))
S("render_sequence_resized/refuse_filter", lambda c: c.e.render_sequence_resized(frames(c, 2), (7, 9), filter="lanczos"))
S("render_sequence_resized/refuse_outs_size", lambda c: c.e.render_sequence_resized(frames(c, 2), (7, 9), outs(c, 2, 8, 12)))

# ---- render_sequence
S("render_sequence/empty", lambda c: c.e.render_sequence([]))
S("render_sequence/alloc", lambda c: c.e.render_sequence(frames(c, 4)))
S("render_sequence/outs", lambda c: c.e.render_sequence(frames(c, 2), outs(c, 2, 8, 12)))
S("render_sequence/outs_ring", lambda c: (lambda o: c.e.render_sequence(frames(c, 4), [o[0], o[1], o[0], o[1]]))(outs(c, 2, 8, 12)))
S("render_sequence/outs_short_leaves_null", lambda c: c.e.render_sequence(frames(c, 3), outs(c, 2, 8, 12)))
S("render_sequence/outs_long", lambda c: c.e.render_sequence(frames(c, 2), outs(c, 3, 8, 12)))
S("render_sequence/outs_and_pinned", lambda c: c.e.render_sequence(frames(c, 2), outs(c, 2, 8, 12), True))
S("render_sequence/pinned", lambda c: c.e.render_sequence(frames(c, 4), pinned=True))
S("render_sequence/pinned_one", lambda c: c.e.render_sequence(frames(c, 1), pinned=True))
S("render_sequence/fail", lambda c: (c.fail("w2x_render_sequence"), c.e.render_sequence(frames(c, 2)))[1])
S("render_sequence/fail_message", lambda c: (c.fail("w2x_render_sequence", say=b"[renderSequence@5] scripted refusal."), c.e.render_sequence(frames(c, 2)))[1])
S("render_sequence/fail_pinned_second_piece", lambda c: (c.fail("w2x_render_sequence", 2), c.e.render_sequence(frames(c, 4), pinned=True))[1])
S("render_sequence/fail_alloc_host", lambda c: (c.fail("w2x_alloc_host", 1), c.e.render_sequence(frames(c, 4), pinned=True))[1])
S("render_sequence/refuse_16bit", lambda c: c.e.render_sequence(frames(c, 2, dtype=u16)))
S("render_sequence/refuse_4ch", lambda c: c.e.render_sequence(frames(c, 2, 4)))
S("render_sequence/refuse_sizes_differ", lambda c: c.e.render_sequence([c.bgr("frame0"), c.bgr("frame1", 4, 5)]))
S("render_sequence/refuse_padded", lambda c: c.e.render_sequence([c.bgr("frame0", pad=1)]))
S("render_sequence/refuse_outs_size", lambda c: c.e.render_sequence(frames(c, 2), outs(c, 2, 7, 12)))
S("render_sequence/never_loaded", lambda c: c.e.render_sequence(frames(c, 2)), loaded=False)

# ---- render_strip / shard_compute / shard_finish / render_sharded
S("render_strip/ok", lambda c: c.e.render_strip(c.bgr(pad=1), c.bgr("dst", 8, 12, pad=2, out=True), 1, 3))
S("render_strip/fail", lambda c: (c.fail("w2x_render_strip"), c.e.render_strip(c.bgr(), c.bgr("dst", 8, 12, out=True), 0, 2))[1])
S("render_strip/refuse_src16", lambda c: c.e.render_strip(c.bgr(dtype=u16), c.bgr("dst", 8, 12, out=True), 0, 2))
S("render_strip/refuse_dst_size", lambda c: c.e.render_strip(c.bgr(), c.bgr("dst", 8, 13, out=True), 0, 2))
S("shard_compute/ok", lambda c: c.e.shard_compute(c.bgr(pad=2), 1, 2))
S("shard_compute/fail", lambda c: (c.fail("w2x_shard_compute"), c.e.shard_compute(c.bgr(), 0, 2))[1])
S("shard_compute/refuse_4ch", lambda c: c.e.shard_compute(c.bgr(ch=4), 0, 2))
S("shard_finish/ok", lambda c: c.e.shard_finish(c.bgr("dst", 8, 12, pad=1, out=True), 2, 3, [c.arr("slab0", (1, 64)).ctypes.data, 0, 0]))
S("shard_finish/devices", lambda c: c.e.shard_finish(c.bgr("dst", 8, 12, out=True), 1, 2, [c.arr("slab0", (1, 64)).ctypes.data, 0], devices=[3, 1]))
S("shard_finish/fail", lambda c: (c.fail("w2x_shard_finish"), c.e.shard_finish(c.bgr("dst", 8, 12, out=True), 0, 1, [0]))[1])
S("shard_finish/refuse_dst16", lambda c: c.e.shard_finish(c.bgr("dst", 8, 12, u16, out=True), 0, 1, [0]))
S("render_sharded/alloc", lambda c: c.m.render_sharded(c.engines, c.bgr(pad=1)), engines=2)
S("render_sharded/dst", lambda c: c.m.render_sharded(c.engines, c.bgr(), c.bgr("dst", 8, 12, pad=1, out=True)), engines=2)
S("render_sharded/fail", lambda c: (c.fail("w2x_render_sharded"), c.m.render_sharded(c.engines, c.bgr()))[1], engines=2)
S("render_sharded/fail_message", lambda c: (c.fail("w2x_render_sharded", say=b"[renderSharded@9] scripted refusal."), c.m.render_sharded(c.engines, c.bgr()))[1], engines=2)
S("render_sharded/refuse_src16", lambda c: c.m.render_sharded(c.engines, c.bgr(dtype=u16)), engines=2)
S("render_sharded/refuse_dst_size", lambda c: c.m.render_sharded(c.engines, c.bgr(), c.bgr("dst", 8, 11, out=True)), engines=2)
S("render_sharded/never_loaded", lambda c: c.m.render_sharded(c.engines, c.bgr()), loaded=False)

# ---- render_yuv / render_yuv_resized
S("render_yuv/alloc", lambda c: c.e.render_yuv(*c.yuv("src", 5, 7)))
S("render_yuv/alloc10_full_bt2020", lambda c: c.e.render_yuv(*c.yuv("src", 4, 6, u16), matrix="bt2020", full_range=True))
S("render_yuv/out_bits10", lambda c: c.e.render_yuv(*c.yuv("src", 4, 6), out_bits=10))
S("render_yuv/out_bits8_padded", lambda c: c.e.render_yuv(*c.yuv("src", 4, 6, u16, pad=2), out_bits=8, matrix="bt601"))
S("render_yuv/out_bits12_goes_to_the_library", lambda c: c.e.render_yuv(*c.yuv("src", 4, 6), out_bits=12))
S("render_yuv/out", lambda c: c.e.render_yuv(*c.yuv("src", 5, 7), out=c.yuv("out", 10, 14, pad=1, out=True)))
S("render_yuv/out_list10", lambda c: c.e.render_yuv(*c.yuv("src", 4, 6), out_bits=10, out=list(c.yuv("out", 8, 12, u16, out=True))))
S("render_yuv/fail_alloc", lambda c: (c.fail("w2x_render_yuv"), c.e.render_yuv(*c.yuv("src", 4, 6)))[1])
S("render_yuv/fail_out", lambda c: (c.fail("w2x_render_yuv"), c.e.render_yuv(*c.yuv("src", 4, 6), out=c.yuv("out", 8, 12, out=True)))[1])
S("render_yuv/refuse_i422_planes", lambda c: c.e.render_yuv(*c.yuv("src", 4, 6, layout="i422")))
S("render_yuv/refuse_mixed_depths", lambda c: (lambda p, q: c.e.render_yuv(p[0], q[1], p[2]))(c.yuv("src", 4, 6), c.yuv("other", 4, 6, u16)))
S("render_yuv/refuse_float", lambda c: c.e.render_yuv(*c.yuv("src", 4, 6, numpy.float32)))
S("render_yuv/refuse_matrix", lambda c: c.e.render_yuv(*c.yuv("src", 4, 6), matrix="bt470"))
S("render_yuv/refuse_out_shapes", lambda c: c.e.render_yuv(*c.yuv("src", 4, 6), out=c.yuv("out", 8, 12, layout="i444", out=True)))
S("render_yuv/refuse_out_depth", lambda c: c.e.render_yuv(*c.yuv("src", 4, 6), out_bits=10, out=c.yuv("out", 8, 12, out=True)))
S("render_yuv/refuse_out_two_planes", lambda c: c.e.render_yuv(*c.yuv("src", 4, 6), out=c.yuv("out", 8, 12, out=True)[:2]))
S("render_yuv/never_loaded_alloc", lambda c: c.e.render_yuv(*c.yuv("src", 4, 6)), loaded=False)
S("render_yuv/never_loaded_out", lambda c: c.e.render_yuv(*c.yuv("src", 4, 6), out=c.yuv("out", 8, 12, out=True)), loaded=False)
S("render_yuv/tuple", lambda c: c.e.render_yuv(c.yuv("src", 5, 7)))
S("render_yuv/layout_i420", lambda c: c.e.render_yuv(*c.yuv("src", 5, 7), layout="i420"))
S("render_yuv/layout_i422_to_i444", lambda c: c.e.render_yuv(c.yuv("src", 5, 7, layout="i422"), layout="i422", out_layout="i444", out_bits=10))
S("render_yuv/out_layout_only", lambda c: c.e.render_yuv(*c.yuv("src", 4, 6, u16), out_layout="nv12", matrix="bt601", full_range=True))
S("render_yuv/nv12", lambda c: c.e.render_yuv(c.yuv("src", 5, 7, layout="nv12", pad=2), layout="nv12"))
S("render_yuv/nv12_positional_to_i420", lambda c: c.e.render_yuv(*c.yuv("src", 5, 7, u16, layout="nv12"), layout="nv12", out_layout="i420"))
S("render_yuv/layout_out", lambda c: c.e.render_yuv(c.yuv("src", 4, 6), out_layout="nv12", out=c.yuv("out", 8, 12, layout="nv12", pad=2, out=True)))
S("render_yuv/layout_fail_alloc", lambda c: (c.fail("w2x_render_yuv_layout"), c.e.render_yuv(c.yuv("src", 4, 6)))[1])
S("render_yuv/layout_fail_out", lambda c: (c.fail("w2x_render_yuv_layout"), c.e.render_yuv(c.yuv("src", 4, 6), out=c.yuv("out", 8, 12, out=True)))[1])
S("render_yuv/layout_refuse_tuple_and_planes", lambda c: (lambda p: c.e.render_yuv(p, p[1]))(c.yuv("src", 4, 6)))
S("render_yuv/layout_refuse_name", lambda c: c.e.render_yuv(c.yuv("src", 4, 6), layout="yuy2"))
S("render_yuv/layout_refuse_planes", lambda c: c.e.render_yuv(c.yuv("src", 4, 6), layout="i444"))
S("render_yuv/layout_refuse_two_planes", lambda c: c.e.render_yuv(c.yuv("src", 4, 6, layout="nv12"), layout="i420"))
S("render_yuv/layout_refuse_out_shapes", lambda c: c.e.render_yuv(c.yuv("src", 4, 6), out_layout="i422", out=c.yuv("out", 8, 12, out=True)))
S("render_yuv/layout_refuse_matrix", lambda c: c.e.render_yuv(c.yuv("src", 4, 6), matrix="bt470"))
S("render_yuv/layout_never_loaded_alloc", lambda c: c.e.render_yuv(c.yuv("src", 4, 6)), loaded=False)
S("render_yuv/layout_never_loaded_out", lambda c: c.e.render_yuv(c.yuv("src", 4, 6), out=c.yuv("out", 8, 12, out=True)), loaded=False)
S("render_yuv_resized/alloc", lambda c: c.e.render_yuv_resized(*c.yuv("src", 5, 7), (9, 11)))
S("render_yuv_resized/options", lambda c: c.e.render_yuv_resized(*c.yuv("src", 4, 6, u16, pad=1), (7, 9), matrix="bt601", full_range=True, out_bits=8, filter="bilinear"))
S("render_yuv_resized/dst", lambda c: c.e.render_yuv_resized(*c.yuv("src", 4, 6), (7, 9), out_bits=10, dst=c.yuv("dst", 7, 9, u16, pad=1, out=True)))
S("render_yuv_resized/empty_target", lambda c: c.e.render_yuv_resized(*c.yuv("src", 4, 6), (0, 9)))
S("render_yuv_resized/fail_alloc", lambda c: (c.fail("w2x_render_yuv_resized"), c.e.render_yuv_resized(*c.yuv("src", 4, 6), (7, 9)))[1])
S("render_yuv_resized/fail_dst", lambda c: (c.fail("w2x_render_yuv_resized"), c.e.render_yuv_resized(*c.yuv("src", 4, 6), (7, 9), dst=c.yuv("dst", 7, 9, out=True)))[1])
S("render_yuv_resized/refuse_i444_planes", lambda c: c.e.render_yuv_resized(*c.yuv("src", 4, 6, layout="i444"), (7, 9)))
S("render_yuv_resized/refuse_filter", lambda c: c.e.render_yuv_resized(*c.yuv("src", 4, 6), (7, 9), filter="lanczos"))
S("render_yuv_resized/refuse_matrix", lambda c: c.e.render_yuv_resized(*c.yuv("src", 4, 6), (7, 9), matrix="bt470"))
S("render_yuv_resized/negative_size_goes_to_the_library", lambda c: c.e.render_yuv_resized(*c.yuv("src", 4, 6), (7, -1)))
S("render_yuv_resized/refuse_dst_shapes", lambda c: c.e.render_yuv_resized(*c.yuv("src", 4, 6), (7, 9), dst=c.yuv("dst", 8, 12, out=True)))
S("render_yuv_resized/refuse_dst_depth", lambda c: c.e.render_yuv_resized(*c.yuv("src", 4, 6), (7, 9), out_bits=10, dst=c.yuv("dst", 7, 9, out=True)))


def yframes(c, n=4, r=4, cc=6, dtype=u8, layout="i420", pad=0):
    return [c.yuv(f"frame{k}", r, cc, dtype, layout, pad) for k in range(n)]


# ---- render_sequence_yuv / render_sequence_yuv_resized
S("render_sequence_yuv/empty", lambda c: c.e.render_sequence_yuv([]))
S("render_sequence_yuv/alloc", lambda c: c.e.render_sequence_yuv(yframes(c, 4, 5, 7)))
S("render_sequence_yuv/options", lambda c: c.e.render_sequence_yuv([list(f) for f in yframes(c, 2, dtype=u16, pad=1)], matrix="bt2020", full_range=True, out_bits=8))
S("render_sequence_yuv/out_bits12_goes_to_the_library", lambda c: c.e.render_sequence_yuv(yframes(c, 2), out_bits=12))
S("render_sequence_yuv/pinned", lambda c: c.e.render_sequence_yuv(yframes(c, 4, 5, 7), pinned=True))
S("render_sequence_yuv/pinned10_two", lambda c: c.e.render_sequence_yuv(yframes(c, 2), out_bits=10, pinned=True))
S("render_sequence_yuv/layout_i420", lambda c: c.e.render_sequence_yuv(yframes(c, 2), layout="i420"))
S("render_sequence_yuv/layout_i444_to_i422", lambda c: c.e.render_sequence_yuv(yframes(c, 2, layout="i444"), layout="i444", out_layout="i422", out_bits=10))
S("render_sequence_yuv/out_layout_only", lambda c: c.e.render_sequence_yuv(yframes(c, 2), out_layout="i444"))
S("render_sequence_yuv/nv12", lambda c: c.e.render_sequence_yuv(yframes(c, 2, 5, 7, layout="nv12"), layout="nv12"))
S("render_sequence_yuv/nv12_pinned", lambda c: c.e.render_sequence_yuv(yframes(c, 4, 5, 7, u16, "nv12"), layout="nv12", pinned=True))
S("render_sequence_yuv/nv12_to_i420_pinned", lambda c: c.e.render_sequence_yuv(yframes(c, 4, layout="nv12"), layout="nv12", out_layout="i420", pinned=True))
S("render_sequence_yuv/fail", lambda c: (c.fail("w2x_render_sequence_yuv"), c.e.render_sequence_yuv(yframes(c, 2)))[1])
S("render_sequence_yuv/fail_message", lambda c: (c.fail("w2x_render_sequence_yuv", say=b"[renderSequenceYuv@4] scripted refusal."), c.e.render_sequence_yuv(yframes(c, 2)))[1])
S("render_sequence_yuv/fail_layout", lambda c: (c.fail("w2x_render_sequence_yuv_layout"), c.e.render_sequence_yuv(yframes(c, 2), layout="i420"))[1])
S("render_sequence_yuv/fail_pinned_second_piece", lambda c: (c.fail("w2x_render_sequence_yuv", 2), c.e.render_sequence_yuv(yframes(c, 4), pinned=True))[1])
S("render_sequence_yuv/fail_layout_pinned_second_piece", lambda c: (c.fail("w2x_render_sequence_yuv_layout", 2),
                                                                     c.e.render_sequence_yuv(yframes(c, 4, layout="nv12"), layout="nv12", pinned=True))[1])
S("render_sequence_yuv/fail_alloc_host", lambda c: (c.fail("w2x_alloc_host", 1), c.e.render_sequence_yuv(yframes(c, 4), pinned=True))[1])
S("render_sequence_yuv/refuse_i422_planes", lambda c: c.e.render_sequence_yuv(yframes(c, 2, layout="i422")))
S("render_sequence_yuv/refuse_second_frame_size", lambda c: c.e.render_sequence_yuv([c.yuv("frame0", 4, 6), c.yuv("frame1", 4, 8)]))
S("render_sequence_yuv/refuse_second_frame_depth", lambda c: c.e.render_sequence_yuv([c.yuv("frame0", 4, 6), c.yuv("frame1", 4, 6, u16)]))
S("render_sequence_yuv/refuse_second_frame_layout", lambda c: c.e.render_sequence_yuv([c.yuv("frame0", 4, 6), c.yuv("frame1", 4, 6, layout="i444")]))
S("render_sequence_yuv/refuse_second_frame_steps", lambda c: c.e.render_sequence_yuv([c.yuv("frame0", 4, 6), c.yuv("frame1", 4, 6, pad=1)]))
S("render_sequence_yuv/refuse_matrix", lambda c: c.e.render_sequence_yuv(yframes(c, 2), matrix="bt470"))
S("render_sequence_yuv/refuse_matrix_pinned", lambda c: c.e.render_sequence_yuv(yframes(c, 2), matrix="bt470", pinned=True))
S("render_sequence_yuv/layout_refuse_name", lambda c: c.e.render_sequence_yuv(yframes(c, 2), layout="yuy2"))
S("render_sequence_yuv/layout_refuse_planes", lambda c: c.e.render_sequence_yuv(yframes(c, 2), layout="nv12"))
S("render_sequence_yuv/layout_refuse_second_frame", lambda c: c.e.render_sequence_yuv([c.yuv("frame0", 4, 6, layout="nv12"), c.yuv("frame1", 4, 6)], layout="nv12"))
S("render_sequence_yuv/two_planes_go_to_the_library", lambda c: c.e.render_sequence_yuv([f[:2] for f in yframes(c, 2)]))
S("render_sequence_yuv/layout_never_loaded", lambda c: c.e.render_sequence_yuv(yframes(c, 2), layout="i420"), loaded=False)
S("render_sequence_yuv/never_loaded_pinned", lambda c: c.e.render_sequence_yuv(yframes(c, 2), pinned=True), loaded=False)
S("render_sequence_yuv/never_loaded", lambda c: c.e.render_sequence_yuv(yframes(c, 2)), loaded=False)
S("render_sequence_yuv_resized/empty", lambda c: c.e.render_sequence_yuv_resized([], (7, 9)))
S("render_sequence_yuv_resized/alloc", lambda c: c.e.render_sequence_yuv_resized(yframes(c, 4, 5, 7), (9, 11)))
S("render_sequence_yuv_resized/options", lambda c: c.e.render_sequence_yuv_resized(yframes(c, 2, dtype=u16, pad=2), (7, 9), matrix="bt601", full_range=True, out_bits=8, filter="bilinear"))
S("render_sequence_yuv_resized/pinned", lambda c: c.e.render_sequence_yuv_resized(yframes(c, 4), (7, 9), out_bits=10, pinned=True))
S("render_sequence_yuv_resized/empty_target", lambda c: c.e.render_sequence_yuv_resized(yframes(c, 2), (0, 9)))
S("render_sequence_yuv_resized/fail", lambda c: (c.fail("w2x_render_sequence_yuv_resized"), c.e.render_sequence_yuv_resized(yframes(c, 2), (7, 9)))[1])
S("render_sequence_yuv_resized/fail_pinned_second_piece", lambda c: (c.fail("w2x_render_sequence_yuv_resized", 2), c.e.render_sequence_yuv_resized(yframes(c, 4), (7, 9), pinned=True))[1])
S("render_sequence_yuv_resized/refuse_i444_planes", lambda c: c.e.render_sequence_yuv_resized(yframes(c, 2, layout="i444"), (7, 9)))
S("render_sequence_yuv_resized/refuse_second_frame", lambda c: c.e.render_sequence_yuv_resized([c.yuv("frame0", 4, 6), c.yuv("frame1", 4, 6, layout="i422")], (7, 9)))
S("render_sequence_yuv_resized/refuse_filter", lambda c: c.e.render_sequence_yuv_resized(yframes(c, 2), (7, 9), filter="lanczos"))

# ---- infer (the blob of a tile batch) and the host bleed
S("infer/ok", lambda c: c.e.infer(c.arr("blob", (BATCH, 3, TILE, TILE), numpy.float32)))
S("infer/converted", lambda c: c.e.infer(numpy.zeros((BATCH, 3, TILE, TILE), numpy.float64)))
S("infer/fail", lambda c: (c.fail("w2x_infer"), c.e.infer(c.arr("blob", (BATCH, 3, TILE, TILE), numpy.float32)))[1])
S("infer/refuse_shape", lambda c: c.e.infer(numpy.zeros((BATCH, 3, TILE, TILE + 1), numpy.float32)))
S("infer/never_loaded", lambda c: c.e.infer(numpy.zeros((BATCH, 3, TILE, TILE), numpy.float32)), loaded=False)
S("alpha_bleed/ok", lambda c: c.m.alpha_bleed(c.bgr("bgr"), c.arr("alpha", (4, 6)), 3))
S("alpha_bleed/padded", lambda c: c.m.alpha_bleed(c.bgr("bgr", pad=2), c.arr("alpha", (4, 6), pad=3), 16))
S("alpha_bleed/empty", lambda c: c.m.alpha_bleed(numpy.zeros((0, 6, 3), u8), numpy.zeros((0, 6), u8), 1))
S("alpha_bleed/fail", lambda c: (c.fail("w2x_alpha_bleed"), c.m.alpha_bleed(c.bgr("bgr"), c.arr("alpha", (4, 6)), 17))[1])
S("alpha_bleed/refuse_bgr_4ch", lambda c: c.m.alpha_bleed(c.bgr("bgr", ch=4), c.arr("alpha", (4, 6)), 3))
S("alpha_bleed/refuse_bgr_unpacked", lambda c: c.m.alpha_bleed(numpy.zeros((4, 6, 4), u8)[..., :3], c.arr("alpha", (4, 6)), 3))
S("alpha_bleed/refuse_alpha_size", lambda c: c.m.alpha_bleed(c.bgr("bgr"), c.arr("alpha", (4, 5)), 3))
S("alpha_bleed/refuse_alpha_16bit", lambda c: c.m.alpha_bleed(c.bgr("bgr"), c.arr("alpha", (4, 6), u16), 3))


def generate(mod=None, scenarios=None):
    """{"symbols": declarations, "exported": sorted names, "scenarios": {name: log}} for the engine module `mod` (default: the package's); scenarios: (name,
    loaded, engines, function of a Ctx) tuples to log instead of SCENARIOS"""
    mod = mod or load_engine()
    real = mod.lib()
    rec = Recorder(real)
    stub = Stub(rec)
    doc = {"symbols": declarations(mod), "exported": sorted(mod.EXPORTED_SYMBOLS), "scenarios": {}}
    saved = mod.lib, mod.np
    for name, loaded, count, fn in (SCENARIOS if scenarios is None else scenarios):
        assert name not in doc["scenarios"], name
        rec.reset()
        engines = [mod.Img2Img() for _ in range(count)]
        try:
            rec.handles = [e._h for e in engines]
            for e in engines:
                e._L = stub
                if loaded:
                    e._scaling, e._batch, e._tile = SCALING, BATCH, TILE
            mod.lib, mod.np = (lambda: stub), NumpyProxy(rec)
            log = {"result": None, "raised": None}
            try:
                log["result"] = rec.describe(fn(Ctx(mod, rec, engines)))
            except Exception as ex:                                 # the type and the text are the record
                log["raised"] = [type(ex).__name__, str(ex)]
            log["calls"], log["allocated"] = rec.calls, rec.allocs
            log["messages"] = [[[int(s), m] for s, m in e.messages] for e in engines]
            log["host_buffers"] = {"handed_out": len(rec.hosts), "all_freed": sorted(rec.hosts) == sorted(rec.freed)}
            doc["scenarios"][name] = log
        finally:
            mod.lib, mod.np = saved
            for e in engines:
                e._L = real
                e.close()
    return doc


def dumps(doc) -> str:
    return json.dumps(doc, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--engine-file") + 1] if "--engine-file" in sys.argv else None
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    text = dumps(generate(load_engine(path)))
    open(out, "w").write(text)
    print(f"{out}: {len(SCENARIOS)} scenarios, {len(text)} bytes")
