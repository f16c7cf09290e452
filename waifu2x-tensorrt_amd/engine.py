"""ctypes binding of libw2x.so mirroring trt::Img2Img (/root/reference/src/tensorrt/img2img.h:14-50):
same five methods (build, load, render, setMessageCallback, setProgressCallback), same config
structs (config.h:12-43) and the same bool-return + message-callback error convention."""
from __future__ import annotations

import ctypes as C
import enum
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
lib_path = os.path.join(_HERE, "libw2x.so")


class W2xError(RuntimeError):
    pass


class Precision(enum.IntEnum):      # config.h:7-10
    TF32 = 0                        # fp32 maps, split-bf16 products (include/w2x/config.h)
    FP16 = 1
    FP32 = 2                        # not in the reference: the same engine with exact fp32 products


RESIZE_FILTERS = {"bicubic": 0, "bilinear": 1}   # W2X_RESIZE_BICUBIC / W2X_RESIZE_BILINEAR (include/w2x/c_api.h)


YUV_MATRICES = {"bt601": 0, "bt709": 1, "bt2020": 2}   # W2X_YUV_BT601 / _BT709 / _BT2020 (include/w2x/c_api.h)


def _matrix_id(name) -> int:
    if name not in YUV_MATRICES:
        raise ValueError(f"matrix must be one of {sorted(YUV_MATRICES)}, got {name!r}")
    return YUV_MATRICES[name]


YUV_LAYOUTS = {"i420": 0, "i422": 1, "i444": 2, "nv12": 3}   # W2X_YUV_I420 .. _NV12 (include/w2x/c_api.h)


YUV_SITINGS = {"left": 0, "center": 1, "topleft": 2}        # W2X_YUV_SITING_LEFT .. _TOPLEFT (include/w2x/c_api_yuv_siting.h)


def _siting_ids(siting, out_siting):
    """the ids of a call's two chroma sitings (out_siting None: the input's); unknown names raise before any library call"""
    out_siting = siting if out_siting is None else out_siting
    for name in (siting, out_siting):
        if name not in YUV_SITINGS:
            raise ValueError(f"siting must be one of {sorted(YUV_SITINGS)}, got {name!r}")
    return YUV_SITINGS[siting], YUV_SITINGS[out_siting]


def _layout_id(name) -> int:
    if name not in YUV_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(YUV_LAYOUTS)}, got {name!r}")
    return YUV_LAYOUTS[name]


def yuv_layout_plane_shapes(rows: int, cols: int, layout: str = "i420"):
    """[(rows, samples per row)] of the planes of a frame of `layout`: Y, U, V - or Y, UV for "nv12" (U and V interleaved: 2 * ceil(cols/2) samples a row)"""
    lid = _layout_id(layout)
    cr = (rows + 1) // 2 if lid in (0, 3) else rows
    cc = cols if lid == 2 else (cols + 1) // 2
    return [(rows, cols), (cr, 2 * cc)] if lid == 3 else [(rows, cols), (cr, cc), (cr, cc)]


def yuv_plane_shapes(rows: int, cols: int):
    """[(rows, cols)] of the Y, U and V planes of a 4:2:0 frame"""
    return yuv_layout_plane_shapes(rows, cols, "i420")


def _yuv_layout_bits(planes, layout, name=None, count_planes=True) -> int:
    """8 for uint8 planes, 10 for uint16 ones; checks the shapes of `layout` and packed samples.  name: what the error calls the layout (default: its
    key); count_planes=False: a frame short of a plane passes here and goes to the library, which refuses it - the 4:2:0-only calls never counted them"""
    y = planes[0]
    if y.ndim != 2 or y.dtype not in (np.uint8, np.uint16):
        raise ValueError("YUV planes must be 2-D uint8 (8-bit) or uint16 (10-bit) arrays")
    shapes = yuv_layout_plane_shapes(*y.shape, layout)
    if (count_planes and len(planes) != len(shapes)) or any(p.dtype != y.dtype or p.shape != shape or p.strides[1] != p.itemsize or p.strides[0] <= 0 for p, shape in zip(planes, shapes)):
        raise ValueError(f"{name or layout} planes of one sample type with packed rows expected: {[q.shape for q in planes]} for {y.shape}")
    return 8 if y.dtype == np.uint8 else 10


def _yuv_bits(planes) -> int:
    """_yuv_layout_bits of a 4:2:0 frame"""
    return _yuv_layout_bits(planes, "i420", "YUV 4:2:0", count_planes=False)


def _plane_args(planes):
    """three pointers and three steps of a frame for the C ABI (an NV12 frame leaves the third NULL / 0)"""
    pad = [None] * (3 - len(planes))
    return [p.ctypes.data for p in planes] + pad, [p.strides[0] for p in planes] + [0] * len(pad)


_COUNT = {3: "three", 4: "four"}
PLANAR_DTYPES = {8: np.uint8, 10: np.uint16, 12: np.uint16, 16: np.uint16, 32: np.float32}   # the sample type of each depth of a planar RGB frame


def planar_plane_bytes(rows: int, cols: int, bits: int) -> int:
    """the bytes of one packed plane of a planar RGB frame (w2x_planar_plane_bytes): 0 for an empty plane or a depth the library refuses"""
    return int(lib().w2x_planar_plane_bytes(int(rows), int(cols), int(bits)))


def _planar_order(order, names="rgb"):
    """where R, G and B (names="rgba": and A) sit in a frame whose planes come in `order` ("rgb", "gbr" - ffmpeg's gbrp -, any permutation; "rgba", "gbra" -
    ffmpeg's gbrap)"""
    if not isinstance(order, str) or sorted(order) != sorted(names):
        raise ValueError(f"order must name the planes {', '.join(names)} once each (\"{names}\", \"gbr{names[3:]}\"), got {order!r}")
    return [order.index(ch) for ch in names]


def _planar_bits(planes, bits=None, error=None, shape=None, empty_ok=False, n=3) -> int:
    """The depth of a planar frame: 8 for uint8, 16 for uint16, 32 for float32 planes; bits= says 10 or 12 for uint16 planes (or restates the default).
    Checks n (three; planar RGBA: four) 2-D planes of one shape (`shape` when given) and type with packed samples; rows may be padded, every plane its own way."""
    error = error or f"planes must be {_COUNT[n]} 2-D arrays of one shape and sample type (uint8, uint16 or float32) with packed samples"
    ok = isinstance(planes, (tuple, list)) and len(planes) == n and all(isinstance(p, np.ndarray) and p.ndim == 2 for p in planes)
    ok = ok and planes[0].dtype in (np.uint8, np.uint16, np.float32) and all(p.dtype == planes[0].dtype and p.shape == planes[0].shape for p in planes)
    ok = ok and (shape is None or planes[0].shape == tuple(shape))
    ok = ok and all((empty_ok and not p.size) or (p.strides[1] == p.itemsize and p.strides[0] > 0) for p in planes)
    if not ok:
        raise ValueError(error)
    dt = planes[0].dtype
    default = 8 if dt == np.uint8 else 16 if dt == np.uint16 else 32
    if bits is None:
        return default
    if int(bits) not in PLANAR_DTYPES or PLANAR_DTYPES[int(bits)] != dt:
        raise ValueError(f"bits={bits} does not go with {dt} planes (uint8: 8; uint16: 10, 12 or 16; float32: 32)")
    return int(bits)


def _filter_id(name) -> int:
    if name not in RESIZE_FILTERS:
        raise ValueError(f"filter must be one of {sorted(RESIZE_FILTERS)}, got {name!r}")
    return RESIZE_FILTERS[name]


def _frame_ok(a, channels, dtypes, error=None, shape=None, rows_packed=False, empty_ok=False) -> bool:
    """The check of every packed interleaved frame: `a` is a [rows, cols, channels] array of one of `dtypes` whose pixels are packed (rows may be padded
    unless rows_packed).  shape: the (rows, cols) it must have; empty_ok: the strides of an empty array are not looked at.  A frame that fails raises
    ValueError(error) - with error=None False is returned, for the callers that refuse through the message callback."""
    b = a.itemsize
    ok = a.dtype in dtypes and a.ndim == 3 and a.shape[2] == channels and (shape is None or a.shape[:2] == tuple(shape)) and (
        (empty_ok and not a.size) or (a.strides[2] == b and a.strides[1] == channels * b and (not rows_packed or a.strides[0] == a.shape[1] * channels * b)))
    if not ok and error is not None:
        raise ValueError(error)
    return ok


def _data(a):
    """the pointer of an array for the C ABI, NULL for an empty one"""
    return a.ctypes.data if a.size else None


def _pointers(arrays, count=None):
    """the pointer array of a C entry that reads `count` of them (default: all): fewer arrays leave NULLs, which the library refuses; more raise IndexError"""
    return (C.c_void_p * (len(arrays) if count is None else count))(*[a.ctypes.data for a in arrays])


class Severity(enum.IntEnum):       # logger.h:11-18
    critical = 0
    error = 1
    warn = 2
    info = 3
    debug = 4
    trace = 5


class _BuildConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "deviceId", "precision", "minBatchSize", "optBatchSize", "maxBatchSize", "minChannels", "optChannels",
        "maxChannels", "minWidth", "optWidth", "maxWidth", "minHeight", "optHeight", "maxHeight")]


class _RenderConfig(C.Structure):
    _fields_ = [("deviceId", C.c_int), ("precision", C.c_int), ("batchSize", C.c_int), ("channels", C.c_int),
                ("height", C.c_int), ("width", C.c_int), ("scaling", C.c_int), ("overlapX", C.c_double),
                ("overlapY", C.c_double), ("tta", C.c_int), ("ttaBugCompat", C.c_int)]


@dataclass
class BuildConfig:                  # defaults of config.h:12-31
    deviceId: int = 0
    precision: Precision = Precision.FP16
    minBatchSize: int = 1
    optBatchSize: int = 1
    maxBatchSize: int = 4
    minChannels: int = 3
    optChannels: int = 3
    maxChannels: int = 3
    minWidth: int = 64
    optWidth: int = 256
    maxWidth: int = 640
    minHeight: int = 64
    optHeight: int = 256
    maxHeight: int = 640

    @staticmethod
    def fixed(batch: int, tile: int, device: int = 0, precision: Precision = Precision.FP16) -> "BuildConfig":
        """min = opt = max, the way the CLI fills it (main.cpp:276-291)."""
        return BuildConfig(device, precision, batch, batch, batch, 3, 3, 3, tile, tile, tile, tile, tile, tile)


@dataclass
class RenderConfig:                 # defaults of config.h:33-43
    deviceId: int = 0
    precision: Precision = Precision.FP16
    batchSize: int = 1
    channels: int = 3
    height: int = 256
    width: int = 256
    scaling: int = 4
    overlap: tuple = (0.0625, 0.0625)
    tta: bool = False
    ttaBugCompat: bool = False


_MSG_FN = C.CFUNCTYPE(None, C.c_int, C.c_char_p, C.c_void_p)
_PROG_FN = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_double, C.c_void_p)

_I, _Z, _D, _F, _P, _S = C.c_int, C.c_size_t, C.c_double, C.c_float, C.c_void_p, C.c_char_p
_FRAME = [_P, _P, _I, _I, _Z]                # engine, frame (or array of frames), rows, cols, step
_YUV = [_P, _P, _I, _I, _I]                  # planes, steps, rows, cols, bits
_YUV2 = [_P] + _YUV + _YUV                   # engine, source frame, destination frame
_YUV2L = [_P] + _YUV + [_I] + _YUV + [_I]    # the same with a layout after each frame
_YUV2S = [_P] + _YUV + [_I, _I] + _YUV + [_I, _I]   # the same with a layout and a chroma siting after each frame
_GRID = [_I] * 7 + [_D, _D]                  # in_w, in_h, out_w, out_h, tile_in, tile_out, scaling, overlap_x, overlap_y
# Every symbol of include/w2x/c_api.h: name -> (restype, argtypes).  A new entry is one row here (tests/test_host_abi.py compares the keys with the header).
# restype None: void (the three calls that take a pointer back); _I on the other void functions is ctypes' default, as before.  argtypes None: not declared.
SYMBOLS = {
    "w2x_create": (_P, None),
    "w2x_destroy": (_I, [_P]),
    "w2x_set_message_callback": (_I, [_P, _MSG_FN, _P]),
    "w2x_set_progress_callback": (_I, [_P, _PROG_FN, _P]),
    "w2x_build": (_I, [_P, _S, C.POINTER(_BuildConfig)]),
    "w2x_load": (_I, [_P, _S, C.POINTER(_RenderConfig)]),
    "w2x_render": (_I, _FRAME + [_P, _Z]),
    "w2x_render16": (_I, _FRAME + [_P, _Z]),
    "w2x_render_resized": (_I, _FRAME + [_P, _I, _I, _Z, _I]),
    "w2x_render16_resized": (_I, _FRAME + [_P, _I, _I, _Z, _I]),
    "w2x_render_strip": (_I, _FRAME + [_P, _Z, _I, _I]),
    "w2x_render_sharded": (_I, [_P, _I, _P, _I, _I, _Z, _P, _Z]),
    "w2x_shard_plan": (_I, _GRID + [_I, _I, _P]),
    "w2x_shard_compute": (_I, _FRAME + [_I, _I]),
    "w2x_shard_slab": (_P, [_P, _P]),
    "w2x_shard_finish": (_I, [_P, _P, _I, _I, _Z, _I, _I, _P, _P]),
    "w2x_ipc_export": (_I, [_P, _P]),
    "w2x_ipc_open": (_P, [_P, _I]),
    "w2x_ipc_close": (None, [_P]),
    "w2x_render_sequence": (_I, _FRAME + [_P, _Z, _I]),
    "w2x_render_sequence_resized": (_I, _FRAME + [_P, _I, _I, _Z, _I, _I]),
    "w2x_render_yuv": (_I, _YUV2 + [_I, _I]),
    "w2x_render_sequence_yuv": (_I, _YUV2 + [_I, _I, _I]),
    "w2x_render_yuv_layout": (_I, _YUV2L + [_I, _I]),
    "w2x_render_sequence_yuv_layout": (_I, _YUV2L + [_I, _I, _I]),
    "w2x_render_yuv_resized": (_I, _YUV2 + [_I, _I, _I]),
    "w2x_render_sequence_yuv_resized": (_I, _YUV2 + [_I, _I, _I, _I]),
    "w2x_render_rgba": (_I, _FRAME + [_P, _Z, _I, _I]),
    "w2x_render_rgba_resized": (_I, _FRAME + [_P, _I, _I, _Z, _I, _I, _I]),
    "w2x_render_sequence_rgba": (_I, _FRAME + [_P, _Z, _I, _I, _I]),
    "w2x_render_sequence_rgba_resized": (_I, _FRAME + [_P, _I, _I, _Z, _I, _I, _I, _I]),
    "w2x_alpha_bleed_device": (_I, _FRAME + [_P, _Z, _I]),
    "w2x_alloc_host": (_P, [_P, _Z]),
    "w2x_free_host": (None, [_P, _P]),
    "w2x_pin_host": (_I, [_P, _P, _Z]),
    "w2x_unpin_host": (None, [_P, _P]),
    "w2x_strip_plan": (_I, _GRID + [_I, _I, _P]),
    "w2x_infer": (_I, [_P, _P, _P]),
    "w2x_output_tile_size": (_I, [_P]),
    "w2x_plan_flops": (_D, [_P]),
    "w2x_pass_tiles": (_I, [_P]),
    "w2x_last_render_ms": (_F, [_P]),
    "w2x_bench_resident": (_F, [_P, _I]),
    "w2x_resident_output": (_I, [_P, _P, _Z]),
    "w2x_profile_frame": (_I, [_P, _P, _I]),
    "w2x_op_times": (_I, [_P, _P, _I]),
    "w2x_calculate_tiles": (_I, _GRID + [_P, _P, _I]),
    "w2x_tile_weights": (_I, [_I, _I, _I, _I, _P]),
    "w2x_resize_weights": (_I, [_I, _I, _I, _P, _P, _I]),
    "w2x_yuv_plane_sizes": (_I, [_I, _I, _I, _P, _P, _P]),
    "w2x_yuv_layout_plane_sizes": (_I, [_I, _I, _I, _I, _P, _P, _P, _P]),
    "w2x_alpha_bleed": (_I, [_P, _Z, _P, _Z, _I, _I, _I, _P, _Z]),
    "w2x_describe_plan": (_I, [_S, _I, _I, _S, _Z]),
    "w2x_describe_plan_precision": (_I, [_S, _I, _I, _I, _S, _Z]),
    "w2x_write_engine_file": (_I, [_S, _I, _I, _S]),
    "w2x_validate_engine_file": (_I, [_S, _S, _Z]),
    "w2x_dead_skip_extents": (_I, [_S] + [_I] * 5 + [_D, _D, _I, _I, _P, _I]),
    "w2x_device_pci_bus_id": (_I, [_I, _S, _Z]),
    "w2x_sha256_hex": (_I, [_P, _Z, _S]),
    "w2x_version": (_S, None),
    "w2x_debug_set": (_I, [_S, _I]),
}
EXPORTED_SYMBOLS = list(SYMBOLS)
# The gray entries of include/w2x/c_api_gray.h, in the row format of SYMBOLS and declared by lib() in the same loop.  A table of their own, not rows of SYMBOLS:
# the golden call log (tests/golden/binding_calls.json) pins SYMBOLS / EXPORTED_SYMBOLS and the names of c_api.h to each other.
GRAY_SYMBOLS = {
    "w2x_render_gray": (_I, _FRAME + [_P, _Z]),
    "w2x_render_gray16": (_I, _FRAME + [_P, _Z]),
    "w2x_render_gray_resized": (_I, _FRAME + [_P, _I, _I, _Z, _I]),
    "w2x_render_gray16_resized": (_I, _FRAME + [_P, _I, _I, _Z, _I]),
    "w2x_render_sequence_gray": (_I, _FRAME + [_P, _Z, _I]),
    "w2x_render_sequence_gray_resized": (_I, _FRAME + [_P, _I, _I, _Z, _I, _I]),
}
# The planar RGB entries of include/w2x/c_api_planar.h, in the row format of SYMBOLS and declared by lib() in the same loop; a table of their own for the
# reason GRAY_SYMBOLS is one.  _YUV is (planes, steps, rows, cols, bits): the planar frames travel the same way.
PLANAR_SYMBOLS = {
    "w2x_render_planar": (_I, _YUV2),
    "w2x_render_planar_resized": (_I, _YUV2 + [_I]),
    "w2x_render_sequence_planar": (_I, _YUV2 + [_I]),
    "w2x_render_sequence_planar_resized": (_I, _YUV2 + [_I, _I]),
    "w2x_planar_plane_bytes": (_Z, [_I, _I, _I]),
}
# The planar RGBA entries of include/w2x/c_api_rgbap.h, a table of their own likewise.  Their names say "rgbap": the planar and the gray table own every exported
# name that holds their word.  _YUV2 + [bleed, skip_uniform_alpha]; the bleed entries: (planes, steps, rows, cols, bits, radius, out planes, out steps[, words]).
RGBAP_SYMBOLS = {
    "w2x_render_rgbap": (_I, _YUV2 + [_I, _I]),
    "w2x_render_rgbap_resized": (_I, _YUV2 + [_I, _I, _I]),
    "w2x_render_sequence_rgbap": (_I, _YUV2 + [_I, _I, _I]),
    "w2x_render_sequence_rgbap_resized": (_I, _YUV2 + [_I, _I, _I, _I]),
    "w2x_alpha_bleed_rgbap": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "w2x_alpha_bleed_rgbap_device": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
}
# The resized YUV entries that carry a layout (include/w2x/c_api_yuv_resized.h), a table of their own likewise: _YUV2L + [matrix, range, filter], the sequence with
# `count` in front of the matrix.
YUV_RESIZED_SYMBOLS = {
    "w2x_render_yuv_layout_resized": (_I, _YUV2L + [_I, _I, _I]),
    "w2x_render_sequence_yuv_layout_resized": (_I, _YUV2L + [_I, _I, _I, _I]),
}
# The YUV entries that carry a chroma siting per side (include/w2x/c_api_yuv_siting.h), a table of their own likewise: _YUV2S + [matrix, range, filter], the
# sequence with `count` in front of the matrix.
YUV_SITED_SYMBOLS = {
    "w2x_render_yuv_sited": (_I, _YUV2S + [_I, _I, _I]),
    "w2x_render_sequence_yuv_sited": (_I, _YUV2S + [_I, _I, _I, _I]),
}
# The dither entries of include/w2x/c_api_dither.h, a table of their own likewise: (engine, mode, phase, advance), its getter, the rank table and one rank
# without an engine, and the test hook (engine, src planes, src steps, rows, cols, dst planes, dst steps, bits).
DITHER_SYMBOLS = {
    "w2x_set_dither": (_I, [_P, _I, C.c_uint, C.c_uint]),
    "w2x_get_dither": (_I, [_P, _P, _P, _P]),
    "w2x_dither_table": (_I, [_I, _P, _P]),
    "w2x_dither_rank": (_I, [_I, C.c_uint, _I, _I, _I]),
    "w2x_dither_planes": (_I, [_P, _P, _P, _I, _I, _P, _P, _I]),
}
DITHER_MODES = {"none": 0, "ordered": 1, "bluenoise": 2}    # W2X_DITHER_NONE .. _BLUENOISE (include/w2x/c_api_dither.h)
# The entries of include/w2x/c_api_resize_light.h, a table of their own likewise: (engine, mode), its getter, the two curve functions without an engine, and
# the test hook (engine, src planes, src steps, rows, cols, dst planes, dst steps, dst rows, dst cols, bits, filter).
RESIZE_LIGHT_SYMBOLS = {
    "w2x_set_resize_light": (_I, [_P, _I]),
    "w2x_get_resize_light": (_I, [_P]),
    "w2x_light_decode": (C.c_float, [_I, C.c_float]),
    "w2x_light_encode": (C.c_float, [_I, C.c_float]),
    "w2x_resize_planes": (_I, [_P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _I]),
}
RESIZE_LIGHTS = {"gamma": 0, "srgb": 1, "bt709": 2}    # W2X_LIGHT_GAMMA .. _BT709 (include/w2x/c_api_resize_light.h)
# The chained renders of include/w2x/c_api_chain.h, a table of their own likewise: (engines, count) in front of the frame arguments of the single entries, then
# depth (interleaved frames), quantize and, resized, the filter; the planar entries say "planes" (PLANAR_SYMBOLS owns every name that holds "planar").
_CHAIN = [_P, _I]
CHAIN_SYMBOLS = {
    "w2x_chain_plan": (_I, [_I, _I, _P, _I, _I, _I, _P]),
    "w2x_render_chained": (_I, _CHAIN + [_P, _I, _I, _Z, _P, _Z, _I, _I]),
    "w2x_render_chained_resized": (_I, _CHAIN + [_P, _I, _I, _Z, _P, _I, _I, _Z, _I, _I, _I]),
    "w2x_render_sequence_chained": (_I, _CHAIN + [_P, _I, _I, _Z, _P, _Z, _I, _I]),
    "w2x_render_sequence_chained_resized": (_I, _CHAIN + [_P, _I, _I, _Z, _P, _I, _I, _Z, _I, _I, _I]),
    "w2x_render_chained_planes": (_I, _CHAIN + _YUV + _YUV + [_I]),
    "w2x_render_chained_planes_resized": (_I, _CHAIN + _YUV + _YUV + [_I, _I]),
}
# The entries of include/w2x/c_api_edge.h, a table of their own likewise: (engine, mode), its getter, the rule without an engine (mode, i, n), the tap table
# under a mode (w2x_resize_weights' arguments with the mode behind the filter) and the two host bleeds with the mode as their last argument.
EDGE_SYMBOLS = {
    "w2x_set_edge": (_I, [_P, _I]),
    "w2x_get_edge": (_I, [_P]),
    "w2x_edge_index": (_I, [_I, C.c_longlong, _I]),
    "w2x_resize_weights_edge": (_I, [_I, _I, _I, _I, _P, _P, _I]),
    "w2x_alpha_bleed_edge": (_I, [_P, _Z, _P, _Z, _I, _I, _I, _P, _Z, _I]),
    "w2x_alpha_bleed_planes_edge": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _I]),
}
EDGE_MODES = {"replicate": 0, "wrap": 1, "mirror": 2}    # W2X_EDGE_REPLICATE .. _MIRROR (include/w2x/c_api_edge.h)
CHAIN_REFUSALS = {1: "count", 2: "scaling", 3: "source", 4: "too_large", 5: "target", 6: "shrink"}    # W2X_CHAIN_COUNT .. _SHRINK
_lib = None


def lib():
    """Load libw2x.so and declare every symbol of include/w2x/c_api.h.  Fails loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(lib_path):
        raise W2xError(f"{lib_path} is missing - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "or `make -C waifu2x-tensorrt_amd` (there is no CPU fallback)")
    L = C.CDLL(lib_path)
    for name, (restype, argtypes) in list(SYMBOLS.items()) + list(GRAY_SYMBOLS.items()) + list(PLANAR_SYMBOLS.items()) + list(RGBAP_SYMBOLS.items()) + list(YUV_RESIZED_SYMBOLS.items()) + list(YUV_SITED_SYMBOLS.items()) + list(DITHER_SYMBOLS.items()) + list(RESIZE_LIGHT_SYMBOLS.items()) + list(CHAIN_SYMBOLS.items()) + list(EDGE_SYMBOLS.items()):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


class Img2Img:
    """trt::Img2Img mirror.  cv::Mat <-> numpy uint8 [rows, cols, 3] BGR."""

    def __init__(self):
        self._L = lib()
        self._h = self._L.w2x_create()
        if not self._h:
            raise W2xError("w2x_create failed")
        self._scaling = self._batch = self._tile = 0     # of the loaded configuration; 0 before a successful load
        self._host_bufs = {}                             # alloc_host() arrays: address -> pointer to free
        self.messages: list[tuple[int, str]] = []
        self._user_msg = None
        self._user_prog = None
        self._msg_cb = _MSG_FN(self._on_msg)
        self._prog_cb = _PROG_FN(self._on_prog)
        self._L.w2x_set_message_callback(self._h, self._msg_cb, None)
        self._L.w2x_set_progress_callback(self._h, self._prog_cb, None)

    def _on_msg(self, sev, msg, _):
        m = msg.decode(errors="replace")
        self.messages.append((sev, m))
        if self._user_msg:
            self._user_msg(Severity(sev), m)

    def _on_prog(self, cur, total, speed, _):
        if self._user_prog:
            self._user_prog(cur, total, speed)

    def close(self):
        if self._h:
            self._L.w2x_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setMessageCallback(self, cb):
        self._user_msg = cb

    def setProgressCallback(self, cb):
        self._user_prog = cb

    def last_error(self) -> str:
        errs = [m for s, m in self.messages if s <= Severity.error]
        return errs[-1] if errs else ""

    def _refuse(self, who, text):
        """a refusal of the wrapper's own, worded and sent like the engine's (the C ABI sees pointers and steps only, so some cv::Mat-style checks live here)"""
        self._on_msg(int(Severity.error), f"[{who}@0] {text}".encode(), None)

    def _finish(self, ok, allocated, fallback):
        """The return convention of the frame calls.  allocated: the array(s) the wrapper made because the caller gave no destination - returned, or W2xError
        with the library's last message (else `fallback`); None, when the caller gave the destination: the bool, like the reference."""
        if allocated is None:
            return bool(ok)
        if not ok:
            raise W2xError(self.last_error() or fallback)
        return allocated

    def _sequence(self, frames, outs, pinned, alloc, copy, run, fallback, check=None):
        """The driver of the sequence calls: run(frames, outs) -> ok of the C entry, over destinations `outs` (one per frame).  outs=None: alloc(False) makes
        each - or, pinned, alloc(True) makes a ring of min(n, 3) page-locked (buffer, destination) pairs: the sequence runs in pieces of the ring's length,
        each result is copied out with copy(destination) and every buffer is freed, also when a later alloc or a piece fails.  check(destination) raises for one that does not fit.  Returns the outputs; W2xError when run fails."""
        n, ring = len(frames), []
        try:
            if outs is None:
                if pinned:
                    for _ in range(min(n, 3)):
                        ring.append(alloc(True))
                else:
                    outs = [alloc(False)[1] for _ in range(n)]
            for o in ([d for _, d in ring] or outs):
                if check:
                    check(o)
            res = [] if ring else outs
            for k0 in range(0, n, len(ring) or n):
                piece = frames[k0:k0 + (len(ring) or n)]
                dsts = [d for _, d in ring[:len(piece)]] if ring else outs
                self._finish(run(piece, dsts), dsts, fallback)
                if ring:
                    res += [copy(d) for d in dsts]
            return res
        finally:
            for buf, _ in ring:
                self.free_host(buf)

    def _packed_sequence(self, frames, channels, out_shape, outs, pinned, outs_error, run, fallback):
        """_sequence for interleaved uint8 frames: every destination a packed out_shape array (page-locked: alloc_host)"""
        def alloc(host):
            buf = self.alloc_host(out_shape) if host else np.empty(out_shape, np.uint8)
            return buf, buf
        return self._sequence(frames, outs, pinned, alloc, np.copy, run, fallback,
                              lambda o: _frame_ok(o, channels, (np.uint8,), outs_error, shape=out_shape[:2], rows_packed=True))

    def build(self, path: str, config: BuildConfig) -> bool:
        c = _BuildConfig(*[int(getattr(config, f[0])) for f in _BuildConfig._fields_])
        return bool(self._L.w2x_build(self._h, os.fsencode(path), C.byref(c)))

    def load(self, path: str, config: RenderConfig) -> bool:
        c = _RenderConfig(config.deviceId, int(config.precision), config.batchSize, config.channels, config.height,
                          config.width, config.scaling, float(config.overlap[0]), float(config.overlap[1]),
                          int(config.tta), int(config.ttaBugCompat))
        ok = bool(self._L.w2x_load(self._h, os.fsencode(path), C.byref(c)))
        self._scaling = config.scaling if ok else 0
        self._batch, self._tile = (config.batchSize, config.height) if ok else (0, 0)
        return ok

    def render(self, src: np.ndarray, dst: np.ndarray | None = None):
        """render(src, dst) -> bool like the reference; render(src) -> dst array or raises."""
        _frame_ok(src, 3, (np.uint8, np.uint16), "src must be a uint8 (or uint16) [rows, cols, 3] BGR array with packed pixels")   # uint16: extension, w2x_render16
        s = self._scaling
        out = np.empty((src.shape[0] * s, src.shape[1] * s, 3), src.dtype) if dst is None else None
        dst = out if dst is None else dst
        # (an engine that was never loaded has s = 0: a dst of any size goes to the library, which refuses the call)
        if s and not _frame_ok(dst, 3, (src.dtype,), shape=(src.shape[0] * s, src.shape[1] * s)):
            self._refuse("render", f"Output image has invalid size: expected {src.shape[1] * s}x{src.shape[0] * s}.")
            return False
        fn = self._L.w2x_render if src.itemsize == 1 else self._L.w2x_render16
        return self._finish(fn(self._h, src.ctypes.data, src.shape[0], src.shape[1], src.strides[0], dst.ctypes.data, dst.strides[0]), out, "render failed")

    def _rgba_frame(self, bgra, who, raises):
        """the checks of a BGRA frame; False after the refusal of a deeper frame (the C ABI carries no sample depth), sent with the engine's message"""
        ok = isinstance(bgra, np.ndarray) and bgra.ndim == 3 and bgra.shape[2] == 4
        if ok and bgra.dtype != np.uint8:
            self._refuse(who, "RGBA input and output images must be 8-bit.")
            if raises:
                raise W2xError(self.last_error())
            return False
        if not ok or not _frame_ok(bgra, 4, (np.uint8,)):
            raise ValueError("bgra must be a uint8 [rows, cols, 4] BGRA array with packed pixels")
        return True

    def render_rgba(self, bgra: np.ndarray, *, bleed: int = 0, skip_uniform_alpha: bool = False, dst: np.ndarray | None = None):
        """render() on a uint8 [rows, cols, 4] BGRA frame in one call (w2x_render_rgba): the colours of the pixels with alpha > 0 are spread `bleed` pixels
        (0..16) under the transparent ones, colour and alpha tiles share one schedule; skip_uniform_alpha: a frame whose alpha plane is one value keeps it
        and runs no alpha tiles.  Rows may be padded (strides[0] >= cols * 4).  With dst=None returns the [rows * s, cols * s, 4] array or raises; with dst
        returns a bool."""
        if not self._rgba_frame(bgra, "renderRgba", dst is None):
            return False
        s = self._scaling
        out = np.empty((bgra.shape[0] * s, bgra.shape[1] * s, 4), np.uint8) if dst is None else None
        dst = out if dst is None else dst
        if s and not _frame_ok(dst, 4, (np.uint8,), shape=(bgra.shape[0] * s, bgra.shape[1] * s)):      # (never loaded: as in render())
            self._refuse("renderRgba", f"Output image has invalid size: expected {bgra.shape[1] * s}x{bgra.shape[0] * s}.")
            return False
        return self._finish(self._L.w2x_render_rgba(self._h, _data(bgra), bgra.shape[0], bgra.shape[1], bgra.strides[0], _data(dst), dst.strides[0],
                                                    int(bleed), 1 if skip_uniform_alpha else 0), out, "render_rgba failed")

    def render_rgba_resized(self, bgra: np.ndarray, size, *, bleed: int = 0, skip_uniform_alpha: bool = False, filter: str = "bicubic", dst: np.ndarray | None = None):
        """render_rgba() with the output resized on the device to size = (rows, cols), each in [input dim, input dim * scaling] (w2x_render_rgba_resized):
        colour and alpha are resized separately and straight, with the filters of render_resized().  With dst=None returns the [rows, cols, 4] array or
        raises; with dst returns a bool."""
        if not self._rgba_frame(bgra, "renderRgbaResized", dst is None):
            return False
        rows, cols = int(size[0]), int(size[1])
        fid = _filter_id(filter)
        out = np.empty((max(rows, 0), max(cols, 0), 4), np.uint8) if dst is None else None
        dst = out if dst is None else dst
        # (an empty target: refused by the library; a wrong dst raises here, where render_rgba() returns False)
        _frame_ok(dst, 4, (np.uint8,), "dst must be a uint8 [rows, cols, 4] array of the target size with packed pixels", shape=(rows, cols), empty_ok=True)
        return self._finish(self._L.w2x_render_rgba_resized(self._h, _data(bgra), bgra.shape[0], bgra.shape[1], bgra.strides[0], _data(dst), rows, cols, dst.strides[0],
                                                            int(bleed), 1 if skip_uniform_alpha else 0, fid), out, "render_rgba_resized failed")

    def render_sequence_rgba(self, frames, *, size=None, bleed: int = 0, skip_uniform_alpha: bool = False, filter: str = "bicubic", outs=None, pinned: bool = False):
        """Equally sized uint8 [rows, cols, 4] BGRA frames with upload / compute / download overlapped (w2x_render_sequence_rgba); with size = (rows, cols) every
        frame is resized like render_rgba_resized() (w2x_render_sequence_rgba_resized).  Output i is the bytes of the single-frame call on frame i.
        outs / pinned as in render_sequence()."""
        if len(frames) == 0:
            return []
        s = self._scaling
        r, c = frames[0].shape[:2]
        for f in frames:
            _frame_ok(f, 4, (np.uint8,), "frames must be packed uint8 [rows, cols, 4] arrays", rows_packed=True)
            if f.shape != (r, c, 4):
                # the C ABI carries one size for the sequence: frames that differ are refused here, with the engine's message (the BGR sequences raise ValueError)
                self._refuse("renderSequenceRgba", "Input images must be of one size.")
                raise W2xError(self.last_error())
        rows, cols = (r * s, c * s) if size is None else (int(size[0]), int(size[1]))
        fid = _filter_id(filter)
        flags = (int(bleed), 1 if skip_uniform_alpha else 0)

        def run(fs, os_):
            if size is None:
                return self._L.w2x_render_sequence_rgba(self._h, _pointers(fs), r, c, c * 4, _pointers(os_, len(fs)), cols * 4, len(fs), *flags)
            return self._L.w2x_render_sequence_rgba_resized(self._h, _pointers(fs), r, c, c * 4, _pointers(os_, len(fs)), rows, cols, cols * 4, len(fs), *flags, fid)
        return self._packed_sequence(frames, 4, (rows, cols, 4), outs, pinned, "outs must be packed uint8 [rows, cols, 4] arrays of the output size", run,
                                     "render_sequence_rgba failed")

    @staticmethod
    def _gray_ok(a, error, shape=None, dtypes=(np.uint8, np.uint16), empty_ok=False):
        """a gray frame: a 2-D array of one of `dtypes` with packed samples (rows may be padded), of `shape` when given; else ValueError(error)"""
        ok = isinstance(a, np.ndarray) and a.ndim == 2 and a.dtype in dtypes and (shape is None or a.shape == tuple(shape)) and (
            (empty_ok and not a.size) or (a.strides[1] == a.itemsize and a.strides[0] > 0))
        if not ok:
            raise ValueError(error)

    def render_gray(self, gray: np.ndarray, dst: np.ndarray | None = None):
        """render() on a gray frame, a 2-D uint8 or uint16 array (w2x_render_gray / w2x_render_gray16): the green channel of render() of the frame
        B = G = R = gray, byte for byte, with one sample per pixel travelling each way.  Rows may be padded, as in render().  With dst=None returns the
        [rows * s, cols * s] array or raises; with dst returns a bool."""
        self._gray_ok(gray, "gray must be a 2-D uint8 (or uint16) array with packed samples")
        s = self._scaling
        out = np.empty((gray.shape[0] * s, gray.shape[1] * s), gray.dtype) if dst is None else None
        dst = out if dst is None else dst
        self._gray_ok(dst, "dst must be a 2-D array of the frame's sample type with packed samples", dtypes=(gray.dtype,), empty_ok=True)
        if s and dst.shape != (gray.shape[0] * s, gray.shape[1] * s):      # (never loaded: as in render())
            self._refuse("renderGray", f"Output image has invalid size: expected {gray.shape[1] * s}x{gray.shape[0] * s}.")
            return False
        fn = self._L.w2x_render_gray if gray.itemsize == 1 else self._L.w2x_render_gray16
        return self._finish(fn(self._h, _data(gray), gray.shape[0], gray.shape[1], gray.strides[0], _data(dst), dst.strides[0]), out, "render_gray failed")

    def render_gray_resized(self, gray: np.ndarray, size, filter: str = "bicubic", dst: np.ndarray | None = None):
        """render_gray() with the output resized on the device to size = (rows, cols), each in [input dim, input dim * scaling] (w2x_render_gray_resized /
        w2x_render_gray16_resized): the green channel of render_resized() of the replicated frame.  With dst=None returns the array or raises; with dst a bool."""
        self._gray_ok(gray, "gray must be a 2-D uint8 (or uint16) array with packed samples")
        rows, cols = int(size[0]), int(size[1])
        fid = _filter_id(filter)
        out = np.empty((max(rows, 0), max(cols, 0)), gray.dtype) if dst is None else None
        dst = out if dst is None else dst
        # (an empty target: refused by the library)
        self._gray_ok(dst, "dst must be a 2-D array of the target size and the frame's sample type with packed samples", shape=(max(rows, 0), max(cols, 0)), dtypes=(gray.dtype,), empty_ok=True)
        fn = self._L.w2x_render_gray_resized if gray.itemsize == 1 else self._L.w2x_render_gray16_resized
        return self._finish(fn(self._h, _data(gray), gray.shape[0], gray.shape[1], gray.strides[0], _data(dst), rows, cols, dst.strides[0], fid), out, "render_gray_resized failed")

    def render_sequence_gray(self, frames, *, size=None, filter: str = "bicubic", outs=None, pinned: bool = False):
        """Equally sized 2-D uint8 gray frames with upload / compute / download overlapped (w2x_render_sequence_gray); with size = (rows, cols) every frame is
        resized like render_gray_resized() (w2x_render_sequence_gray_resized).  Output i is the bytes of the single-frame call on frame i.  The frames share
        one row stride (rows may be padded); outs / pinned as in render_sequence()."""
        if len(frames) == 0:
            return []
        fid = _filter_id(filter)
        for f in frames:
            if isinstance(f, np.ndarray) and f.ndim == 2 and f.dtype == np.uint16:
                raise ValueError("a gray sequence takes 8-bit frames (16-bit frames go through render_gray())")
            self._gray_ok(f, "frames must be 2-D uint8 arrays with packed samples", dtypes=(np.uint8,))
            if f.shape != frames[0].shape or f.strides[0] != frames[0].strides[0]:
                raise ValueError("frames must be 2-D uint8 arrays of one size and one row stride")
        s = self._scaling
        r, c = frames[0].shape
        step = frames[0].strides[0]
        rows, cols = (r * s, c * s) if size is None else (int(size[0]), int(size[1]))
        out_shape = (max(rows, 0), max(cols, 0))

        def alloc(host):
            buf = self.alloc_host(out_shape) if host else np.empty(out_shape, np.uint8)
            return buf, buf

        def check(o):
            self._gray_ok(o, "outs must be packed 2-D uint8 arrays of the output size", shape=out_shape, dtypes=(np.uint8,), empty_ok=True)
            if o.size and o.strides[0] != cols:
                raise ValueError("outs must be packed 2-D uint8 arrays of the output size")

        def run(fs, os_):
            if size is None:
                return self._L.w2x_render_sequence_gray(self._h, _pointers(fs), r, c, step, _pointers(os_, len(fs)), cols, len(fs))
            return self._L.w2x_render_sequence_gray_resized(self._h, _pointers(fs), r, c, step, _pointers(os_, len(fs)), rows, cols, cols, len(fs), fid)
        return self._sequence(frames, outs, pinned, alloc, np.copy, run, "render_sequence_gray failed", check)

    def _planar_call(self, planes, size, bits, out_bits, order, dst, who, names="rgb"):
        """what the single planar calls share: the checks of both sides and the arguments of the C entry up to dst_bits (planes in R, G, B order; names="rgba": the
        four planes of a planar RGBA frame in R, G, B, A order)"""
        n = len(names)
        idx = _planar_order(order, names)
        bits = _planar_bits(planes, bits, n=n)
        ob = bits if out_bits is None else int(out_bits)
        if ob not in PLANAR_DTYPES:
            raise ValueError(f"out_bits must be one of {sorted(PLANAR_DTYPES)}, got {out_bits!r}")
        r, c = planes[0].shape
        s = self._scaling
        rows, cols = (r * s, c * s) if size is None else (max(int(size[0]), 0), max(int(size[1]), 0))
        out = tuple(np.empty((rows, cols), PLANAR_DTYPES[ob]) for _ in range(n)) if dst is None else None
        dst = out if dst is None else tuple(dst)
        # the C ABI sees pointers and steps only: the shapes and the sample type of out_bits are checked here (an empty target: refused by the library)
        error = f"dst must be {_COUNT[n]} 2-D {np.dtype(PLANAR_DTYPES[ob]).name} planes of one shape with packed samples"
        _planar_bits(dst, ob, error, empty_ok=True, n=n)
        if size is not None and dst[0].shape != (rows, cols):
            raise ValueError(f"dst must be {_COUNT[n]} planes of the target size {(rows, cols)}")
        if size is None and s and dst[0].shape != (rows, cols):     # (never loaded: as in render())
            self._refuse(who, f"Output image has invalid size: expected {cols}x{rows}.")
            return None, out
        src = [planes[k] for k in idx]
        d = [dst[k] for k in idx]
        args = (self._h, (C.c_void_p * n)(*[_data(p) for p in src]), (C.c_size_t * n)(*[p.strides[0] for p in src]), r, c, bits,
                (C.c_void_p * n)(*[_data(p) for p in d]), (C.c_size_t * n)(*[p.strides[0] for p in d]),
                int(size[0]) if size is not None else rows, int(size[1]) if size is not None else cols, ob)
        return args, out

    def render_planar(self, planes, *, bits: int | None = None, out_bits: int | None = None, order: str = "rgb", dst=None):
        """render() on a planar RGB frame (w2x_render_planar): three 2-D planes of uint8 (8 bits), uint16 (16; bits=10 / 12 for codes in the low bits) or
        float32 (nominal [0, 1]) samples; out_bits (8, 10, 12, 16 or 32 for float32; default the input's) sets the output's sample format independently.
        At 8 / 8 and 16 / 16 bits the planes are those of render() of the interleaved frame, byte for byte.  order: how the planes are ordered, "rgb" or "gbr"
        (ffmpeg's gbrp); the result comes back in the same order.  Rows may be padded, every plane its own way.  With dst=None returns the three planes or
        raises; with dst (three planes, views allowed) returns a bool."""
        args, out = self._planar_call(planes, None, bits, out_bits, order, dst, "renderPlanar")
        return self._finish(self._L.w2x_render_planar(*args) if args else 0, out, "render_planar failed")

    def render_planar_resized(self, planes, size, *, bits: int | None = None, out_bits: int | None = None, order: str = "rgb", filter: str = "bicubic", dst=None):
        """render_planar() with the output resized on the device to size = (rows, cols), each in [input dim, input dim * scaling]
        (w2x_render_planar_resized): at 8 / 8 and 16 / 16 bits the planes of render_resized().  With dst=None returns the planes or raises; with dst a bool."""
        fid = _filter_id(filter)
        args, out = self._planar_call(planes, size, bits, out_bits, order, dst, "renderPlanarResized")
        return self._finish(self._L.w2x_render_planar_resized(*args, fid), out, "render_planar_resized failed")

    def render_sequence_planar(self, frames, size=None, *, bits: int | None = None, out_bits: int | None = None, order: str = "rgb", filter: str = "bicubic",
                               outs=None, pinned: bool = False):
        """Equally sized planar RGB frames [(p0, p1, p2), ...] of one depth with upload / compute / download overlapped (w2x_render_sequence_planar); with
        size = (rows, cols) every frame is resized like render_planar_resized() (w2x_render_sequence_planar_resized).  Output i is the bytes of the single
        call on frame i.  The frames share one set of row strides (rows may be padded); outs: pre-allocated plane triples of one set of strides;
        pinned=True takes the output planes from alloc_host() (a ring of three frames; copies of the results are returned)."""
        return self._planar_sequence(frames, size, bits, out_bits, order, filter, outs, pinned, "rgb", (),
                                     self._L.w2x_render_sequence_planar, self._L.w2x_render_sequence_planar_resized, "render_sequence_planar failed")

    def _planar_sequence(self, frames, size, bits, out_bits, order, filter, outs, pinned, names, options, plain, resized, fallback):
        """what the planar sequence calls share, over len(names) planes per frame: the checks, the outputs and the two C entries, whose arguments end
        ..., dst_bits, count, *options[, filter]"""
        if len(frames) == 0:
            return []
        n = len(names)
        fid = _filter_id(filter)
        idx = _planar_order(order, names)
        frames = [tuple(f) if isinstance(f, (tuple, list)) else f for f in frames]
        bits = _planar_bits(frames[0], bits, n=n)
        ob = bits if out_bits is None else int(out_bits)
        if ob not in PLANAR_DTYPES:
            raise ValueError(f"out_bits must be one of {sorted(PLANAR_DTYPES)}, got {out_bits!r}")
        r, c = frames[0][0].shape
        steps = [p.strides[0] for p in frames[0]]
        for f in frames[1:]:
            try:
                fb = _planar_bits(f, bits, n=n)
            except ValueError:
                fb = None                                                       # (planes of another sample type, or no planar frame at all)
            if fb != bits or f[0].shape != (r, c) or [p.strides[0] for p in f] != steps:
                raise ValueError("frames must be planar frames of one size, one depth and one set of row strides")
        s = self._scaling
        rows, cols = (r * s, c * s) if size is None else (int(size[0]), int(size[1]))
        shape = (max(rows, 0), max(cols, 0))
        dt = np.dtype(PLANAR_DTYPES[ob])
        nb = shape[0] * shape[1] * dt.itemsize

        def alloc(host):
            if not host:
                return None, tuple(np.empty(shape, dt) for _ in range(n))
            buf = self.alloc_host((max(n * nb, 1),))          # one page-locked block per frame, carved into its planes
            return buf, tuple(buf[k * nb:(k + 1) * nb].view(dt).reshape(shape) for k in range(n))

        first = []

        def check(o):
            _planar_bits(o, ob, f"outs must hold {_COUNT[n]} 2-D {dt.name} planes of the output size with packed samples each", shape=shape, empty_ok=True, n=n)
            first.append([p.strides[0] for p in o])
            if first[-1] != first[0]:
                raise ValueError("outs must share one set of row strides")

        def run(fs, os_):
            m = len(fs)
            sp = (C.c_void_p * (n * m))(*[_data(f[k]) for f in fs for k in idx])
            dp = (C.c_void_p * (n * m))(*[_data(o[k]) for o in list(os_)[:m] for k in idx] + [None] * (n * (m - len(os_[:m]))))
            a = (self._h, sp, (C.c_size_t * n)(*[steps[k] for k in idx]), r, c, bits, dp, (C.c_size_t * n)(*[os_[0][k].strides[0] for k in idx]), rows, cols, ob, m, *options)
            return plain(*a) if size is None else resized(*a, fid)
        return self._sequence(frames, outs, pinned, alloc, lambda d: tuple(p.copy() for p in d), run, fallback, check)

    def render_planar_rgba(self, planes, *, bits: int | None = None, out_bits: int | None = None, order: str = "rgba", bleed: int = 0,
                           skip_uniform_alpha: bool = False, dst=None):
        """render_rgba() on a planar RGBA frame (w2x_render_rgbap): four 2-D planes of uint8, uint16 (bits=10 / 12 for codes in the low bits) or float32 samples,
        out_bits independent, as in render_planar(); alpha is straight.  The colour planes are render_planar() of alpha_bleed_planes(planes, bleed), the alpha
        plane is the G plane of render_planar((A, A, A)), byte for byte; at 8 / 8 bits the planes are render_rgba()'s bytes.  bleed: 0..16 (float32 planes: 0).
        skip_uniform_alpha: a frame whose alpha plane is one value runs no alpha tiles.  order: "rgba" or "gbra" (ffmpeg's gbrap); the result comes back in the
        same order.  With dst=None returns the four planes or raises; with dst (four planes, views allowed) returns a bool."""
        args, out = self._planar_call(planes, None, bits, out_bits, order, dst, "renderPlanarRgba", "rgba")
        return self._finish(self._L.w2x_render_rgbap(*args, int(bleed), int(bool(skip_uniform_alpha))) if args else 0, out, "render_planar_rgba failed")

    def render_planar_rgba_resized(self, planes, size, *, bits: int | None = None, out_bits: int | None = None, order: str = "rgba", bleed: int = 0,
                                   skip_uniform_alpha: bool = False, filter: str = "bicubic", dst=None):
        """render_planar_rgba() with the output resized on the device to size = (rows, cols), each in [input dim, input dim * scaling]
        (w2x_render_rgbap_resized); colour and alpha are resized separately and straight.  With dst=None returns the planes or raises; with dst a bool."""
        fid = _filter_id(filter)
        args, out = self._planar_call(planes, size, bits, out_bits, order, dst, "renderPlanarRgbaResized", "rgba")
        return self._finish(self._L.w2x_render_rgbap_resized(*args, int(bleed), int(bool(skip_uniform_alpha)), fid), out, "render_planar_rgba_resized failed")

    def render_sequence_planar_rgba(self, frames, size=None, *, bits: int | None = None, out_bits: int | None = None, order: str = "rgba", bleed: int = 0,
                                    skip_uniform_alpha: bool = False, filter: str = "bicubic", outs=None, pinned: bool = False):
        """Equally sized planar RGBA frames [(p0, p1, p2, p3), ...] of one depth and one set of options with upload / compute / download overlapped
        (w2x_render_sequence_rgbap; with size = (rows, cols): w2x_render_sequence_rgbap_resized).  Output i is the bytes of the single call on frame i;
        skip_uniform_alpha is decided per frame.  Strides, outs and pinned as in render_sequence_planar()."""
        return self._planar_sequence(frames, size, bits, out_bits, order, filter, outs, pinned, "rgba", (int(bleed), int(bool(skip_uniform_alpha))),
                                     self._L.w2x_render_sequence_rgbap, self._L.w2x_render_sequence_rgbap_resized, "render_sequence_planar_rgba failed")

    def set_dither(self, mode="none", phase: int = 0, advance: int = 0) -> bool:
        """The dither of every integer sample the following frame calls write (w2x_set_dither, c_api_dither.h states the rule): mode "none", "ordered" (8 x 8
        Bayer) or "bluenoise" (64 x 64 void-and-cluster table) - or its number, which the engine checks.  phase moves the pattern; frame i of a sequence call is
        dithered as the single call at phase + i * advance (advance 0: a still pattern, 1: temporal dither).  Alpha and float outputs are never dithered.  The
        setting stays until it is changed and may be made before load().  An unknown name raises ValueError; an unknown number returns False (message
        callback) and leaves the previous setting."""
        if isinstance(mode, str):
            if mode not in DITHER_MODES:
                raise ValueError(f"dither mode must be one of {sorted(DITHER_MODES)}, got {mode!r}")
            mode = DITHER_MODES[mode]
        return bool(self._L.w2x_set_dither(self._h, int(mode), int(phase) & 0xFFFFFFFF, int(advance) & 0xFFFFFFFF))

    def dither(self):
        """the current setting as (mode name, phase, advance) (w2x_get_dither)"""
        m, p, a = C.c_int(0), C.c_uint(0), C.c_uint(0)
        if not self._L.w2x_get_dither(self._h, C.byref(m), C.byref(p), C.byref(a)):
            raise W2xError("w2x_get_dither failed")
        return {v: k for k, v in DITHER_MODES.items()}[m.value], int(p.value), int(a.value)

    def dither_planes(self, planes, bits: int, dst=None):
        """Test hook (w2x_dither_planes): three 2-D float32 planes of one shape (views with padded rows allowed) -> three planes of `bits` (8: uint8; 10, 12, 16:
        uint16), every sample quantised on the device from V = v * (2^bits - 1) by the store of the compose and resample kernels with the current set_dither()
        setting (none: sat(rint(V))); plane k has plane index k.  dst: three pre-allocated planes of that depth's dtype (views allowed), which are returned."""
        src = [np.asarray(p) for p in planes]
        if len(src) != 3 or any(p.ndim != 2 or p.dtype != np.float32 or p.shape != src[0].shape or p.strides[1] != 4 for p in src):
            raise ValueError("planes must be three 2-D float32 planes of one shape with packed samples")
        bits = int(bits)
        if bits not in (8, 10, 12, 16):
            raise ValueError(f"bits must be 8, 10, 12 or 16, got {bits!r}")
        r, c = src[0].shape
        dt = np.dtype(PLANAR_DTYPES[bits])
        out = tuple(np.empty((r, c), dt) for _ in range(3)) if dst is None else tuple(dst)
        if len(out) != 3 or any(p.ndim != 2 or p.dtype != dt or p.shape != (r, c) or p.strides[1] != dt.itemsize for p in out):
            raise ValueError(f"dst must be three 2-D {dt.name} planes of the input's shape with packed samples")
        ok = self._L.w2x_dither_planes(self._h, (C.c_void_p * 3)(*[_data(p) for p in src]), (C.c_size_t * 3)(*[p.strides[0] for p in src]), r, c,
                                       (C.c_void_p * 3)(*[_data(p) for p in out]), (C.c_size_t * 3)(*[p.strides[0] for p in out]), bits)
        return self._finish(ok, out, "dither_planes failed")

    def set_resize_light(self, mode="gamma") -> bool:
        """The light every following resized frame is averaged in (w2x_set_resize_light, c_api_resize_light.h states the rule): "gamma" - the encoded values as
        they are, the default -, "srgb" or "bt709" - the canvas decoded by that curve, resized in linear light and encoded again ahead of quantisation, dither
        and the Y'CbCr matrix - or the mode's number, which the engine checks.  Alpha is never touched; a call at the scaled size stays the plain call.  The
        setting stays until it is changed and may be made before load().  An unknown name raises ValueError; an unknown number returns False (message
        callback) and leaves the previous setting."""
        if isinstance(mode, str):
            if mode not in RESIZE_LIGHTS:
                raise ValueError(f"resize light must be one of {sorted(RESIZE_LIGHTS)}, got {mode!r}")
            mode = RESIZE_LIGHTS[mode]
        return bool(self._L.w2x_set_resize_light(self._h, int(mode)))

    def resize_light(self) -> str:
        """the current setting's name (w2x_get_resize_light)"""
        return {v: k for k, v in RESIZE_LIGHTS.items()}[int(self._L.w2x_get_resize_light(self._h))]

    def set_edge(self, mode="replicate") -> bool:
        """What every following frame call of the RGB family reads beyond the frame edge (w2x_set_edge, c_api_edge.h states the rule): "replicate" - the edge
        pixel repeated, the default -, "wrap" - the frame is one period of a texture that tiles - or "mirror" - reflection without repeating the edge sample -, or
        the mode's number, which the engine checks.  It acts on the tiles' borders, on the colour bleed (wrap) and on the taps of the resized calls.  The setting
        stays until it is changed and may be made before load().  YUV calls, strips and shards are refused under wrap and mirror.  An unknown name raises
        ValueError; an unknown number returns False (message callback) and leaves the previous setting."""
        if isinstance(mode, str):
            if mode not in EDGE_MODES:
                raise ValueError(f"edge mode must be one of {sorted(EDGE_MODES)}, got {mode!r}")
            mode = EDGE_MODES[mode]
        return bool(self._L.w2x_set_edge(self._h, int(mode)))

    def edge(self) -> str:
        """the current setting's name (w2x_get_edge)"""
        return {v: k for k, v in EDGE_MODES.items()}[int(self._L.w2x_get_edge(self._h))]

    def resize_planes(self, planes, size, bits: int, filter: str = "bicubic", dst=None):
        """Test hook (w2x_resize_planes): three 2-D float32 planes of one shape (views with padded rows allowed) are taken as the canvas of a resized frame and
        go the production way - the canvas kernels' decode, the planar resize kernel, its store - under the current set_resize_light() and set_dither()
        settings -> three planes of size = (rows, cols) and `bits` (8: uint8; 10, 12, 16: uint16; 32: float32).  The target lies between a quarter of the
        source size and the source size per axis.  dst: three pre-allocated planes of that shape and dtype (views allowed), which are returned."""
        src = [np.asarray(p) for p in planes]
        if len(src) != 3 or any(p.ndim != 2 or p.dtype != np.float32 or p.shape != src[0].shape or p.strides[1] != 4 for p in src):
            raise ValueError("planes must be three 2-D float32 planes of one shape with packed samples")
        bits = int(bits)
        if bits not in PLANAR_DTYPES:
            raise ValueError(f"bits must be one of {sorted(PLANAR_DTYPES)}, got {bits!r}")
        if filter not in RESIZE_FILTERS:
            raise ValueError(f"filter must be one of {sorted(RESIZE_FILTERS)}, got {filter!r}")
        r, c = src[0].shape
        orows, ocols = int(size[0]), int(size[1])
        dt = np.dtype(PLANAR_DTYPES[bits])
        out = tuple(np.empty((orows, ocols), dt) for _ in range(3)) if dst is None else tuple(dst)
        if len(out) != 3 or any(p.ndim != 2 or p.dtype != dt or p.shape != (orows, ocols) or p.strides[1] != dt.itemsize for p in out):
            raise ValueError(f"dst must be three 2-D {dt.name} planes of the target's shape with packed samples")
        ok = self._L.w2x_resize_planes(self._h, (C.c_void_p * 3)(*[_data(p) for p in src]), (C.c_size_t * 3)(*[p.strides[0] for p in src]), r, c,
                                       (C.c_void_p * 3)(*[_data(p) for p in out]), (C.c_size_t * 3)(*[p.strides[0] for p in out]), orows, ocols, bits,
                                       RESIZE_FILTERS[filter])
        return self._finish(ok, out, "resize_planes failed")

    def alpha_bleed_planes_device(self, planes, radius: int, *, bits: int | None = None, order: str = "rgba", words: bool = False):
        """Test hook (w2x_alpha_bleed_rgbap_device): the device bleed alone on a planar RGBA frame -> the three colour planes the tiles are read from, in R, G, B
        order; words=True: (planes, (max(key), max(top - key))) - the alpha range the kernel reduced (c_api_rgbap.h)"""
        idx = _planar_order(order, "rgba")
        bits = _planar_bits(planes, bits, n=4)
        src = [planes[k] for k in idx]
        r, c = src[0].shape
        out = tuple(np.empty((r, c), src[0].dtype) for _ in range(3))
        w = (C.c_uint * 2)(0, 0)
        ok = self._L.w2x_alpha_bleed_rgbap_device(self._h, (C.c_void_p * 4)(*[_data(p) for p in src]), (C.c_size_t * 4)(*[p.strides[0] for p in src]), r, c, bits,
                                                  int(radius), (C.c_void_p * 3)(*[_data(p) for p in out]), (C.c_size_t * 3)(*[p.strides[0] for p in out]), w)
        return self._finish(ok, (out, (int(w[0]), int(w[1]))) if words else out, "alpha_bleed_planes_device failed")

    def alpha_bleed_device(self, bgra: np.ndarray, radius: int) -> np.ndarray:
        """Test hook (w2x_alpha_bleed_device): the device bleed alone on a uint8 [rows, cols, 4] BGRA frame -> the [rows, cols, 3] BGR frame the tiles are read from"""
        _frame_ok(bgra, 4, (np.uint8,), "bgra must be a uint8 [rows, cols, 4] BGRA array with packed pixels")
        out = np.empty((bgra.shape[0], bgra.shape[1], 3), np.uint8)
        return self._finish(self._L.w2x_alpha_bleed_device(self._h, _data(bgra), bgra.shape[0], bgra.shape[1], bgra.strides[0], _data(out), out.strides[0], int(radius)),
                            out, "alpha_bleed_device failed")

    def render_resized(self, src: np.ndarray, size, filter: str = "bicubic", dst: np.ndarray | None = None):
        """render() followed by an antialiased resize on the device to size = (rows, cols), each in [input dim, input dim * scaling]
        (w2x_render_resized / w2x_render16_resized; uint8 or uint16 frames).  With dst=None returns the array or raises; with dst returns a bool."""
        _frame_ok(src, 3, (np.uint8, np.uint16), "src must be a uint8 (or uint16) [rows, cols, 3] BGR array with packed pixels")
        rows, cols = int(size[0]), int(size[1])
        fid = _filter_id(filter)
        out = np.empty((max(rows, 0), max(cols, 0), 3), src.dtype) if dst is None else None
        dst = out if dst is None else dst
        # (an empty target: refused by the library; a wrong dst raises here, where render() returns False)
        _frame_ok(dst, 3, (src.dtype,), "dst must be a packed [rows, cols, 3] array of the target size and the frame's sample type", shape=(rows, cols), empty_ok=True)
        fn = self._L.w2x_render_resized if src.itemsize == 1 else self._L.w2x_render16_resized
        return self._finish(fn(self._h, src.ctypes.data, src.shape[0], src.shape[1], src.strides[0], _data(dst), rows, cols, dst.strides[0], fid), out, "render_resized failed")

    def render_sequence_resized(self, frames, size, outs=None, pinned: bool = False, filter: str = "bicubic"):
        """render_sequence() with every frame resized to size = (rows, cols) like render_resized() (w2x_render_sequence_resized; uint8 frames).
        outs / pinned as in render_sequence()."""
        if len(frames) == 0:
            return []
        rows, cols = int(size[0]), int(size[1])
        fid = _filter_id(filter)
        r, c = frames[0].shape[:2]
        for f in frames:
            _frame_ok(f, 3, (np.uint8,), "frames must be packed uint8 [rows, cols, 3] arrays of one size", shape=(r, c), rows_packed=True)

        def run(fs, os_):
            return self._L.w2x_render_sequence_resized(self._h, _pointers(fs), r, c, c * 3, _pointers(os_, len(fs)), rows, cols, cols * 3, len(fs), fid)
        return self._packed_sequence(frames, 3, (rows, cols, 3), outs, pinned, "outs must be packed uint8 arrays of the target size", run, "render_sequence_resized failed")

    def render_strip(self, src: np.ndarray, dst: np.ndarray, part: int, parts: int) -> bool:
        """One device's share of a frame split into tile-column strips (w2x_render_strip): writes only its columns of dst."""
        s = self._scaling
        _frame_ok(src, 3, (np.uint8,), "src must be a uint8 [rows, cols, 3] BGR array with packed pixels")
        _frame_ok(dst, 3, (np.uint8,), "dst must be a packed uint8 array of the scaled size", shape=(src.shape[0] * s, src.shape[1] * s))
        return bool(self._L.w2x_render_strip(self._h, src.ctypes.data, src.shape[0], src.shape[1], src.strides[0],
                                             dst.ctypes.data, dst.strides[0], int(part), int(parts)))

    # ---- one frame over several PROCESSES (one engine each): w2x_shard_compute / w2x_shard_slab / w2x_shard_finish + the IPC helpers below
    def shard_compute(self, src: np.ndarray, part: int, parts: int) -> bool:
        _frame_ok(src, 3, (np.uint8,), "src must be a uint8 [rows, cols, 3] BGR array with packed pixels")
        return bool(self._L.w2x_shard_compute(self._h, src.ctypes.data, src.shape[0], src.shape[1], src.strides[0], int(part), int(parts)))

    def shard_slab_handle(self):
        """(device pointer, 64-byte IPC handle) of this engine's tile slab (changes only when a larger frame makes the slab grow)"""
        ptr = self._L.w2x_shard_slab(self._h, None)
        buf = (C.c_uint8 * 64)()
        if not ptr or not self._L.w2x_ipc_export(ptr, buf):
            raise W2xError("could not export the tile slab (hipIpcGetMemHandle)")
        return int(ptr), bytes(buf)

    def shard_finish(self, dst: np.ndarray, part: int, parts: int, slabs, devices=None) -> bool:
        """slabs[q]: device pointer (int) of part q's slab in THIS process (w2x ipc_open of its handle; 0 for parts that are not needed)"""
        _frame_ok(dst, 3, (np.uint8,), "dst must be a packed uint8 [rows, cols, 3] array of the scaled size")
        arr = (C.c_void_p * parts)(*[C.c_void_p(int(p) or None) for p in slabs])
        dev = (C.c_int * parts)(*[int(d) for d in devices]) if devices is not None else None
        return bool(self._L.w2x_shard_finish(self._h, dst.ctypes.data, dst.shape[0], dst.shape[1], dst.strides[0], int(part), int(parts), arr, dev))

    def render_yuv(self, y, u: np.ndarray | None = None, v: np.ndarray | None = None, *, matrix: str = "bt709", full_range: bool = False, out_bits: int | None = None,
                   out=None, layout: str | None = None, out_layout: str | None = None, siting: str = "left", out_siting: str | None = None):
        """render() on a YUV 4:2:0 frame (w2x_render_yuv): uint8 planes are 8-bit, uint16 planes 10-bit; out_bits (8 or 10, default the input's)
        sets the output depth.  Returns (Y, U, V) at the scaled size, or raises.  out: pre-allocated planes (then a bool is returned).
        With the frame given as one tuple of planes, or with layout= / out_layout= ("i420", "i422", "i444", "nv12"; out_layout defaults to the input's), the
        call goes through w2x_render_yuv_layout: an "nv12" frame is (y, uv) with uv of ceil(rows/2) x 2 * ceil(cols/2) samples (10-bit: P010, codes << 6),
        and the result is the tuple of out_layout's planes (yuv_layout_plane_shapes).
        siting= / out_siting= ("left", "center", "topleft"; out_siting defaults to the input's): where the chroma samples of the frame / of the result sit
        (DESIGN 9l).  With both "left" the call is the one above; any other pair goes through w2x_render_yuv_sited at the scaled size."""
        sid, osid = _siting_ids(siting, out_siting)
        with_layout = isinstance(y, (tuple, list)) or layout is not None or out_layout is not None
        if isinstance(y, (tuple, list)) and (u is not None or v is not None):
            raise ValueError("give the frame as one tuple of planes or as three positional planes, not both")
        if not with_layout:
            planes = (y, u, v)
        else:
            planes = tuple(y) if isinstance(y, (tuple, list)) else tuple(p for p in (y, u, v) if p is not None)
        layout = layout or "i420"
        out_layout = layout if out_layout is None else out_layout
        lid, olid = _layout_id(layout), _layout_id(out_layout)
        bits = _yuv_layout_bits(planes, layout) if with_layout else _yuv_bits(planes)
        ob = bits if out_bits is None else int(out_bits)
        rows, cols = planes[0].shape
        s = self._scaling
        dt = np.uint16 if ob == 10 else np.uint8
        shapes = yuv_layout_plane_shapes(rows * s, cols * s, out_layout)
        dst = tuple(np.empty(shape, dt) for shape in shapes) if out is None else tuple(out)
        # the C ABI sees pointers and steps only: the plane shapes and the sample type of out_bits are checked here
        # (the three-plane call does not look at planes it allocated itself: on an engine that was never loaded it reaches the library, the layout call raises)
        if (with_layout or out is not None) and (
                len(dst) != len(shapes) or any(not isinstance(p, np.ndarray) or p.dtype != dt or p.shape != shape or p.strides[1] != p.itemsize for p, shape in zip(dst, shapes))):
            raise ValueError(f"out must be the 2-D planes of the scaled {out_layout} shapes, uint8 for 8-bit and uint16 for 10-bit output, with packed rows" if with_layout else
                             "out must be three 2-D planes of the scaled 4:2:0 shapes, uint8 for 8-bit and uint16 for 10-bit output, with packed rows")
        (sp, ss), (dp, ds) = _plane_args(planes), _plane_args(dst)
        a = (self._h, (C.c_void_p * 3)(*sp), (C.c_size_t * 3)(*ss), rows, cols, bits, (C.c_void_p * 3)(*dp), (C.c_size_t * 3)(*ds), rows * s, cols * s, ob,
             _matrix_id(matrix), 1 if full_range else 0)
        if sid or osid:
            ok = self._L.w2x_render_yuv_sited(*a[:6], lid, sid, *a[6:11], olid, osid, *a[11:], RESIZE_FILTERS["bicubic"])
        else:
            ok = self._L.w2x_render_yuv_layout(*a[:6], lid, *a[6:11], olid, *a[11:]) if with_layout else self._L.w2x_render_yuv(*a)
        return self._finish(ok, dst if out is None else None, "render_yuv failed")

    def render_yuv_resized(self, y: np.ndarray, u: np.ndarray, v: np.ndarray, size, *, matrix: str = "bt709", full_range: bool = False,
                           out_bits: int | None = None, filter: str = "bicubic", dst=None):
        """render_yuv() with the canvas resized on the device to size = (rows, cols), each in [input dim, input dim * scaling], before it is encoded
        (w2x_render_yuv_resized).  Returns (Y, U, V) at the target size, or raises.  dst: pre-allocated planes (then a bool is returned).
        4:2:0 planes only, both sides: planes of another layout's shapes raise the ValueError that names 4:2:0 (the other layouts: render_yuv_layout_resized)."""
        bits = _yuv_bits((y, u, v))
        ob = bits if out_bits is None else int(out_bits)
        rows, cols = int(size[0]), int(size[1])
        fid = _filter_id(filter)
        dt = np.uint16 if ob == 10 else np.uint8
        shapes = yuv_plane_shapes(max(rows, 0), max(cols, 0))
        out = tuple(np.empty(shape, dt) for shape in shapes) if dst is None else tuple(dst)
        if len(out) != 3 or any(not isinstance(p, np.ndarray) or p.dtype != dt or p.shape != shape or (p.size and p.strides[1] != p.itemsize) for p, shape in zip(out, shapes)):
            raise ValueError("dst must be three 2-D planes of the target's 4:2:0 shapes, uint8 for 8-bit and uint16 for 10-bit output, with packed rows")
        dp = (C.c_void_p * 3)(*[_data(p) for p in out])   # (an empty target: refused by the library)
        ok = self._L.w2x_render_yuv_resized(self._h, _pointers((y, u, v)), (C.c_size_t * 3)(*[p.strides[0] for p in (y, u, v)]), y.shape[0], y.shape[1], bits,
                                            dp, (C.c_size_t * 3)(*[p.strides[0] for p in out]), rows, cols, ob, _matrix_id(matrix), 1 if full_range else 0, fid)
        return self._finish(ok, out if dst is None else None, "render_yuv_resized failed")

    def render_sequence_yuv_resized(self, frames, size, *, matrix: str = "bt709", full_range: bool = False, out_bits: int | None = None, pinned: bool = False,
                                    filter: str = "bicubic"):
        """render_sequence_yuv() with every frame resized to size = (rows, cols) like render_yuv_resized() (w2x_render_sequence_yuv_resized); 4:2:0 planes only
        (the other layouts: render_sequence_yuv_layout_resized)"""
        return self._sequence_yuv(frames, (int(size[0]), int(size[1])), _filter_id(filter), matrix, full_range, out_bits, pinned)

    def render_yuv_layout_resized(self, planes, size, *, layout: str = "i420", out_layout: str | None = None, matrix: str = "bt709", full_range: bool = False,
                                  out_bits: int | None = None, filter: str = "bicubic", dst=None, siting: str = "left", out_siting: str | None = None):
        """render_yuv_resized() on frames of any layout (w2x_render_yuv_layout_resized): planes is the tuple of `layout`'s planes - (y, u, v), or (y, uv) for
        "nv12" (10-bit: P010, codes << 6) -, out_layout (default: layout) the layout of the result, size = (rows, cols) the target, each in [input dim,
        input dim * scaling].  Returns the tuple of out_layout's planes at the target size (yuv_layout_plane_shapes), or raises.  dst: pre-allocated planes
        (then a bool is returned).  Planes that do not have the named layout's shapes and unknown names raise ValueError before any library call.
        siting= / out_siting= as in render_yuv(): any pair but "left" / "left" goes through w2x_render_yuv_sited."""
        sid, osid = _siting_ids(siting, out_siting)
        out_layout = layout if out_layout is None else out_layout
        lid, olid = _layout_id(layout), _layout_id(out_layout)
        if not isinstance(planes, (tuple, list)):
            raise ValueError("give the frame as one tuple of the layout's planes")
        planes = tuple(planes)
        bits = _yuv_layout_bits(planes, layout)
        ob = bits if out_bits is None else int(out_bits)
        rows, cols = int(size[0]), int(size[1])
        fid, mid = _filter_id(filter), _matrix_id(matrix)
        dt = np.uint16 if ob == 10 else np.uint8
        shapes = yuv_layout_plane_shapes(max(rows, 0), max(cols, 0), out_layout)
        out = tuple(np.empty(shape, dt) for shape in shapes) if dst is None else tuple(dst)
        if len(out) != len(shapes) or any(not isinstance(p, np.ndarray) or p.dtype != dt or p.shape != shape or (p.size and p.strides[1] != p.itemsize) for p, shape in zip(out, shapes)):
            raise ValueError(f"dst must be the 2-D planes of the target's {out_layout} shapes, uint8 for 8-bit and uint16 for 10-bit output, with packed rows")
        sp, ss = _plane_args(planes)
        dp = [_data(p) for p in out] + [None] * (3 - len(out))   # (an empty target: refused by the library)
        ds = [p.strides[0] for p in out] + [0] * (3 - len(out))
        if sid or osid:
            ok = self._L.w2x_render_yuv_sited(self._h, (C.c_void_p * 3)(*sp), (C.c_size_t * 3)(*ss), planes[0].shape[0], planes[0].shape[1], bits, lid, sid,
                                              (C.c_void_p * 3)(*dp), (C.c_size_t * 3)(*ds), rows, cols, ob, olid, osid, mid, 1 if full_range else 0, fid)
        else:
            ok = self._L.w2x_render_yuv_layout_resized(self._h, (C.c_void_p * 3)(*sp), (C.c_size_t * 3)(*ss), planes[0].shape[0], planes[0].shape[1], bits, lid,
                                                       (C.c_void_p * 3)(*dp), (C.c_size_t * 3)(*ds), rows, cols, ob, olid, mid, 1 if full_range else 0, fid)
        return self._finish(ok, out if dst is None else None, "render_yuv_layout_resized failed")

    def render_sequence_yuv_layout_resized(self, frames, size, *, layout: str = "i420", out_layout: str | None = None, matrix: str = "bt709", full_range: bool = False,
                                           out_bits: int | None = None, filter: str = "bicubic", pinned: bool = False, siting: str = "left",
                                           out_siting: str | None = None):
        """render_sequence_yuv() over frames of `layout` with every frame resized to size = (rows, cols) like render_yuv_layout_resized()
        (w2x_render_sequence_yuv_layout_resized): every frame a tuple of `layout`'s planes, every result a tuple of out_layout's.  siting= / out_siting= as in
        render_yuv(), one pair for the sequence (any but "left" / "left": w2x_render_sequence_yuv_sited)"""
        return self._sequence_yuv(frames, (int(size[0]), int(size[1])), _filter_id(filter), matrix, full_range, out_bits, pinned, layout, out_layout or layout,
                                  _siting_ids(siting, out_siting))

    def render_sequence_yuv(self, frames, *, matrix: str = "bt709", full_range: bool = False, out_bits: int | None = None, pinned: bool = False,
                            layout: str | None = None, out_layout: str | None = None, siting: str = "left", out_siting: str | None = None):
        """render_yuv() over equally sized frames [(y, u, v), ...] through the pipeline of render_sequence() (w2x_render_sequence_yuv).
        pinned=True takes the output planes from alloc_host() (a ring of three frames; copies of the results are returned).
        layout= / out_layout= as in render_yuv() (w2x_render_sequence_yuv_layout): every frame is a tuple of `layout`'s planes - [(y, uv), ...] for "nv12" -
        and a frame of another layout's shapes raises ValueError.  siting= / out_siting= as in render_yuv(), one pair for the sequence (any but "left" / "left":
        w2x_render_sequence_yuv_sited at the scaled size)."""
        return self._sequence_yuv(frames, None, None, matrix, full_range, out_bits, pinned, layout, out_layout, _siting_ids(siting, out_siting))

    def _sequence_yuv(self, frames, size, fid, matrix, full_range, out_bits, pinned, layout=None, out_layout=None, sitings=(0, 0)):
        """the YUV sequence calls: size = None the scaled size (w2x_render_sequence_yuv; with a layout given w2x_render_sequence_yuv_layout), else the target of
        w2x_render_sequence_yuv_resized with filter fid (with a layout given w2x_render_sequence_yuv_layout_resized); sitings other than (left, left):
        w2x_render_sequence_yuv_sited, at the scaled size with the bicubic filter's id, which no resize uses there"""
        if len(frames) == 0:
            return []
        with_layout = layout is not None or out_layout is not None
        layout = layout or "i420"
        out_layout = out_layout or layout
        lid, olid = _layout_id(layout), _layout_id(out_layout)
        frames = [tuple(f) for f in frames]
        bits = _yuv_layout_bits(frames[0], layout) if with_layout else _yuv_bits(frames[0])
        ob = bits if out_bits is None else int(out_bits)
        rows, cols = frames[0][0].shape
        steps = [p.strides[0] for p in frames[0]]
        for f in frames[1:]:
            try:
                fb = _yuv_layout_bits(f, layout) if with_layout else _yuv_bits(f)
            except ValueError:
                fb = None                                                       # (the planes of another layout)
            if fb != bits or f[0].shape != (rows, cols) or [p.strides[0] for p in f] != steps:
                raise ValueError("frames must be YUV planes of one size, depth and layout")
        s = self._scaling
        orows, ocols = (rows * s, cols * s) if size is None else size
        shapes = yuv_layout_plane_shapes(max(orows, 1), max(ocols, 1), out_layout)   # (an empty target: refused by the library)
        steps = steps + [0] * (3 - len(steps))
        dt = np.uint8 if ob != 10 else np.uint16
        sizes = [r * c * np.dtype(dt).itemsize for r, c in shapes]

        def alloc(host):
            if not host:
                return None, tuple(np.empty(shape, dt) for shape in shapes)
            buf = self.alloc_host((sum(sizes),))          # one page-locked block per frame, carved into its planes
            starts = [sum(sizes[:k]) for k in range(len(sizes))]
            return buf, tuple(buf[o:o + nb].view(dt).reshape(shape) for o, nb, shape in zip(starts, sizes, shapes))

        def run(fs, os_):
            m = len(fs)
            sp = (C.c_void_p * (3 * m))(*[q for f in fs for q in _plane_args(f)[0]])
            dp = (C.c_void_p * (3 * m))(*[q for o in os_ for q in _plane_args(o)[0]])
            # (the matrix is looked at here: a pinned call with an unknown one has taken its ring by now, and gives it back)
            a = (self._h, sp, (C.c_size_t * 3)(*steps), rows, cols, bits, dp, (C.c_size_t * 3)(*_plane_args(os_[0])[1]), orows, ocols, ob, m,
                 _matrix_id(matrix), 1 if full_range else 0)
            if sitings[0] or sitings[1]:
                return self._L.w2x_render_sequence_yuv_sited(*a[:6], lid, sitings[0], *a[6:11], olid, sitings[1], *a[11:], RESIZE_FILTERS["bicubic"] if fid is None else fid)
            if size is not None and with_layout:
                return self._L.w2x_render_sequence_yuv_layout_resized(*a[:6], lid, *a[6:11], olid, *a[11:], fid)
            if size is not None:
                return self._L.w2x_render_sequence_yuv_resized(*a, fid)
            return self._L.w2x_render_sequence_yuv_layout(*a[:6], lid, *a[6:11], olid, *a[11:]) if with_layout else self._L.w2x_render_sequence_yuv(*a)
        return self._sequence(frames, None, pinned, alloc, lambda d: tuple(p.copy() for p in d), run, "render_sequence_yuv failed" if size is None else "render_sequence_yuv_layout_resized failed" if with_layout else "render_sequence_yuv_resized failed")

    def alloc_host(self, shape) -> np.ndarray:
        """A uint8 array over page-locked memory owned by the engine (w2x_alloc_host): frame buffers whose PCIe copies
        render_sequence() can overlap with the kernels.  Valid until free_host(arr) / close()."""
        n = int(np.prod(shape))
        ptr = self._L.w2x_alloc_host(self._h, n)
        if not ptr:
            raise W2xError("w2x_alloc_host failed")
        arr = np.frombuffer((C.c_uint8 * n).from_address(ptr), np.uint8).reshape(shape)
        self._host_bufs[arr.ctypes.data] = ptr
        return arr

    def free_host(self, arr: np.ndarray) -> None:
        ptr = self._host_bufs.pop(arr.ctypes.data, None)
        if ptr:
            self._L.w2x_free_host(self._h, ptr)

    def render_sequence(self, frames, outs=None, pinned: bool = False):
        """Equally sized frames with upload / compute / download overlapped (w2x_render_sequence).  outs: list of pre-allocated
        arrays (may repeat, e.g. a ring of buffers) or None; pinned=True takes the output buffers it allocates from alloc_host()
        (copies of the results are returned) - pass alloc_host() arrays as frames / outs yourself to avoid that copy."""
        if len(frames) == 0:
            return []
        s = self._scaling
        r, c = frames[0].shape[:2]
        for f in frames:
            _frame_ok(f, 3, (np.uint8,), "frames must be packed uint8 [rows, cols, 3] arrays of one size", shape=(r, c), rows_packed=True)

        def run(fs, os_):
            return self._L.w2x_render_sequence(self._h, _pointers(fs), r, c, c * 3, _pointers(os_, len(fs)), c * s * 3, len(fs))
        return self._packed_sequence(frames, 3, (r * s, c * s, 3), outs, pinned, "outs must be packed uint8 arrays of the scaled size", run, "render_sequence failed")

    def infer(self, x: np.ndarray) -> np.ndarray:
        """Private trt::Img2Img::infer (img2img_infer.cpp:41-93) as a test hook: [B,3,T,T] f32 -> [B,3,T',T'] f32."""
        x = np.ascontiguousarray(x, np.float32)
        b, t = self._batch, self._tile
        if not b:
            raise W2xError("infer called before a successful load")
        if x.shape != (b, 3, t, t):        # img2img_infer.cpp:43-68: batch count and tile shape must be the loaded configuration's
            raise ValueError(f"infer expects a [{b}, 3, {t}, {t}] blob, got {list(x.shape)}")
        to = self.output_tile_size
        y = np.empty((b, 3, to, to), np.float32)
        return self._finish(self._L.w2x_infer(self._h, x.ctypes.data, y.ctypes.data), y, "infer failed")

    @property
    def output_tile_size(self) -> int:
        return self._L.w2x_output_tile_size(self._h)

    @property
    def pass_tiles(self) -> int:
        return self._L.w2x_pass_tiles(self._h)

    @property
    def plan_flops(self) -> float:
        return self._L.w2x_plan_flops(self._h)

    @property
    def last_render_ms(self) -> float:
        return self._L.w2x_last_render_ms(self._h)

    def bench_resident(self, iters: int) -> float:
        return self._L.w2x_bench_resident(self._h, iters)

    def resident_output(self, dst: np.ndarray) -> bool:
        """Copy the output frame the last bench_resident() step left on the device into dst (packed [rows * s, cols * s, 3] of the frame's sample type)."""
        if not dst.flags.c_contiguous:
            raise ValueError("dst must be a packed array")
        return bool(self._L.w2x_resident_output(self._h, dst.ctypes.data, dst.nbytes))

    def profile_frame(self) -> dict:
        """HIP-event time per kernel family for one resident frame: {family: (ms, launches, flop)}, plus 'frame_ms'."""
        out = np.zeros(31, np.float64)
        if not self._L.w2x_profile_frame(self._h, out.ctypes.data, 31):
            raise W2xError(self.last_error() or "profile failed")
        names = ["gemm", "attention", "se_scale", "gather", "compose", "mlp"]
        d = {n: (float(out[5 * i]), int(out[5 * i + 1]), float(out[5 * i + 2])) for i, n in enumerate(names)}
        d["frame_ms"] = float(out[30])
        return d

    def op_times(self) -> np.ndarray:
        out = np.zeros(4096, np.float64)
        n = self._L.w2x_op_times(self._h, out.ctypes.data, 4096)
        return out[:n].copy()


def render_sharded(engines, src: np.ndarray, dst: np.ndarray = None) -> np.ndarray:
    """ONE frame over several engines of this process, every tile computed once (w2x_render_sharded): engine k takes the k-th contiguous
    range of the tile order, the seam bands travel device to device, each engine composes and downloads its own cells of `dst`."""
    s = engines[0]._scaling
    _frame_ok(src, 3, (np.uint8,), "src must be a uint8 [rows, cols, 3] BGR array with packed pixels")
    if dst is None:
        dst = np.empty((src.shape[0] * s, src.shape[1] * s, 3), np.uint8)
    _frame_ok(dst, 3, (np.uint8,), "dst must be a packed uint8 array of the scaled size", shape=(src.shape[0] * s, src.shape[1] * s))
    handles = (C.c_void_p * len(engines))(*[e._h for e in engines])
    if not lib().w2x_render_sharded(handles, len(engines), src.ctypes.data, src.shape[0], src.shape[1], src.strides[0], dst.ctypes.data, dst.strides[0]):
        raise W2xError(engines[0].last_error() or "sharded render failed")
    return dst


def chain_plan(rows: int, cols: int, scalings, size=None) -> dict:
    """The frames of a chained render (w2x_chain_plan, host only): a rows x cols frame through stages of the scale factors `scalings` (2 to 4 of them), the last
    stage's canvas resized to size = (rows, cols) or, size=None, left as it is.  Returns {"stages": [(rows, cols) of the frame each stage reads], "canvas": the
    last stage's, "target": (rows, cols), "scale": S}; ValueError naming the rule (CHAIN_REFUSALS) for a chain the library refuses."""
    sc = [int(v) for v in scalings]
    n = len(sc)
    out = (C.c_int * (2 * max(n, 0) + 5))()
    dr, dc = (0, 0) if size is None else (int(size[0]), int(size[1]))
    if size is not None and (dr <= 0 or dc <= 0):
        raise ValueError("chain refused: target")
    why = lib().w2x_chain_plan(int(rows), int(cols), (C.c_int * max(n, 1))(*sc), n, dr, dc, out)
    if why:
        raise ValueError(f"chain refused: {CHAIN_REFUSALS.get(why, why)}")
    v = list(out)
    return {"stages": [(v[2 * k], v[2 * k + 1]) for k in range(n)], "canvas": (v[2 * n], v[2 * n + 1]), "target": (v[2 * n + 2], v[2 * n + 3]), "scale": v[2 * n + 4]}


def _chain(engines):
    """the handle array and the total scale factor of the engines of a chained call (0 while one of them is not loaded: the library refuses the call)"""
    if not isinstance(engines, (list, tuple)) or not 2 <= len(engines) <= 4 or not all(isinstance(e, Img2Img) and e._h for e in engines):
        raise ValueError("engines must be a list of 2 to 4 open Img2Img engines (the same engine may appear more than once)")
    total = 1
    for e in engines:
        total *= e._scaling
    return (C.c_void_p * len(engines))(*[e._h for e in engines]), len(engines), total


def render_chained(engines, src: np.ndarray, quantize: bool = False, dst: np.ndarray | None = None):
    """ONE frame through 2 to 4 engines one after the other (w2x_render_chained): x4 from two x2 models, x8, x16, the frame staying on the device between the
    stages.  src: a uint8 or uint16 [rows, cols, 3] BGR frame; the result has rows * S x cols * S, S the product of the engines' scale factors.  quantize=False:
    the frame between two stages is unrounded - the bytes of render_planar(out_bits=32) followed by render_planar() of that -; quantize=True: it is rounded to
    the frame's depth - the bytes of b.render(a.render(src)).  engines[0] reports messages and progress.  With dst=None returns the array or raises; with dst a bool."""
    h, n, S = _chain(engines)
    _frame_ok(src, 3, (np.uint8, np.uint16), "src must be a uint8 (or uint16) [rows, cols, 3] BGR array with packed pixels")
    out = np.empty((src.shape[0] * S, src.shape[1] * S, 3), src.dtype) if dst is None else None
    dst = out if dst is None else dst
    if S and not _frame_ok(dst, 3, (src.dtype,), shape=(src.shape[0] * S, src.shape[1] * S)):
        engines[0]._refuse("renderChained", f"Output image has invalid size: expected {src.shape[1] * S}x{src.shape[0] * S}.")
        return False
    ok = lib().w2x_render_chained(h, n, _data(src), src.shape[0], src.shape[1], src.strides[0], _data(dst), dst.strides[0], src.itemsize * 8, int(bool(quantize)))
    return engines[0]._finish(ok, out, "render_chained failed")


def render_chained_resized(engines, src: np.ndarray, size, quantize: bool = False, filter: str = "bicubic", dst: np.ndarray | None = None):
    """render_chained() with the last stage's canvas resized on the device to size = (rows, cols), each in [input dim, input dim * S] and at least a quarter of
    that canvas (w2x_render_chained_resized; chain_plan() holds the rules).  At the full size it is render_chained()."""
    h, n, S = _chain(engines)
    _frame_ok(src, 3, (np.uint8, np.uint16), "src must be a uint8 (or uint16) [rows, cols, 3] BGR array with packed pixels")
    rows, cols = int(size[0]), int(size[1])
    fid = _filter_id(filter)
    out = np.empty((max(rows, 0), max(cols, 0), 3), src.dtype) if dst is None else None
    dst = out if dst is None else dst
    _frame_ok(dst, 3, (src.dtype,), "dst must be a packed [rows, cols, 3] array of the target size and the frame's sample type", shape=(rows, cols), empty_ok=True)
    ok = lib().w2x_render_chained_resized(h, n, _data(src), src.shape[0], src.shape[1], src.strides[0], _data(dst), rows, cols, dst.strides[0], src.itemsize * 8,
                                          int(bool(quantize)), fid)
    return engines[0]._finish(ok, out, "render_chained_resized failed")


def render_sequence_chained(engines, frames, size=None, quantize: bool = False, filter: str = "bicubic", outs=None, pinned: bool = False):
    """Equally sized uint8 frames through the chain with upload, stages and download overlapped (w2x_render_sequence_chained; size = (rows, cols):
    w2x_render_sequence_chained_resized).  Output i is the bytes of the single call on frame i.  outs / pinned as in render_sequence() (page-locked buffers
    come from engines[0])."""
    h, n, S = _chain(engines)
    if len(frames) == 0:
        return []
    fid = _filter_id(filter)
    r, c = frames[0].shape[:2]
    rows, cols = (r * S, c * S) if size is None else (int(size[0]), int(size[1]))
    for f in frames:
        _frame_ok(f, 3, (np.uint8,), "frames must be packed uint8 [rows, cols, 3] arrays of one size", shape=(r, c), rows_packed=True)
    q = int(bool(quantize))

    def run(fs, os_):
        if size is None:
            return lib().w2x_render_sequence_chained(h, n, _pointers(fs), r, c, c * 3, _pointers(os_, len(fs)), cols * 3, len(fs), q)
        return lib().w2x_render_sequence_chained_resized(h, n, _pointers(fs), r, c, c * 3, _pointers(os_, len(fs)), rows, cols, cols * 3, len(fs), q, fid)
    return engines[0]._packed_sequence(frames, 3, (max(rows, 0), max(cols, 0), 3), outs, pinned, "outs must be packed uint8 arrays of the output size", run,
                                       "render_sequence_chained failed")


def render_chained_planar(engines, planes, size=None, *, bits: int | None = None, out_bits: int | None = None, order: str = "rgb", quantize: bool = False,
                          filter: str = "bicubic", dst=None):
    """render_chained() on a planar RGB frame (w2x_render_chained_planes; size = (rows, cols): w2x_render_chained_planes_resized): planes, bits, out_bits, order
    and dst as in render_planar().  quantize=False gives the bytes of b.render_planar(a.render_planar(planes, out_bits=32), out_bits=out_bits); quantize=True
    (integer samples) those of b.render_planar(a.render_planar(planes), out_bits=out_bits)."""
    h, n, S = _chain(engines)
    fid = _filter_id(filter)
    first = engines[0]
    keep = first._scaling
    first._scaling = S                                      # (the planar frame-argument path sizes the output by the caller's scale factor: here the chain's)
    try:
        args, out = first._planar_call(planes, size, bits, out_bits, order, dst, "renderChainedPlanar")
    finally:
        first._scaling = keep
    if args is None:
        return first._finish(0, out, "render_chained_planar failed")
    a = (h, n) + tuple(args[1:]) + (int(bool(quantize)),)
    ok = lib().w2x_render_chained_planes(*a) if size is None else lib().w2x_render_chained_planes_resized(*a, fid)
    return first._finish(ok, out, "render_chained_planar failed")


class debug_switches:
    """Test hook (w2x_debug_set, csrc/switches.h): the reference paths the A/B tests compare the shipped plans and kernels with -
    `with debug_switches(no_fuse_attn=1): eng.build(...)`.  Process-wide; every switch goes back to 0 on exit."""

    def __init__(self, **switches):
        self.switches = switches

    def __enter__(self):
        for k, v in self.switches.items():
            if not lib().w2x_debug_set(k.encode(), int(v)):
                raise W2xError(f"no such switch: {k}")
        return self

    def __exit__(self, *exc):
        for k in self.switches:
            lib().w2x_debug_set(k.encode(), 0)
        return False


def device_pci_bus_id(device: int):
    """PCI bus id of HIP device `device` of this process (W2X_DEVICE_MAP applied), or None: w2x_device_pci_bus_id.  Initialises the HIP runtime."""
    buf = C.create_string_buffer(64)
    return buf.value.decode() if lib().w2x_device_pci_bus_id(int(device), buf, 64) else None


def ipc_open(handle: bytes, device: int) -> int:
    """open another process's 64-byte device-memory handle on logical device `device` -> device pointer (0: failed)"""
    buf = (C.c_uint8 * 64)(*handle)
    return int(lib().w2x_ipc_open(buf, int(device)) or 0)


def ipc_close(ptr: int) -> None:
    if ptr:
        lib().w2x_ipc_close(C.c_void_p(ptr))


def shard_plan(in_w, in_h, out_w, out_h, tile_in, tile_out, scaling, overlap, part, parts):
    """Host logic of the every-tile-once split of one frame -> (first_tile, tile_count, halo_first, [(x, y, w, h), ...])."""
    out = np.zeros(16, np.int32)
    lib().w2x_shard_plan(in_w, in_h, out_w, out_h, tile_in, tile_out, scaling, float(overlap[0]), float(overlap[1]), int(part), int(parts), out.ctypes.data)
    return int(out[0]), int(out[1]), int(out[2]), [tuple(int(v) for v in out[4 + 4 * r:8 + 4 * r]) for r in range(int(out[3]))]


def strip_plan(in_w, in_h, out_w, out_h, tile_in, tile_out, scaling, overlap, part, parts):
    """Host logic of the multi-GPU single-frame split -> (first_tile, tile_count, x0, x1)."""
    out = np.zeros(4, np.int32)
    lib().w2x_strip_plan(in_w, in_h, out_w, out_h, tile_in, tile_out, scaling, float(overlap[0]), float(overlap[1]), int(part), int(parts), out.ctypes.data)
    return tuple(int(v) for v in out)


def calculate_tiles(in_w, in_h, out_w, out_h, tile_in, tile_out, scaling, overlap):
    """calculateTiles (img2img_render.cpp:7-66) through the C ABI -> (count, in_rects[N,4], out_rects[N,4])."""
    L = lib()
    cap = 1 << 16
    a = np.zeros((cap, 4), np.int32)
    b = np.zeros((cap, 4), np.int32)
    n = L.w2x_calculate_tiles(in_w, in_h, out_w, out_h, tile_in, tile_out, scaling, float(overlap[0]), float(overlap[1]),
                              a.ctypes.data, b.ctypes.data, cap)
    if n < 0:
        raise W2xError("tile capacity exceeded")
    return n, a[:n].copy(), b[:n].copy()


def tile_weights(which, ovx, ovy, size):
    L = lib()
    out = np.empty((size, size), np.float32)
    if not L.w2x_tile_weights(which, ovx, ovy, size, out.ctypes.data):
        raise W2xError("bad arguments")
    return out


def _edge_id(mode) -> int:
    if isinstance(mode, str):
        if mode not in EDGE_MODES:
            raise ValueError(f"edge mode must be one of {sorted(EDGE_MODES)}, got {mode!r}")
        return EDGE_MODES[mode]
    return int(mode)


def edge_index(mode, i: int, n: int) -> int:
    """The edge rule (w2x_edge_index): the source index of coordinate i in a dimension of n samples under `mode`, a name of EDGE_MODES or its number; -1 for an
    unknown number or n <= 0."""
    return int(lib().w2x_edge_index(_edge_id(mode), int(i), int(n)))


def resize_weights(in_size: int, out_size: int, filter: str = "bicubic", edge=None):
    """Tap tables of the resized renders along one axis (w2x_resize_weights) -> (first[out] int32, weights[out, taps] float32).  edge (a name of EDGE_MODES or
    its number): the table under that mode (w2x_resize_weights_edge) - under "wrap" and "mirror" every output has its full support, first may be negative and
    first + k may pass in_size; tap k reads the sample edge_index(edge, first + k, in_size)."""
    L = lib()
    fid = _filter_id(filter)
    if edge is None:
        call = lambda *a: L.w2x_resize_weights(int(in_size), int(out_size), fid, *a)
    else:
        mode = _edge_id(edge)
        call = lambda *a: L.w2x_resize_weights_edge(int(in_size), int(out_size), fid, mode, *a)
    taps = call(None, None, 0)
    if taps <= 0:
        raise W2xError(f"invalid resize {in_size} -> {out_size}")
    first = np.zeros(out_size, np.int32)
    w = np.zeros((out_size, taps), np.float32)
    if call(first.ctypes.data, w.ctypes.data, w.size) != taps:
        raise W2xError("w2x_resize_weights failed")
    return first, w


def alpha_bleed_planes(planes, radius: int, *, bits: int | None = None, order: str = "rgba", edge=None):
    """The colour bleed of the planar RGBA renders on the host (w2x_alpha_bleed_rgbap): four 2-D uint8 or uint16 planes (bits=10 / 12 for codes in the low bits),
    radius 0..16 -> the three colour planes R, G, B with every code clamped to 2^bits - 1 and the colours of the visible pixels (clamped alpha > 0) spread
    under the others; integer and exact (tiles.h alpha_bleed_planes)."""
    idx = _planar_order(order, "rgba")
    bits = _planar_bits(planes, bits, n=4)
    if bits == 32:
        raise ValueError("Colour bleed takes integer samples.")
    src = [planes[k] for k in idx]
    out = tuple(np.empty(src[0].shape, src[0].dtype) for _ in range(3))
    args = ((C.c_void_p * 4)(*[_data(p) for p in src]), (C.c_size_t * 4)(*[p.strides[0] for p in src]), src[0].shape[0], src[0].shape[1], bits,
            int(radius), (C.c_void_p * 3)(*[_data(p) for p in out]), (C.c_size_t * 3)(*[p.strides[0] for p in out]))
    if not (lib().w2x_alpha_bleed_rgbap(*args) if edge is None else lib().w2x_alpha_bleed_planes_edge(*args, _edge_id(edge))):   # (edge: the bleed under that mode, c_api_edge.h)
        raise ValueError(f"alpha_bleed_planes refused planes of {src[0].shape} at radius {radius}")
    return out


def light_decode(mode, v: float) -> float:
    """The host statement of a curve's decode (w2x_light_decode): v clamped to [0, 1] -> linear light in the engine's fp32 arithmetic; mode a name of
    RESIZE_LIGHTS or its number ("gamma": the clamped value); NaN for an unknown number."""
    m = RESIZE_LIGHTS.get(mode, -1) if isinstance(mode, str) else int(mode)
    return float(lib().w2x_light_decode(m, float(v)))


def light_encode(mode, v: float) -> float:
    """The host statement of a curve's encode (w2x_light_encode), likewise."""
    m = RESIZE_LIGHTS.get(mode, -1) if isinstance(mode, str) else int(mode)
    return float(lib().w2x_light_encode(m, float(v)))


def dither_table(mode) -> np.ndarray:
    """The rank table of a dither mode (w2x_dither_table): "ordered" the 8 x 8 Bayer matrix, "bluenoise" the 64 x 64 void-and-cluster table; uint16 [side, side],
    every rank 0 .. side^2 - 1 once.  The threshold of a sample is (rank + 0.5) / side^2."""
    m = DITHER_MODES.get(mode, mode) if isinstance(mode, str) else int(mode)
    side = C.c_int(0)
    if not isinstance(m, int) or not lib().w2x_dither_table(m, None, C.byref(side)):
        raise ValueError(f"dither_table: no table for mode {mode!r}")
    out = np.empty((side.value, side.value), np.uint16)
    lib().w2x_dither_table(m, _data(out), C.byref(side))
    return out


def dither_rank(mode, phase: int, c: int, x: int, y: int) -> int:
    """The rank of sample (x, y) of plane index c at `phase` (w2x_dither_rank); -1 for mode none, an unknown mode, c outside 0 .. 2 or a negative position."""
    m = DITHER_MODES.get(mode, -1) if isinstance(mode, str) else int(mode)
    return int(lib().w2x_dither_rank(m, int(phase) & 0xFFFFFFFF, int(c), int(x), int(y)))


def alpha_bleed(bgr: np.ndarray, alpha: np.ndarray, radius: int, edge=None) -> np.ndarray:
    """The colour bleed of the RGBA renders on the host (w2x_alpha_bleed): bgr uint8 [rows, cols, 3], alpha uint8 [rows, cols], radius 0..16 -> the frame with
    the colours of the pixels of alpha > 0 spread `radius` pixels outward under the pixels of alpha == 0; raises for invalid arguments"""
    _frame_ok(bgr, 3, (np.uint8,), "bgr must be a uint8 [rows, cols, 3] array with packed pixels", empty_ok=True)
    if alpha.dtype != np.uint8 or alpha.shape != bgr.shape[:2] or (alpha.size and alpha.strides[1] != 1):
        raise ValueError("alpha must be a uint8 [rows, cols] array of the frame's size with packed rows")
    out = np.empty(bgr.shape, np.uint8)
    args = (_data(bgr), bgr.strides[0], _data(alpha), alpha.strides[0], bgr.shape[0], bgr.shape[1], int(radius), _data(out), out.strides[0])
    if not (lib().w2x_alpha_bleed(*args) if edge is None else lib().w2x_alpha_bleed_edge(*args, _edge_id(edge))):   # (edge: the bleed under that mode - "wrap" takes the neighbours round the frame)
        raise W2xError(f"invalid alpha bleed: a {bgr.shape[1]}x{bgr.shape[0]} frame at radius {radius}")
    return out


def yuv_layout_plane_sizes(rows: int, cols: int, bits: int, layout: str = "i420"):
    """(plane_rows, plane_cols in samples, plane_bytes), one entry per plane of a packed frame of `layout` - two for "nv12" - (w2x_yuv_layout_plane_sizes);
    raises for invalid arguments"""
    n, pr, pc, pb = C.c_int(0), (C.c_int * 3)(), (C.c_int * 3)(), (C.c_size_t * 3)()
    if not lib().w2x_yuv_layout_plane_sizes(int(rows), int(cols), int(bits), _layout_id(layout), C.byref(n), pr, pc, pb):
        raise W2xError(f"invalid YUV frame {rows}x{cols} at {bits} bits")
    return list(pr)[:n.value], list(pc)[:n.value], list(pb)[:n.value]


def yuv_plane_sizes(rows: int, cols: int, bits: int):
    """(plane_rows[3], plane_cols[3], plane_bytes[3]) of a packed YUV 4:2:0 frame (w2x_yuv_plane_sizes); raises for invalid arguments"""
    pr, pc, pb = (C.c_int * 3)(), (C.c_int * 3)(), (C.c_size_t * 3)()
    if not lib().w2x_yuv_plane_sizes(int(rows), int(cols), int(bits), pr, pc, pb):
        raise W2xError(f"invalid YUV frame {rows}x{cols} at {bits} bits")
    return list(pr), list(pc), list(pb)


def describe_plan(onnx_path, batch, tile, precision=None) -> str:
    L = lib()
    buf = C.create_string_buffer(1 << 20)
    ok = L.w2x_describe_plan_precision(os.fsencode(onnx_path), batch, tile, int(Precision.FP16 if precision is None else precision), buf, len(buf))
    s = buf.value.decode(errors="replace")
    if not ok:
        raise W2xError(s)
    return s


EXTENT_FIELDS = ("kind", "W", "H", "cx", "wx", "cy", "wy", "rx", "ry", "ws", "t_in", "t_out", "t_res", "kh", "kw", "stride", "x0", "y0", "r",
                 "in_W", "in_H", "out_W", "out_H", "live_units", "total_units")


def dead_skip_extents(onnx_path, batch, tile, in_w, in_h, scaling, overlap, tile_index, tta=False) -> list[dict]:
    """w2x_dead_skip_extents: per plan op the live part of its row map for tile `tile_index` of an in_w x in_h frame (tile_index < 0: w2x_infer, "all").  Host only."""
    L = lib()
    n = -L.w2x_dead_skip_extents(os.fsencode(onnx_path), batch, tile, in_w, in_h, scaling, float(overlap[0]), float(overlap[1]), int(tile_index), int(bool(tta)), None, 0)
    if n <= 0:
        raise W2xError("w2x_dead_skip_extents failed")
    out = np.zeros((n, len(EXTENT_FIELDS)), np.int32)
    if L.w2x_dead_skip_extents(os.fsencode(onnx_path), batch, tile, in_w, in_h, scaling, float(overlap[0]), float(overlap[1]), int(tile_index), int(bool(tta)), out.ctypes.data, out.size) != n:
        raise W2xError("w2x_dead_skip_extents failed")
    return [dict(zip(EXTENT_FIELDS, (int(v) for v in row))) for row in out]


def write_engine_file(onnx_path, batch, tile, out_path) -> bool:
    """Host-only half of build(): lower the graph and write the plan file (no device needed)."""
    return bool(lib().w2x_write_engine_file(os.fsencode(onnx_path), batch, tile, os.fsencode(out_path)))


def validate_engine_file(path) -> tuple[bool, str]:
    """Host-only half of load(): deserialize + consistency checks -> (ok, reason)."""
    buf = C.create_string_buffer(4096)
    ok = lib().w2x_validate_engine_file(os.fsencode(path), buf, len(buf))
    return bool(ok), buf.value.decode(errors="replace")


def sha256_hex(data: bytes) -> str:
    L = lib()
    out = C.create_string_buffer(65)
    L.w2x_sha256_hex(data, len(data), out)
    return out.value.decode()
