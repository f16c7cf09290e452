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


def yuv_plane_shapes(rows: int, cols: int):
    """[(rows, cols)] of the Y, U and V planes of a 4:2:0 frame"""
    return [(rows, cols), ((rows + 1) // 2, (cols + 1) // 2), ((rows + 1) // 2, (cols + 1) // 2)]


def _yuv_bits(planes) -> int:
    """8 for uint8 planes, 10 for uint16 ones; checks the 4:2:0 shapes and packed samples"""
    y = planes[0]
    if y.ndim != 2 or y.dtype not in (np.uint8, np.uint16):
        raise ValueError("YUV planes must be 2-D uint8 (8-bit) or uint16 (10-bit) arrays")
    for p, shape in zip(planes, yuv_plane_shapes(*y.shape)):
        if p.dtype != y.dtype or p.shape != shape or p.strides[1] != p.itemsize or p.strides[0] <= 0:
            raise ValueError(f"YUV 4:2:0 planes of one sample type with packed rows expected: {[q.shape for q in planes]} for {y.shape}")
    return 8 if y.dtype == np.uint8 else 10


YUV_LAYOUTS = {"i420": 0, "i422": 1, "i444": 2, "nv12": 3}   # W2X_YUV_I420 .. _NV12 (include/w2x/c_api.h)


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


def _yuv_layout_bits(planes, layout) -> int:
    """_yuv_bits for a frame of `layout`"""
    y = planes[0]
    if y.ndim != 2 or y.dtype not in (np.uint8, np.uint16):
        raise ValueError("YUV planes must be 2-D uint8 (8-bit) or uint16 (10-bit) arrays")
    shapes = yuv_layout_plane_shapes(*y.shape, layout)
    if len(planes) != len(shapes) or any(p.dtype != y.dtype or p.shape != shape or p.strides[1] != p.itemsize or p.strides[0] <= 0 for p, shape in zip(planes, shapes)):
        raise ValueError(f"{layout} planes of one sample type with packed rows expected: {[q.shape for q in planes]} for {y.shape}")
    return 8 if y.dtype == np.uint8 else 10


def _plane_args(planes):
    """three pointers and three steps of a frame for the C ABI (an NV12 frame leaves the third NULL / 0)"""
    pad = [None] * (3 - len(planes))
    return [p.ctypes.data for p in planes] + pad, [p.strides[0] for p in planes] + [0] * len(pad)


def _filter_id(name) -> int:
    if name not in RESIZE_FILTERS:
        raise ValueError(f"filter must be one of {sorted(RESIZE_FILTERS)}, got {name!r}")
    return RESIZE_FILTERS[name]


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
    vp = C.c_void_p
    L.w2x_create.restype = vp
    L.w2x_destroy.argtypes = [vp]
    L.w2x_set_message_callback.argtypes = [vp, _MSG_FN, vp]
    L.w2x_set_progress_callback.argtypes = [vp, _PROG_FN, vp]
    L.w2x_build.argtypes = [vp, C.c_char_p, C.POINTER(_BuildConfig)]; L.w2x_build.restype = C.c_int
    L.w2x_load.argtypes = [vp, C.c_char_p, C.POINTER(_RenderConfig)]; L.w2x_load.restype = C.c_int
    L.w2x_render.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t]; L.w2x_render.restype = C.c_int
    L.w2x_render16.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t]; L.w2x_render16.restype = C.c_int
    L.w2x_render_resized.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_int, C.c_int, C.c_size_t, C.c_int]; L.w2x_render_resized.restype = C.c_int
    L.w2x_render16_resized.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_int, C.c_int, C.c_size_t, C.c_int]; L.w2x_render16_resized.restype = C.c_int
    L.w2x_render_sequence_resized.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int]; L.w2x_render_sequence_resized.restype = C.c_int
    L.w2x_resize_weights.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, C.c_int]; L.w2x_resize_weights.restype = C.c_int
    L.w2x_render_yuv.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]; L.w2x_render_yuv.restype = C.c_int
    L.w2x_render_sequence_yuv.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.w2x_render_sequence_yuv.restype = C.c_int
    L.w2x_render_yuv_resized.argtypes = L.w2x_render_yuv.argtypes + [C.c_int]; L.w2x_render_yuv_resized.restype = C.c_int
    L.w2x_render_sequence_yuv_resized.argtypes = L.w2x_render_sequence_yuv.argtypes + [C.c_int]; L.w2x_render_sequence_yuv_resized.restype = C.c_int
    L.w2x_render_rgba.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int]; L.w2x_render_rgba.restype = C.c_int
    L.w2x_render_rgba_resized.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int]; L.w2x_render_rgba_resized.restype = C.c_int
    L.w2x_render_sequence_rgba.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, C.c_int]; L.w2x_render_sequence_rgba.restype = C.c_int
    L.w2x_render_sequence_rgba_resized.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int]
    L.w2x_render_sequence_rgba_resized.restype = C.c_int
    L.w2x_alpha_bleed_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t, C.c_int]; L.w2x_alpha_bleed_device.restype = C.c_int
    L.w2x_alpha_bleed.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, C.c_size_t]; L.w2x_alpha_bleed.restype = C.c_int
    L.w2x_yuv_plane_sizes.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp]; L.w2x_yuv_plane_sizes.restype = C.c_int
    L.w2x_render_yuv_layout.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]; L.w2x_render_yuv_layout.restype = C.c_int
    L.w2x_render_sequence_yuv_layout.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.w2x_render_sequence_yuv_layout.restype = C.c_int
    L.w2x_yuv_layout_plane_sizes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]; L.w2x_yuv_layout_plane_sizes.restype = C.c_int
    L.w2x_render_strip.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int]; L.w2x_render_strip.restype = C.c_int
    L.w2x_render_sequence.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t, C.c_int]; L.w2x_render_sequence.restype = C.c_int
    L.w2x_alloc_host.argtypes = [vp, C.c_size_t]; L.w2x_alloc_host.restype = vp
    L.w2x_free_host.argtypes = [vp, vp]; L.w2x_free_host.restype = None
    L.w2x_pin_host.argtypes = [vp, vp, C.c_size_t]; L.w2x_pin_host.restype = C.c_int
    L.w2x_unpin_host.argtypes = [vp, vp]; L.w2x_unpin_host.restype = None
    L.w2x_strip_plan.argtypes = [C.c_int] * 7 + [C.c_double, C.c_double, C.c_int, C.c_int, vp]; L.w2x_strip_plan.restype = C.c_int
    L.w2x_render_sharded.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t]; L.w2x_render_sharded.restype = C.c_int
    L.w2x_shard_compute.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int]; L.w2x_shard_compute.restype = C.c_int
    L.w2x_shard_slab.argtypes = [vp, vp]; L.w2x_shard_slab.restype = vp
    L.w2x_shard_finish.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, vp, vp]; L.w2x_shard_finish.restype = C.c_int
    L.w2x_ipc_export.argtypes = [vp, vp]; L.w2x_ipc_export.restype = C.c_int
    L.w2x_ipc_open.argtypes = [vp, C.c_int]; L.w2x_ipc_open.restype = vp
    L.w2x_ipc_close.argtypes = [vp]; L.w2x_ipc_close.restype = None
    L.w2x_shard_plan.argtypes = [C.c_int] * 7 + [C.c_double, C.c_double, C.c_int, C.c_int, vp]; L.w2x_shard_plan.restype = C.c_int
    L.w2x_infer.argtypes = [vp, vp, vp]; L.w2x_infer.restype = C.c_int
    L.w2x_output_tile_size.argtypes = [vp]; L.w2x_output_tile_size.restype = C.c_int
    L.w2x_pass_tiles.argtypes = [vp]; L.w2x_pass_tiles.restype = C.c_int
    L.w2x_plan_flops.argtypes = [vp]; L.w2x_plan_flops.restype = C.c_double
    L.w2x_last_render_ms.argtypes = [vp]; L.w2x_last_render_ms.restype = C.c_float
    L.w2x_bench_resident.argtypes = [vp, C.c_int]; L.w2x_bench_resident.restype = C.c_float
    L.w2x_resident_output.argtypes = [vp, vp, C.c_size_t]; L.w2x_resident_output.restype = C.c_int
    L.w2x_profile_frame.argtypes = [vp, vp, C.c_int]; L.w2x_profile_frame.restype = C.c_int
    L.w2x_op_times.argtypes = [vp, vp, C.c_int]; L.w2x_op_times.restype = C.c_int
    L.w2x_calculate_tiles.argtypes = [C.c_int] * 7 + [C.c_double, C.c_double, vp, vp, C.c_int]; L.w2x_calculate_tiles.restype = C.c_int
    L.w2x_tile_weights.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp]; L.w2x_tile_weights.restype = C.c_int
    L.w2x_describe_plan.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]; L.w2x_describe_plan.restype = C.c_int
    L.w2x_describe_plan_precision.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]; L.w2x_describe_plan_precision.restype = C.c_int
    L.w2x_write_engine_file.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p]; L.w2x_write_engine_file.restype = C.c_int
    L.w2x_validate_engine_file.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]; L.w2x_validate_engine_file.restype = C.c_int
    L.w2x_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, C.c_size_t]; L.w2x_device_pci_bus_id.restype = C.c_int
    L.w2x_sha256_hex.argtypes = [vp, C.c_size_t, C.c_char_p]
    L.w2x_version.restype = C.c_char_p
    L.w2x_debug_set.argtypes = [C.c_char_p, C.c_int]; L.w2x_debug_set.restype = C.c_int
    L.w2x_dead_skip_extents.argtypes = [C.c_char_p] + [C.c_int] * 5 + [C.c_double, C.c_double, C.c_int, C.c_int, vp, C.c_int]; L.w2x_dead_skip_extents.restype = C.c_int
    _lib = L
    return L


EXPORTED_SYMBOLS = [
    "w2x_create", "w2x_destroy", "w2x_set_message_callback", "w2x_set_progress_callback", "w2x_build", "w2x_load",
    "w2x_render", "w2x_render16", "w2x_infer", "w2x_output_tile_size", "w2x_plan_flops", "w2x_pass_tiles", "w2x_last_render_ms", "w2x_bench_resident", "w2x_resident_output", "w2x_profile_frame", "w2x_op_times",
    "w2x_render_resized", "w2x_render16_resized", "w2x_render_sequence_resized", "w2x_resize_weights",
    "w2x_render_yuv", "w2x_render_sequence_yuv", "w2x_yuv_plane_sizes", "w2x_render_yuv_resized", "w2x_render_sequence_yuv_resized",
    "w2x_render_yuv_layout", "w2x_render_sequence_yuv_layout", "w2x_yuv_layout_plane_sizes",
    "w2x_render_rgba", "w2x_render_rgba_resized", "w2x_render_sequence_rgba", "w2x_render_sequence_rgba_resized", "w2x_alpha_bleed_device", "w2x_alpha_bleed", "w2x_dead_skip_extents",
    "w2x_render_strip", "w2x_strip_plan", "w2x_render_sharded", "w2x_shard_plan", "w2x_shard_compute", "w2x_shard_slab", "w2x_shard_finish", "w2x_ipc_export", "w2x_ipc_open", "w2x_ipc_close", "w2x_render_sequence", "w2x_alloc_host", "w2x_free_host", "w2x_pin_host", "w2x_unpin_host", "w2x_calculate_tiles", "w2x_tile_weights", "w2x_describe_plan", "w2x_describe_plan_precision", "w2x_write_engine_file", "w2x_validate_engine_file", "w2x_device_pci_bus_id", "w2x_sha256_hex", "w2x_version", "w2x_debug_set"]


class Img2Img:
    """trt::Img2Img mirror.  cv::Mat <-> numpy uint8 [rows, cols, 3] BGR."""

    def __init__(self):
        self._L = lib()
        self._h = self._L.w2x_create()
        if not self._h:
            raise W2xError("w2x_create failed")
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
        bps = src.dtype.itemsize                  # uint8 frames, or uint16 ones (extension: w2x_render16)
        if src.dtype not in (np.uint8, np.uint16) or src.ndim != 3 or src.shape[2] != 3 or src.strides[2] != bps or src.strides[1] != 3 * bps:
            raise ValueError("src must be a uint8 (or uint16) [rows, cols, 3] BGR array with packed pixels")
        ret_array = dst is None
        if dst is None:
            s = getattr(self, "_scaling", 0)
            dst = np.empty((src.shape[0] * s, src.shape[1] * s, 3), src.dtype)
        s = getattr(self, "_scaling", 0)
        if s and (dst.dtype != src.dtype or dst.shape != (src.shape[0] * s, src.shape[1] * s, 3) or dst.strides[2] != bps or dst.strides[1] != 3 * bps):
            # the C ABI only sees pointers and steps, so the cv::Mat-style size check lives here
            self._on_msg(int(Severity.error), f"[render@0] Output image has invalid size: expected {src.shape[1] * s}x{src.shape[0] * s}.".encode(), None)
            return False
        fn = self._L.w2x_render if bps == 1 else self._L.w2x_render16
        ok = bool(fn(self._h, src.ctypes.data, src.shape[0], src.shape[1], src.strides[0], dst.ctypes.data, dst.strides[0]))
        if ret_array:
            if not ok:
                raise W2xError(self.last_error() or "render failed")
            return dst
        return ok

    def render_rgba(self, bgra: np.ndarray, *, bleed: int = 0, skip_uniform_alpha: bool = False, dst: np.ndarray | None = None):
        """render() on a uint8 [rows, cols, 4] BGRA frame in one call (w2x_render_rgba): the colours of the pixels with alpha > 0 are spread `bleed` pixels
        (0..16) under the transparent ones, colour and alpha tiles share one schedule; skip_uniform_alpha: a frame whose alpha plane is one value keeps it
        and runs no alpha tiles.  Rows may be padded (strides[0] >= cols * 4).  With dst=None returns the [rows * s, cols * s, 4] array or raises; with dst
        returns a bool."""
        ret_array = dst is None
        s = getattr(self, "_scaling", 0)
        ok = isinstance(bgra, np.ndarray) and bgra.ndim == 3 and bgra.shape[2] == 4
        if ok and bgra.dtype != np.uint8:
            # the C ABI carries no sample depth: deeper frames are refused here, with the engine's message
            self._on_msg(int(Severity.error), b"[renderRgba@0] RGBA input and output images must be 8-bit.", None)
            if ret_array:
                raise W2xError(self.last_error())
            return False
        if not ok or bgra.strides[2] != 1 or bgra.strides[1] != 4:
            raise ValueError("bgra must be a uint8 [rows, cols, 4] BGRA array with packed pixels")
        if dst is None:
            dst = np.empty((bgra.shape[0] * s, bgra.shape[1] * s, 4), np.uint8)
        if s and (dst.dtype != np.uint8 or dst.shape != (bgra.shape[0] * s, bgra.shape[1] * s, 4) or dst.strides[2] != 1 or dst.strides[1] != 4):
            # the C ABI only sees pointers and steps, so the cv::Mat-style size check lives here
            self._on_msg(int(Severity.error), f"[renderRgba@0] Output image has invalid size: expected {bgra.shape[1] * s}x{bgra.shape[0] * s}.".encode(), None)
            return False
        ok = bool(self._L.w2x_render_rgba(self._h, bgra.ctypes.data if bgra.size else None, bgra.shape[0], bgra.shape[1], bgra.strides[0],
                                          dst.ctypes.data if dst.size else None, dst.strides[0], int(bleed), 1 if skip_uniform_alpha else 0))
        if ret_array:
            if not ok:
                raise W2xError(self.last_error() or "render_rgba failed")
            return dst
        return ok

    def render_rgba_resized(self, bgra: np.ndarray, size, *, bleed: int = 0, skip_uniform_alpha: bool = False, filter: str = "bicubic", dst: np.ndarray | None = None):
        """render_rgba() with the output resized on the device to size = (rows, cols), each in [input dim, input dim * scaling] (w2x_render_rgba_resized):
        colour and alpha are resized separately and straight, with the filters of render_resized().  With dst=None returns the [rows, cols, 4] array or
        raises; with dst returns a bool."""
        ret_array = dst is None
        ok = isinstance(bgra, np.ndarray) and bgra.ndim == 3 and bgra.shape[2] == 4
        if ok and bgra.dtype != np.uint8:
            # the C ABI carries no sample depth: deeper frames are refused here, with the engine's message
            self._on_msg(int(Severity.error), b"[renderRgbaResized@0] RGBA input and output images must be 8-bit.", None)
            if ret_array:
                raise W2xError(self.last_error())
            return False
        if not ok or bgra.strides[2] != 1 or bgra.strides[1] != 4:
            raise ValueError("bgra must be a uint8 [rows, cols, 4] BGRA array with packed pixels")
        rows, cols = int(size[0]), int(size[1])
        fid = _filter_id(filter)
        if dst is None:
            dst = np.empty((max(rows, 0), max(cols, 0), 4), np.uint8)
        if dst.dtype != np.uint8 or dst.shape != (rows, cols, 4) or (dst.size and (dst.strides[2] != 1 or dst.strides[1] != 4)):
            raise ValueError("dst must be a uint8 [rows, cols, 4] array of the target size with packed pixels")   # (an empty target: refused by the library)
        ok = bool(self._L.w2x_render_rgba_resized(self._h, bgra.ctypes.data if bgra.size else None, bgra.shape[0], bgra.shape[1], bgra.strides[0],
                                                  dst.ctypes.data if dst.size else None, rows, cols, dst.strides[0], int(bleed), 1 if skip_uniform_alpha else 0, fid))
        if ret_array:
            if not ok:
                raise W2xError(self.last_error() or "render_rgba_resized failed")
            return dst
        return ok

    def render_sequence_rgba(self, frames, *, size=None, bleed: int = 0, skip_uniform_alpha: bool = False, filter: str = "bicubic", outs=None, pinned: bool = False):
        """Equally sized uint8 [rows, cols, 4] BGRA frames with upload / compute / download overlapped (w2x_render_sequence_rgba); with size = (rows, cols) every
        frame is resized like render_rgba_resized() (w2x_render_sequence_rgba_resized).  Output i is the bytes of the single-frame call on frame i.
        outs / pinned as in render_sequence()."""
        s = getattr(self, "_scaling", 0)
        n = len(frames)
        if n == 0:
            return []
        r, c = frames[0].shape[:2]
        for f in frames:
            if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 4 or f.strides != (f.shape[1] * 4, 4, 1):
                raise ValueError("frames must be packed uint8 [rows, cols, 4] arrays")
            if f.shape != (r, c, 4):
                # the C ABI carries one size for the sequence: frames that differ are refused here, with the engine's message
                self._on_msg(int(Severity.error), b"[renderSequenceRgba@0] Input images must be of one size.", None)
                raise W2xError(self.last_error())
        rows, cols = (r * s, c * s) if size is None else (int(size[0]), int(size[1]))
        fid = _filter_id(filter)
        own = []
        if outs is None:
            if pinned:
                own = [self.alloc_host((rows, cols, 4)) for _ in range(min(n, 3))]
            else:
                outs = [np.empty((rows, cols, 4), np.uint8) for _ in range(n)]
        for o in (own or outs):
            if o.dtype != np.uint8 or o.shape != (rows, cols, 4) or o.strides != (cols * 4, 4, 1):
                raise ValueError("outs must be packed uint8 [rows, cols, 4] arrays of the output size")
        flags = (int(bleed), 1 if skip_uniform_alpha else 0)

        def run(fs, os_):
            m = len(fs)
            sp = (C.c_void_p * m)(*[f.ctypes.data for f in fs]); dp = (C.c_void_p * m)(*[o.ctypes.data for o in os_])
            if size is None:
                ok = self._L.w2x_render_sequence_rgba(self._h, sp, r, c, c * 4, dp, cols * 4, m, *flags)
            else:
                ok = self._L.w2x_render_sequence_rgba_resized(self._h, sp, r, c, c * 4, dp, rows, cols, cols * 4, m, *flags, fid)
            if not ok:
                raise W2xError(self.last_error() or "render_sequence_rgba failed")
        if own:          # a ring of engine-owned buffers: the sequence in pieces, each result copied out
            res = []
            try:
                for k0 in range(0, n, len(own)):
                    m = min(len(own), n - k0)
                    run(frames[k0:k0 + m], own[:m])
                    res += [o.copy() for o in own[:m]]
            finally:
                for o in own:
                    self.free_host(o)
            return res
        run(frames, outs)
        return outs

    def alpha_bleed_device(self, bgra: np.ndarray, radius: int) -> np.ndarray:
        """Test hook (w2x_alpha_bleed_device): the device bleed alone on a uint8 [rows, cols, 4] BGRA frame -> the [rows, cols, 3] BGR frame the tiles are read from"""
        if bgra.dtype != np.uint8 or bgra.ndim != 3 or bgra.shape[2] != 4 or bgra.strides[2] != 1 or bgra.strides[1] != 4:
            raise ValueError("bgra must be a uint8 [rows, cols, 4] BGRA array with packed pixels")
        out = np.empty((bgra.shape[0], bgra.shape[1], 3), np.uint8)
        if not self._L.w2x_alpha_bleed_device(self._h, bgra.ctypes.data if bgra.size else None, bgra.shape[0], bgra.shape[1], bgra.strides[0],
                                              out.ctypes.data if out.size else None, out.strides[0], int(radius)):
            raise W2xError(self.last_error() or "alpha_bleed_device failed")
        return out

    def render_resized(self, src: np.ndarray, size, filter: str = "bicubic", dst: np.ndarray | None = None):
        """render() followed by an antialiased resize on the device to size = (rows, cols), each in [input dim, input dim * scaling]
        (w2x_render_resized / w2x_render16_resized; uint8 or uint16 frames).  With dst=None returns the array or raises; with dst returns a bool."""
        bps = src.dtype.itemsize
        if src.dtype not in (np.uint8, np.uint16) or src.ndim != 3 or src.shape[2] != 3 or src.strides[2] != bps or src.strides[1] != 3 * bps:
            raise ValueError("src must be a uint8 (or uint16) [rows, cols, 3] BGR array with packed pixels")
        rows, cols = int(size[0]), int(size[1])
        fid = _filter_id(filter)
        ret_array = dst is None
        if dst is None:
            dst = np.empty((max(rows, 0), max(cols, 0), 3), src.dtype)
        if dst.dtype != src.dtype or dst.shape != (rows, cols, 3) or (dst.size and (dst.strides[2] != bps or dst.strides[1] != 3 * bps)):
            raise ValueError("dst must be a packed [rows, cols, 3] array of the target size and the frame's sample type")   # (an empty target: refused by the library)
        fn = self._L.w2x_render_resized if bps == 1 else self._L.w2x_render16_resized
        ok = bool(fn(self._h, src.ctypes.data, src.shape[0], src.shape[1], src.strides[0], dst.ctypes.data if dst.size else None, rows, cols,
                     dst.strides[0], fid))
        if ret_array:
            if not ok:
                raise W2xError(self.last_error() or "render_resized failed")
            return dst
        return ok

    def render_sequence_resized(self, frames, size, outs=None, pinned: bool = False, filter: str = "bicubic"):
        """render_sequence() with every frame resized to size = (rows, cols) like render_resized() (w2x_render_sequence_resized; uint8 frames).
        outs / pinned as in render_sequence()."""
        n = len(frames)
        if n == 0:
            return []
        rows, cols = int(size[0]), int(size[1])
        fid = _filter_id(filter)
        r, c = frames[0].shape[:2]
        for f in frames:
            if f.dtype != np.uint8 or f.shape != (r, c, 3) or f.strides != (c * 3, 3, 1):
                raise ValueError("frames must be packed uint8 [rows, cols, 3] arrays of one size")
        own = []
        if outs is None:
            if pinned:
                own = [self.alloc_host((rows, cols, 3)) for _ in range(min(n, 3))]
            else:
                outs = [np.empty((rows, cols, 3), np.uint8) for _ in range(n)]
        for o in (own or outs):
            if o.dtype != np.uint8 or o.shape != (rows, cols, 3) or o.strides != (cols * 3, 3, 1):
                raise ValueError("outs must be packed uint8 arrays of the target size")

        def run(fs, os_):
            m = len(fs)
            if not self._L.w2x_render_sequence_resized(self._h, (C.c_void_p * m)(*[f.ctypes.data for f in fs]), r, c, c * 3,
                                                       (C.c_void_p * m)(*[o.ctypes.data for o in os_]), rows, cols, cols * 3, m, fid):
                raise W2xError(self.last_error() or "render_sequence_resized failed")
        if own:          # a ring of engine-owned buffers: the sequence in pieces, each result copied out
            res = []
            try:
                for k0 in range(0, n, len(own)):
                    m = min(len(own), n - k0)
                    run(frames[k0:k0 + m], own[:m])
                    res += [o.copy() for o in own[:m]]
            finally:
                for o in own:
                    self.free_host(o)
            return res
        run(frames, outs)
        return outs

    def render_strip(self, src: np.ndarray, dst: np.ndarray, part: int, parts: int) -> bool:
        """One device's share of a frame split into tile-column strips (w2x_render_strip): writes only its columns of dst."""
        s = getattr(self, "_scaling", 0)
        if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3 or src.strides[2] != 1 or src.strides[1] != 3:
            raise ValueError("src must be a uint8 [rows, cols, 3] BGR array with packed pixels")
        if dst.dtype != np.uint8 or dst.shape != (src.shape[0] * s, src.shape[1] * s, 3) or dst.strides[2] != 1 or dst.strides[1] != 3:
            raise ValueError("dst must be a packed uint8 array of the scaled size")
        return bool(self._L.w2x_render_strip(self._h, src.ctypes.data, src.shape[0], src.shape[1], src.strides[0],
                                             dst.ctypes.data, dst.strides[0], int(part), int(parts)))

    # ---- one frame over several PROCESSES (one engine each): w2x_shard_compute / w2x_shard_slab / w2x_shard_finish + the IPC helpers below
    def shard_compute(self, src: np.ndarray, part: int, parts: int) -> bool:
        if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3 or src.strides[2] != 1 or src.strides[1] != 3:
            raise ValueError("src must be a uint8 [rows, cols, 3] BGR array with packed pixels")
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
        if dst.dtype != np.uint8 or dst.ndim != 3 or dst.shape[2] != 3 or dst.strides[2] != 1 or dst.strides[1] != 3:
            raise ValueError("dst must be a packed uint8 [rows, cols, 3] array of the scaled size")
        arr = (C.c_void_p * parts)(*[C.c_void_p(int(p) or None) for p in slabs])
        dev = (C.c_int * parts)(*[int(d) for d in devices]) if devices is not None else None
        return bool(self._L.w2x_shard_finish(self._h, dst.ctypes.data, dst.shape[0], dst.shape[1], dst.strides[0], int(part), int(parts), arr, dev))

    def _yuv_out(self, rows, cols, bits):
        s = getattr(self, "_scaling", 0)
        dt = np.uint8 if bits == 8 else np.uint16
        return tuple(np.empty(shape, dt) for shape in yuv_plane_shapes(rows * s, cols * s))

    def render_yuv(self, y, u: np.ndarray | None = None, v: np.ndarray | None = None, *, matrix: str = "bt709", full_range: bool = False, out_bits: int | None = None,
                   out=None, layout: str | None = None, out_layout: str | None = None):
        """render() on a YUV 4:2:0 frame (w2x_render_yuv): uint8 planes are 8-bit, uint16 planes 10-bit; out_bits (8 or 10, default the input's)
        sets the output depth.  Returns (Y, U, V) at the scaled size, or raises.  out: pre-allocated planes (then a bool is returned).
        With the frame given as one tuple of planes, or with layout= / out_layout= ("i420", "i422", "i444", "nv12"; out_layout defaults to the input's), the
        call goes through w2x_render_yuv_layout: an "nv12" frame is (y, uv) with uv of ceil(rows/2) x 2 * ceil(cols/2) samples (10-bit: P010, codes << 6),
        and the result is the tuple of out_layout's planes (yuv_layout_plane_shapes)."""
        if isinstance(y, (tuple, list)) or layout is not None or out_layout is not None:
            if isinstance(y, (tuple, list)) and (u is not None or v is not None):
                raise ValueError("give the frame as one tuple of planes or as three positional planes, not both")
            planes = tuple(y) if isinstance(y, (tuple, list)) else tuple(p for p in (y, u, v) if p is not None)
            return self._render_yuv_layout(planes, layout or "i420", out_layout, matrix, full_range, out_bits, out)
        bits = _yuv_bits((y, u, v))
        ob = bits if out_bits is None else int(out_bits)
        ret_array = out is None
        dst = self._yuv_out(*y.shape, ob if ob in (8, 10) else 8) if out is None else tuple(out)
        if out is not None:
            # the C ABI sees pointers and steps only: the plane shapes and the sample type of out_bits are checked here
            s = getattr(self, "_scaling", 0)
            dt = np.uint16 if ob == 10 else np.uint8
            if len(dst) != 3 or any(not isinstance(p, np.ndarray) or p.dtype != dt or p.ndim != 2 or p.shape != shape or p.strides[1] != p.itemsize
                                    for p, shape in zip(dst, yuv_plane_shapes(y.shape[0] * s, y.shape[1] * s))):
                raise ValueError("out must be three 2-D planes of the scaled 4:2:0 shapes, uint8 for 8-bit and uint16 for 10-bit output, with packed rows")
        dp = (C.c_void_p * 3)(*[p.ctypes.data for p in dst])
        ok = bool(self._L.w2x_render_yuv(self._h, (C.c_void_p * 3)(*[p.ctypes.data for p in (y, u, v)]), (C.c_size_t * 3)(*[p.strides[0] for p in (y, u, v)]),
                                         y.shape[0], y.shape[1], bits, dp, (C.c_size_t * 3)(*[p.strides[0] for p in dst]), dst[0].shape[0], dst[0].shape[1], ob,
                                         _matrix_id(matrix), 1 if full_range else 0))
        if ret_array:
            if not ok:
                raise W2xError(self.last_error() or "render_yuv failed")
            return dst
        return ok

    def _render_yuv_layout(self, planes, layout, out_layout, matrix, full_range, out_bits, out):
        """render_yuv() through w2x_render_yuv_layout"""
        out_layout = layout if out_layout is None else out_layout
        lid, olid = _layout_id(layout), _layout_id(out_layout)
        bits = _yuv_layout_bits(planes, layout)
        ob = bits if out_bits is None else int(out_bits)
        rows, cols = planes[0].shape
        s = getattr(self, "_scaling", 0)
        dt = np.uint16 if ob == 10 else np.uint8
        shapes = yuv_layout_plane_shapes(rows * s, cols * s, out_layout)
        ret_array = out is None
        dst = tuple(np.empty(shape, dt) for shape in shapes) if out is None else tuple(out)
        if len(dst) != len(shapes) or any(not isinstance(p, np.ndarray) or p.dtype != dt or p.shape != shape or p.strides[1] != p.itemsize for p, shape in zip(dst, shapes)):
            raise ValueError(f"out must be the 2-D planes of the scaled {out_layout} shapes, uint8 for 8-bit and uint16 for 10-bit output, with packed rows")
        (sp, ss), (dp, ds) = _plane_args(planes), _plane_args(dst)
        ok = bool(self._L.w2x_render_yuv_layout(self._h, (C.c_void_p * 3)(*sp), (C.c_size_t * 3)(*ss), rows, cols, bits, lid,
                                                (C.c_void_p * 3)(*dp), (C.c_size_t * 3)(*ds), rows * s, cols * s, ob, olid, _matrix_id(matrix), 1 if full_range else 0))
        if ret_array:
            if not ok:
                raise W2xError(self.last_error() or "render_yuv failed")
            return dst
        return ok

    def render_yuv_resized(self, y: np.ndarray, u: np.ndarray, v: np.ndarray, size, *, matrix: str = "bt709", full_range: bool = False,
                           out_bits: int | None = None, filter: str = "bicubic", dst=None):
        """render_yuv() with the canvas resized on the device to size = (rows, cols), each in [input dim, input dim * scaling], before it is encoded
        (w2x_render_yuv_resized).  Returns (Y, U, V) at the target size, or raises.  dst: pre-allocated planes (then a bool is returned).
        4:2:0 planes only, both sides (resample_yuv_kernel encodes 4:2:0): planes of another layout's shapes raise the ValueError that names 4:2:0."""
        bits = _yuv_bits((y, u, v))
        ob = bits if out_bits is None else int(out_bits)
        rows, cols = int(size[0]), int(size[1])
        fid = _filter_id(filter)
        dt = np.uint16 if ob == 10 else np.uint8
        shapes = yuv_plane_shapes(max(rows, 0), max(cols, 0))
        ret_array = dst is None
        out = tuple(np.empty(shape, dt) for shape in shapes) if dst is None else tuple(dst)
        if len(out) != 3 or any(not isinstance(p, np.ndarray) or p.dtype != dt or p.shape != shape or (p.size and p.strides[1] != p.itemsize) for p, shape in zip(out, shapes)):
            raise ValueError("dst must be three 2-D planes of the target's 4:2:0 shapes, uint8 for 8-bit and uint16 for 10-bit output, with packed rows")
        dp = (C.c_void_p * 3)(*[p.ctypes.data if p.size else None for p in out])   # (an empty target: refused by the library)
        ok = bool(self._L.w2x_render_yuv_resized(self._h, (C.c_void_p * 3)(*[p.ctypes.data for p in (y, u, v)]), (C.c_size_t * 3)(*[p.strides[0] for p in (y, u, v)]),
                                                 y.shape[0], y.shape[1], bits, dp, (C.c_size_t * 3)(*[p.strides[0] for p in out]), rows, cols, ob,
                                                 _matrix_id(matrix), 1 if full_range else 0, fid))
        if ret_array:
            if not ok:
                raise W2xError(self.last_error() or "render_yuv_resized failed")
            return out
        return ok

    def render_sequence_yuv_resized(self, frames, size, *, matrix: str = "bt709", full_range: bool = False, out_bits: int | None = None, pinned: bool = False,
                                    filter: str = "bicubic"):
        """render_sequence_yuv() with every frame resized to size = (rows, cols) like render_yuv_resized() (w2x_render_sequence_yuv_resized); 4:2:0 planes only"""
        return self._sequence_yuv(frames, (int(size[0]), int(size[1])), _filter_id(filter), matrix, full_range, out_bits, pinned)

    def render_sequence_yuv(self, frames, *, matrix: str = "bt709", full_range: bool = False, out_bits: int | None = None, pinned: bool = False,
                            layout: str | None = None, out_layout: str | None = None):
        """render_yuv() over equally sized frames [(y, u, v), ...] through the pipeline of render_sequence() (w2x_render_sequence_yuv).
        pinned=True takes the output planes from alloc_host() (a ring of three frames; copies of the results are returned).
        layout= / out_layout= as in render_yuv() (w2x_render_sequence_yuv_layout): every frame is a tuple of `layout`'s planes - [(y, uv), ...] for "nv12" -
        and a frame of another layout's shapes raises ValueError."""
        return self._sequence_yuv(frames, None, None, matrix, full_range, out_bits, pinned, layout, out_layout)

    def _sequence_yuv(self, frames, size, fid, matrix, full_range, out_bits, pinned, layout=None, out_layout=None):
        """the YUV sequence calls: size = None the scaled size (w2x_render_sequence_yuv; with a layout given w2x_render_sequence_yuv_layout), else the target of
        w2x_render_sequence_yuv_resized with filter fid"""
        n = len(frames)
        if n == 0:
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
        s = getattr(self, "_scaling", 0)
        orows, ocols = (rows * s, cols * s) if size is None else size
        shapes = yuv_layout_plane_shapes(max(orows, 1), max(ocols, 1), out_layout)   # (an empty target: refused by the library)
        steps = steps + [0] * (3 - len(steps))
        dt = np.uint8 if ob != 10 else np.uint16
        own = []
        if pinned:
            for _ in range(min(n, 3)):
                sizes = [r * c * np.dtype(dt).itemsize for r, c in shapes]
                buf = self.alloc_host((sum(sizes),))
                planes, o = [], 0
                for (r, c), nb in zip(shapes, sizes):
                    planes.append(buf[o:o + nb].view(dt).reshape(r, c)); o += nb
                own.append((buf, tuple(planes)))
        outs = [own[k % len(own)][1] for k in range(n)] if own else [tuple(np.empty(shape, dt) for shape in shapes) for _ in range(n)]
        dsteps = (C.c_size_t * 3)(*_plane_args(outs[0])[1])

        def run(fs, os_):
            m = len(fs)
            sp = (C.c_void_p * (3 * m))(*[q for f in fs for q in _plane_args(f)[0]])
            dp = (C.c_void_p * (3 * m))(*[q for o in os_ for q in _plane_args(o)[0]])
            args = (self._h, sp, (C.c_size_t * 3)(*steps), rows, cols, bits, dp, dsteps, orows, ocols, ob, m, _matrix_id(matrix), 1 if full_range else 0)
            if with_layout and size is None:
                if not self._L.w2x_render_sequence_yuv_layout(*args[:6], lid, *args[6:11], olid, *args[11:]):
                    raise W2xError(self.last_error() or "render_sequence_yuv failed")
                return
            if not (self._L.w2x_render_sequence_yuv(*args) if size is None else self._L.w2x_render_sequence_yuv_resized(*args, fid)):
                raise W2xError(self.last_error() or ("render_sequence_yuv failed" if size is None else "render_sequence_yuv_resized failed"))
        if own:
            res = []
            try:
                for k0 in range(0, n, len(own)):
                    m = min(len(own), n - k0)
                    run(frames[k0:k0 + m], outs[k0:k0 + m])
                    res += [tuple(p.copy() for p in o) for o in outs[k0:k0 + m]]
            finally:
                for buf, _ in own:
                    self.free_host(buf)
            return res
        run(frames, outs)
        return outs

    def alloc_host(self, shape) -> np.ndarray:
        """A uint8 array over page-locked memory owned by the engine (w2x_alloc_host): frame buffers whose PCIe copies
        render_sequence() can overlap with the kernels.  Valid until free_host(arr) / close()."""
        n = int(np.prod(shape))
        ptr = self._L.w2x_alloc_host(self._h, n)
        if not ptr:
            raise W2xError("w2x_alloc_host failed")
        arr = np.frombuffer((C.c_uint8 * n).from_address(ptr), np.uint8).reshape(shape)
        self._host_bufs = getattr(self, "_host_bufs", {})
        self._host_bufs[arr.ctypes.data] = ptr
        return arr

    def free_host(self, arr: np.ndarray) -> None:
        ptr = getattr(self, "_host_bufs", {}).pop(arr.ctypes.data, None)
        if ptr:
            self._L.w2x_free_host(self._h, ptr)

    def render_sequence(self, frames, outs=None, pinned: bool = False):
        """Equally sized frames with upload / compute / download overlapped (w2x_render_sequence).  outs: list of pre-allocated
        arrays (may repeat, e.g. a ring of buffers) or None; pinned=True takes the output buffers it allocates from alloc_host()
        (copies of the results are returned) - pass alloc_host() arrays as frames / outs yourself to avoid that copy."""
        s = getattr(self, "_scaling", 0)
        n = len(frames)
        if n == 0:
            return []
        r, c = frames[0].shape[:2]
        for f in frames:
            if f.dtype != np.uint8 or f.shape != (r, c, 3) or f.strides != (c * 3, 3, 1):
                raise ValueError("frames must be packed uint8 [rows, cols, 3] arrays of one size")
        own = []
        if outs is None:
            if pinned:
                own = [self.alloc_host((r * s, c * s, 3)) for _ in range(min(n, 3))]
                outs = [own[k % len(own)] for k in range(n)]
            else:
                outs = [np.empty((r * s, c * s, 3), np.uint8) for _ in range(n)]
        for o in outs:
            if o.dtype != np.uint8 or o.shape != (r * s, c * s, 3) or o.strides != (c * s * 3, 3, 1):
                raise ValueError("outs must be packed uint8 arrays of the scaled size")
        import ctypes as C
        sp = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        dp = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        if own:          # a ring of three engine-owned buffers: run the sequence in pieces and copy each result out
            res = []
            try:
                for k0 in range(0, n, len(own)):
                    m = min(len(own), n - k0)
                    if not self._L.w2x_render_sequence(self._h, (C.c_void_p * m)(*[f.ctypes.data for f in frames[k0:k0 + m]]), r, c, c * 3,
                                                       (C.c_void_p * m)(*[o.ctypes.data for o in own[:m]]), c * s * 3, m):
                        raise W2xError(self.last_error() or "render_sequence failed")
                    res += [o.copy() for o in own[:m]]
            finally:
                for o in own:
                    self.free_host(o)
            return res
        if not self._L.w2x_render_sequence(self._h, sp, r, c, c * 3, dp, c * s * 3, n):
            raise W2xError(self.last_error() or "render_sequence failed")
        return outs

    def infer(self, x: np.ndarray) -> np.ndarray:
        """Private trt::Img2Img::infer (img2img_infer.cpp:41-93) as a test hook: [B,3,T,T] f32 -> [B,3,T',T'] f32."""
        x = np.ascontiguousarray(x, np.float32)
        b, t = getattr(self, "_batch", 0), getattr(self, "_tile", 0)
        if not b:
            raise W2xError("infer called before a successful load")
        if x.shape != (b, 3, t, t):        # img2img_infer.cpp:43-68: batch count and tile shape must be the loaded configuration's
            raise ValueError(f"infer expects a [{b}, 3, {t}, {t}] blob, got {list(x.shape)}")
        to = self.output_tile_size
        y = np.empty((b, 3, to, to), np.float32)
        if not self._L.w2x_infer(self._h, x.ctypes.data, y.ctypes.data):
            raise W2xError(self.last_error() or "infer failed")
        return y

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
    s = getattr(engines[0], "_scaling", 0)
    if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3 or src.strides[2] != 1 or src.strides[1] != 3:
        raise ValueError("src must be a uint8 [rows, cols, 3] BGR array with packed pixels")
    if dst is None:
        dst = np.empty((src.shape[0] * s, src.shape[1] * s, 3), np.uint8)
    if dst.dtype != np.uint8 or dst.shape != (src.shape[0] * s, src.shape[1] * s, 3) or dst.strides[2] != 1 or dst.strides[1] != 3:
        raise ValueError("dst must be a packed uint8 array of the scaled size")
    handles = (C.c_void_p * len(engines))(*[e._h for e in engines])
    if not lib().w2x_render_sharded(handles, len(engines), src.ctypes.data, src.shape[0], src.shape[1], src.strides[0], dst.ctypes.data, dst.strides[0]):
        raise W2xError(engines[0].last_error() or "sharded render failed")
    return dst


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


def resize_weights(in_size: int, out_size: int, filter: str = "bicubic"):
    """Tap tables of the resized renders along one axis (w2x_resize_weights) -> (first[out] int32, weights[out, taps] float32)."""
    L = lib()
    fid = _filter_id(filter)
    taps = L.w2x_resize_weights(int(in_size), int(out_size), fid, None, None, 0)
    if taps <= 0:
        raise W2xError(f"invalid resize {in_size} -> {out_size}")
    first = np.zeros(out_size, np.int32)
    w = np.zeros((out_size, taps), np.float32)
    if L.w2x_resize_weights(int(in_size), int(out_size), fid, first.ctypes.data, w.ctypes.data, w.size) != taps:
        raise W2xError("w2x_resize_weights failed")
    return first, w


def alpha_bleed(bgr: np.ndarray, alpha: np.ndarray, radius: int) -> np.ndarray:
    """The colour bleed of the RGBA renders on the host (w2x_alpha_bleed): bgr uint8 [rows, cols, 3], alpha uint8 [rows, cols], radius 0..16 -> the frame with
    the colours of the pixels of alpha > 0 spread `radius` pixels outward under the pixels of alpha == 0; raises for invalid arguments"""
    if bgr.dtype != np.uint8 or bgr.ndim != 3 or bgr.shape[2] != 3 or (bgr.size and (bgr.strides[2] != 1 or bgr.strides[1] != 3)):
        raise ValueError("bgr must be a uint8 [rows, cols, 3] array with packed pixels")
    if alpha.dtype != np.uint8 or alpha.shape != bgr.shape[:2] or (alpha.size and alpha.strides[1] != 1):
        raise ValueError("alpha must be a uint8 [rows, cols] array of the frame's size with packed rows")
    out = np.empty(bgr.shape, np.uint8)
    if not lib().w2x_alpha_bleed(bgr.ctypes.data if bgr.size else None, bgr.strides[0], alpha.ctypes.data if alpha.size else None, alpha.strides[0],
                                 bgr.shape[0], bgr.shape[1], int(radius), out.ctypes.data if out.size else None, out.strides[0]):
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
