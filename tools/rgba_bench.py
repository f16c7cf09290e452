"""RGBA frames at config 3 (swin_unet/art x4 noise 3, batch 4, tile 256, blend 1/16, fp16): milliseconds per call, host frame in -> host frame out, of
  two_calls    the route renderRgba replaces, restated here: render(bgr), np.repeat of the alpha plane, render(gray), the green channel extracted and stacked
  rgba         render_rgba(bleed=0)
  rgba_bleed8  render_rgba(bleed=8)
  rgba_bleed16 render_rgba(bleed=16)
  rgba_uniform render_rgba(skip_uniform_alpha=True) on the same frame with an opaque alpha plane
  bgr          render() of the BGR frame alone (context: what colour costs on its own)
on a 1920 x 1080 cut-out frame, and two_calls / rgba on a 200 x 200 sprite (one tile: the two calls take two passes, the packed schedule one).
Every call ends in the engine's stream synchronise, so a host clock around it is the call's time.  The modes are timed in turns (one call of each per
round, --calls rounds after --warmup rounds) and the median per mode is reported; one JSON line on stdout.

--group resize times, on the same 1080p frame at the x2 and the x3 target (3840 x 2160, 5760 x 3240),
  two_resized  the route renderRgbaResized replaces: render_resized(bgr), np.repeat of the alpha plane, render_resized(gray), the green channel extracted and stacked
  rgba_resized render_rgba_resized(bleed=0)
--group sequence times, per frame, 16 different 1080p frames in page-locked buffers (alloc_host; the outputs go to a ring of four page-locked buffers)
  rgba_loop     a loop of render_rgba() calls, frame by frame
  rgba_sequence one render_sequence_rgba() call on the same buffers
with the same method (modes in turns, median).

--only MODE runs that mode alone (for `rocprofv3 --kernel-trace --stats -- python tools/rgba_bench.py --only rgba_bleed8`, which gives the device time of
alpha_bleed_kernel / gather_rgba_kernel / compose_rgba_kernel).  --bytes prints the bytes each route moves across PCIe and exits (no GPU).  Not part of
bench.py."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

W, H, S, MODEL, NOISE, BATCH, TILE, BLEND = 1920, 1080, 4, "swin_unet/art", 3, 4, 256, 0.0625
SPRITE = 200
MODES = ["two_calls", "rgba", "rgba_bleed8", "rgba_bleed16", "rgba_uniform", "bgr"]


def route_bytes(w: int, h: int) -> dict:
    """bytes per frame uploaded and downloaded by the two routes"""
    px, opx = w * h, w * S * h * S
    return {"two_calls": {"up": 2 * 3 * px, "down": 2 * 3 * opx}, "rgba": {"up": 4 * px, "down": 4 * opx}, "bgr": {"up": 3 * px, "down": 3 * opx}}


def cutout(np, rows, cols, seed):
    """a smooth picture with noise; alpha: an ellipse with a soft edge, fully transparent outside it (black underneath, as a drawing tool leaves it)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float32)
    img = 127.0 + 40.0 * np.sin(xx[..., None] * 0.01 + yy[..., None] * 0.013 + rng.uniform(0, 6.28, 3))
    bgr = np.clip(img + rng.integers(-4, 5, img.shape), 0, 255).astype(np.uint8)
    d = np.hypot((yy - rows / 2) / rows, (xx - cols / 2) / cols)
    a = np.clip((0.40 - d) * 2000, 0, 255).astype(np.uint8)
    bgr[a == 0] = 0
    return np.ascontiguousarray(np.dstack([bgr, a]))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9, help="timed calls per mode (at least 7)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="one of " + ",".join(MODES) + ": run that mode alone on the 1080p frame")
    ap.add_argument("--group", default="frames", choices=["frames", "resize", "sequence"], help="frames: the modes above; resize / sequence: the modes of DESIGN 9e")
    ap.add_argument("--work", default=os.path.join(tempfile.gettempdir(), "w2x_rgba_bench"), help="where the synthetic model and its engine file go")
    ap.add_argument("--bytes", action="store_true", help="print the bytes per frame of each route and exit (no GPU)")
    a = ap.parse_args()
    if a.bytes:
        print(json.dumps({"1920x1080": route_bytes(W, H), f"{SPRITE}x{SPRITE}": route_bytes(SPRITE, SPRITE)}))
        return 0
    group_modes = {"frames": MODES, "resize": ["two_resized", "rgba_resized"], "sequence": ["rgba_loop", "rgba_sequence"]}[a.group]
    if a.only and a.only not in group_modes:
        raise SystemExit(f"--only: {a.only} not in {group_modes}")
    calls = max(a.calls, 7)
    import numpy as np
    import synth_models as sm
    import __graft_entry__ as g
    pkg = g.package()
    path = sm.model_path(a.work, MODEL, S, NOISE)
    if not os.path.exists(path):
        sm.export_onnx(sm.make_model(MODEL, S, seed=1234 + NOISE), path, BATCH, TILE, dynamic=True)
    eng = pkg.Img2Img()
    if not eng.build(path, pkg.BuildConfig.fixed(BATCH, TILE)):
        raise SystemExit("build failed: " + eng.last_error())
    if not eng.load(path, pkg.RenderConfig(batchSize=BATCH, height=TILE, width=TILE, scaling=S, overlap=(BLEND, BLEND))):
        raise SystemExit("load failed: " + eng.last_error())

    def routes(bgra):
        """mode -> a call that renders `bgra` host to host and returns the BGRA (or BGR) output"""
        rows, cols = bgra.shape[:2]
        bgr = np.ascontiguousarray(bgra[..., :3])
        opaque = bgra.copy(); opaque[..., 3] = 255
        out4 = np.empty((rows * S, cols * S, 4), np.uint8)
        out3 = np.empty((rows * S, cols * S, 3), np.uint8)
        gray_out = np.empty((rows * S, cols * S, 3), np.uint8)

        def two_calls():
            # what a caller of the library had to write: split, render the colour, replicate the alpha plane, render it, extract, stack
            assert eng.render(np.ascontiguousarray(bgra[..., :3]), out3)
            gray = np.repeat(bgra[..., 3:4], 3, axis=2)
            assert eng.render(gray, gray_out)
            out4[..., :3] = out3
            out4[..., 3] = gray_out[..., 1]
            return out4

        def rgba(**kw):
            def call():
                assert eng.render_rgba(bgra if not kw.get("skip_uniform_alpha") else opaque, dst=out4, **kw), eng.last_error()
                return out4
            return call

        def plain():
            assert eng.render(bgr, out3)
            return out3
        return {"two_calls": two_calls, "rgba": rgba(), "rgba_bleed8": rgba(bleed=8), "rgba_bleed16": rgba(bleed=16),
                "rgba_uniform": rgba(skip_uniform_alpha=True), "bgr": plain}

    def measure(tag, bgra, modes):
        r = routes(bgra)
        batches = {}
        seen = []
        eng.setProgressCallback(lambda cur, total, speed: seen.append(total))
        for m in modes:                                   # the batches each route reports (a route of two calls: both)
            seen.clear(); r[m](); batches[m] = len(seen)
        eng.setProgressCallback(None)
        if "two_calls" in modes and "rgba" in modes:      # the routes agree before they are timed
            x = r["two_calls"]().copy()
            assert np.array_equal(x, r["rgba"]()), "render_rgba(bleed=0) differs from the two calls"
        for _ in range(a.warmup):
            for m in modes:
                r[m]()
        times = {m: [] for m in modes}
        for _ in range(calls):
            for m in modes:
                t0 = time.perf_counter()
                r[m]()
                times[m].append((time.perf_counter() - t0) * 1e3)
        return {m: {"ms_per_call_median": round(statistics.median(times[m]), 3), "ms_min": round(min(times[m]), 3), "ms_max": round(max(times[m]), 3),
                    "batches_reported": batches[m]} for m in modes}

    def timed(r, modes, check=None):
        """the method of measure() on a dict of calls: an equality check first, warm-up rounds, then the modes in turns"""
        if check:
            x = r[check[0]]().copy()
            assert np.array_equal(x, r[check[1]]()), f"{check[1]} differs from {check[0]}"
        for _ in range(a.warmup):
            for m in modes:
                r[m]()
        times = {m: [] for m in modes}
        for _ in range(calls):
            for m in modes:
                t0 = time.perf_counter()
                r[m]()
                times[m].append((time.perf_counter() - t0) * 1e3)
        return times

    def measure_resized(bgra, factor, modes):
        rows, cols = bgra.shape[:2]
        size = (rows * factor, cols * factor)
        out4 = np.empty(size + (4,), np.uint8)
        out3 = np.empty(size + (3,), np.uint8)
        gray_out = np.empty(size + (3,), np.uint8)

        def two_resized():
            assert eng.render_resized(np.ascontiguousarray(bgra[..., :3]), size, dst=out3)
            gray = np.repeat(bgra[..., 3:4], 3, axis=2)
            assert eng.render_resized(gray, size, dst=gray_out)
            out4[..., :3] = out3
            out4[..., 3] = gray_out[..., 1]
            return out4

        def rgba_resized():
            assert eng.render_rgba_resized(bgra, size, dst=out4), eng.last_error()
            return out4
        r = {"two_resized": two_resized, "rgba_resized": rgba_resized}
        times = timed(r, modes, ("two_resized", "rgba_resized") if len(modes) == 2 else None)
        return {m: {"ms_per_call_median": round(statistics.median(times[m]), 3), "ms_min": round(min(times[m]), 3), "ms_max": round(max(times[m]), 3)} for m in modes}

    def measure_sequence(modes, count=16, ring=4):
        frames = [eng.alloc_host((H, W, 4)) for _ in range(count)]
        outs = [eng.alloc_host((H * S, W * S, 4)) for _ in range(ring)]
        for k, f in enumerate(frames):
            f[...] = cutout(np, H, W, 10 + k)
        dsts = [outs[k % ring] for k in range(count)]

        def rgba_loop():
            for k in range(count):
                assert eng.render_rgba(frames[k], dst=dsts[k]), eng.last_error()
            return dsts[count - 1]

        def rgba_sequence():
            eng.render_sequence_rgba(frames, outs=dsts)
            return dsts[count - 1]
        r = {"rgba_loop": rgba_loop, "rgba_sequence": rgba_sequence}
        times = timed(r, modes, ("rgba_loop", "rgba_sequence") if len(modes) == 2 else None)
        for buf in frames + outs:
            eng.free_host(buf)
        return {m: {"ms_per_frame_median": round(statistics.median(times[m]) / count, 3), "ms_per_frame_min": round(min(times[m]) / count, 3),
                    "ms_per_frame_max": round(max(times[m]) / count, 3), "frames": count} for m in modes}

    res = {}
    frame = cutout(np, H, W, 3)
    if a.group == "resize":
        modes = [a.only] if a.only else ["two_resized", "rgba_resized"]
        for factor in (2, 3):
            res[f"{W}x{H} -> {W * factor}x{H * factor}"] = measure_resized(frame, factor, modes)
    elif a.group == "sequence":
        res[f"{W}x{H} x16 pinned"] = measure_sequence([a.only] if a.only else ["rgba_loop", "rgba_sequence"])
    elif a.only:
        res[f"{W}x{H}"] = measure("frame", frame, [a.only])
    else:
        res[f"{W}x{H}"] = measure("frame", frame, MODES)
        res[f"{SPRITE}x{SPRITE}"] = measure("sprite", cutout(np, SPRITE, SPRITE, 4), ["two_calls", "rgba"])
    eng.close()
    print(json.dumps({"tool": "rgba_bench", "workload": f"{MODEL} x{S} noise{NOISE} batch{BATCH} tile{TILE} fp16, blend 1/16, BGRA frames host to host ({'page-locked buffers' if a.group == 'sequence' else 'pageable numpy arrays'}), group {a.group}, "
                      f"median of {calls} calls per mode after {a.warmup} warm-up rounds, modes timed in turns", "bytes": {"1920x1080": route_bytes(W, H)}, "results": res}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
