"""Resize in linear light at config 3 (1080p, swin_unet/art x4 noise 3, batch 4, tile 256, blend 1/16), 1920x1080 -> 3840x2160 (the network's 7680x4320 canvas
halved): host frames in -> host frames out through the resized sequence calls with page-locked buffers, for bgr24 (renderSequenceResized) and yuv420p
(renderSequenceYuvResized), the three settings of setResizeLight alternating region by region so that clocks and neighbours on the machine hit all of them
alike.  Median ms per frame over --regions timed regions of --steps frames per setting, after warm-up; one JSON line on stdout (tools/resize_bench.py's sibling).

The device time of the canvas and resample kernels per setting comes from a run of this script under `rocprofv3 --kernel-trace --stats`: the decoding / encoding
instantiations carry LightArgs in their names, so one trace holds all three.  Not part of bench.py."""
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
LIGHTS = ("gamma", "srgb", "bt709")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6, help="frames per timed region")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1, help="untimed regions per setting")
    ap.add_argument("--formats", default="bgr24,yuv420p")
    ap.add_argument("--work", default=os.path.join(tempfile.gettempdir(), "w2x_resize_bench"), help="where the synthetic model and its engine file go")
    a = ap.parse_args()
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
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = 127.0 + 40.0 * np.sin(xx[..., None] * 0.01 + yy[..., None] * 0.013 + rng.uniform(0, 6.28, 3))
    frame = np.clip(img + rng.integers(-4, 5, img.shape), 0, 255).astype(np.uint8)
    size = (2 * H, 2 * W)
    n = max(a.steps, 3)
    held = []

    def host(arr):
        p = eng.alloc_host(arr.shape)
        p[...] = arr
        held.append(p)
        return p

    res = {}
    for fmt in a.formats.split(","):
        if fmt == "bgr24":
            pf = host(frame)
            ring = [host(np.zeros((size[0], size[1], 3), np.uint8)) for _ in range(3)]
            region = lambda: eng.render_sequence_resized([pf] * n, size, outs=[ring[k % 3] for k in range(n)])
        elif fmt == "yuv420p":
            planes = (host(frame[..., 1]), host(frame[::2, ::2, 0]), host(frame[::2, ::2, 2]))   # (any codes do: the time does not depend on them)
            region = lambda: eng.render_sequence_yuv_resized([planes] * n, size, pinned=True)
        else:
            raise SystemExit("unknown format " + fmt)
        times = {m: [] for m in LIGHTS}
        for r in range(a.warmup + a.regions):
            for m in LIGHTS:
                eng.set_resize_light(m)
                t0 = time.perf_counter()
                region()
                if r >= a.warmup:
                    times[m].append((time.perf_counter() - t0) * 1e3 / n)
        res[fmt] = {m: {"ms_per_frame_median": round(statistics.median(t), 4), "ms_per_frame": [round(v, 4) for v in t]} for m, t in times.items()}
    eng.set_resize_light("gamma")
    for p in held:
        eng.free_host(p)
    eng.close()
    print(json.dumps({"tool": "resize_light_bench", "workload": f"{MODEL} x{S} noise{NOISE} batch{BATCH} tile{TILE} fp16, {W}x{H} -> {size[1]}x{size[0]}, blend 1/16, resized sequences "
                      f"host to host, page-locked buffers, {a.regions} regions x {n} frames per setting after {a.warmup} warm-up region(s), settings alternating", "results": res}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
