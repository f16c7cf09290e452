"""Edge modes at config 3 (1080p, swin_unet/art x4 noise 3, batch 4, tile 256, blend 1/16): host frames in -> host frames out through renderSequence
(1920x1080 -> 7680x4320) and renderSequenceResized (-> 3840x2160) with page-locked buffers, the three settings of setEdge alternating region by region so
that clocks and neighbours on the machine hit all of them alike.  Median ms per frame over --regions timed regions of --steps frames per setting, after
warm-up; one JSON line on stdout (tools/resize_light_bench.py's sibling).

--seam: the seam measure instead, on a small periodic texture (one period of a sum of sines, 96 x 128, with a little noise that is periodic too): the x4 output
under replicate and under wrap is tiled 2 x 2, and the mean absolute step across the joint (last column -> first column, last row -> first row) is set against
the step between two interior neighbours.  A texture that tiles has the same step everywhere.

The device time of the gather and resample kernels per mode comes from a run of this script under `rocprofv3 --kernel-trace --stats`: the instantiations carry
the mode (gather: a template argument; resize: EdgeArgs) in their names, so one trace holds all three.  Not part of bench.py."""
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
MODES = ("replicate", "wrap", "mirror")


def engine(pkg, work, batch, tile):
    import synth_models as sm
    path = sm.model_path(work, MODEL, S, NOISE)
    if not os.path.exists(path):
        sm.export_onnx(sm.make_model(MODEL, S, seed=1234 + NOISE), path, batch, tile, dynamic=True)
    eng = pkg.Img2Img()
    if not eng.build(path, pkg.BuildConfig.fixed(batch, tile)):
        raise SystemExit("build failed: " + eng.last_error())
    if not eng.load(path, pkg.RenderConfig(batchSize=batch, height=tile, width=tile, scaling=S, overlap=(BLEND, BLEND))):
        raise SystemExit("load failed: " + eng.last_error())
    return eng


def seam(pkg, work) -> dict:
    import numpy as np
    eng = engine(pkg, os.path.join(work, "seam"), 2, 64)
    rows, cols = 96, 128
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    img = np.zeros((rows, cols, 3))
    for k in range(1, 5):                                          # whole periods along both axes: the texture tiles
        img += 28.0 / k * np.sin(2 * np.pi * (k * xx[..., None] / cols + (k + 1) * yy[..., None] / rows) + rng.uniform(0, 6.28, 3))
    frame = np.clip(127.0 + img + rng.integers(-3, 4, img.shape), 0, 255).astype(np.uint8)
    res = {}
    for mode in ("replicate", "wrap"):
        eng.set_edge(mode)
        out = eng.render(frame).astype(np.float64)
        tiled = np.tile(out, (2, 2, 1))
        r, c = out.shape[:2]
        res[mode] = {
            "step_across_the_vertical_joint": round(float(np.abs(tiled[:, c] - tiled[:, c - 1]).mean()), 4),
            "step_between_interior_columns": round(float(np.abs(tiled[:, c // 2] - tiled[:, c // 2 - 1]).mean()), 4),
            "step_across_the_horizontal_joint": round(float(np.abs(tiled[r] - tiled[r - 1]).mean()), 4),
            "step_between_interior_rows": round(float(np.abs(tiled[r // 2] - tiled[r // 2 - 1]).mean()), 4),
        }
    eng.set_edge("replicate")
    eng.close()
    return {"tool": "edge_bench --seam", "workload": f"{MODEL} x{S} noise{NOISE} batch2 tile64 fp16, a periodic {cols}x{rows} texture, output tiled 2 x 2; mean absolute step in 8-bit codes", "results": res}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6, help="frames per timed region")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1, help="untimed regions per setting")
    ap.add_argument("--calls", default="plain,resized")
    ap.add_argument("--seam", action="store_true", help="the seam measure instead of the timings")
    ap.add_argument("--work", default=os.path.join(tempfile.gettempdir(), "w2x_edge_bench"), help="where the synthetic model and its engine file go")
    a = ap.parse_args()
    import numpy as np
    import __graft_entry__ as g
    pkg = g.package()
    if a.seam:
        print(json.dumps(seam(pkg, a.work)))
        return 0
    eng = engine(pkg, a.work, BATCH, TILE)
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = 127.0 + 40.0 * np.sin(xx[..., None] * 0.01 + yy[..., None] * 0.013 + rng.uniform(0, 6.28, 3))
    frame = np.clip(img + rng.integers(-4, 5, img.shape), 0, 255).astype(np.uint8)
    n = max(a.steps, 3)
    held = []

    def host(arr):
        p = eng.alloc_host(arr.shape)
        p[...] = arr
        held.append(p)
        return p

    pf = host(frame)
    res = {}
    for call in a.calls.split(","):
        if call == "plain":
            ring = [host(np.zeros((S * H, S * W, 3), np.uint8)) for _ in range(3)]
            region = lambda: eng.render_sequence([pf] * n, outs=[ring[k % 3] for k in range(n)])
        elif call == "resized":
            size = (2 * H, 2 * W)
            ring2 = [host(np.zeros((size[0], size[1], 3), np.uint8)) for _ in range(3)]
            region = lambda: eng.render_sequence_resized([pf] * n, size, outs=[ring2[k % 3] for k in range(n)])
        else:
            raise SystemExit("unknown call " + call)
        times = {m: [] for m in MODES}
        for r in range(a.warmup + a.regions):
            for m in MODES:
                eng.set_edge(m)
                t0 = time.perf_counter()
                region()
                if r >= a.warmup:
                    times[m].append((time.perf_counter() - t0) * 1e3 / n)
        res[call] = {m: {"ms_per_frame_median": round(statistics.median(t), 4), "ms_per_frame": [round(v, 4) for v in t]} for m, t in times.items()}
    eng.set_edge("replicate")
    for p in held:
        eng.free_host(p)
    eng.close()
    print(json.dumps({"tool": "edge_bench", "workload": f"{MODEL} x{S} noise{NOISE} batch{BATCH} tile{TILE} fp16, {W}x{H} -> x{S} (plain) / x2 (resized), blend 1/16, sequences host to host, "
                      f"page-locked buffers, {a.regions} regions x {n} frames per setting after {a.warmup} warm-up region(s), settings alternating", "results": res}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
