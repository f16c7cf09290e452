"""Gray frames at config 3 (swin_unet/art x4 noise 3, batch 4, tile 256, blend 1/16, fp16, 1920 x 1080) or config 5 (--config 5: swin_unet/art_scan x4,
batch 16, tile 640, 3840 x 2160 -> 15360 x 8640, the scan configuration): milliseconds per call, host frame in -> host frame out, of
  replicated      the route a caller had before renderGray, restated here: np.repeat of the plane into BGR, render(), the green channel picked out
  replicated_gpu  the same without the two host passes: render() of an already replicated frame into a BGR buffer (what the engine and PCIe cost alone)
  gray            render_gray()
--group resize times, at the x2 target,
  replicated_resized / replicated_resized_gpu   render_resized() of the replicated frame, with and without the host passes
  gray_resized                                  render_gray_resized()
--group sequence times, per frame, 16 different frames in page-locked buffers (alloc_host; the outputs go to a ring of four page-locked buffers)
  bgr_sequence    render_sequence() of the replicated frames (replicated beforehand: the host passes are not in the time)
  gray_sequence   render_sequence_gray()
Every call ends in the engine's stream synchronise, so a host clock around it is the call's time.  The modes are timed in turns (one call of each per round,
--calls rounds after --warmup rounds) and every figure is taken twice: the whole procedure - warm-up rounds, then the timed rounds - runs two times one after
the other in the process, and the median of each run is reported next to the median of both, so the spread between two runs of the same code stands beside
every difference between two routes.  One JSON line on stdout.

--only MODE runs that mode alone (for `rocprofv3 --kernel-trace --stats -- python tools/gray_bench.py --only gray`, which gives the device time of
gather_planes_kernel / compose_planes_kernel at one plane against gather_kernel / compose_kernel under --only replicated_gpu; with --group resize the canvas and resample
kernels).  --bytes prints the bytes each route moves across PCIe per frame and exits (no GPU).  Not part of bench.py."""
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

CONFIGS = {3: dict(w=1920, h=1080, model="swin_unet/art", batch=4, tile=256), 5: dict(w=3840, h=2160, model="swin_unet/art_scan", batch=16, tile=640)}
S, NOISE, BLEND = 4, 3, 0.0625
GROUPS = {"frames": ["replicated", "replicated_gpu", "gray"], "resize": ["replicated_resized", "replicated_resized_gpu", "gray_resized"],
          "sequence": ["bgr_sequence", "gray_sequence"]}


def route_bytes(w: int, h: int, factor: int = S) -> dict:
    """bytes per frame uploaded and downloaded by the two routes, at an output of `factor` times the input"""
    px, opx = w * h, w * factor * h * factor
    return {"replicated": {"up": 3 * px, "down": 3 * opx}, "gray": {"up": px, "down": opx}}


def page(np, rows, cols, seed):
    """a gray page: smooth shading, hard strokes and a little noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float32)
    img = 200.0 + 40.0 * np.sin(xx * 0.011 + yy * 0.007 + seed)
    img[(xx.astype(np.int32) // 7 + yy.astype(np.int32) // 11 + seed) % 9 == 0] = 30.0
    return np.clip(img + rng.integers(-4, 5, img.shape), 0, 255).astype(np.uint8)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3, choices=sorted(CONFIGS))
    ap.add_argument("--calls", type=int, default=8, help="timed calls per mode and run (at least 6; there are two runs)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--group", default="frames", choices=sorted(GROUPS))
    ap.add_argument("--only", default="", help="run one mode of the group alone")
    ap.add_argument("--work", default=os.path.join(tempfile.gettempdir(), "w2x_gray_bench"), help="where the synthetic model and its engine file go")
    ap.add_argument("--bytes", action="store_true", help="print the bytes per frame of each route and exit (no GPU)")
    a = ap.parse_args()
    cfg = CONFIGS[a.config]
    W, H, MODEL, BATCH, TILE = cfg["w"], cfg["h"], cfg["model"], cfg["batch"], cfg["tile"]
    if a.bytes:
        print(json.dumps({f"config {k}: {c['w']}x{c['h']}": {"x4": route_bytes(c["w"], c["h"]), "x2": route_bytes(c["w"], c["h"], 2)} for k, c in CONFIGS.items()}))
        return 0
    modes = GROUPS[a.group]
    if a.only:
        if a.only not in modes:
            raise SystemExit(f"--only: {a.only} not in {modes}")
        modes = [a.only]
    calls = max(a.calls, 6)
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

    def timed(r, per=1, check=None):
        """an equality check first; then, two times over, warm-up rounds and the modes in turns; per mode the median of each run and of both"""
        if check and all(m in r for m in check):
            x = r[check[0]]().copy()
            assert np.array_equal(x, r[check[1]]()), f"{check[1]} differs from {check[0]}"
        runs = []
        for _ in range(2):
            for _ in range(a.warmup):
                for m in r:
                    r[m]()
            times = {m: [] for m in r}
            for _ in range(calls):
                for m in r:
                    t0 = time.perf_counter()
                    r[m]()
                    times[m].append((time.perf_counter() - t0) * 1e3 / per)
            runs.append(times)
        return {m: {"ms_median": round(statistics.median(runs[0][m] + runs[1][m]), 3), "ms_median_run1": round(statistics.median(runs[0][m]), 3),
                    "ms_median_run2": round(statistics.median(runs[1][m]), 3), "ms_min": round(min(runs[0][m] + runs[1][m]), 3),
                    "ms_max": round(max(runs[0][m] + runs[1][m]), 3)} for m in r}

    res = {}
    gray = page(np, H, W, 3)
    if a.group in ("frames", "resize"):
        factor = S if a.group == "frames" else 2
        size = (H * factor, W * factor)
        rep = np.ascontiguousarray(np.repeat(gray[..., None], 3, axis=2))
        out3, out1, picked = np.empty(size + (3,), np.uint8), np.empty(size, np.uint8), np.empty(size, np.uint8)

        def bgr_call(frame):
            if a.group == "frames":
                assert eng.render(frame, out3), eng.last_error()
            else:
                assert eng.render_resized(frame, size, dst=out3), eng.last_error()

        def replicated():
            bgr_call(np.repeat(gray[..., None], 3, axis=2))        # what a caller of the library had to write: replicate, render, pick a channel
            picked[...] = out3[..., 1]
            return picked

        def replicated_gpu():
            bgr_call(rep)
            return out3[..., 1]

        def gray_call():
            if a.group == "frames":
                assert eng.render_gray(gray, out1), eng.last_error()
            else:
                assert eng.render_gray_resized(gray, size, dst=out1), eng.last_error()
            return out1
        names = GROUPS[a.group]
        r = {m: f for m, f in zip(names, (replicated, replicated_gpu, gray_call)) if m in modes}
        res[f"{W}x{H} -> {size[1]}x{size[0]}"] = timed(r, check=(names[0], names[2]))
        nbytes = route_bytes(W, H, factor)
    else:
        count, ring = 16, 4
        frames1 = [eng.alloc_host((H, W)) for _ in range(count)]
        frames3 = [eng.alloc_host((H, W, 3)) for _ in range(count)] if "bgr_sequence" in modes else []
        outs1 = [eng.alloc_host((H * S, W * S)) for _ in range(ring)]
        outs3 = [eng.alloc_host((H * S, W * S, 3)) for _ in range(ring)] if "bgr_sequence" in modes else []
        for k, f in enumerate(frames1):
            f[...] = page(np, H, W, 10 + k)
            if frames3:
                frames3[k][...] = f[..., None]
        d1 = [outs1[k % ring] for k in range(count)]
        d3 = [outs3[k % ring] for k in range(count)] if outs3 else []

        def bgr_sequence():
            eng.render_sequence(frames3, d3)
            return d3[count - 1][..., 1]

        def gray_sequence():
            eng.render_sequence_gray(frames1, outs=d1)
            return d1[count - 1]
        r = {m: f for m, f in (("bgr_sequence", bgr_sequence), ("gray_sequence", gray_sequence)) if m in modes}
        res[f"{W}x{H} x{count} page-locked, per frame"] = timed(r, per=count, check=("bgr_sequence", "gray_sequence"))
        for buf in frames1 + frames3 + outs1 + outs3:
            eng.free_host(buf)
        nbytes = route_bytes(W, H)
    eng.close()
    print(json.dumps({"tool": "gray_bench", "workload": f"config {a.config}: {MODEL} x{S} noise{NOISE} batch{BATCH} tile{TILE} fp16, blend 1/16, {W}x{H} gray frames host to host "
                      f"({'page-locked buffers' if a.group == 'sequence' else 'pageable numpy arrays'}), group {a.group}, two runs of {calls} calls per mode, each after "
                      f"{a.warmup} warm-up rounds, modes timed in turns; median of each run and of both", "bytes_per_frame": nbytes, "results": res}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
