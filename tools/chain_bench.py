"""Chained renders against the two-call route, cunet/art x2 . x2, batch 4, tile 256, blend 1/16, 8-bit bgr24, page-locked frames host to host:
  x4:      1920x1080 -> 7680x4320, render_chained([a, b], f) against b.render(a.render(f)) - the only route there was: the 3840x2160 frame between the two
           stages is quantised, downloaded and uploaded again, with the host waiting in between;
  resized: 854x480 -> 1920x1080, render_chained_resized([a, b], f, 1080p) against b.render_resized(a.render(f), 1080p).
a is the model at noise 1, b the scale-only model (noise -1): the rule of waifu2x-caffe.  The routes ALTERNATE: every region of --steps frames is run once per
route before the next region starts, so a drifting clock or a busy neighbour meets both alike; a route's figure is the median over --regions regions after
--warmup regions, and its spread the range over them.  Before timing, the quantised chain is compared with the two-call route byte for byte (the unquantised
chain has no two-call route of 8-bit frames to be equal to).  One GPU process; every step runs under a time limit of its own (--limit seconds: SIGALRM ends
the process).  One JSON line on stdout.

--mode handoff: no timing here.  --frames frames through the chain (compose_px_kernel / gather_px_kernel: one 8-byte pixel vector per pixel between the stages)
and through the float planar route b.render_planar(a.render_planar(f, out_bits=32)) (compose_planes_kernel / gather_planes_kernel on three fp32 planes: 12 bytes
per pixel in three streams) on the same 3840x2160 frame between the stages, for a run under `rocprofv3 --kernel-trace --stats`: the two hand-offs' kernels
carry their names, and the per-launch times of the two are read off the statistics.  Not part of bench.py, which never chains."""
from __future__ import annotations

import argparse
import json
import os
import signal
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MODEL, S, BATCH, TILE, BLEND = "cunet/art", 2, 4, 256, 0.0625
CASES = {"x4": (1080, 1920, None), "resized": (480, 854, (1080, 1920))}


class Step:
    """a time limit around one step: the process ends there rather than hang"""
    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        def late(signum, frame):
            sys.stderr.write(f"chain_bench: step '{self.name}' passed its limit of {self.seconds} s\n")
            os._exit(124)
        signal.signal(signal.SIGALRM, late)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="e2e", choices=("e2e", "handoff"))
    ap.add_argument("--cases", default="x4,resized")
    ap.add_argument("--steps", type=int, default=4, help="frames per timed region")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2, help="warm-up regions per route")
    ap.add_argument("--frames", type=int, default=3, help="--mode handoff: frames per route")
    ap.add_argument("--limit", type=int, default=120, help="seconds a step may take")
    ap.add_argument("--work", default=os.path.join(tempfile.gettempdir(), "w2x_chain_bench"), help="where the synthetic models and their engine files go")
    a = ap.parse_args()
    import numpy as np
    import synth_models as sm
    import __graft_entry__ as g
    pkg = g.package()
    engines = []
    with Step("engines", a.limit):
        for noise in (1, -1):
            path = sm.model_path(a.work, MODEL, S, noise)
            if not os.path.exists(path):
                sm.export_onnx(sm.make_model(MODEL, S, seed=1234 + noise), path, BATCH, TILE, dynamic=True)
            eng = pkg.Img2Img()
            if not eng.build(path, pkg.BuildConfig.fixed(BATCH, TILE)):
                raise SystemExit("build failed: " + eng.last_error())
            if not eng.load(path, pkg.RenderConfig(batchSize=BATCH, height=TILE, width=TILE, scaling=S, overlap=(BLEND, BLEND))):
                raise SystemExit("load failed: " + eng.last_error())
            engines.append(eng)
    ea, eb = engines
    rng = np.random.default_rng(3)

    def frame_of(h, w):
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        img = 127.0 + 40.0 * np.sin(xx[..., None] * 0.01 + yy[..., None] * 0.013 + rng.uniform(0, 6.28, 3))
        return np.clip(img + rng.integers(-4, 5, img.shape), 0, 255).astype(np.uint8)

    if a.mode == "handoff":
        h, w, _ = CASES["x4"]
        f = frame_of(h, w)
        planes = tuple(np.ascontiguousarray(f[..., k]) for k in (2, 1, 0))
        with Step("handoff", a.limit):
            for _ in range(a.frames):
                pkg.render_chained_planar([ea, eb], planes)
            for _ in range(a.frames):
                eb.render_planar(ea.render_planar(planes, out_bits=32), out_bits=8)
        print(json.dumps({"mode": "handoff", "frames_per_route": a.frames, "between": [2 * h, 2 * w]}))
        return 0

    res = {}
    for case in a.cases.split(","):
        h, w, size = CASES[case]
        held = []

        def host(shape):
            held.append(ea.alloc_host(shape))
            return held[-1]
        out_shape = (h * 4, w * 4, 3) if size is None else (size[0], size[1], 3)
        pf, mid, out = host((h, w, 3)), host((2 * h, 2 * w, 3)), host(out_shape)
        pf[...] = frame_of(h, w)

        def chained(quantize=False):
            if size is None:
                return pkg.render_chained([ea, eb], pf, quantize=quantize, dst=out)
            return pkg.render_chained_resized([ea, eb], pf, size, quantize=quantize, dst=out)

        def two_calls():
            ok = ea.render(pf, mid)
            return ok and (eb.render(mid, out) if size is None else eb.render_resized(mid, size, dst=out))
        with Step(case + " equality", a.limit):
            assert two_calls(), eb.last_error()
            want = out.copy()
            assert chained(quantize=True), ea.last_error()
            equal = bool((out == want).all())
        routes = {"chained": chained, "two_calls": two_calls}
        times = {k: [] for k in routes}
        for region in range(a.warmup + a.regions):
            for name, run in routes.items():
                with Step(f"{case} {name} region {region}", a.limit):
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        assert run(), ea.last_error()
                    dt = (time.perf_counter() - t0) / a.steps * 1e3
                if region >= a.warmup:
                    times[name].append(dt)
        res[case] = {"in": [h, w], "out": list(out_shape[:2]), "quantised_chain_equals_two_calls": equal}
        for name, ts in times.items():
            res[case][name + "_ms"] = {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}
        for buf in held:
            ea.free_host(buf)
    print(json.dumps({"mode": "e2e", "model": MODEL, "batch": BATCH, "tile": TILE, "steps": a.steps, "regions": a.regions, "warmup": a.warmup, "cases": res}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
