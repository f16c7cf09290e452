"""Dithered output at config 3 (1080p, swin_unet/art x4 noise 3, batch 4, tile 256, blend 1/16), 8-bit: host frame in -> host frame out through the sequence
calls with page-locked buffers, for dither none, ordered and bluenoise (Img2Img::setDither), on bgr24 frames (renderSequence), yuv420p frames
(renderSequenceYuv) and, for the resample kernels, bgr24 resized to 3840x2160 (renderSequenceResized).  The modes ALTERNATE: every region of --steps frames is
run once per mode before the next region starts, so a drifting clock or a busy neighbour meets all modes alike; the figure of a mode is the median over
--regions regions, after warm-up.  One JSON line on stdout.

The device times of the compose and resample kernels per mode come from a separate run of this script under `rocprofv3 --kernel-trace --stats` (no counters):
the dithered instantiations carry their mode in the kernel name.  Not part of bench.py, which never sets the option."""
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
MODES = ("none", "ordered", "bluenoise")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8, help="frames per timed region")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2, help="warm-up regions per mode")
    ap.add_argument("--work", default=os.path.join(tempfile.gettempdir(), "w2x_dither_bench"), help="where the synthetic model and its engine file go")
    ap.add_argument("--formats", default="bgr24,yuv420p,bgr24_resized")
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
    n = max(a.steps, 3)
    res = {}
    for fmt in a.formats.split(","):
        held = []

        def host(shape):
            held.append(eng.alloc_host(shape))
            return held[-1]
        if fmt == "yuv420p":
            planes = (host((H, W)), host((H // 2, W // 2)), host((H // 2, W // 2)))
            planes[0][...] = frame[..., 1]
            planes[1][...] = 128 + (frame[::2, ::2, 0].astype(np.int16) - frame[::2, ::2, 1]) // 2
            planes[2][...] = 128 + (frame[::2, ::2, 2].astype(np.int16) - frame[::2, ::2, 1]) // 2

            def region():
                eng.render_sequence_yuv([planes] * n, pinned=True)    # (page-locked outputs: a ring of three frames, each copied out once)
            out = f"{W * S}x{H * S}"
        else:
            size = (H * S, W * S) if fmt == "bgr24" else (H * 2, W * 2)
            pf = host(frame.shape)
            pf[...] = frame
            ring = [host((size[0], size[1], 3)) for _ in range(3)]

            def region():
                frames, outs = [pf] * n, [ring[k % 3] for k in range(n)]
                if fmt == "bgr24":
                    eng.render_sequence(frames, outs=outs)
                else:
                    eng.render_sequence_resized(frames, size, outs=outs)
            out = f"{size[1]}x{size[0]}"
        times = {m: [] for m in MODES}
        for rnd in range(a.warmup + a.regions):
            for m in MODES:                                            # alternating: one region per mode, then the next round
                assert eng.set_dither(m)
                t0 = time.perf_counter()
                region()
                if rnd >= a.warmup:
                    times[m].append((time.perf_counter() - t0) * 1e3 / n)
        eng.set_dither("none")
        res[fmt] = {"out": out, **{m: {"ms_per_frame_median": round(statistics.median(t), 4), "ms_per_frame": [round(x, 4) for x in t]} for m, t in times.items()}}
        for h in held:
            eng.free_host(h)
    eng.close()
    print(json.dumps({"tool": "dither_bench", "workload": f"{MODEL} x{S} noise{NOISE} batch{BATCH} tile{TILE} fp16, {W}x{H} frames, blend 1/16, 8-bit, sequence calls host to host, "
                      f"page-locked buffers, modes alternating, {a.regions} regions x {n} frames after {a.warmup} warm-up regions per mode", "results": res}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
