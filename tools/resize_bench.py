"""Resized output at config 3 (1080p, swin_unet/art x4 noise 3, batch 4, tile 256, blend 1/16): host frame in -> host frame out through
renderSequence / renderSequenceResized with engine-owned page-locked buffers, plain (1920x1080 -> 7680x4320), --outscale 2 (3840x2160) and
--outscale 3 (5760x3240).  Median ms per frame over --regions timed regions of --steps frames each, after warm-up; one JSON line on stdout.

The device time of the two resize kernels comes from a separate run of this script under `rocprofv3 --kernel-trace --stats`; --bytes prints the
bytes they move per frame (the roofline figures beside those times).  Not part of bench.py."""
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


def kernel_bytes(outscale: float) -> dict:
    """bytes per frame the resize path moves beyond the u8 compose it replaces (algorithmic: every sample once)"""
    cw, ch = W * S, H * S
    ow, oh = round(W * outscale), round(H * outscale)
    canvas = cw * ch * 3 * 4
    return {"canvas_write": canvas, "canvas_read": canvas, "out_write": ow * oh * 3, "u8_compose_write": cw * ch * 3}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8, help="frames per timed region")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--work", default=os.path.join(tempfile.gettempdir(), "w2x_resize_bench"), help="where the synthetic model and its engine file go")
    ap.add_argument("--modes", default="plain,2,3")
    ap.add_argument("--bytes", action="store_true", help="print the algorithmic bytes per frame and exit (no GPU)")
    a = ap.parse_args()
    if a.bytes:
        print(json.dumps({str(f): kernel_bytes(f) for f in (2, 3)}))
        return 0
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
    pf = eng.alloc_host(frame.shape)
    pf[...] = frame
    res = {}
    for mode in a.modes.split(","):
        size = (H * S, W * S) if mode == "plain" else (round(H * float(mode)), round(W * float(mode)))
        ring = [eng.alloc_host((size[0], size[1], 3)) for _ in range(3)]
        n = max(a.steps, 3)

        def region():
            frames, outs = [pf] * n, [ring[k % 3] for k in range(n)]
            if mode == "plain":
                eng.render_sequence(frames, outs=outs)
            else:
                eng.render_sequence_resized(frames, size, outs=outs)
        for _ in range(a.warmup):
            region()
        times = []
        for _ in range(a.regions):
            t0 = time.perf_counter()
            region()
            times.append((time.perf_counter() - t0) * 1e3 / n)
        res[mode] = {"out": f"{size[1]}x{size[0]}", "ms_per_frame_median": round(statistics.median(times), 4),
                     "ms_per_frame": [round(t, 4) for t in times]}
        for r in ring:
            eng.free_host(r)
    eng.free_host(pf)
    eng.close()
    print(json.dumps({"tool": "resize_bench", "workload": f"{MODEL} x{S} noise{NOISE} batch{BATCH} tile{TILE} fp16, {W}x{H} frames, blend 1/16, "
                      f"renderSequence(Resized) host to host, page-locked buffers, {a.regions} regions x {max(a.steps, 3)} frames after {a.warmup} warm-up regions",
                      "results": res, "bytes_per_frame": {m: kernel_bytes(float(m)) for m in res if m != "plain"}}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
