"""Planar RGBA frames at config 3 (swin_unet/art x4 noise 3, batch 4, tile 256, blend 1/16, fp16, 1920 x 1080 -> 7680 x 4320; --half: 960 x 540 -> 3840 x 2160):
milliseconds per frame, host frame in -> host frame out, of
sequences of --frames different frames in page-locked buffers (alloc_host; the outputs go to a ring of four page-locked frames, two at float output), per pair of depths
  --pair 8/8      rgba_sequence   render_sequence_rgba() of the interleaved 8-bit BGRA frames: what the one-call path replaces at 8 bits
                  rgbap_sequence  render_sequence_planar_rgba() of the same frames as four planes
  --pair 10/10, 16/16, 8/32
                  two_sequences   the two-call route of the parent commit: render_sequence_planar() of the colour planes, then render_sequence_planar() of the
                                  alpha plane three times (the same page-locked plane named three times: nothing is replicated in the time), G kept
                  rgbap_sequence  render_sequence_planar_rgba()
An equality check of the two routes comes first (bleed 0).  Every call ends in the engine's stream synchronise, so a host clock around it is the call's time.
The modes are timed in turns (--calls rounds after --warmup rounds) and the whole procedure runs twice in the process: the median of each run stands beside the
median of both, so the spread between two runs of the same code stands beside every difference between two routes.  --bleed R adds the bleed to the one-call
route (the two-call route has none on the device at these depths).  One JSON line on stdout.

--only MODE runs that mode alone (for `rocprofv3 --kernel-trace --stats -- python tools/planar_rgba_bench.py --pair 16/16 --only rgbap_sequence`, which gives
the device time of alpha_bleed_planes_kernel, gather_planes_rgba_kernel and compose_planes_rgba_kernel).  Not part of bench.py."""
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

MODEL, S, NOISE, BLEND, BATCH, TILE = "swin_unet/art", 4, 3, 0.0625, 4, 256
PAIRS = {"8/8": (8, 8), "10/10": (10, 10), "16/16": (16, 16), "8/32": (8, 32)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pair", default="8/8", choices=sorted(PAIRS))
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--calls", type=int, default=6, help="timed calls per mode and run (there are two runs)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bleed", type=int, default=0)
    ap.add_argument("--half", action="store_true", help="960 x 540 frames (3840 x 2160 out) instead of 1920 x 1080")
    ap.add_argument("--only", default="", help="run one mode alone")
    ap.add_argument("--work", default=os.path.join(tempfile.gettempdir(), "w2x_planar_rgba_bench"), help="where the synthetic model and its engine file go")
    a = ap.parse_args()
    W, H = (960, 540) if a.half else (1920, 1080)
    bits, out_bits = PAIRS[a.pair]
    import numpy as np
    import synth_models as sm
    import __graft_entry__ as g
    pkg = g.package()
    engine = sys.modules[pkg.__name__ + ".engine"]
    dt, odt = engine.PLANAR_DTYPES[bits], engine.PLANAR_DTYPES[out_bits]
    path = sm.model_path(a.work, MODEL, S, NOISE)
    if not os.path.exists(path):
        sm.export_onnx(sm.make_model(MODEL, S, seed=1234 + NOISE), path, BATCH, TILE, dynamic=True)
    eng = pkg.Img2Img()
    if not eng.build(path, pkg.BuildConfig.fixed(BATCH, TILE)):
        raise SystemExit("build failed: " + eng.last_error())
    if not eng.load(path, pkg.RenderConfig(batchSize=BATCH, height=TILE, width=TILE, scaling=S, overlap=(BLEND, BLEND))):
        raise SystemExit("load failed: " + eng.last_error())
    count, ring, m = a.frames, 2 if out_bits == 32 else 4, (1 << bits) - 1
    held = []

    def host(shape, dtype):
        buf = eng.alloc_host((int(np.prod(shape)) * np.dtype(dtype).itemsize,))
        held.append(buf)
        return buf.view(dtype).reshape(shape)

    def planes(n, shape, dtype):
        block = host((n,) + shape, dtype)
        return tuple(block[k] for k in range(n))

    yy, xx = np.mgrid[0:H, 0:W]
    frames = []
    for k in range(count):                                          # noise colours under a soft-edged shape with holes: about a third of the frame is transparent
        rng = np.random.default_rng(10 + k)
        f = planes(4, (H, W), dt)
        for p in f[:3]:
            p[...] = rng.integers(0, m + 1, (H, W))
        d = np.hypot((yy - H / 2) / H, (xx - W / 2 - 20 * k) / W)
        alpha = np.clip((0.42 - d) * 8 * m, 0, m)
        alpha[(yy // 37 + xx // 29) % 9 == 0] = 0
        f[3][...] = alpha
        frames.append(f)
    outs4 = [planes(4, (H * S, W * S), odt) for _ in range(ring)]
    d4 = [outs4[k % ring] for k in range(count)]
    modes = {}
    if a.pair == "8/8":
        bgra = [host((H, W, 4), np.uint8) for _ in range(count)]
        for b, f in zip(bgra, frames):
            b[...] = np.stack([f[2], f[1], f[0], f[3]], axis=2)
        outs_i = [host((H * S, W * S, 4), np.uint8) for _ in range(ring)]
        di = [outs_i[k % ring] for k in range(count)]

        def reference():
            eng.render_sequence_rgba(bgra, outs=di, bleed=a.bleed)
            return tuple(di[count - 1][..., k] for k in (2, 1, 0, 3))
        modes["rgba_sequence"] = reference
    else:
        outs3 = [planes(3, (H * S, W * S), odt) for _ in range(ring)]
        outs_a = [planes(3, (H * S, W * S), odt) for _ in range(ring)]
        d3, da = [outs3[k % ring] for k in range(count)], [outs_a[k % ring] for k in range(count)]

        def reference():
            eng.render_sequence_planar([f[:3] for f in frames], bits=bits, out_bits=out_bits, outs=d3)
            eng.render_sequence_planar([(f[3],) * 3 for f in frames], bits=bits, out_bits=out_bits, outs=da)
            return d3[count - 1] + (da[count - 1][1],)
        modes["two_sequences"] = reference

    def one_call():
        eng.render_sequence_planar_rgba(frames, bits=bits, out_bits=out_bits, bleed=a.bleed, outs=d4)
        return d4[count - 1]
    modes["rgbap_sequence"] = one_call
    if a.only:
        if a.only not in modes:
            raise SystemExit(f"--only: {a.only} not in {sorted(modes)}")
        modes = {a.only: modes[a.only]}
    elif a.bleed == 0 or a.pair == "8/8":
        want = [p.copy() for p in reference()]
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(want, one_call())), "the one-call route differs from the route it replaces"
    runs = []
    for _ in range(2):
        for _ in range(a.warmup):
            for f in modes.values():
                f()
        times = {name: [] for name in modes}
        for _ in range(a.calls):
            for name, f in modes.items():
                t0 = time.perf_counter()
                f()
                times[name].append((time.perf_counter() - t0) * 1e3 / count)
        runs.append(times)
    res = {name: {"ms_median": round(statistics.median(runs[0][name] + runs[1][name]), 3), "ms_median_run1": round(statistics.median(runs[0][name]), 3),
                  "ms_median_run2": round(statistics.median(runs[1][name]), 3), "ms_min": round(min(runs[0][name] + runs[1][name]), 3),
                  "ms_max": round(max(runs[0][name] + runs[1][name]), 3)} for name in modes}
    for buf in held:
        eng.free_host(buf)
    eng.close()
    px, opx, b, ob = W * H, W * S * H * S, np.dtype(dt).itemsize, np.dtype(odt).itemsize
    nbytes = {"rgbap_sequence": {"up": 4 * px * b, "down": 4 * opx * ob}, "rgba_sequence": {"up": 4 * px, "down": 4 * opx}, "two_sequences": {"up": 6 * px * b, "down": 6 * opx * ob}}
    print(json.dumps({"tool": "planar_rgba_bench", "workload": f"config 3: {MODEL} x{S} noise{NOISE} batch{BATCH} tile{TILE} fp16, blend 1/16, {W}x{H} -> {W * S}x{H * S}, planar RGBA "
                      f"{a.pair} bits, bleed {a.bleed}, sequences of {count} frames host to host in page-locked buffers, per frame; two runs of {a.calls} calls per mode, each after "
                      f"{a.warmup} warm-up rounds, modes timed in turns; median of each run and of both", "bytes_per_frame": {k: v for k, v in nbytes.items() if k in res}, "results": res}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
