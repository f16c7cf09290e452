"""Planar RGB frames at config 3 (swin_unet/art x4 noise 3, batch 4, tile 256, blend 1/16, fp16, 1920 x 1080 -> 7680 x 4320): milliseconds per frame, host
frame in -> host frame out.
--group sequence (the default) times, per frame, 8 different frames in page-locked buffers (alloc_host; the outputs go to a ring of three page-locked buffers)
  bgr_sequence      render_sequence() of the interleaved 8-bit frames: the baseline
  planar_8_8 / planar_8_10 / planar_10_10 / planar_16_16 / planar_8_f32
                    render_sequence_planar() at that pair of depths (input / output; f32: float output, 4 bytes per sample down)
--group frames times the single calls from pageable numpy arrays
  bgr               render() of the interleaved frame
  interleaved       the route a caller of planar frames had before renderPlanar, restated here: np.stack of the planes into BGR, render(), the three planes
                    picked apart again
  planar_8_8 / planar_16_16 / planar_8_f32
                    render_planar()
Every call ends in the engine's stream synchronise, so a host clock around it is the call's time.  The modes are timed in turns (one call of each per round,
--calls rounds after --warmup rounds) and every figure is taken twice: the whole procedure - warm-up rounds, then the timed rounds - runs two times one after
the other in the process, and the median of each run is reported next to the median of both, so the spread between two runs of the same code stands beside
every difference between two routes.  One JSON line on stdout.

--only MODE runs that mode alone (for `rocprofv3 --kernel-trace --stats -- python tools/planar_bench.py --only planar_8_8`, which gives the device time of
gather_planes_kernel / compose_planes_kernel against gather_kernel / compose_kernel under --only bgr_sequence).  --resized renders to the x2 target instead
(the canvas compose and resample_planes_kernel against resample_kernel).  --bytes prints the bytes each mode moves across PCIe per frame and exits (no GPU).
Not part of bench.py."""
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

W, H, MODEL, BATCH, TILE = 1920, 1080, "swin_unet/art", 4, 256
S, NOISE, BLEND = 4, 3, 0.0625
PAIRS = {"planar_8_8": (8, 8), "planar_8_10": (8, 10), "planar_10_10": (10, 10), "planar_16_16": (16, 16), "planar_8_f32": (8, 32)}
GROUPS = {"sequence": ["bgr_sequence"] + list(PAIRS), "frames": ["bgr", "interleaved", "planar_8_8", "planar_16_16", "planar_8_f32"]}


def sample_bytes(bits: int) -> int:
    return 4 if bits == 32 else 2 if bits > 8 else 1


def route_bytes(factor: int = S) -> dict:
    """bytes per frame uploaded and downloaded by every mode, at an output of `factor` times the input"""
    px, opx = W * H, W * factor * H * factor
    d = {"bgr": {"up": 3 * px, "down": 3 * opx}}
    for name, (i, o) in PAIRS.items():
        d[name] = {"up": 3 * px * sample_bytes(i), "down": 3 * opx * sample_bytes(o)}
    return d


def picture(np, rows, cols, seed):
    """a colour frame: smooth shading, hard strokes and a little noise; [rows, cols, 3] uint8 BGR"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float32)
    img = np.stack([140.0 + 90.0 * np.sin(xx * (0.009 + 0.002 * c) + yy * (0.006 + 0.001 * c) + seed + c) for c in range(3)], axis=2)
    img[(xx.astype(np.int32) // 7 + yy.astype(np.int32) // 11 + seed) % 9 == 0] = 30.0
    return np.clip(img + rng.integers(-4, 5, img.shape), 0, 255).astype(np.uint8)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=8, help="timed calls per mode and run (at least 6; there are two runs)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--group", default="sequence", choices=sorted(GROUPS))
    ap.add_argument("--only", default="", help="run one mode of the group alone")
    ap.add_argument("--resized", action="store_true", help="render to the x2 target (1080p -> 2160p) instead of the scaled size")
    ap.add_argument("--work", default=os.path.join(tempfile.gettempdir(), "w2x_planar_bench"), help="where the synthetic model and its engine file go")
    ap.add_argument("--bytes", action="store_true", help="print the bytes per frame of each mode and exit (no GPU)")
    a = ap.parse_args()
    factor = 2 if a.resized else S
    if a.bytes:
        print(json.dumps({f"{W}x{H}": {"x4": route_bytes(), "x2": route_bytes(2)}}))
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
    size = (H * factor, W * factor)
    target = size if a.resized else None
    DT = {8: np.uint8, 10: np.uint16, 12: np.uint16, 16: np.uint16, 32: np.float32}

    def widen(plane, bits):
        """an 8-bit plane as codes of `bits`: the same picture at the wider depth"""
        return plane if bits == 8 else (plane.astype(np.uint32) * ((1 << bits) - 1) // 255).astype(np.uint16)

    def timed(r, per=1):
        """two times over, warm-up rounds and the modes in turns; per mode the median of each run and of both"""
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

    res, r, held, dsts = {}, {}, [], {}

    def host(shape, dtype):
        """a page-locked array of `dtype`"""
        buf = eng.alloc_host((int(np.prod(shape)) * np.dtype(dtype).itemsize,))
        held.append(buf)
        return buf.view(dtype).reshape(shape)

    if a.group == "sequence":
        count, ring = 8, 3
        pics = [picture(np, H, W, 10 + k) for k in range(count)]
        if "bgr_sequence" in modes:
            frames3 = [host((H, W, 3), np.uint8) for _ in range(count)]
            for f, p in zip(frames3, pics):
                f[...] = p
            outs3 = [host(size + (3,), np.uint8) for _ in range(ring)]
            d3 = [outs3[k % ring] for k in range(count)]
            r["bgr_sequence"] = (lambda: eng.render_sequence_resized(frames3, size, outs=d3)) if a.resized else (lambda: eng.render_sequence(frames3, d3))
        for name, (ib, ob) in PAIRS.items():
            if name not in modes:
                continue
            fr = [tuple(host((H, W), DT[ib]) for _ in range(3)) for _ in range(count)]
            for f, p in zip(fr, pics):
                for k in range(3):
                    f[k][...] = widen(p[..., 2 - k], ib)
            outs = [tuple(host(size, DT[ob]) for _ in range(3)) for _ in range(ring)]
            d = dsts[name] = [outs[k % ring] for k in range(count)]
            r[name] = lambda fr=fr, d=d, ib=ib, ob=ob: eng.render_sequence_planar(fr, target, bits=ib, out_bits=ob, outs=d)
        if "bgr_sequence" in r and "planar_8_8" in r and not a.only:      # the contract, once, before anything is timed
            r["bgr_sequence"](); r["planar_8_8"]()
            assert all(np.array_equal(dsts["planar_8_8"][count - 1][k], d3[count - 1][..., 2 - k]) for k in range(3)), "planar 8 / 8 differs from render_sequence()"
        res[f"{W}x{H} -> {size[1]}x{size[0]} x{count} page-locked, per frame"] = timed(r, per=count)
    else:
        pic = picture(np, H, W, 3)
        planes = {b: tuple(np.ascontiguousarray(widen(pic[..., 2 - k], b)) for k in range(3)) for b in (8, 16)}
        out3 = np.empty(size + (3,), np.uint8)
        outs = {b: tuple(np.empty(size, DT[b]) for _ in range(3)) for b in (8, 16, 32)}
        picked = tuple(np.empty(size, np.uint8) for _ in range(3))

        def bgr_call(frame):
            ok = eng.render_resized(frame, size, dst=out3) if a.resized else eng.render(frame, out3)
            assert ok, eng.last_error()

        def interleaved():
            bgr_call(np.stack(planes[8][::-1], axis=2))            # what a caller of the library had to write: interleave, render, pick the planes apart
            for k in range(3):
                picked[k][...] = out3[..., 2 - k]
            return picked

        def planar(ib, ob):
            ok = eng.render_planar_resized(planes[ib], size, out_bits=ob, dst=outs[ob]) if a.resized else eng.render_planar(planes[ib], out_bits=ob, dst=outs[ob])
            assert ok, eng.last_error()
            return outs[ob]
        every = {"bgr": lambda: bgr_call(pic), "interleaved": interleaved, "planar_8_8": lambda: planar(8, 8), "planar_16_16": lambda: planar(16, 16),
                 "planar_8_f32": lambda: planar(8, 32)}
        r = {m: every[m] for m in modes}
        if "interleaved" in r and "planar_8_8" in r:
            x = [p.copy() for p in interleaved()]
            assert all(np.array_equal(p, q) for p, q in zip(x, planar(8, 8))), "planar 8 / 8 differs from the interleaved route"
        res[f"{W}x{H} -> {size[1]}x{size[0]} pageable, per call"] = timed(r)
    for buf in held:
        eng.free_host(buf)
    eng.close()
    print(json.dumps({"tool": "planar_bench", "workload": f"config 3: {MODEL} x{S} noise{NOISE} batch{BATCH} tile{TILE} fp16, blend 1/16, {W}x{H} frames host to host "
                      f"({'page-locked buffers' if a.group == 'sequence' else 'pageable numpy arrays'}), group {a.group}{', resized to x2' if a.resized else ''}, two runs of "
                      f"{calls} calls per mode, each after {a.warmup} warm-up rounds, modes timed in turns; median of each run and of both",
                      "bytes_per_frame": route_bytes(factor), "results": res}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
