"""YUV 4:2:0 frames at config 3 (1080p, swin_unet/art x4 noise 3, batch 4, tile 256, blend 1/16): host frame in -> host frame out through
renderSequence (bgr24, 1920x1080 -> 7680x4320) and through renderSequenceYuv at 8/8 and 10/10 bits (BT.709 limited), all with engine-owned
page-locked buffers.  Median ms per frame over --regions timed regions of --steps frames each, after warm-up; one JSON line on stdout.

--outsize WxH renders every mode to that raster instead of the x4 one (renderSequenceResized for bgr24, renderSequenceYuvResized for the YUV modes,
bicubic): 3840x2160 is the 1080p -> 2160p case of DESIGN 9c.

The device time of gather_yuv_kernel / compose_yuv_kernel comes from a separate run of this script under `rocprofv3 --kernel-trace --stats`;
--bytes prints the bytes each path moves across PCIe per frame.  Not part of bench.py.

--in-layout / --out-layout {i420,i422,i444,nv12} give the YUV modes' frames another layout on either side (renderSequenceYuv through
w2x_render_sequence_yuv_layout; with both i420, the default, the call is w2x_render_sequence_yuv as before).  With --outsize the call is
w2x_render_sequence_yuv_layout_resized (with both i420 w2x_render_sequence_yuv_resized as before): `--outsize 3840x2160 --in-layout nv12 --out-layout
nv12 --modes 8/8` is the nv12 -> nv12 pair of profiles/yuv_resize_layouts/.

--siting {left,center,topleft} gives the YUV modes' frames that chroma siting on both sides.  "left", the default, changes nothing about the calls
above; the others go through w2x_render_sequence_yuv_sited (at the x4 raster as well: there it is the plain sequence)."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, S, MODEL, NOISE, BATCH, TILE, BLEND = 1920, 1080, 4, "swin_unet/art", 3, 4, 256, 0.0625


def frame_bytes(mode: str, ow: int = W * S, oh: int = H * S, lin: str = "i420", lout: str = "i420") -> dict:
    """bytes per frame uploaded and downloaded: bgr24 3 samples per pixel, 4:2:0 (i420, nv12) 1.5, 4:2:2 2, 4:4:4 3; 10-bit samples take 2 bytes"""
    if mode == "bgr24":
        return {"up": W * H * 3, "down": ow * oh * 3}
    bps = 2 if mode == "10/10" else 1
    chroma = lambda w, h, l: 2 * (w * h if l == "i444" else ((w + 1) // 2) * (h if l == "i422" else (h + 1) // 2))
    return {"up": (W * H + chroma(W, H, lin)) * bps, "down": (ow * oh + chroma(ow, oh, lout)) * bps}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8, help="frames per timed region")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--work", default=os.path.join(tempfile.gettempdir(), "w2x_yuv_bench"), help="where the synthetic model and its engine file go")
    ap.add_argument("--modes", default="bgr24,8/8,10/10")
    ap.add_argument("--outsize", default="", help="WxH: render to this raster (between 1920x1080 and 7680x4320) instead of the x4 one")
    ap.add_argument("--in-layout", default="i420", choices=["i420", "i422", "i444", "nv12"], help="the layout of the YUV modes' input frames")
    ap.add_argument("--out-layout", default="i420", choices=["i420", "i422", "i444", "nv12"], help="the layout of the YUV modes' output frames")
    ap.add_argument("--siting", default="left", choices=["left", "center", "topleft"], help="the chroma siting of the YUV modes' frames, both sides")
    ap.add_argument("--bytes", action="store_true", help="print the bytes per frame of each mode and exit (no GPU)")
    a = ap.parse_args()
    OW, OH = (int(v) for v in a.outsize.split("x")) if a.outsize else (W * S, H * S)
    resized = (OW, OH) != (W * S, H * S)
    LIN, LOUT = a.in_layout, a.out_layout
    with_layout = (LIN, LOUT) != ("i420", "i420")
    if a.bytes:
        print(json.dumps({m: frame_bytes(m, OW, OH, LIN, LOUT) for m in a.modes.split(",")}))
        return 0
    import ctypes as C
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

    def pinned_planes(rows, cols, bits, layout="i420"):
        """the layout's planes as views into one alloc_host buffer (the buffer first, to free it)"""
        dt = np.dtype(np.uint8 if bits == 8 else np.uint16)
        shapes = pkg.engine.yuv_layout_plane_shapes(rows, cols, layout) if with_layout else pkg.engine.yuv_plane_shapes(rows, cols)
        buf = eng.alloc_host((sum(r * c for r, c in shapes) * dt.itemsize,))
        planes, o = [], 0
        for r, c in shapes:
            planes.append(buf[o:o + r * c * dt.itemsize].view(dt).reshape(r, c)); o += r * c * dt.itemsize
        return buf, planes

    res = {}
    for mode in a.modes.split(","):
        bufs = []
        if mode == "bgr24":
            pf = eng.alloc_host(frame.shape); pf[...] = frame; bufs.append(pf)
            ring = [eng.alloc_host((OH, OW, 3)) for _ in range(3)]; bufs += ring

            def region():
                if resized:
                    eng.render_sequence_resized([pf] * n, (OH, OW), outs=[ring[k % 3] for k in range(n)])
                else:
                    eng.render_sequence([pf] * n, outs=[ring[k % 3] for k in range(n)])
        else:
            bits = 10 if mode == "10/10" else 8
            import yuv_ref   # (tests/yuv_ref.py: the frame's planes)
            if with_layout:
                import yuv_layout_ref   # (tests/yuv_layout_ref.py)
                src = yuv_layout_ref.encode(frame[..., ::-1] / 255.0, LIN, matrix="bt709", bits=bits)
            else:
                src = yuv_ref.encode(frame[..., ::-1] / 255.0, matrix="bt709", bits=bits)
            buf, planes = pinned_planes(H, W, bits, LIN); bufs.append(buf)
            for p, q in zip(planes, src):
                p[...] = q
            outs = []
            for _ in range(3):
                b, o = pinned_planes(OH, OW, bits, LOUT); bufs.append(b); outs.append(o)
            three = lambda vals, fill: list(vals) + [fill] * (3 - len(vals))     # (an nv12 frame: two planes, the third pointer NULL)
            sp = (C.c_void_p * (3 * n))(*[q for _ in range(n) for q in three([p.ctypes.data for p in planes], None)])
            dp = (C.c_void_p * (3 * n))(*[q for k in range(n) for q in three([p.ctypes.data for p in outs[k % 3]], None)])
            ss = (C.c_size_t * 3)(*three([p.strides[0] for p in planes], 0))
            ds = (C.c_size_t * 3)(*three([p.strides[0] for p in outs[0]], 0))

            def region():
                args = (eng._h, sp, ss, H, W, bits, dp, ds, OH, OW, bits, n, 1, 0)
                if a.siting != "left":
                    sid = pkg.YUV_SITINGS[a.siting]
                    sargs = (*args[:6], pkg.YUV_LAYOUTS[LIN], sid, *args[6:11], pkg.YUV_LAYOUTS[LOUT], sid, *args[11:])
                    if not eng._L.w2x_render_sequence_yuv_sited(*sargs, 0):
                        raise SystemExit("render_sequence_yuv_sited failed: " + eng.last_error())
                    return
                if with_layout:
                    largs = (*args[:6], pkg.YUV_LAYOUTS[LIN], *args[6:11], pkg.YUV_LAYOUTS[LOUT], *args[11:])
                    if not (eng._L.w2x_render_sequence_yuv_layout_resized(*largs, 0) if resized else eng._L.w2x_render_sequence_yuv_layout(*largs)):
                        raise SystemExit("render_sequence_yuv_layout failed: " + eng.last_error())
                    return
                if not (eng._L.w2x_render_sequence_yuv_resized(*args, 0) if resized else eng._L.w2x_render_sequence_yuv(*args)):
                    raise SystemExit("render_sequence_yuv failed: " + eng.last_error())
        for _ in range(a.warmup):
            region()
        times = []
        for _ in range(a.regions):
            t0 = time.perf_counter()
            region()
            times.append((time.perf_counter() - t0) * 1e3 / n)
        res[mode] = {"ms_per_frame_median": round(statistics.median(times), 4), "ms_per_frame": [round(t, 4) for t in times], "bytes": frame_bytes(mode, OW, OH, LIN, LOUT)}
        for b in bufs:
            eng.free_host(b)
    eng.close()
    layouts = (f", {LIN} in -> {LOUT} out" if with_layout else "") + (f", chroma sited {a.siting}" if a.siting != "left" else "")
    print(json.dumps({"tool": "yuv_bench", "workload": f"{MODEL} x{S} noise{NOISE} batch{BATCH} tile{TILE} fp16, {W}x{H} -> {OW}x{OH} frames, blend 1/16, "
                      f"{'renderSequenceResized (bgr24) / renderSequenceYuvResized' if resized else 'renderSequence (bgr24) / renderSequenceYuv'} (BT.709 limited, in/out bits{layouts}) host to host, page-locked buffers, "
                      f"{a.regions} regions x {n} frames after {a.warmup} warm-up regions", "results": res}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
