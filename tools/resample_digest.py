"""The bytes of every resize kernel's output, as digests: one line per case - the call, the filter, source and target size - with the sha256 of every output
plane.  Two builds of the library computed the same iff their outputs of this tool are the same file; run it on the commit before and after a change to the
resize kernels (k_resample.hip, k_resample_yuv.hip, the resample kernels of k_planar / k_rgba / k_planar_rgba.hip, pixel_device.h) on one machine and diff.

Engines as the GPU tests build them: the small synthetic swin_unet x4 (batch 2, tile 64, blend 1/16), and the same network with four times the gain in its image
head, whose canvas leaves [0, 1] under the bicubic filter, so that the clamp between the resize and the YUV coding cuts (tests/test_gpu_yuv_resize_layouts.py).
Sources: noise 45 x 57 and a smooth picture 50 x 66, the shapes of the suites, and 12 x 20 for the targets below one tile.  Targets, by what they reach:
    13 x 22, 15 x 61      below 16 rows and below 64 columns: one ragged tile
    45 x 57               the source size, one column tile; 57 ends one pixel into a four-pixel group
    47 x 65, 101 x 129, 51 x 193   one column past a tile boundary: the last tile is its halo-fed first chroma site alone; odd rows and columns (has_b / has_r)
    91 x 115, 90 x 114    three and two pixels into a group; odd x odd and even x even
    150 x 198, 175 x 250  the x3 and x3.5 targets of the suites
    180 x 228, 200 x 264  the full factor: with bicubic taps the largest rows_max
Calls, each with both filters: render_resized at 8 and 16 bits, render_yuv_resized at 8 and 10 bits out, render_yuv_layout_resized to NV12, P010, I422 and
I444, render_planar_resized 8 / 8, render_rgba_resized; then one call of each kind into a caller's dst that is a slice at an odd column of a wider array.  The
kernels write the engine's own device planes, whose rows are padded to 16 bytes, and the frame is copied out from there, so a caller's rows do not reach the
kernels' stores: their sample-by-sample paths are taken by the groups the right edge cuts and, BGR, by the rows of an odd width, whose rows are packed.
A few seconds on one GPU.  Not part of bench.py."""
from __future__ import annotations

import argparse
import hashlib
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

S, BATCH, TILE, BLEND = 4, 2, 64, 0.0625
FILTERS = ("bicubic", "bilinear")
TARGETS = {(45, 57): [(45, 57), (47, 65), (91, 115), (90, 114), (180, 228)],
           (50, 66): [(150, 198), (175, 250), (101, 129), (51, 193), (200, 264)],
           (12, 20): [(13, 22), (15, 61)]}


def sha(planes) -> str:
    import numpy as np
    planes = planes if isinstance(planes, (tuple, list)) else (planes,)
    return " ".join(hashlib.sha256(np.ascontiguousarray(p).tobytes()).hexdigest() for p in planes)


def picture(rows, cols, seed):
    """uint8 BGR: noise for the 45 x 57 source, smooth waves with a little noise for the others"""
    import numpy as np
    rng = np.random.default_rng(seed)
    if (rows, cols) == (45, 57):
        return rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    ph = rng.random(3) * 6.28
    img = np.stack([127.5 + 115.0 * np.sin(xx / (7 + 5 * k) + yy / (11 + 3 * k) + ph[k]) for k in range(3)], -1)
    return np.clip(np.rint(img + rng.integers(-3, 4, img.shape)), 0, 255).astype(np.uint8)


def yuv_source(bgr, bits):
    """4:2:0 planes of legal limited-range codes made from the picture's channels (any legal planes do: the digests compare two builds on the same input)"""
    import numpy as np
    dt, top = (np.uint8, 1) if bits == 8 else (np.uint16, 4)
    y = (16 + bgr[..., 1].astype(np.int64) * 219 // 255) * top
    u = (16 + bgr[::2, ::2, 0].astype(np.int64) * 224 // 255) * top
    v = (16 + bgr[::2, ::2, 2].astype(np.int64) * 224 // 255) * top
    return y.astype(dt), u.astype(dt), v.astype(dt)


def offset_view(shape, dtype):
    """a [rows, cols(, channels)] view that starts one sample (pixel) into the rows of a wider array: its rows are not 8-byte aligned"""
    import numpy as np
    big = np.zeros((shape[0], shape[1] + 5) + tuple(shape[2:]), dtype)
    return big[:, 1:1 + shape[1]]


def cases(eng, tag, sources, filters, out):
    import numpy as np
    for (r, c), targets in sources.items():
        bgr = picture(r, c, 7 * r + c)
        bgr16 = bgr.astype(np.uint16) * 257
        bgra = np.concatenate([bgr, picture(r, c, r + 3 * c)[..., :1]], -1)
        yuv8, yuv10 = yuv_source(bgr, 8), yuv_source(bgr, 10)
        rgb = tuple(np.ascontiguousarray(bgr[..., k]) for k in (2, 1, 0))
        for size in targets:
            for f in filters:
                name = f"{tag} {f} {r}x{c}->{size[0]}x{size[1]}"
                out(f"{name} bgr8", eng.render_resized(bgr, size, filter=f))
                out(f"{name} bgr16", eng.render_resized(bgr16, size, filter=f))
                out(f"{name} i420 8", eng.render_yuv_resized(*yuv8, size, filter=f))
                out(f"{name} i420 10", eng.render_yuv_resized(*yuv8, size, out_bits=10, filter=f))
                out(f"{name} i420 10 from 10", eng.render_yuv_resized(*yuv10, size, filter=f))
                for lay in ("nv12", "i422", "i444"):
                    for ob in (8, 10):
                        out(f"{name} {'p010' if (lay, ob) == ('nv12', 10) else lay} {ob}", eng.render_yuv_layout_resized(yuv8, size, out_layout=lay, out_bits=ob, filter=f))
                out(f"{name} planar 8/8", eng.render_planar_resized(rgb, size, filter=f))
                out(f"{name} rgba", eng.render_rgba_resized(bgra, size, filter=f))
                out(f"{name} rgba uniform", eng.render_rgba_resized(np.concatenate([bgr, np.full_like(bgr[..., :1], 200)], -1), size, skip_uniform_alpha=True, filter=f))


def dst_cases(eng, pkg_shapes, out):
    """one call of each kind into a caller's dst at an odd column of a wider array; pkg_shapes: the package's yuv_layout_plane_shapes"""
    import numpy as np
    r, c, size, f = 45, 57, (91, 115), "bicubic"
    bgr = picture(r, c, 7 * r + c)
    yuv8 = yuv_source(bgr, 8)
    name = f"dst+1 {f} {r}x{c}->{size[0]}x{size[1]}"

    def into(label, dst, call):
        assert call(dst), eng.last_error()
        out(f"{name} {label}", dst)
    into("bgr8", offset_view(size + (3,), np.uint8), lambda d: eng.render_resized(bgr, size, filter=f, dst=d))
    into("bgr16", offset_view(size + (3,), np.uint16), lambda d: eng.render_resized(bgr.astype(np.uint16) * 257, size, filter=f, dst=d))
    for ob, dt in ((8, np.uint8), (10, np.uint16)):
        into(f"i420 {ob}", tuple(offset_view(s, dt) for s in pkg_shapes(*size, "i420")), lambda d: eng.render_yuv_resized(*yuv8, size, out_bits=ob, filter=f, dst=d))
        for lay in ("nv12", "i422", "i444"):
            into(f"{lay} {ob}", tuple(offset_view(s, dt) for s in pkg_shapes(*size, lay)),
                 lambda d: eng.render_yuv_layout_resized(yuv8, size, out_layout=lay, out_bits=ob, filter=f, dst=d))
    rgb = tuple(np.ascontiguousarray(bgr[..., k]) for k in (2, 1, 0))
    into("planar 8/8", tuple(offset_view(size, np.uint8) for _ in range(3)), lambda d: eng.render_planar_resized(rgb, size, filter=f, dst=d))
    bgra = np.concatenate([bgr, picture(r, c, r + 3 * c)[..., :1]], -1)
    into("rgba", offset_view(size + (4,), np.uint8), lambda d: eng.render_rgba_resized(bgra, size, filter=f, dst=d))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default=os.path.join(tempfile.gettempdir(), "w2x_resample_digest"), help="where the synthetic models and their engine files go")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    import torch
    import synth_models as sm
    import __graft_entry__ as g
    pkg = g.package()
    lines = []

    def out(name, planes):
        lines.append(f"{name}: {sha(planes)}")
        print(lines[-1], flush=True)

    def engine(sub, seed, gain):
        net = sm.make_model("swin_unet/art", S, seed=seed, small=True)
        if gain != 1.0:
            with torch.no_grad():
                net.to_image.proj.weight.mul_(gain)
        path = sm.model_path(os.path.join(a.work, sub), "swin_unet/art", S, 3)
        sm.export_onnx(net, path, BATCH, TILE, dynamic=True)
        eng = pkg.Img2Img()
        if not eng.build(path, pkg.BuildConfig.fixed(BATCH, TILE)):
            raise SystemExit("build failed: " + eng.last_error())
        if not eng.load(path, pkg.RenderConfig(batchSize=BATCH, height=TILE, width=TILE, scaling=S, overlap=(BLEND, BLEND))):
            raise SystemExit("load failed: " + eng.last_error())
        return eng

    eng = engine("plain", 1237, 1.0)
    cases(eng, "swin", TARGETS, FILTERS, out)
    dst_cases(eng, pkg.yuv_layout_plane_shapes, out)
    eng.close()
    eng = engine("gain4", 1237, 4.0)       # the canvas leaves [0, 1]: the clamp between the resize and the coding cuts
    cases(eng, "gain4", {(50, 66): [(150, 198), (175, 250)]}, ("bicubic",), out)
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
