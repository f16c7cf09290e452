"""Edge modes without a device: the rule (w2x_edge_index) against its statement in numpy (tests/edge_ref.py) and against np.pad, the tap table
under a mode against the un-truncated table, the host bleed under a mode, the entries of include/w2x/c_api_edge.h on a null and a never-loaded engine, the
refusals that need no device, and --edge on the command line - through `w2x --print-config` and through the stand-alone sanitizer driver `make asan` builds
(w2x_parse_check, plain g++, its own main - never through Python)."""
import ctypes as C
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import edge_ref as ref
import rgba_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "waifu2x-tensorrt_amd")
W2X = os.path.join(PKG, "w2x")
CHECK = os.path.join(PKG, "w2x_parse_check")
BASE = ["--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "2", "--tileSize", "64"]
ENTRIES = {"w2x_set_edge", "w2x_get_edge", "w2x_edge_index", "w2x_resize_weights_edge", "w2x_alpha_bleed_edge", "w2x_alpha_bleed_planes_edge"}
SIZES = (1, 2, 3, 17)


@pytest.fixture(scope="module")
def engine_module(pkg):
    return importlib.import_module("waifu2x-tensorrt_amd.engine")


# ---- 1, 2. the rule
@pytest.mark.parametrize("mode", ref.MODES)
def test_edge_index_against_the_rule(pkg, mode):
    """i from far below 0 to far above n - many periods, so the rule folds more than once - at n = 1, 2, 3, 17"""
    for n in SIZES:
        i = np.arange(-7 * n - 40, 8 * n + 41)
        got = np.array([pkg.edge_index(mode, int(v), n) for v in i])
        want = ref.index(mode, i, n)
        assert (got == want).all(), (mode, n, i[got != want][:8])
        assert got.min() >= 0 and got.max() <= n - 1
        assert (got[(i >= 0) & (i < n)] == i[(i >= 0) & (i < n)]).all()          # inside the frame: the identity
        for far in (-2 ** 40 - 3, 2 ** 40 + 5, -2 ** 31, 2 ** 31 - 1):
            assert pkg.edge_index(mode, far, n) == int(ref.index(mode, far, n)), (mode, n, far)
    # the known answers of the statement
    assert [pkg.edge_index("mirror", v, 5) for v in (-1, 5, -4, 8, -5, 9)] == [1, 3, 4, 0, 3, 1]
    assert [pkg.edge_index("wrap", v, 5) for v in (-1, 5, -6, 11)] == [4, 0, 4, 1]
    assert [pkg.edge_index("replicate", v, 5) for v in (-9, 5, 99)] == [0, 4, 4]


@pytest.mark.parametrize("mode", ref.MODES)
def test_numpy_pad_agrees_with_the_rule(pkg, mode):
    for n in SIZES:
        a = np.arange(100, 100 + n)
        for pad in (1, n, 3 * n + 2):
            if mode == "mirror" and n == 1:
                continue                                                         # (np.pad refuses to reflect a single sample; the rule gives 0)
            want = np.pad(a, pad, mode=ref.NP_PAD[mode])
            got = a[[pkg.edge_index(mode, i, n) for i in range(-pad, n + pad)]]
            assert (got == want).all(), (mode, n, pad)
            assert (a[ref.index(mode, np.arange(-pad, n + pad), n)] == want).all()
    assert pkg.edge_index("mirror", -3, 1) == 0 and pkg.edge_index("mirror", 4, 1) == 0


def test_unknown_modes_and_sizes(pkg):
    L = pkg.lib()
    for bad in (3, -1, 99):
        assert L.w2x_edge_index(bad, 0, 5) == -1
    assert L.w2x_edge_index(1, 0, 0) == -1 and L.w2x_edge_index(1, 0, -4) == -1
    with pytest.raises(ValueError):
        pkg.edge_index("clamp", 0, 5)


# ---- 3, 4. the tap table
RATIOS = [(100, 75), (101, 76), (64, 32), (71, 36), (128, 32), (99, 25), (17, 17), (5, 4)]


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
@pytest.mark.parametrize("mode", ["wrap", "mirror"])
def test_tap_table_against_the_reference(pkg, mode, filt):
    """ratios 3/4, 1/2 and 1/4 (exact and ragged), the identity and a tiny canvas: full support for every output sample, rows that sum to 1"""
    for n_in, n_out in RATIOS:
        first, w = pkg.resize_weights(n_in, n_out, filt, edge=mode)
        rf, rw = ref.taps(n_in, n_out, filt)
        assert w.shape == rw.shape and (first == rf).all(), (n_in, n_out)
        assert np.abs(w.astype(np.float64) - rw).max() <= 2.0 ** -24, (n_in, n_out)           # the double weights rounded to fp32 once
        assert (w == rw.astype(np.float32)).all()
        assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() <= w.shape[1] * 2.0 ** -24
        if n_in != n_out or filt == "bicubic":                                                 # (the triangle at ratio 1 reaches no neighbour)
            assert first.min() < 0 and (first + w.shape[1]).max() > n_in                       # nothing is cut off at the border ...
        # ... so every row is the row of an interior sample: the same weights wherever the phase repeats
        if n_in % n_out == 0:
            assert (w == w[0]).all() and (np.diff(first) == n_in // n_out).all()
        # a table is the same for both modes: the mode only says where a tap reads
        other = pkg.resize_weights(n_in, n_out, filt, edge="mirror" if mode == "wrap" else "wrap")
        assert (other[0] == first).all() and (other[1] == w).all()


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
def test_replicate_table_is_resize_weights_to_the_bit(pkg, filt):
    for n_in, n_out in RATIOS:
        a, b = pkg.resize_weights(n_in, n_out, filt), pkg.resize_weights(n_in, n_out, filt, edge="replicate")
        assert (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes()
        assert np.abs(a[1].astype(np.float64).sum(1) - 1.0).max() <= a[1].shape[1] * 2.0 ** -24
        assert a[0].min() >= 0


def test_tap_table_refusals(pkg):
    L = pkg.lib()
    assert L.w2x_resize_weights_edge(10, 5, 0, 3, None, None, 0) == 0 and L.w2x_resize_weights_edge(10, 5, 0, -1, None, None, 0) == 0
    assert L.w2x_resize_weights_edge(0, 5, 0, 1, None, None, 0) == 0 and L.w2x_resize_weights_edge(10, 5, 2, 1, None, None, 0) == 0
    taps = L.w2x_resize_weights_edge(10, 5, 0, 1, None, None, 0)
    assert taps == 9
    first, w = np.zeros(5, np.int32), np.zeros((5, taps), np.float32)
    assert L.w2x_resize_weights_edge(10, 5, 0, 1, first.ctypes.data, w.ctypes.data, 5 * taps - 1) == -taps and not w.any()
    with pytest.raises(ValueError):
        pkg.resize_weights(10, 5, "bicubic", edge="clamp")


def test_the_table_resizes_like_the_padded_reference():
    """edge_ref's two statements check each other: the tap table read through the rule against torch on the np.pad'ed canvas (float64: rounding alone apart)"""
    rng = np.random.default_rng(5)
    canvas = rng.uniform(-0.05, 1.05, (23, 37, 3))
    for mode in ("wrap", "mirror", "replicate"):
        for size, filt in (((17, 28), "bicubic"), ((6, 10), "bilinear"), ((23, 19), "bicubic")):
            if mode == "replicate":
                continue                                                         # (torch on an edge-padded canvas is not the clipped table: the engine's Replicate is)
            a, b = ref.resized_by_taps(canvas, size, filt, mode), ref.resized(canvas, size, filt, mode)
            assert np.abs(a - b).max() <= 1e-12, (mode, size, filt)


# ---- 5. the host bleed
@pytest.mark.parametrize("mode", ref.MODES)
def test_host_bleed_under_a_mode(pkg, mode):
    """Wrap: rgba_ref.bleed of the frame extended by radius + 1 pixels per side through the rule, cropped.  Mirror and Replicate: the plain bleed."""
    differs = 0
    for name, bgr, alpha, radii in rgba_ref.cases():
        for radius in radii:
            got = pkg.alpha_bleed(bgr, alpha, radius, edge=mode)
            want = ref.bleed(bgr, alpha, radius, mode)
            assert np.array_equal(got, want), (mode, name, radius)
            plain = rgba_ref.bleed(bgr, alpha, radius)
            if mode == "wrap":
                differs += not np.array_equal(want, plain)
            else:
                assert np.array_equal(got, plain) and np.array_equal(got, pkg.alpha_bleed(bgr, alpha, radius))
    if mode == "wrap":
        assert differs >= 10                                                     # colour does cross the joint
    with pytest.raises(Exception):
        pkg.alpha_bleed(bgr, alpha, 17, edge=mode)
    with pytest.raises(ValueError):
        pkg.alpha_bleed(bgr, alpha, 1, edge="clamp")
    out = np.full_like(bgr, 7)
    assert pkg.lib().w2x_alpha_bleed_edge(bgr.ctypes.data, bgr.strides[0], alpha.ctypes.data, alpha.strides[0], bgr.shape[0], bgr.shape[1], 1, out.ctypes.data, out.strides[0], 3) == 0
    assert (out == 7).all()


@pytest.mark.parametrize("bits", [8, 10, 16])
def test_host_bleed_of_planes_under_wrap(pkg, bits):
    """the planes' bleed is the interleaved one's arithmetic: at 8 bits against edge_ref, deeper against itself on the wrapped frame extended and cropped"""
    rng = np.random.default_rng(bits)
    rows, cols, radius = 21, 33, 3
    dt = np.uint8 if bits == 8 else np.uint16
    planes = [rng.integers(0, 1 << bits, (rows, cols)).astype(dt) for _ in range(3)]
    alpha = (rng.integers(0, 1 << bits, (rows, cols)) * (rng.random((rows, cols)) < 0.15)).astype(dt)
    got = pkg.alpha_bleed_planes(planes + [alpha], radius, bits=bits, edge="wrap")
    p = radius + 1
    ext = [np.ascontiguousarray(ref.extend(q, "wrap", p)) for q in planes + [alpha]]
    want = [q[p:-p, p:-p] for q in pkg.alpha_bleed_planes(ext, radius, bits=bits)]
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert not all(np.array_equal(a, b) for a, b in zip(got, pkg.alpha_bleed_planes(planes + [alpha], radius, bits=bits)))
    for mode in ("mirror", "replicate"):
        assert all(np.array_equal(a, b) for a, b in zip(pkg.alpha_bleed_planes(planes + [alpha], radius, bits=bits, edge=mode), pkg.alpha_bleed_planes(planes + [alpha], radius, bits=bits)))
    if bits == 8:
        bgr = np.ascontiguousarray(np.stack(planes[::-1], -1))
        assert np.array_equal(np.stack(got[::-1], -1), ref.bleed(bgr, alpha, radius, "wrap"))


# ---- 6. the C entries
def declared(header):
    hdr = open(os.path.join(ROOT, "include", "w2x", header)).read()
    return set(re.findall(r"\b(w2x_[a-z0-9_]+)\s*\(", hdr[hdr.index('extern "C"'):]))


def test_header_library_and_table_agree(pkg, engine_module):
    names = declared("c_api_edge.h")
    assert names == ENTRIES == set(engine_module.EDGE_SYMBOLS) == set(pkg.EDGE_SYMBOLS)
    raw = C.CDLL(pkg.lib_path)
    for n in names:
        assert hasattr(raw, n), f"libw2x.so does not export {n}"
        assert not any(word in n for word in ("planar", "gray", "rgbap", "chain")), n          # those words belong to the tables of their headers
    for other in ("c_api.h", "c_api_gray.h", "c_api_planar.h", "c_api_rgbap.h", "c_api_yuv_resized.h", "c_api_yuv_siting.h", "c_api_dither.h", "c_api_resize_light.h", "c_api_chain.h"):
        assert not names & declared(other), other
    for tab in ("SYMBOLS", "EXPORTED_SYMBOLS", "GRAY_SYMBOLS", "PLANAR_SYMBOLS", "RGBAP_SYMBOLS", "YUV_RESIZED_SYMBOLS", "YUV_SITED_SYMBOLS", "DITHER_SYMBOLS", "RESIZE_LIGHT_SYMBOLS", "CHAIN_SYMBOLS"):
        assert not names & set(getattr(engine_module, tab)), tab
    hdr = open(os.path.join(ROOT, "include", "w2x", "c_api_edge.h")).read()
    assert '#include "c_api.h"' in hdr
    assert [int(re.search(rf"#define W2X_EDGE_{k} (\d)", hdr).group(1)) for k in ("REPLICATE", "WRAP", "MIRROR")] == [0, 1, 2]
    assert engine_module.EDGE_MODES == {"replicate": 0, "wrap": 1, "mirror": 2} == pkg.EDGE_MODES


def test_set_and_get_before_load(pkg):
    L, eng = pkg.lib(), pkg.Img2Img()
    assert L.w2x_set_edge(None, 1) == 0 and L.w2x_get_edge(None) == -1
    assert eng.messages == []
    assert eng.edge() == "replicate"
    assert eng.set_edge("wrap") is True and eng.edge() == "wrap"
    assert L.w2x_set_edge(eng._h, 2) == 1 and L.w2x_get_edge(eng._h) == 2 and eng.edge() == "mirror"
    for bad in (3, -1, 99):
        del eng.messages[:]
        assert L.w2x_set_edge(eng._h, bad) == 0
        assert len(eng.messages) == 1 and eng.messages[0][0] == 1 and f"Unknown edge mode {bad}" in eng.messages[0][1] and eng.messages[0][1].startswith("[setEdge@")
        assert eng.edge() == "mirror"
    with pytest.raises(ValueError):
        eng.set_edge("clamp")
    assert eng.edge() == "mirror"
    assert eng.set_edge("replicate") is True and eng.edge() == "replicate"
    # the other settings are other settings
    assert eng.set_dither("ordered", 3, 1) and eng.set_resize_light("srgb") and eng.set_edge("wrap")
    assert eng.dither() == ("ordered", 3, 1) and eng.resize_light() == "srgb" and eng.edge() == "wrap"
    eng.close()


# ---- 7. the refusals that need no device: they come before the engine looks at anything else, a missing load included
def test_refusals_before_load_name_set_edge(pkg):
    L, eng = pkg.lib(), pkg.Img2Img()
    src = np.zeros((8, 8, 3), np.uint8)
    dst = np.full((32, 32, 3), 9, np.uint8)
    y = np.zeros((8, 8), np.uint8); u = np.zeros((4, 4), np.uint8)
    oy = np.full((32, 32), 9, np.uint8); ou = np.full((16, 16), 9, np.uint8)
    planes = lambda ps: (C.c_void_p * 3)(*[q.ctypes.data for q in ps])
    steps = lambda ps: (C.c_size_t * 3)(*[q.strides[0] for q in ps])
    calls = {
        "renderStrip": lambda: L.w2x_render_strip(eng._h, src.ctypes.data, 8, 8, src.strides[0], dst.ctypes.data, dst.strides[0], 0, 2),
        "shardCompute": lambda: L.w2x_shard_compute(eng._h, src.ctypes.data, 8, 8, src.strides[0], 0, 2),
        "renderYuv": lambda: L.w2x_render_yuv(eng._h, planes([y, u, u]), steps([y, u, u]), 8, 8, 8, planes([oy, ou, ou]), steps([oy, ou, ou]), 32, 32, 8, 1, 0),
    }
    for mode in ("wrap", "mirror"):
        assert eng.set_edge(mode)
        for who, call in calls.items():
            del eng.messages[:]
            assert call() == 0, who
            assert len(eng.messages) == 1, (who, eng.messages)
            sev, text = eng.messages[0]
            assert sev == 1 and text.startswith(f"[{who}@") and f"setEdge({mode})" in text and "not built" in text, text
        assert (dst == 9).all() and (oy == 9).all() and (ou == 9).all()
    # under replicate the same calls meet the engine's usual first question
    assert eng.set_edge("replicate")
    for who, call in calls.items():
        del eng.messages[:]
        assert call() == 0
        assert len(eng.messages) == 1 and "setEdge" not in eng.messages[0][1] and "before a successful load" in eng.messages[0][1], (who, eng.messages)
    eng.close()


# ---- 8. the command line
def w2x(*args):
    return subprocess.run([W2X, *args], capture_output=True, text=True)


def test_edge_is_parsed_and_printed(tmp_path):
    png = tmp_path / "tile.png"
    png.write_bytes(b"")                                           # --print-config stops after parsing: the file only has to exist
    plain = json.loads(w2x(*BASE, "render", "-i", str(png), "--print-config").stdout)
    assert plain["edge"] == "replicate"
    for mode in ("replicate", "wrap", "mirror", "Wrap", "MIRROR"):
        r = w2x(*BASE, "render", "-i", str(png), "--edge", mode, "--print-config")
        assert r.returncode == 0, r.stderr
        cfg = json.loads(r.stdout)
        assert cfg["edge"] == mode.lower() and cfg["outputs"] == plain["outputs"] and cfg["suffix"] == plain["suffix"]
    assert json.loads(w2x(*BASE, "render", "-i", str(png), "--edge=wrap", "--print-config").stdout)["edge"] == "wrap"
    # every route of the RGB family takes it
    for extra in (("--outscale", "2.5"), ("--outsize", "300x200"), ("--deep",), ("--gray",), ("--outsize", "300x200", "--gray"),
                  ("--rgb-in", "gbrp10le", "--rgb-out", "gbrp"), ("--rgba-in", "gbrap", "--rgba-out", "gbrap12le"), ("--alpha-bleed", "4"),
                  ("--chain", "2"), ("--chain", "2", "--outscale", "6"), ("--outscale", "2", "--dither", "ordered", "--resize-light", "srgb"), ("--tta",)):
        r = w2x(*BASE, "render", "-i", str(png), "--edge", "wrap", *extra, "--print-config")
        assert r.returncode == 0 and json.loads(r.stdout)["edge"] == "wrap", (extra, r.stderr)
    assert json.loads(w2x(*BASE, "build", "--print-config").stdout)["edge"] == "replicate"


@pytest.mark.parametrize("extra,command,starts", [
    (("--edge", "clamp"), "render", "--edge:"),
    (("--edge", ""), "render", "--edge:"),
    (("--edge",), "render", "--edge:"),
    (("--edge", "wrap", "--outsize", "300x200", "--colorspace", "bt709"), "render", "--edge: not together with --colorspace"),
    (("--edge", "replicate", "--outsize", "300x200", "--colorspace", "bt709"), "render", "--edge: not together with --colorspace"),
    (("--edge", "wrap"), "build", "--edge: only with render")])
def test_parse_errors_name_the_option(tmp_path, extra, command, starts):
    png = tmp_path / "tile.png"
    png.write_bytes(b"")
    args = [*BASE, command] + (["-i", str(png)] if command == "render" else []) + [*extra, "--print-config"]
    r = w2x(*args)
    assert r.returncode != 0 and r.stderr.startswith(starts), (r.returncode, r.stderr)
    assert r.stdout == ""


def test_a_still_over_several_devices_is_a_parse_error(tmp_path):
    png = tmp_path / "tile.png"
    png.write_bytes(b"")
    r = w2x(*BASE, "--devices", "2", "render", "-i", str(png), "--edge", "mirror", "--print-config")
    assert r.returncode != 0 and r.stderr.startswith("--edge mirror: a still over --devices 2"), r.stderr
    assert w2x(*BASE, "--devices", "2", "render", "-i", str(png), "--edge", "replicate", "--print-config").returncode == 0


def test_help_lists_the_option():
    r = w2x("--help")
    assert r.returncode == 0 and "--edge TEXT [replicate]" in r.stdout and "{replicate,wrap,mirror}" in r.stdout
    assert r.stdout.index("--resize-light") < r.stdout.index("--edge TEXT") < r.stdout.index("--colorspace TEXT")


# ---- the option parser under ASan + UBSan: the stand-alone driver, built by `make asan`
@pytest.fixture(scope="module")
def check():
    r = subprocess.run(["make", "-C", PKG, "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return lambda *a: subprocess.run([CHECK, *a], capture_output=True, text=True)


def test_sanitizer_driver_parses_the_option(check, tmp_path):
    png = tmp_path / "tile.png"
    png.write_bytes(b"")
    r = check("args", *BASE, "render", "-i", str(png), "--outsize", "300x200", "--edge", "mirror")
    assert r.returncode == 0 and json.loads(r.stdout[4:])["edge"] == "mirror", r.stderr
    r = check("args", *BASE, "render", "-i", str(png), "--edge", "clamp")
    assert r.returncode == 2 and "--edge" in r.stderr
    r = check("args", *BASE, "render", "-i", str(png), "--edge", "wrap", "--outsize", "300x200", "--colorspace", "bt709")
    assert r.returncode == 2 and "--edge: not together with --colorspace" in r.stderr
