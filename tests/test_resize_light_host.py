"""Resize in linear light without a device: the host statement of the two curve functions (w2x_light_decode / w2x_light_encode) against the rule
written independently in numpy (tests/light_ref.py), the exact end points, the round trip of every code at 8 to 16 bits, the entries of
include/w2x/c_api_resize_light.h on a null and a never-loaded engine, the wrapper, and --resize-light on the command line - through `w2x --print-config` and
through the stand-alone sanitizer driver `make asan` builds (w2x_parse_check, plain g++, its own main - never through Python)."""
import ctypes as C
import importlib
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import light_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "waifu2x-tensorrt_amd")
W2X = os.path.join(PKG, "w2x")
CHECK = os.path.join(PKG, "w2x_parse_check")
BASE = ["--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "2", "--tileSize", "64"]
ENTRIES = {"w2x_set_resize_light", "w2x_get_resize_light", "w2x_light_decode", "w2x_light_encode", "w2x_resize_planes"}
CURVES = ("srgb", "bt709")


@pytest.fixture(scope="module")
def engine_module(pkg):
    return importlib.import_module("waifu2x-tensorrt_amd.engine")


def host(pkg, fn, mode, values):
    f = getattr(pkg.lib(), fn)
    m = pkg.RESIZE_LIGHTS[mode]
    return np.array([f(m, float(v)) for v in values], np.float32)


# ---- the two functions
@pytest.mark.parametrize("mode", CURVES)
def test_host_curves_against_numpy(pkg, mode):
    """fp32 with a stated log2 / exp2 chain against float64: a few ulp of the value.  decode's error is relative to a base >= 0.09 (2^-24 / 0.09 times the exponent);
    encode's is that of the power.  1e-6 absolute on values in [0, 1] is 8 fp32 ulp at 1 and far below half a 16-bit code (7.6e-6)."""
    t, k, a, g = ref.CURVES[mode]
    e = np.concatenate([np.linspace(0, 1, 4097), [t, np.nextafter(np.float32(t), 0), np.nextafter(np.float32(t), 1), 1e-6, 1 - 1e-6]]).astype(np.float32)
    d = host(pkg, "w2x_light_decode", mode, e)
    err_d = float(np.abs(d.astype(np.float64) - ref.decode(e.astype(np.float64), mode)).max())
    l = np.concatenate([np.linspace(0, 1, 4097), [t / k, np.nextafter(np.float32(t / k), 0), np.nextafter(np.float32(t / k), 1), 1e-7, 1 - 1e-6]]).astype(np.float32)
    c = host(pkg, "w2x_light_encode", mode, l)
    err_e = float(np.abs(c.astype(np.float64) - ref.encode(l.astype(np.float64), mode)).max())
    print(f"LIGHT host {mode}: decode max error {err_d:.3e}, encode max error {err_e:.3e}")
    assert err_d <= 1e-6 and err_e <= 1e-6
    # monotonic over the grid, the toe's end included
    assert (np.diff(d[:4097]) >= 0).all() and (np.diff(c[:4097]) >= 0).all()
    # the wrapper is the same entry; values outside [0, 1] and NaN are clamped first
    assert pkg.light_decode(mode, 0.5) == float(d[2048]) and pkg.light_encode(mode, 0.5) == float(c[2048])
    assert pkg.light_decode(mode, -3.0) == 0.0 and pkg.light_decode(mode, 7.0) == 1.0 and pkg.light_encode(mode, float("nan")) == 0.0


def test_end_points_are_exact_and_gamma_is_the_identity(pkg):
    for mode in CURVES:
        assert pkg.light_decode(mode, 0.0) == 0.0 and pkg.light_decode(mode, 1.0) == 1.0
        assert pkg.light_encode(mode, 0.0) == 0.0 and pkg.light_encode(mode, 1.0) == 1.0
    for v in (0.0, 0.25, 0.7, 1.0):
        assert pkg.light_decode("gamma", v) == np.float32(v) and pkg.light_encode("gamma", v) == np.float32(v)
    assert math.isnan(pkg.light_decode(3, 0.5)) and math.isnan(pkg.light_encode(-1, 0.5)) and math.isnan(pkg.light_decode("pq", 0.5))
    # the known answer of the issue: a 0 / 1 pattern averages to light 0.5, which sRGB encodes as code 188
    assert round(pkg.light_encode("srgb", 0.5) * 255) == 188 and round(ref.encode(0.5, "srgb") * 255) == 188


@pytest.mark.parametrize("bits", [8, 10, 12, 16])
@pytest.mark.parametrize("mode", CURVES)
def test_every_code_survives_the_round_trip(pkg, mode, bits):
    """encode(decode(c / q)) rounds back to c: a constant frame is unchanged by a resize in linear light"""
    q = (1 << bits) - 1
    codes = np.arange(q + 1)
    e = (codes.astype(np.float32) / np.float32(q)).astype(np.float32)
    L, m = pkg.lib(), pkg.RESIZE_LIGHTS[mode]
    back = np.array([L.w2x_light_encode(m, L.w2x_light_decode(m, float(v))) for v in e], np.float32)
    got = np.rint(back.astype(np.float32) * np.float32(q)).astype(np.int64)
    assert (got == codes).all(), (mode, bits, codes[got != codes][:8])
    # and in the numpy float32 model of the rule
    model = np.rint(ref.encode(ref.decode(e, mode, np.float32), mode, np.float32) * np.float32(q)).astype(np.int64)
    assert (model == codes).all()


# ---- the C entries
def declared(header):
    hdr = open(os.path.join(ROOT, "include", "w2x", header)).read()
    return set(re.findall(r"\b(w2x_[a-z0-9_]+)\s*\(", hdr[hdr.index('extern "C"'):]))


def test_header_library_and_table_agree(pkg, engine_module):
    names = declared("c_api_resize_light.h")
    assert names == ENTRIES == set(engine_module.RESIZE_LIGHT_SYMBOLS) == set(pkg.RESIZE_LIGHT_SYMBOLS)
    raw = C.CDLL(pkg.lib_path)
    for n in names:
        assert hasattr(raw, n), f"libw2x.so does not export {n}"
    for other in ("c_api.h", "c_api_gray.h", "c_api_planar.h", "c_api_rgbap.h", "c_api_yuv_resized.h", "c_api_yuv_siting.h", "c_api_dither.h"):
        assert not names & declared(other), other
    hdr = open(os.path.join(ROOT, "include", "w2x", "c_api_resize_light.h")).read()
    assert [int(re.search(rf"#define W2X_LIGHT_{k} (\d)", hdr).group(1)) for k in ("GAMMA", "SRGB", "BT709")] == [0, 1, 2]
    assert engine_module.RESIZE_LIGHTS == {"gamma": 0, "srgb": 1, "bt709": 2}
    # the header states the constants the reference uses
    for mode in CURVES:
        for c in ref.CURVES[mode][:3]:
            assert repr(c) in hdr, (mode, c)


def test_set_and_get_before_load(pkg):
    L, eng = pkg.lib(), pkg.Img2Img()
    assert L.w2x_set_resize_light(None, 1) == 0 and L.w2x_get_resize_light(None) == -1
    assert eng.messages == []
    assert eng.resize_light() == "gamma"
    assert eng.set_resize_light("srgb") is True and eng.resize_light() == "srgb"
    assert L.w2x_set_resize_light(eng._h, 2) == 1 and L.w2x_get_resize_light(eng._h) == 2 and eng.resize_light() == "bt709"
    for bad in (3, -1, 99):
        del eng.messages[:]
        assert L.w2x_set_resize_light(eng._h, bad) == 0
        assert len(eng.messages) == 1 and eng.messages[0][0] == 1 and f"Unknown resize light {bad}" in eng.messages[0][1] and eng.messages[0][1].startswith("[setResizeLight@")
        assert eng.resize_light() == "bt709"
    with pytest.raises(ValueError):
        eng.set_resize_light("pq")
    assert eng.resize_light() == "bt709"
    assert eng.set_resize_light("gamma") is True and eng.resize_light() == "gamma"
    # the dither setting is another setting
    assert eng.set_dither("ordered", 3, 1) and eng.set_resize_light("srgb") and eng.dither() == ("ordered", 3, 1) and eng.resize_light() == "srgb"
    # the test hook on a null and on a never-loaded engine
    src = [np.zeros((8, 12), np.float32) for _ in range(3)]
    dst = [np.zeros((4, 6), np.uint8) for _ in range(3)]
    planes = lambda ps: (C.c_void_p * 3)(*[q.ctypes.data for q in ps])
    steps = lambda ps: (C.c_size_t * 3)(*[q.strides[0] for q in ps])
    del eng.messages[:]
    assert L.w2x_resize_planes(None, planes(src), steps(src), 8, 12, planes(dst), steps(dst), 4, 6, 8, 0) == 0 and eng.messages == []
    assert L.w2x_resize_planes(eng._h, planes(src), steps(src), 8, 12, planes(dst), steps(dst), 4, 6, 8, 0) == 0
    assert len(eng.messages) == 1 and eng.messages[0][1].startswith("[resizePlanes@") and "before a successful load" in eng.messages[0][1]
    del eng.messages[:]
    assert L.w2x_resize_planes(eng._h, planes(src), steps(src), 8, 12, planes(dst), steps(dst), 4, 6, 8, 7) == 0
    assert len(eng.messages) == 1 and "Unknown resize filter 7" in eng.messages[0][1]
    for bad in ((src[:2], (4, 6), 8), ([q.astype(np.float64) for q in src], (4, 6), 8), (src, (4, 6), 9), (src, (4, 6), 8, "lanczos")):
        with pytest.raises(ValueError):
            eng.resize_planes(*bad)
    eng.close()


# ---- the command line
def w2x(*args):
    return subprocess.run([W2X, *args], capture_output=True, text=True)


def test_resize_light_is_parsed_and_printed(tmp_path):
    png = tmp_path / "page.png"
    png.write_bytes(b"")                                           # --print-config stops after parsing: the file only has to exist
    plain = json.loads(w2x(*BASE, "render", "-i", str(png), "--outscale", "2", "--print-config").stdout)
    assert plain["resize_light"] == "gamma"
    assert json.loads(w2x(*BASE, "render", "-i", str(png), "--print-config").stdout)["resize_light"] == "gamma"
    for mode in ("gamma", "srgb", "bt709", "sRGB", "BT709"):
        r = w2x(*BASE, "render", "-i", str(png), "--outscale", "2", "--resize-light", mode, "--print-config")
        assert r.returncode == 0, r.stderr
        cfg = json.loads(r.stdout)
        assert cfg["resize_light"] == mode.lower() and cfg["outputs"] == plain["outputs"] and cfg["suffix"] == plain["suffix"]
    cfg = json.loads(w2x(*BASE, "render", "-i", str(png), "--outsize", "300x200", "--resize-light=bt709", "--resize-filter", "bilinear", "--print-config").stdout)
    assert cfg["resize_light"] == "bt709" and cfg["resize_filter"] == "bilinear"
    # every route that takes --outscale / --outsize takes it
    for extra in (("--outscale", "2.5"), ("--outsize", "300x200"), ("--outscale", "3", "--deep"), ("--outsize", "300x200", "--gray"),
                  ("--outsize", "300x200", "--colorspace", "bt709"), ("--outsize", "300x200", "--colorspace", "bt2020", "--pix_fmt", "yuv420p10le", "--chroma-loc", "topleft"),
                  ("--outsize", "300x200", "--rgb-in", "gbrp10le", "--rgb-out", "gbrp"), ("--outsize", "300x200", "--rgba-in", "gbrap", "--rgba-out", "gbrap12le"),
                  ("--outscale", "2", "--alpha-bleed", "4"), ("--outscale", "2", "--dither", "ordered")):
        r = w2x(*BASE, "render", "-i", str(png), "--resize-light", "srgb", *extra, "--print-config")
        assert r.returncode == 0 and json.loads(r.stdout)["resize_light"] == "srgb", (extra, r.stderr)
    assert json.loads(w2x(*BASE, "build", "--print-config").stdout)["resize_light"] == "gamma"


@pytest.mark.parametrize("extra,command,starts", [
    (("--resize-light", "srgb"), "render", "--resize-light: needs --outscale or --outsize"),
    (("--resize-light", "gamma"), "render", "--resize-light: needs --outscale or --outsize"),
    (("--outscale", "2", "--resize-light", "pq"), "render", "--resize-light:"),
    (("--outscale", "2", "--resize-light", ""), "render", "--resize-light:"),
    (("--outscale", "2", "--resize-light"), "render", "--resize-light:"),
    (("--resize-light", "srgb"), "build", "--resize-light: only with render")])
def test_parse_errors_name_the_option(tmp_path, extra, command, starts):
    png = tmp_path / "page.png"
    png.write_bytes(b"")
    args = [*BASE, command] + (["-i", str(png)] if command == "render" else []) + [*extra, "--print-config"]
    r = w2x(*args)
    assert r.returncode != 0 and r.stderr.startswith(starts), (r.returncode, r.stderr)
    assert r.stdout == ""


def test_help_lists_the_option():
    r = w2x("--help")
    assert r.returncode == 0 and "--resize-light TEXT [gamma]" in r.stdout and "{gamma,srgb,bt709}" in r.stdout
    assert r.stdout.index("--resize-filter") < r.stdout.index("--resize-light") < r.stdout.index("--colorspace TEXT")


# ---- the option parser under ASan + UBSan: the stand-alone driver, built by `make asan`
@pytest.fixture(scope="module")
def check():
    r = subprocess.run(["make", "-C", PKG, "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return lambda *a: subprocess.run([CHECK, *a], capture_output=True, text=True)


def test_sanitizer_driver_parses_the_option(check, tmp_path):
    png = tmp_path / "page.png"
    png.write_bytes(b"")
    r = check("args", *BASE, "render", "-i", str(png), "--outsize", "300x200", "--resize-light", "bt709")
    assert r.returncode == 0 and json.loads(r.stdout[4:])["resize_light"] == "bt709", r.stderr
    r = check("args", *BASE, "render", "-i", str(png), "--outscale", "2", "--resize-light", "pq")
    assert r.returncode == 2 and "--resize-light" in r.stderr
    r = check("args", *BASE, "render", "-i", str(png), "--resize-light", "srgb")
    assert r.returncode == 2 and "needs --outscale or --outsize" in r.stderr
