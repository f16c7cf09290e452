"""Chained renders without a device: w2x_chain_plan - the one place the size rules live - against a few lines of Python, the entries of
include/w2x/c_api_chain.h against libw2x.so and engine.CHAIN_SYMBOLS, their refusals on null and never-loaded engines, the wrapper's own refusals, and
--chain / --chain-noise / --chain-quantize on the command line, through `w2x --print-config` and through the sanitizer build of the parser (w2x_parse_check)."""
import ctypes as C
import itertools
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W2X = os.path.join(ROOT, "waifu2x-tensorrt_amd", "w2x")
BASE = ["--model", "cunet/art", "--scale", "2", "--noise", "1", "--batchSize", "2", "--tileSize", "64"]
ENTRIES = {"w2x_chain_plan", "w2x_render_chained", "w2x_render_chained_resized", "w2x_render_sequence_chained", "w2x_render_sequence_chained_resized",
           "w2x_render_chained_planes", "w2x_render_chained_planes_resized"}


def declared(header):
    hdr = open(os.path.join(ROOT, "include", "w2x", header)).read()
    return set(re.findall(r"\b(w2x_[a-z0-9_]+)\s*\(", hdr[hdr.index('extern "C"'):]))


@pytest.fixture(scope="module")
def engine_module(pkg):
    import importlib
    return importlib.import_module("waifu2x-tensorrt_amd.engine")


# ---- the plan
def plan_ref(rows, cols, scalings, size):
    """the rules in Python: (refusal name or None, stages, canvas, target, S)"""
    n = len(scalings)
    if not 2 <= n <= 4:
        return "count", None
    if any(not 1 <= s <= 4 for s in scalings):
        return "scaling", None
    if rows <= 0 or cols <= 0:
        return "source", None
    stages, r, c, S = [(rows, cols)], rows, cols, 1
    for s in scalings:
        r, c, S = r * s, c * s, S * s
        if r > 65536 or c > 65536:
            return "too_large", None
        stages.append((r, c))
    tr, tc = (r, c) if size is None else size
    if not (rows <= tr <= r and cols <= tc <= c):
        return "target", None
    if tr * 4 < r or tc * 4 < c:
        return "shrink", None
    return None, {"stages": stages[:-1], "canvas": stages[-1], "target": (tr, tc), "scale": S}


def test_chain_plan_against_python(pkg):
    sizes = [(70, 90), (1, 1), (480, 854), (9000, 5)]
    chains = [[2, 2], [2, 4], [4, 4], [1, 2], [2, 2, 2], [2, 1, 4], [2, 2, 2, 2], [4, 4, 4, 4], [2], [], [2, 2, 2, 2, 2], [2, 5], [0, 2], [2, -1]]
    seen = set()
    for (rows, cols), sc in itertools.product(sizes, chains):
        S = int(np.prod(sc)) if sc else 1
        targets = [None, (rows, cols), (rows * S, cols * S), (rows * S // 4, cols * S), (rows * S, max(cols * S // 4 - 1, 1)), (rows - 1, cols), (rows, cols * S + 1),
                   (int(rows * 2.25), int(cols * 2.25)), (rows * 3, cols)]
        for size in targets:
            why, want = plan_ref(rows, cols, sc, size)
            seen.add(why)
            if size is not None and (size[0] <= 0 or size[1] <= 0):
                continue
            if why is None:
                assert pkg.chain_plan(rows, cols, sc, size) == want, (rows, cols, sc, size)
            else:
                with pytest.raises(ValueError, match=f"chain refused: {why}$"):
                    pkg.chain_plan(rows, cols, sc, size)
    assert seen >= {None, "count", "scaling", "too_large", "target", "shrink"}
    for bad in ((0, 9), (9, 0), (-3, 9)):
        with pytest.raises(ValueError, match="chain refused: source$"):
            pkg.chain_plan(*bad, [2, 2])
    assert pkg.chain_plan(480, 854, [2, 2], (1080, 1920)) == {"stages": [(480, 854), (960, 1708)], "canvas": (1920, 3416), "target": (1080, 1920), "scale": 4}
    assert pkg.chain_plan(70, 90, [2, 2, 2, 2])["scale"] == 16 and pkg.chain_plan(70, 90, [2, 2, 2, 2])["canvas"] == (1120, 1440)


def test_chain_plan_through_the_c_entry(pkg):
    L = pkg.lib()
    out = (C.c_int * 16)(*([-7] * 16))
    sc = (C.c_int * 3)(2, 4, 2)
    assert L.w2x_chain_plan(10, 20, sc, 3, 0, 0, out) == 0
    assert list(out)[:11] == [10, 20, 20, 40, 80, 160, 160, 320, 160, 320, 16] and list(out)[11:] == [-7] * 5
    out = (C.c_int * 16)(*([-7] * 16))
    for args, code in (((10, 20, sc, 1, 0, 0), 1), ((10, 20, sc, 5, 0, 0), 1), ((10, 20, None, 3, 0, 0), 1), ((0, 20, sc, 3, 0, 0), 3), ((10, 20, sc, 3, 9, 20), 5),
                       ((10, 20, sc, 3, 39, 320), 6), ((10, 5000, sc, 3, 0, 0), 4), ((10, 20, (C.c_int * 3)(2, 8, 2), 3, 0, 0), 2)):
        assert L.w2x_chain_plan(*args, out) == code, (args[:2], args[3:], code)
        assert list(out) == [-7] * 16, "a refused plan wrote"
    assert L.w2x_chain_plan(10, 20, sc, 3, 0, 0, None) != 0
    assert pkg.CHAIN_REFUSALS == {1: "count", 2: "scaling", 3: "source", 4: "too_large", 5: "target", 6: "shrink"}
    hdr = open(os.path.join(ROOT, "include", "w2x", "c_api_chain.h")).read()
    for code, name in pkg.CHAIN_REFUSALS.items():
        assert re.search(rf"#define W2X_CHAIN_{name.upper()} {code}\b", hdr), name


# ---- the header, the library and the wrapper's table name the same entries
def test_header_library_and_table_agree(pkg, engine_module):
    names = declared("c_api_chain.h")
    assert names == ENTRIES == set(engine_module.CHAIN_SYMBOLS) == set(pkg.CHAIN_SYMBOLS)
    raw = C.CDLL(pkg.lib_path)
    for n in names:
        assert hasattr(raw, n), f"libw2x.so does not export {n}"
    exported = subprocess.run(["nm", "-D", "--defined-only", pkg.lib_path], capture_output=True, text=True) if shutil.which("nm") else None
    if exported is not None and exported.returncode == 0:
        assert {s for s in re.findall(r"\bT (w2x_[a-z0-9_]+)", exported.stdout) if "chain" in s} == names
    for other in ("c_api.h", "c_api_gray.h", "c_api_planar.h", "c_api_rgbap.h", "c_api_yuv_resized.h", "c_api_yuv_siting.h", "c_api_dither.h", "c_api_resize_light.h"):
        assert not names & declared(other), other
    for tab in ("SYMBOLS", "EXPORTED_SYMBOLS", "GRAY_SYMBOLS", "PLANAR_SYMBOLS", "RGBAP_SYMBOLS", "YUV_RESIZED_SYMBOLS", "YUV_SITED_SYMBOLS", "DITHER_SYMBOLS", "RESIZE_LIGHT_SYMBOLS"):
        assert not names & set(getattr(engine_module, tab)), tab
    assert not any(w in n for n in names for w in ("planar", "gray", "rgbap")), "those words belong to the tables of their headers"
    L = pkg.lib()
    for n, (restype, argtypes) in engine_module.CHAIN_SYMBOLS.items():
        assert getattr(L, n).restype is restype and list(getattr(L, n).argtypes) == argtypes, n
    assert '#include "c_api.h"' in open(os.path.join(ROOT, "include", "w2x", "c_api_chain.h")).read()


# ---- refusals that need no device
def test_c_entries_refuse_null_and_unloaded_engines(pkg):
    L = pkg.lib()
    a, b = pkg.Img2Img(), pkg.Img2Img()
    f = np.zeros((4, 6, 3), np.uint8)
    d = np.full((16, 24, 3), 0x5A, np.uint8)
    two = (C.c_void_p * 2)(a._h, b._h)
    frame = (f.ctypes.data, 4, 6, f.strides[0], d.ctypes.data, d.strides[0], 8, 0)
    assert L.w2x_render_chained(None, 2, *frame) == 0
    assert L.w2x_render_chained((C.c_void_p * 2)(a._h, None), 2, *frame) == 0 and not a.messages
    assert L.w2x_render_chained(two, 0, *frame) == 0 and not a.messages
    for count, text in ((1, "2 to 4 stages"), (2, "before a successful load (engine 0)")):
        n = len(a.messages)
        assert L.w2x_render_chained(two, count, *frame) == 0
        assert text in a.messages[-1][1] and len(a.messages) == n + 1 and not b.messages, a.messages
    assert "[renderChained@" in a.last_error()
    five = (C.c_void_p * 5)(*[a._h] * 5)
    assert L.w2x_render_chained(five, 5, *frame) == 0 and "2 to 4 stages" in a.last_error()
    planes = lambda arrs: (C.c_void_p * 3)(*[p.ctypes.data for p in arrs])
    steps = lambda arrs: (C.c_size_t * 3)(*[p.strides[0] for p in arrs])
    sp, dp = [np.zeros((4, 6), np.uint8) for _ in range(3)], [np.zeros((16, 24), np.uint8) for _ in range(3)]
    assert L.w2x_render_chained_planes(two, 2, planes(sp), steps(sp), 4, 6, 8, planes(dp), steps(dp), 16, 24, 8, 0) == 0 and "engine 0" in a.last_error()
    assert L.w2x_render_chained_planes_resized(two, 2, planes(sp), steps(sp), 4, 6, 8, planes(dp), steps(dp), 16, 24, 8, 0, 9) == 0 and "Unknown resize filter 9" in a.last_error()
    assert L.w2x_render_chained_resized(two, 2, f.ctypes.data, 4, 6, f.strides[0], d.ctypes.data, 16, 24, d.strides[0], 8, 0, -1) == 0 and "Unknown resize filter -1" in a.last_error()
    ptrs = (C.c_void_p * 1)(f.ctypes.data)
    outs = (C.c_void_p * 1)(d.ctypes.data)
    assert L.w2x_render_sequence_chained(two, 2, ptrs, 4, 6, f.strides[0], outs, d.strides[0], -1, 0) == 0
    assert L.w2x_render_sequence_chained(two, 2, None, 4, 6, f.strides[0], outs, d.strides[0], 1, 0) == 0
    assert L.w2x_render_sequence_chained(two, 2, ptrs, 4, 6, f.strides[0], outs, d.strides[0], 1, 0) == 0 and "[renderSequenceChained@" in a.last_error()
    assert L.w2x_render_sequence_chained_resized(two, 2, ptrs, 4, 6, f.strides[0], outs, 16, 24, d.strides[0], 1, 0, 5) == 0 and "Unknown resize filter 5" in a.last_error()
    assert (d == 0x5A).all(), "a refused call wrote"
    a.close()
    b.close()


def test_wrappers_refuse_bad_arguments(pkg):
    a, b = pkg.Img2Img(), pkg.Img2Img()
    f = np.zeros((4, 6, 3), np.uint8)
    for engines in ([a], [], [a] * 5, (a, None), [a, "b"], None, a):
        with pytest.raises(ValueError, match="2 to 4 open Img2Img engines"):
            pkg.render_chained(engines, f)
        with pytest.raises(ValueError, match="2 to 4 open Img2Img engines"):
            pkg.render_chained_planar(engines, (f[..., 0], f[..., 1], f[..., 2]))
    with pytest.raises(ValueError, match="src must be a uint8"):
        pkg.render_chained([a, b], f.astype(np.float32))
    with pytest.raises(ValueError, match="src must be a uint8"):
        pkg.render_chained_resized([a, b], f[..., :2], (8, 12))
    with pytest.raises(ValueError, match="filter must be one of"):
        pkg.render_chained_resized([a, b], f, (8, 12), filter="lanczos")
    with pytest.raises(ValueError, match="dst must be a packed"):
        pkg.render_chained_resized([a, b], f, (8, 12), dst=np.zeros((8, 13, 3), np.uint8))
    with pytest.raises(ValueError, match="frames must be packed uint8"):
        pkg.render_sequence_chained([a, b], [f, f[:3]])
    with pytest.raises(ValueError, match="planes must be three 2-D arrays"):
        pkg.render_chained_planar([a, b], (f[..., 0], f[..., 1]))
    with pytest.raises(ValueError, match="out_bits must be one of"):
        pkg.render_chained_planar([a, b], tuple(np.zeros((4, 6), np.uint8) for _ in range(3)), out_bits=9)
    assert pkg.render_sequence_chained([a, b], []) == []
    # engines that were never loaded: the library refuses, through engines[0]'s messages
    with pytest.raises(pkg.W2xError, match="before a successful load"):
        pkg.render_chained([a, b], f)
    assert pkg.render_chained([a, b], f, dst=np.zeros((4, 6, 3), np.uint8)) is False and not b.messages
    with pytest.raises(pkg.W2xError, match="before a successful load"):
        pkg.render_chained_planar([a, b], tuple(np.zeros((4, 6), np.uint8) for _ in range(3)), (8, 12))
    c = pkg.Img2Img()
    c.close()
    with pytest.raises(ValueError, match="open Img2Img engines"):
        pkg.render_chained([a, c], f)
    assert a._scaling == 0, "the planar wrapper leaves the engine's scale factor as it found it"
    a.close()
    b.close()


# ---- the command line
def w2x(*args):
    return subprocess.run([W2X, *args], capture_output=True, text=True, cwd=ROOT)


@pytest.fixture(scope="module")
def png(tmp_path_factory):
    p = tmp_path_factory.mktemp("chain_cli") / "in.png"
    p.write_bytes(b"")                                              # (--print-config stops after parsing: the path only has to exist)
    return p


def test_chain_options_parse(pkg, png):
    plain = json.loads(w2x(*BASE, "render", "-i", str(png), "--print-config").stdout)
    assert (plain["chain"], plain["chain_noise"], plain["chain_quantize"], plain["chain_model_path"]) == (1, -1, False, None) and "chain" not in plain["suffix"]
    c = json.loads(w2x(*BASE, "render", "-i", str(png), "--chain", "2", "--print-config").stdout)
    assert (c["chain"], c["chain_noise"], c["chain_quantize"]) == (2, -1, False)
    assert c["model_path"] == "models/cunet/art/noise1_scale2x.onnx" and c["chain_model_path"] == "models/cunet/art/scale2x.onnx"
    assert c["suffix"] == "(cunet_art)(noise1)(scale2)(chain2)" and c["outputs"][0].endswith("in(cunet_art)(noise1)(scale2)(chain2).png")
    c = json.loads(w2x(*BASE, "render", "-i", str(png), "--chain=3", "--chain-noise", "1", "--chain-quantize", "--tta", "--outscale", "2.25", "--print-config").stdout)
    assert (c["chain"], c["chain_noise"], c["chain_quantize"], c["chain_model_path"]) == (3, 1, True, "models/cunet/art/noise1_scale2x.onnx")
    assert c["suffix"] == "(cunet_art)(noise1)(scale2)(chain3)(outscale2.25)(tta)"
    c = json.loads(w2x(*BASE, "render", "-i", str(png), "--chain", "2", "--outsize", "1920x1080", "--rgb-in", "gbrp10le", "--dither", "ordered", "--print-config").stdout)
    assert c["suffix"] == "(cunet_art)(noise1)(scale2)(chain2)(1920x1080)" and c["rgb_in"] == "gbrp10le"
    assert json.loads(w2x(*BASE, "build", "--chain", "4", "--print-config").stdout)["chain"] == 4
    for scale in ("3", "4"):                                          # --outscale ranges up to scale^N with a chain ...
        r = w2x(*BASE, "render", "-i", str(png), "--chain", "2", "--outscale", scale, "--print-config")
        assert r.returncode == 0, r.stderr
    r = w2x(*BASE, "render", "-i", str(png), "--outscale", "3", "--print-config")   # ... and to --scale without, as ever
    assert r.returncode != 0 and "--outscale: 3 not in [1, 2]" in r.stderr
    # the cunet x4 error stays as it is
    r = w2x("--model", "cunet/art", "--scale", "4", "--noise", "1", "--batchSize", "2", "--tileSize", "64", "render", "-i", str(png), "--chain", "2", "--print-config")
    assert r.returncode != 0 and "cunet/art does not support scale factor 4." in r.stderr


REFUSED = [
    (["--chain", "1"], "--chain: 1 not in"), (["--chain", "5"], "--chain: 5 not in"), (["--chain", "two"], "--chain"),
    (["--chain", "2", "--chain-noise", "4"], "--chain-noise: 4 not in"), (["--chain-noise", "1"], "--chain-noise: needs --chain"),
    (["--chain-quantize"], "--chain-quantize: needs --chain"),
    (["--chain", "2", "--colorspace", "bt709"], "--chain: not together with --colorspace"), (["--chain", "2", "--gray"], "--chain: not together with --gray"),
    (["--chain", "2", "--rgba-in", "gbrap"], "--chain: not together with --rgba-in"), (["--chain", "2", "--rgba-out", "gbrap"], "--chain: not together with --rgba-out"),
    (["--chain", "2", "--alpha-bleed", "2"], "--chain: not together with --alpha-bleed"), (["--chain", "2", "--devices", "2"], "--chain: not with --devices 2"),
    (["--chain", "2", "--outscale", "4.5"], "--outscale: 4.5 not in [1, 4]"), (["--chain", "3", "--outscale", "1.5"], "--outscale: 1.5 is below a quarter of the chain's factor 8"),
]


@pytest.mark.parametrize("extra,text", REFUSED)
def test_chain_options_refused(pkg, png, extra, text):
    r = w2x(*BASE, "render", "-i", str(png), *extra, "--print-config")
    assert r.returncode != 0 and text in r.stderr, (extra, r.stderr)


def test_chain_needs_a_scaling_model(pkg, png):
    r = w2x("--model", "cunet/art", "--scale", "1", "--noise", "1", "--batchSize", "2", "--tileSize", "64", "render", "-i", str(png), "--chain", "2", "--print-config")
    assert r.returncode != 0 and "--chain: needs --scale 2 or 4" in r.stderr


def test_chain_options_through_the_sanitizer_build(pkg, png):
    """the same parser under AddressSanitizer and UBSan (make asan: w2x_parse_check args ...)"""
    pkg_dir = os.path.join(ROOT, "waifu2x-tensorrt_amd")
    check = os.path.join(pkg_dir, "w2x_parse_check")
    if not os.path.exists(check):
        subprocess.run(["make", "-C", pkg_dir, "asan"], check=True, capture_output=True)
    run = lambda *args: subprocess.run([check, "args", *args], capture_output=True, text=True, cwd=ROOT)
    r = run(*BASE, "render", "-i", str(png), "--chain", "3", "--chain-noise", "0", "--chain-quantize", "--outsize", "400x300")
    assert r.returncode == 0 and r.stdout.startswith("ok: "), r.stdout + r.stderr
    c = json.loads(r.stdout[4:])
    assert (c["chain"], c["chain_noise"], c["chain_quantize"], c["suffix"]) == (3, 0, True, "(cunet_art)(noise1)(scale2)(chain3)(400x300)")
    for extra, text in REFUSED:
        r = run(*BASE, "render", "-i", str(png), *extra)
        assert text in r.stdout + r.stderr and "ERROR: " not in r.stderr and not r.stdout.startswith("ok: "), (extra, r.stdout, r.stderr)
    r = run(*BASE, "render", "-i", str(png), "--chain")
    assert "--chain: 1 required value missing" in r.stdout + r.stderr
