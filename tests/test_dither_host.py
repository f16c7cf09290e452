"""Dithered output without a device: the blue-noise table and its spectrum, dither_rank against the rule written independently in numpy
(tests/dither_ref.py), the plane and phase offsets, the entries of include/w2x/c_api_dither.h on a null and a never-loaded engine, the wrapper, --dither on the
command line (--print-config stops after parsing), and csrc/dither.cpp under ASan + UBSan through the stand-alone driver `make asan` builds (w2x_parse_check,
plain g++, its own main - never through Python)."""
import ctypes as C
import importlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dither_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "waifu2x-tensorrt_amd")
W2X = os.path.join(PKG, "w2x")
CHECK = os.path.join(PKG, "w2x_parse_check")
BASE = ["--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "2", "--tileSize", "64"]
ENTRIES = {"w2x_set_dither", "w2x_get_dither", "w2x_dither_table", "w2x_dither_rank", "w2x_dither_planes"}


@pytest.fixture(scope="module")
def engine_module(pkg):
    return importlib.import_module("waifu2x-tensorrt_amd.engine")


@pytest.fixture(scope="module")
def table(pkg):
    return pkg.dither_table("bluenoise")


# ---- the table
def test_table_is_a_permutation(pkg, table):
    assert table.shape == (64, 64) and table.dtype == np.uint16
    assert sorted(table.ravel().tolist()) == list(range(4096))
    bayer = pkg.dither_table("ordered")
    assert bayer.shape == (8, 8) and sorted(bayer.ravel().tolist()) == list(range(64))
    assert bayer[0].tolist() == [0, 32, 8, 40, 2, 34, 10, 42] and bayer[1].tolist() == [48, 16, 56, 24, 50, 18, 58, 26]
    for bad in ("none", "floyd", 0, 3, -1):
        with pytest.raises(ValueError):
            pkg.dither_table(bad)


def low_frequency_share(t):
    """mean of the power spectrum P of the mean-removed table over 0 < |f| < 0.125 cycles per pixel, over its mean over all non-zero frequencies"""
    a = t.astype(np.float64)
    P = np.abs(np.fft.fft2(a - a.mean())) ** 2
    f = np.fft.fftfreq(t.shape[0])
    r = np.hypot(f[:, None], f[None, :])
    return float(P[(r > 0) & (r < 0.125)].mean() / P[r > 0].mean())


def test_table_is_blue_noise(table):
    share = low_frequency_share(table)
    white = low_frequency_share(np.random.default_rng(1).permutation(4096).reshape(64, 64))
    print(f"DITHER table: low-frequency share {share:.6f}; a random permutation {white:.4f}")
    assert share <= 1 / 20
    assert white > 1 / 20                                          # the condition tells a white-noise table from this one


def test_table_is_what_the_generator_writes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "blue_noise.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- dither_rank: the closed form, the offsets
def test_ordered_rank_is_the_closed_form(pkg):
    for phase in (0, 1, 5, 2 ** 32 - 1):
        for c in range(3):
            want = ref.ranks("ordered", (19, 23), c, phase)
            got = np.array([[pkg.dither_rank("ordered", phase, c, x, y) for x in range(23)] for y in range(19)])
            assert (got == want).all(), (phase, c)


def test_plane_and_phase_offsets(pkg, table):
    B8 = pkg.dither_table("ordered").astype(np.int64)
    for phase in (0, 1, 7):
        for c in range(3):
            dx, dy = 17 * c + 23 * phase, 29 * c + 41 * phase
            for x, y in ((0, 0), (5, 9), (63, 64), (1000, 77)):
                assert pkg.dither_rank("bluenoise", phase, c, x, y) == int(table[(y + dy) & 63, (x + dx) & 63])
                assert pkg.dither_rank("ordered", phase, c, x, y) == int(B8[(y + dy) & 7, (x + dx) & 7])
    assert (ref.ranks("bluenoise", (70, 90), 2, 3, table) == np.array([[pkg.dither_rank(2, 3, 2, x, y) for x in range(90)] for y in range(70)])).all()
    for args in (("none", 0, 0, 0, 0), (3, 0, 0, 0, 0), ("ordered", 0, 3, 0, 0), ("ordered", 0, -1, 0, 0), ("bluenoise", 0, 0, -1, 0), ("bluenoise", 0, 0, 0, -1)):
        assert pkg.dither_rank(*args) == -1, args
    t = ref.thresholds("bluenoise", (64, 64), 0, 0, table)
    assert t.min() == np.float32(0.5 / 4096) and t.max() == np.float32(1 - 0.5 / 4096) and len(np.unique(t)) == 4096


# ---- the C entries
def declared(header):
    hdr = open(os.path.join(ROOT, "include", "w2x", header)).read()
    return set(re.findall(r"\b(w2x_[a-z0-9_]+)\s*\(", hdr[hdr.index('extern "C"'):]))


def test_header_library_and_table_agree(pkg, engine_module):
    names = declared("c_api_dither.h")
    assert names == ENTRIES == set(engine_module.DITHER_SYMBOLS) == set(pkg.DITHER_SYMBOLS)
    raw = C.CDLL(pkg.lib_path)
    for n in names:
        assert hasattr(raw, n), f"libw2x.so does not export {n}"
    for other in ("c_api.h", "c_api_gray.h", "c_api_planar.h", "c_api_rgbap.h", "c_api_yuv_resized.h", "c_api_yuv_siting.h"):
        assert not names & declared(other), other
    for tab in ("SYMBOLS", "EXPORTED_SYMBOLS", "GRAY_SYMBOLS", "PLANAR_SYMBOLS", "RGBAP_SYMBOLS", "YUV_RESIZED_SYMBOLS", "YUV_SITED_SYMBOLS"):
        assert not names & set(getattr(engine_module, tab)), tab
    hdr = open(os.path.join(ROOT, "include", "w2x", "c_api_dither.h")).read()
    assert [int(re.search(rf"#define W2X_DITHER_{k} (\d)", hdr).group(1)) for k in ("NONE", "ORDERED", "BLUENOISE")] == [0, 1, 2]
    assert engine_module.DITHER_MODES == {"none": 0, "ordered": 1, "bluenoise": 2}


def test_c_entries_refuse_a_null_engine_and_unknown_modes(pkg):
    L, eng = pkg.lib(), pkg.Img2Img()
    m, p, a = C.c_int(9), C.c_uint(9), C.c_uint(9)
    src = [np.zeros((4, 6), np.float32) for _ in range(3)]
    dst = [np.zeros((4, 6), np.uint8) for _ in range(3)]
    planes = lambda ps: (C.c_void_p * 3)(*[q.ctypes.data for q in ps])
    steps = lambda ps: (C.c_size_t * 3)(*[q.strides[0] for q in ps])
    # a null engine: 0, no message
    assert L.w2x_set_dither(None, 1, 0, 0) == 0 and L.w2x_get_dither(None, C.byref(m), C.byref(p), C.byref(a)) == 0
    assert L.w2x_dither_planes(None, planes(src), steps(src), 4, 6, planes(dst), steps(dst), 8) == 0
    assert eng.messages == []
    # the setting before load(): kept, read back, unknown modes refused with one message each and nothing changed
    assert eng.dither() == ("none", 0, 0)
    assert L.w2x_set_dither(eng._h, 2, 5, 1) == 1 and eng.dither() == ("bluenoise", 5, 1)
    assert L.w2x_get_dither(eng._h, C.byref(m), None, None) == 1 and m.value == 2
    for bad in (3, -1, 99):
        del eng.messages[:]
        assert L.w2x_set_dither(eng._h, bad, 0, 0) == 0
        assert len(eng.messages) == 1 and eng.messages[0][0] == 1 and f"Unknown dither mode {bad}" in eng.messages[0][1] and eng.messages[0][1].startswith("[setDither@")
        assert eng.dither() == ("bluenoise", 5, 1)
    assert eng.set_dither("ordered", 2 ** 32 - 1, 3) is True and eng.dither() == ("ordered", 2 ** 32 - 1, 3)
    with pytest.raises(ValueError):
        eng.set_dither("floyd")
    assert eng.set_dither("none") is True and eng.dither() == ("none", 0, 0)
    # the table entry: no engine; none and unknown modes: 0
    side = C.c_int(0)
    for bad in (0, 3, -1):
        assert L.w2x_dither_table(bad, None, C.byref(side)) == 0
    assert L.w2x_dither_table(1, None, C.byref(side)) == 1 and side.value == 8
    assert L.w2x_dither_table(2, None, None) == 1
    # the test hook on a never-loaded engine: the engine's own refusal
    del eng.messages[:]
    assert L.w2x_dither_planes(eng._h, planes(src), steps(src), 4, 6, planes(dst), steps(dst), 8) == 0
    assert len(eng.messages) == 1 and eng.messages[0][1].startswith("[ditherPlanes@") and "before a successful load" in eng.messages[0][1]
    for bad in ((src[:2], 8), ([q.astype(np.float64) for q in src], 8), (src, 9), (src, 32)):
        with pytest.raises(ValueError):
            eng.dither_planes(*bad)
    eng.close()


# ---- the command line
def w2x(*args):
    return subprocess.run([W2X, *args], capture_output=True, text=True)


def test_dither_options_are_parsed_and_printed(tmp_path):
    png = tmp_path / "sky.png"
    png.write_bytes(b"")                                           # --print-config stops after parsing: the file only has to exist
    r = w2x(*BASE, "render", "-i", str(png), "--print-config")
    assert r.returncode == 0, r.stderr
    plain = json.loads(r.stdout)
    assert plain["dither"] == "none" and plain["dither_temporal"] is False
    for mode in ("ordered", "bluenoise", "BlueNoise", "none"):
        cfg = json.loads(w2x(*BASE, "render", "-i", str(png), "--dither", mode, "--print-config").stdout)
        assert cfg["dither"] == mode.lower() and cfg["dither_temporal"] is False
        assert cfg["outputs"] == plain["outputs"] and cfg["suffix"] == plain["suffix"]
    cfg = json.loads(w2x(*BASE, "render", "-i", str(png), "--dither=ordered", "--dither-temporal", "--print-config").stdout)
    assert cfg["dither"] == "ordered" and cfg["dither_temporal"] is True
    # every route takes it: --deep, --gray, alpha options, raw video formats, --colorspace, --outsize / --outscale
    for extra in (("--deep",), ("--gray",), ("--alpha-bleed", "4", "--alpha-skip-uniform"), ("--rgb-in", "gbrp10le", "--rgb-out", "gbrp"), ("--rgba-in", "gbrap", "--rgba-out", "gbrap12le"),
                  ("--colorspace", "bt709"), ("--colorspace", "bt2020", "--pix_fmt", "yuv420p10le", "--outsize", "300x200"), ("--outscale", "2.5"), ("--devices", "2")):
        r = w2x(*BASE, "render", "-i", str(png), "--dither", "bluenoise", *extra, "--print-config")
        assert r.returncode == 0 and json.loads(r.stdout)["dither"] == "bluenoise", (extra, r.stderr)
    assert json.loads(w2x(*BASE, "build", "--print-config").stdout)["dither"] == "none"


@pytest.mark.parametrize("extra,command,starts", [
    (("--dither", "floyd"), "render", "--dither:"), (("--dither", ""), "render", "--dither:"), (("--dither",), "render", "--dither:"),
    (("--dither-temporal",), "render", "--dither-temporal:"), (("--dither", "none", "--dither-temporal"), "render", "--dither-temporal:"),
    (("--dither", "ordered"), "build", "--dither:"), (("--dither", "ordered", "--dither-temporal"), "build", "--dither-temporal:")])
def test_dither_parse_errors_name_the_option(tmp_path, extra, command, starts):
    png = tmp_path / "sky.png"
    png.write_bytes(b"")
    args = [*BASE, command] + (["-i", str(png)] if command == "render" else []) + [*extra, "--print-config"]
    r = w2x(*args)
    assert r.returncode != 0 and r.stderr.startswith(starts), (r.returncode, r.stderr)
    assert r.stdout == ""


def test_help_lists_the_options():
    r = w2x("--help")
    assert r.returncode == 0 and "--dither TEXT [none]" in r.stdout and "--dither-temporal" in r.stdout
    assert "{none,ordered,bluenoise}" in r.stdout and "Alpha and float output are never dithered" in r.stdout


# ---- dither.cpp under ASan + UBSan: the stand-alone driver, built by `make asan`
@pytest.fixture(scope="module")
def check():
    r = subprocess.run(["make", "-C", PKG, "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return lambda *a: subprocess.run([CHECK, *a], capture_output=True, text=True)


def test_sanitizer_driver_prints_the_rule(check, table):
    r = check("dither", "table")
    assert r.returncode == 0, r.stderr
    assert (np.array([[int(v) for v in line.split()] for line in r.stdout.splitlines()]) == table).all()
    for mode, phase, c, x0, y0, w, h in (("ordered", 0, 0, 0, 0, 8, 8), ("ordered", 5, 2, 3, 60, 37, 11), ("bluenoise", 1, 1, 50, 40, 70, 30), ("bluenoise", 4294967295, 2, 4000, 0, 100, 3)):
        r = check("dither", mode, str(phase), str(c), str(x0), str(y0), str(w), str(h))
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert lines[h] == "thresholds" and len(lines) == 2 * h + 1
        ranks = np.array([[int(v) for v in line.split()] for line in lines[:h]])
        thr = np.array([[float(v) for v in line.split()] for line in lines[h + 1:]])
        want = ref.ranks(mode, (y0 + h, x0 + w), c, phase, table)[y0:, x0:]
        assert (ranks == want).all(), (mode, phase, c)
        assert (thr == (want + 0.5) / ref.LEVELS[mode]).all()
    for bad in (("dither", "none", "0", "0", "0", "0", "4", "4"), ("dither", "floyd", "0", "0", "0", "0", "4", "4"), ("dither", "ordered", "0", "3", "0", "0", "4", "4"),
                ("dither", "ordered", "0", "0", "-1", "0", "4", "4"), ("dither", "ordered", "0", "0", "0", "0", "0", "4"), ("dither", "ordered", "0", "0", "0", "0", "4"),
                ("dither", "ordered", "0", "0", "0", "0", "5000", "4")):
        r = check(*bad)
        assert r.returncode == 2 and r.stderr.startswith("rejected:"), (bad, r.returncode, r.stderr)


def test_sanitizer_driver_parses_the_options(check, tmp_path):
    png = tmp_path / "sky.png"
    png.write_bytes(b"")
    r = check("args", *BASE, "render", "-i", str(png), "--dither", "ordered", "--dither-temporal")
    assert r.returncode == 0 and json.loads(r.stdout[4:])["dither"] == "ordered", r.stderr
    r = check("args", *BASE, "render", "-i", str(png), "--dither", "floyd")
    assert r.returncode == 2 and "--dither" in r.stderr
