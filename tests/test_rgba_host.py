"""RGBA frames on the host (no GPU): the colour bleed of w2x_alpha_bleed (tiles.cpp alpha_bleed) against its numpy statement (tests/rgba_ref.py), byte for
byte; the identities of the algorithm; the command line's --alpha-bleed / --alpha-skip-uniform; the C symbols; the sanitizer build's bleed mode."""
import json
import os
import subprocess

import numpy as np
import pytest

import rgba_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W2X = os.path.join(ROOT, "waifu2x-tensorrt_amd", "w2x")
BASE = ["--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "4", "--tileSize", "256"]


def test_the_two_statements_of_the_reference_agree():
    """padded shifts against plain loops, on the small cases (the loops are slow)"""
    for name, bgr, alpha, radii in rgba_ref.cases():
        if bgr.shape[0] * bgr.shape[1] > 64 * 64:
            continue
        for r in radii:
            if r > 5 and bgr.shape[0] * bgr.shape[1] > 17:
                continue
            assert np.array_equal(rgba_ref.bleed(bgr, alpha, r), rgba_ref.bleed_loops(bgr, alpha, r)), (name, r)


def test_the_cases_meet_every_neighbour_count():
    seen = set()
    for name, bgr, alpha, radii in rgba_ref.cases():
        seen |= rgba_ref.neighbour_counts(alpha)
    assert set(range(1, 9)) <= seen


def test_alpha_bleed_matches_the_reference(pkg):
    for name, bgr, alpha, radii in rgba_ref.cases():
        for r in radii:
            got = pkg.alpha_bleed(bgr, alpha, r)
            assert got.shape == bgr.shape and got.dtype == np.uint8
            ref = rgba_ref.bleed(bgr, alpha, r)
            assert np.array_equal(got, ref), f"{name} at radius {r}: {int((got != ref).sum())} bytes differ"


def test_alpha_bleed_identities(pkg):
    rng = np.random.default_rng(7)
    bgr = rng.integers(0, 256, (40, 52, 3), dtype=np.uint8)
    alpha = (rng.integers(0, 256, (40, 52), dtype=np.uint8) * (rng.random((40, 52)) < 0.3)).astype(np.uint8)
    assert np.array_equal(pkg.alpha_bleed(bgr, alpha, 0), bgr)                                          # R = 0 is the identity
    for r in (1, 7, 16):
        assert np.array_equal(pkg.alpha_bleed(bgr, np.zeros_like(alpha), r), bgr)                       # nothing known: nothing to spread
        assert np.array_equal(pkg.alpha_bleed(bgr, np.full_like(alpha, 3), r), bgr)                     # everything known
        out = pkg.alpha_bleed(bgr, alpha, r)
        assert np.array_equal(out[alpha > 0], bgr[alpha > 0])                                           # a known pixel never changes
    # a core out of reach keeps its colour: a hole of 40 x 40 at radius 5
    a = np.full((60, 60), 255, np.uint8); a[10:50, 10:50] = 0
    c = rng.integers(0, 256, (60, 60, 3), dtype=np.uint8)
    out = pkg.alpha_bleed(c, a, 5)
    assert np.array_equal(out[15:45, 15:45], c[15:45, 15:45]) and not np.array_equal(out[10:15, 10:50], c[10:15, 10:50])
    # the value of alpha does not matter beyond zero / non-zero
    assert np.array_equal(pkg.alpha_bleed(bgr, alpha, 4), pkg.alpha_bleed(bgr, ((alpha > 0) * 255).astype(np.uint8), 4))
    # one known pixel: its colour, exactly, everywhere within the radius (Chebyshev distance), nothing beyond
    a = np.zeros((30, 30), np.uint8); a[0, 0] = 9
    out = pkg.alpha_bleed(c[:30, :30].copy(), a, 6)
    assert (out[:7, :7] == c[0, 0]).all() and np.array_equal(out[7:], c[7:30, :30]) and np.array_equal(out[:, 7:], c[:30, 7:30])


def test_alpha_bleed_takes_padded_rows_and_refuses_bad_arguments(pkg):
    rng = np.random.default_rng(8)
    big = rng.integers(0, 256, (20, 40, 3), dtype=np.uint8)
    abig = (rng.integers(0, 2, (20, 40), dtype=np.uint8) * 255).astype(np.uint8)
    bgr, alpha = big[:, :25], abig[:, :31][:, :25]                           # row steps larger than the rows
    assert np.array_equal(pkg.alpha_bleed(bgr, alpha, 3), rgba_ref.bleed(np.ascontiguousarray(bgr), np.ascontiguousarray(alpha), 3))
    for r in (-1, 17, 1000):
        with pytest.raises(pkg.W2xError):
            pkg.alpha_bleed(np.ascontiguousarray(bgr), np.ascontiguousarray(alpha), r)
    with pytest.raises(pkg.W2xError):
        pkg.alpha_bleed(np.zeros((0, 4, 3), np.uint8), np.zeros((0, 4), np.uint8), 1)
    with pytest.raises(ValueError):
        pkg.alpha_bleed(np.ascontiguousarray(bgr), np.zeros((3, 3), np.uint8), 1)


def test_the_c_symbols_are_exported(pkg):
    L = pkg.lib()
    for name in ("w2x_render_rgba", "w2x_alpha_bleed_device", "w2x_alpha_bleed"):
        assert hasattr(L, name), name
    eng = pkg.Img2Img()
    assert hasattr(eng, "render_rgba") and hasattr(eng, "alpha_bleed_device")
    # an engine that was never loaded refuses with a message instead of touching a device
    assert eng.render_rgba(np.zeros((4, 4, 4), np.uint8), dst=np.zeros((4, 4, 4), np.uint8)) is False
    assert "before a successful load" in eng.last_error()
    eng.close()


# ---- the command line (cli/args.cpp; --print-config stops after parsing, no GPU)
def w2x(*args):
    assert os.path.exists(W2X), "w2x was not built"
    return subprocess.run([W2X, *args], capture_output=True, text=True, timeout=120)


def test_cli_alpha_options_in_print_config(pkg, tmp_path):
    png = tmp_path / "sprite.png"; png.write_bytes(b"x")
    r = w2x(*BASE, "render", "-i", str(png), "--print-config")
    assert r.returncode == 0, r.stderr
    cfg = json.loads(r.stdout)
    assert cfg["alpha_bleed"] == 0 and cfg["alpha_skip_uniform"] is False
    r = w2x(*BASE, "render", "-i", str(png), "--alpha-bleed", "16", "--alpha-skip-uniform", "--print-config")
    assert r.returncode == 0, r.stderr
    cfg = json.loads(r.stdout)
    assert cfg["alpha_bleed"] == 16 and cfg["alpha_skip_uniform"] is True
    assert cfg["outputs"] == [str(tmp_path / "sprite(swin_unet_art)(noise3)(scale4).png")]      # output names unchanged
    r = w2x(*BASE, "render", "-i", str(png), "--alpha-bleed=0", "--deep", "--print-config")          # a radius of 0 bleeds nothing: fine with --deep
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("extra,msg", [
    (["--alpha-bleed", "17"], "not in [0, 16]"),
    (["--alpha-bleed", "-1"], "not in [0, 16]"),
    (["--alpha-bleed", "four"], "not an integer"),
    (["--alpha-bleed"], "--alpha-bleed"),
    (["--alpha-bleed", "4", "--deep"], "not together with --deep"),
])
def test_cli_alpha_options_are_checked(pkg, tmp_path, extra, msg):
    png = tmp_path / "sprite.png"; png.write_bytes(b"x")
    r = w2x(*BASE, "render", "-i", str(png), *extra, "--print-config")
    assert r.returncode != 0 and msg in r.stderr, (r.returncode, r.stderr)


@pytest.mark.parametrize("extra", [["--alpha-bleed", "4"], ["--alpha-skip-uniform"]])
def test_cli_alpha_options_belong_to_render(pkg, extra):
    r = w2x(*BASE, "build", *extra, "--print-config")
    assert r.returncode != 0 and "only with render" in r.stderr, r.stderr


def test_cli_help_lists_the_alpha_options(pkg):
    r = w2x("--help")
    assert r.returncode == 0 and "--alpha-bleed" in r.stdout and "--alpha-skip-uniform" in r.stdout


def test_the_sanitizer_build_runs_alpha_bleed(pkg, tmp_path):
    """`make asan` covers alpha_bleed: w2x_parse_check bleed reads an image and bleeds it in exact-size buffers with padded rows"""
    Image = pytest.importorskip("PIL.Image")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "waifu2x-tensorrt_amd"), "asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    check = os.path.join(ROOT, "waifu2x-tensorrt_amd", "w2x_parse_check")
    rng = np.random.default_rng(9)
    rgba = rng.integers(0, 256, (37, 53, 4), dtype=np.uint8)
    rgba[..., 3] = (rng.random((37, 53)) < 0.2) * 255
    Image.fromarray(rgba).save(tmp_path / "a.png")
    Image.fromarray(rgba[..., :3]).save(tmp_path / "opaque.png")
    for name, radius, code in (("a.png", 0, 0), ("a.png", 5, 0), ("a.png", 16, 0), ("opaque.png", 16, 0), ("a.png", 17, 2), ("a.png", -3, 2)):
        r = subprocess.run([check, "bleed", str(tmp_path / name), str(radius)], capture_output=True, text=True, timeout=120)
        assert r.returncode == code, (name, radius, r.returncode, r.stdout, r.stderr[-1500:])
    r = subprocess.run([check, "bleed", str(tmp_path / "a.png"), "5"], capture_output=True, text=True, timeout=120)
    changed = int((rgba_ref.bleed(np.ascontiguousarray(rgba[..., 2::-1]), np.ascontiguousarray(rgba[..., 3]), 5) != rgba[..., 2::-1]).sum())
    assert f"{changed} bytes changed" in r.stdout, r.stdout
    r = subprocess.run([check, "args", *BASE, "render", "-i", str(tmp_path / "a.png"), "--alpha-bleed", "99"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "not in [0, 16]" in r.stderr
