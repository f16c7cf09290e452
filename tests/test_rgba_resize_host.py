"""Host side of the resized RGBA render and the RGBA sequences, no GPU: the three C functions and the two Python methods exist with their
argument lists, an engine that was never loaded refuses them with a message, and the command line takes --alpha-bleed / --alpha-skip-uniform together with
--outsize / --outscale (--print-config stops after parsing)."""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W2X = os.path.join(ROOT, "waifu2x-tensorrt_amd", "w2x")
BASE = ["--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "4", "--tileSize", "256"]


def w2x(*args):
    assert os.path.exists(W2X), "w2x was not built"
    return subprocess.run([W2X, *args], capture_output=True, text=True, timeout=120)


def c_arguments(name):
    """the parameter names of a function declared in include/w2x/c_api.h"""
    hdr = open(os.path.join(ROOT, "include", "w2x", "c_api.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in c_api.h"
    return [re.sub(r"[\[\]]", "", a.strip()).split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]


def test_c_functions_and_their_argument_lists(pkg):
    L = ctypes.CDLL(pkg.lib_path)
    for name in ("w2x_render_rgba_resized", "w2x_render_sequence_rgba", "w2x_render_sequence_rgba_resized"):
        assert hasattr(L, name), f"libw2x.so does not export {name}"
    one = c_arguments("w2x_render_rgba")
    assert one == ["e", "src", "rows", "cols", "src_step", "dst", "dst_step", "bleed", "skip_uniform_alpha"]
    # w2x_render_rgba's list plus dst_rows, dst_cols, count and filter, placed as in w2x_render_resized / w2x_render_sequence_resized
    assert c_arguments("w2x_render_rgba_resized") == ["e", "src", "rows", "cols", "src_step", "dst", "dst_rows", "dst_cols", "dst_step", "bleed", "skip_uniform_alpha", "filter"]
    assert c_arguments("w2x_render_sequence_rgba") == ["e", "srcs", "rows", "cols", "src_step", "dsts", "dst_step", "count", "bleed", "skip_uniform_alpha"]
    assert c_arguments("w2x_render_sequence_rgba_resized") == ["e", "srcs", "rows", "cols", "src_step", "dsts", "dst_rows", "dst_cols", "dst_step", "count", "bleed",
                                                               "skip_uniform_alpha", "filter"]
    assert c_arguments("w2x_render_sequence_resized")[:10] == c_arguments("w2x_render_sequence_rgba_resized")[:10]
    lib = pkg.lib()
    assert len(lib.w2x_render_rgba_resized.argtypes) == 12 and len(lib.w2x_render_sequence_rgba.argtypes) == 10 and len(lib.w2x_render_sequence_rgba_resized.argtypes) == 13


def test_python_methods_and_their_signatures(pkg):
    one = inspect.signature(pkg.Img2Img.render_rgba_resized).parameters
    assert list(one) == ["self", "bgra", "size", "bleed", "skip_uniform_alpha", "filter", "dst"]
    assert all(one[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("bleed", "skip_uniform_alpha", "filter", "dst"))
    assert (one["bleed"].default, one["skip_uniform_alpha"].default, one["filter"].default, one["dst"].default) == (0, False, "bicubic", None)
    seq = inspect.signature(pkg.Img2Img.render_sequence_rgba).parameters
    assert list(seq) == ["self", "frames", "size", "bleed", "skip_uniform_alpha", "filter", "outs", "pinned"]
    assert all(seq[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("size", "bleed", "skip_uniform_alpha", "filter", "outs", "pinned"))
    assert (seq["size"].default, seq["bleed"].default, seq["skip_uniform_alpha"].default, seq["filter"].default, seq["outs"].default, seq["pinned"].default) == \
           (None, 0, False, "bicubic", None, False)


def test_an_engine_that_was_never_loaded_refuses(pkg):
    eng = pkg.Img2Img()
    bgra = np.zeros((4, 4, 4), np.uint8)
    assert eng.render_rgba_resized(bgra, (6, 6), dst=np.zeros((6, 6, 4), np.uint8)) is False
    assert "before a successful load" in eng.last_error()
    with pytest.raises(pkg.W2xError, match="before a successful load"):
        eng.render_sequence_rgba([bgra, bgra], size=(6, 6))
    with pytest.raises(ValueError):
        eng.render_rgba_resized(bgra, (6, 6), filter="lanczos", dst=np.zeros((6, 6, 4), np.uint8))
    with pytest.raises(ValueError):
        eng.render_rgba_resized(bgra[..., :3], (6, 6))
    assert eng.render_sequence_rgba([]) == []
    eng.close()


def test_cli_alpha_options_with_a_resize_in_print_config(pkg, tmp_path):
    png = tmp_path / "sprite.png"; png.write_bytes(b"x")
    r = w2x(*BASE, "render", "-i", str(png), "--alpha-bleed", "4", "--outsize", "1920x1080", "--print-config")
    assert r.returncode == 0, r.stderr
    c = json.loads(r.stdout)
    assert c["alpha_bleed"] == 4 and c["alpha_skip_uniform"] is False and c["outsize"] == [1920, 1080] and c["outscale"] is None
    assert c["outputs"] == [str(tmp_path / "sprite(swin_unet_art)(noise3)(scale4)(1920x1080).png")]
    r = w2x(*BASE, "render", "-i", str(png), "--outscale", "3", "--alpha-bleed=16", "--alpha-skip-uniform", "--resize-filter", "bilinear", "--print-config")
    assert r.returncode == 0, r.stderr
    c = json.loads(r.stdout)
    assert c["alpha_bleed"] == 16 and c["alpha_skip_uniform"] is True and c["outsize"] is None and c["resize_filter"] == "bilinear"
    assert c["suffix"].endswith("(outscale3)")
    r = w2x(*BASE, "render", "-i", str(png), "--outsize", "1920x1080", "--alpha-bleed", "17", "--print-config")
    assert r.returncode != 0 and "not in [0, 16]" in r.stderr
