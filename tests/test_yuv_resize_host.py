"""Host side of the resized YUV renders, no GPU: the two C functions and the two Python methods exist with their argument lists, and the
command line's --outsize is parsed, named and rejected as documented (--print-config stops after parsing)."""
import ctypes
import inspect
import json
import os
import re
import subprocess

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


def test_c_functions_are_the_yuv_pair_plus_a_filter(pkg):
    L = ctypes.CDLL(pkg.lib_path)
    for plain in ("w2x_render_yuv", "w2x_render_sequence_yuv"):
        resized = plain + "_resized"
        assert hasattr(L, resized), f"libw2x.so does not export {resized}"
        assert c_arguments(resized) == c_arguments(plain) + ["filter"]


def test_python_methods_and_their_signatures(pkg):
    one = inspect.signature(pkg.Img2Img.render_yuv_resized).parameters
    assert list(one) == ["self", "y", "u", "v", "size", "matrix", "full_range", "out_bits", "filter", "dst"]
    assert all(one[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("matrix", "full_range", "out_bits", "filter", "dst"))
    assert (one["matrix"].default, one["full_range"].default, one["out_bits"].default, one["filter"].default, one["dst"].default) == ("bt709", False, None, "bicubic", None)
    seq = inspect.signature(pkg.Img2Img.render_sequence_yuv_resized).parameters
    assert list(seq) == ["self", "frames", "size", "matrix", "full_range", "out_bits", "pinned", "filter"]
    assert all(seq[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("matrix", "full_range", "out_bits", "pinned", "filter"))
    assert (seq["pinned"].default, seq["filter"].default) == (False, "bicubic")


def test_outsize_in_print_config_and_names(pkg, tmp_path):
    img = tmp_path / "a.png"; img.write_bytes(b"x")
    r = w2x(*BASE, "render", "-i", str(img), "--outsize", "1920x1080", "--print-config")
    assert r.returncode == 0, r.stderr
    c = json.loads(r.stdout)
    assert c["outsize"] == [1920, 1080] and c["outscale"] is None and c["resize_filter"] == "bicubic"
    assert c["suffix"] == "(swin_unet_art)(noise3)(scale4)(1920x1080)"
    assert c["outputs"] == [str(tmp_path / "a(swin_unet_art)(noise3)(scale4)(1920x1080).png")]
    r = w2x(*BASE, "render", "-i", str(img), "--outsize=721x577", "--resize-filter", "bilinear", "--tta", "--print-config")
    assert r.returncode == 0, r.stderr
    c = json.loads(r.stdout)
    assert c["outsize"] == [721, 577] and c["resize_filter"] == "bilinear" and c["suffix"] == "(swin_unet_art)(noise3)(scale4)(721x577)(tta)"
    r = w2x(*BASE, "render", "-i", str(img), "--print-config")              # without it: null, and the names of today
    assert r.returncode == 0, r.stderr
    c = json.loads(r.stdout)
    assert c["outsize"] is None and c["suffix"] == "(swin_unet_art)(noise3)(scale4)"
    r = w2x(*BASE, "render", "-i", str(img), "--outscale", "2", "--print-config")
    assert r.returncode == 0 and json.loads(r.stdout)["outsize"] is None and json.loads(r.stdout)["suffix"].endswith("(outscale2)")


def test_help_lists_outsize(pkg):
    r = w2x("--help")
    assert r.returncode == 0 and "--outsize WxH" in r.stdout


@pytest.mark.parametrize("extra", [
    ["--outsize", "1920"], ["--outsize", "1920x"], ["--outsize", "x1080"], ["--outsize", "1920x1080x3"], ["--outsize", "1920*1080"], ["--outsize", "1e3x500"],
    ["--outsize", "19.5x10"], ["--outsize", "0x1080"], ["--outsize", "1920x0"], ["--outsize", "-1920x1080"], ["--outsize", ""],
    ["--outsize", "1920x1080", "--outscale", "2"], ["--outscale", "2", "--outsize", "1920x1080"],
    ["--outsize", "1920x1080", "--resize-filter", "lanczos"],
    ["--outsize", "1920x1080", "--devices", "2"],
])
def test_outsize_parse_errors_name_the_option(pkg, tmp_path, extra):
    img = tmp_path / "a.png"; img.write_bytes(b"x")
    r = w2x(*BASE, "render", "-i", str(img), *extra, "--print-config")
    named = "--resize-filter" if "lanczos" in extra else "--outsize"
    assert r.returncode != 0 and named in r.stderr, (r.returncode, r.stderr)


def test_outsize_is_a_render_option(pkg):
    r = w2x(*BASE, "build", "--outsize", "1920x1080", "--print-config")
    assert r.returncode != 0 and "--outsize" in r.stderr and "only with render" in r.stderr, r.stderr


def test_outsize_on_a_video_over_several_devices_is_accepted(pkg, tmp_path):
    """only a still over --devices > 1 is refused (as --outscale)"""
    clip = tmp_path / "clip.mkv"; clip.write_bytes(b"x")
    assert w2x(*BASE, "render", "-i", str(clip), "--outsize", "1920x1080", "--devices", "2", "--print-config").returncode == 0


def test_resize_filter_alone_still_needs_a_resize(pkg, tmp_path):
    img = tmp_path / "a.png"; img.write_bytes(b"x")
    r = w2x(*BASE, "render", "-i", str(img), "--resize-filter", "bilinear", "--print-config")
    assert r.returncode != 0 and "--resize-filter" in r.stderr and "--outsize" in r.stderr


def test_colorspace_takes_outsize_and_still_refuses_outscale(pkg, tmp_path):
    clip = tmp_path / "clip.mkv"; clip.write_bytes(b"x")
    r = w2x(*BASE, "render", "-i", str(clip), "--colorspace", "bt709", "--outscale", "2", "--print-config")
    assert r.returncode != 0 and "--outscale" in r.stderr and "--outsize" in r.stderr, r.stderr
    r = w2x(*BASE, "render", "-i", str(clip), "--colorspace", "bt709", "--outsize", "1920x1080", "--print-config")
    assert r.returncode == 0, r.stderr
    c = json.loads(r.stdout)
    assert c["colorspace"] == "bt709" and c["outsize"] == [1920, 1080]
    assert c["outputs"] == [str(tmp_path / "clip(swin_unet_art)(noise3)(scale4)(1920x1080).png")]
