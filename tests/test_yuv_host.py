"""YUV 4:2:0 on the host (no GPU): known answers and properties of the float64 reference (tests/yuv_ref.py) that holds renderYuv to its contract,
and the plane sizes of the C ABI helper w2x_yuv_plane_sizes."""
import numpy as np
import pytest

import yuv_ref


def one(rgb, **kw):
    y, u, v = yuv_ref.encode(np.array([[rgb]], np.float64), **kw)
    return int(y[0, 0]), int(u[0, 0]), int(v[0, 0])


def test_known_answers():
    assert one((1, 1, 1), matrix="bt709") == (235, 128, 128)
    assert one((0, 0, 0), matrix="bt709") == (16, 128, 128)
    assert one((1, 0, 0), matrix="bt709") == (63, 102, 240)
    assert one((1, 0, 0), matrix="bt601") == (81, 90, 240)
    assert one((1, 1, 1), matrix="bt2020", bits=10) == (940, 512, 512)
    assert one((0, 0, 0), matrix="bt709", bits=10) == (64, 512, 512)
    # full range: the extremes of the code range; chroma of pure blue / red at the top of theirs
    assert one((1, 1, 1), matrix="bt709", full_range=True) == (255, 128, 128)
    assert one((0, 0, 0), matrix="bt709", full_range=True, bits=10) == (0, 512, 512)
    assert one((0, 0, 1), matrix="bt709", full_range=True)[1] == 255
    assert one((1, 0, 0), matrix="bt2020", full_range=True, bits=10)[2] == 1023
    # out-of-range canvas values are clamped before coding
    assert one((1.5, 1.2, 2.0), matrix="bt709") == (235, 128, 128)
    assert one((-0.3, -1.0, 0.0), matrix="bt601") == (16, 128, 128)
    # decode of the known answers gives the colours back
    for matrix in yuv_ref.MATRICES:
        y, u, v = yuv_ref.encode(np.array([[[1.0, 0.0, 0.0]]]), matrix=matrix, bits=10)
        assert np.allclose(yuv_ref.decode(y, u, v, matrix=matrix, bits=10)[0, 0], (1, 0, 0), atol=4e-3)


@pytest.mark.parametrize("matrix", sorted(yuv_ref.MATRICES))
@pytest.mark.parametrize("bits,full_range", [(8, False), (10, False), (8, True), (10, True)])
@pytest.mark.parametrize("rows,cols", [(6, 8), (7, 9)])
def test_decode_after_encode_is_identity_on_flat_chroma(matrix, bits, full_range, rows, cols):
    """flat chroma: upsampling and the chroma filter see one value, so decode(encode(decode(planes))) gives the planes back within 1 code"""
    rng = np.random.default_rng(rows * cols + bits)
    yo, ys, co, cs = yuv_ref.levels(bits, full_range)
    dt = np.uint8 if bits == 8 else np.uint16
    shapes = yuv_ref.plane_shapes(rows, cols)
    # codes whose colours lie inside the RGB cube (no clamping on the way): grey-ish chroma
    y = rng.integers(int(yo + 0.25 * ys), int(yo + 0.75 * ys), shapes[0]).astype(dt)
    u = np.full(shapes[1], int(co + 0.05 * cs), dt)
    v = np.full(shapes[2], int(co - 0.04 * cs), dt)
    rgb = yuv_ref.decode(y, u, v, matrix=matrix, full_range=full_range, bits=bits)
    assert rgb.min() > 0 and rgb.max() < 1
    back = yuv_ref.encode(rgb, matrix=matrix, full_range=full_range, bits=bits)
    for a, b in zip(back, (y, u, v)):
        assert a.dtype == dt and a.shape == b.shape
        assert np.abs(a.astype(int) - b.astype(int)).max() <= 1


@pytest.mark.parametrize("rows,cols", [(8, 10), (7, 9)])
def test_upsampling_siting_on_impulses(rows, cols):
    """one chroma sample raised: its weight on the luma grid is the MPEG-2 "left" siting (x = 2j, y = 2i + 1/2), clamped at the edges"""
    ch, cw = (rows + 1) // 2, (cols + 1) // 2
    for (i, j) in [(1, 2), (0, 0), (ch - 1, cw - 1)]:
        c = np.zeros((ch, cw))
        c[i, j] = 1.0
        up = yuv_ref.upsample(c, rows, cols)
        want = np.zeros((rows, cols))
        for yy in range(rows):
            k = yy // 2
            rws = [(max(k - 1, 0), 0.25), (k, 0.75)] if yy % 2 == 0 else [(k, 0.75), (min(k + 1, ch - 1), 0.25)]
            for xx in range(cols):
                cls = [(xx // 2, 1.0)] if xx % 2 == 0 else [(xx // 2, 0.5), (min(xx // 2 + 1, cw - 1), 0.5)]
                want[yy, xx] = sum(wr * wc for r, wr in rws for cc, wc in cls if (r, cc) == (i, j))
        assert np.allclose(up, want), (i, j)
        # the weights of any one luma pixel sum to 1
        assert np.allclose(yuv_ref.upsample(np.ones((ch, cw)), rows, cols), 1.0)


@pytest.mark.parametrize("rows,cols", [(8, 10), (7, 9)])
def test_chroma_filter_siting_on_impulses(rows, cols):
    """one luma pixel of pure blue on black: it reaches chroma site (i, j) with weight (1/4, 1/2, 1/4) over columns 2j-1, 2j, 2j+1 times 1/2 over
    rows 2i, 2i+1, coordinates clamped"""
    for (py, px) in [(2, 3), (2, 4), (0, 0), (rows - 1, cols - 1)]:
        rgb = np.zeros((rows, cols, 3))
        rgb[py, px, 2] = 1.0
        _, u, _ = yuv_ref.encode(rgb, matrix="bt709", full_range=True, bits=10)
        got = (u.astype(np.float64) - 512) / 1023 * 2        # Cb' = (B - Kb B) / (2 (1 - Kb)) = B / 2: the blue weight the site saw
        want = np.zeros(u.shape)
        for i in range(u.shape[0]):
            for j in range(u.shape[1]):
                wy = sum(0.5 for r in (2 * i, min(2 * i + 1, rows - 1)) if r == py)
                wx = sum(w for c, w in ((max(2 * j - 1, 0), 0.25), (2 * j, 0.5), (min(2 * j + 1, cols - 1), 0.25)) if c == px)
                want[i, j] = wy * wx
        assert np.abs(got - want).max() <= 1.0 / 1023, (py, px)     # (half a code of rounding)


def test_plane_sizes_of_the_c_abi(pkg):
    assert pkg.yuv_plane_sizes(1080, 1920, 8) == ([1080, 540, 540], [1920, 960, 960], [1920 * 1080, 960 * 540, 960 * 540])
    assert pkg.yuv_plane_sizes(7, 9, 10) == ([7, 4, 4], [9, 5, 5], [126, 40, 40])
    assert pkg.yuv_plane_sizes(1, 1, 8) == ([1, 1, 1], [1, 1, 1], [1, 1, 1])
    for bad in ((0, 4, 8), (4, -1, 8), (4, 4, 9), (4, 4, 16)):
        with pytest.raises(pkg.W2xError):
            pkg.yuv_plane_sizes(*bad)


# ---- the command line: --colorspace / --color_range (parsed in cli/args.cpp; --print-config stops after parsing, no GPU)
import json  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402

W2X = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "waifu2x-tensorrt_amd", "w2x")
BASE = ["--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "4", "--tileSize", "256"]


def w2x(*args):
    assert os.path.exists(W2X), "w2x was not built"
    return subprocess.run([W2X, *args], capture_output=True, text=True, timeout=120)


def test_cli_colour_options_in_print_config(pkg, tmp_path):
    clip = tmp_path / "clip.mkv"; clip.write_bytes(b"x")
    r = w2x(*BASE, "render", "-i", str(clip), "--print-config")
    assert r.returncode == 0, r.stderr
    cfg = json.loads(r.stdout)
    assert cfg["colorspace"] is None and cfg["color_range"] == "tv" and cfg["pix_fmt"] == "yuv420p"
    r = w2x(*BASE, "render", "-i", str(clip), "--colorspace", "BT2020", "--color_range", "pc", "--pix_fmt", "yuv420p10le", "--print-config")
    assert r.returncode == 0, r.stderr
    cfg = json.loads(r.stdout)
    assert (cfg["colorspace"], cfg["color_range"], cfg["pix_fmt"]) == ("bt2020", "pc", "yuv420p10le")
    assert cfg["outputs"] == [str(tmp_path / "clip(swin_unet_art)(noise3)(scale4).png")]      # output names unchanged
    r = w2x(*BASE, "render", "-i", str(clip), "--colorspace", "bt601", "--print-config")
    assert r.returncode == 0 and json.loads(r.stdout)["colorspace"] == "bt601" and json.loads(r.stdout)["color_range"] == "tv"


@pytest.mark.parametrize("extra,msg", [
    (["--colorspace", "bt709", "--pix_fmt", "yuv444p"], "--pix_fmt"),
    (["--colorspace", "bt709", "--pix_fmt", "rgb24"], "--pix_fmt"),
    (["--color_range", "pc"], "needs --colorspace"),
    (["--colorspace", "bt709", "--outscale", "2"], "--outscale"),
    (["--colorspace", "smpte240m"], "--colorspace"),
    (["--colorspace", "bt709", "--color_range", "studio"], "--color_range"),
])
def test_cli_colour_options_are_checked(pkg, tmp_path, extra, msg):
    clip = tmp_path / "clip.mkv"; clip.write_bytes(b"x")
    r = w2x(*BASE, "render", "-i", str(clip), *extra, "--print-config")
    assert r.returncode != 0 and msg in r.stderr, (r.returncode, r.stderr)
    r = w2x(*BASE, "build", *extra[:2], "--print-config")
    assert r.returncode != 0 and "only with render" in r.stderr, r.stderr


def test_cli_help_lists_the_colour_options(pkg):
    r = w2x("--help")
    assert r.returncode == 0 and "--colorspace" in r.stdout and "--color_range" in r.stdout and "yuv420p10le" in r.stdout


def test_cli_yuv_video_without_ffmpeg_names_the_reason(pkg, tmp_path):
    """a --colorspace run on a video with no ffmpeg on PATH fails before any engine is needed, and says why"""
    clip = tmp_path / "clip.mkv"; clip.write_bytes(b"x" * 64)
    env = dict(os.environ, PATH=os.pathsep.join(p for p in os.environ["PATH"].split(os.pathsep) if not os.path.exists(os.path.join(p, "ffmpeg"))))
    r = subprocess.run([W2X, *BASE, "--models", str(tmp_path / "none"), "render", "-i", str(clip), "--colorspace", "bt709"], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode != 0
