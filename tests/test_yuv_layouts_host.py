"""The YUV layouts (YuvLayout) without a GPU: the float64 reference of the four layouts (tests/yuv_layout_ref.py) against yuv_ref and against
known answers, the plane sizes of the C ABI, and the command line's --yuv-in / --yuv-out."""
import json
import os
import subprocess

import numpy as np
import pytest

import yuv_layout_ref as ref
import yuv_ref


@pytest.mark.parametrize("rows,cols,bits", [(8, 10, 8), (7, 9, 10), (45, 67, 8)])
def test_i420_of_the_layout_reference_is_yuv_ref(rows, cols, bits):
    """decode / encode with layout i420 return yuv_ref's arrays to the bit, on noise and on a smooth picture, both ranges"""
    for full in (False, True):
        for planes in (yuv_ref.random_planes(rows, cols, bits, 3, full_range=full), yuv_ref.smooth_planes(rows, cols, bits, 4, "bt601", full)):
            a = ref.decode(planes, "i420", matrix="bt601", full_range=full, bits=bits)
            b = yuv_ref.decode(*planes, matrix="bt601", full_range=full, bits=bits)
            assert np.array_equal(a, b)
            for ob in (8, 10):
                got = ref.encode(a, "i420", matrix="bt601", full_range=full, bits=ob)
                want = yuv_ref.encode(b, matrix="bt601", full_range=full, bits=ob)
                assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(got, want))
    assert ref.plane_shapes(rows, cols, "i420") == yuv_ref.plane_shapes(rows, cols)


@pytest.mark.parametrize("rows,cols", [(8, 10), (7, 9)])
def test_i422_decode_siting_on_impulses(rows, cols):
    """one chroma sample of an i422 plane reaches luma row y of its own row only: even x at full weight, the odd neighbours at 1/2, the last odd column
    (odd width: none; even width: clamped) at full weight from the last sample"""
    cw = (cols + 1) // 2
    for (i, j) in [(1, 2), (0, 0), (rows - 1, cw - 1)]:
        c = np.zeros((rows, cw))
        c[i, j] = 1.0
        up = ref.upsample_cols(c, cols)
        want = np.zeros((rows, cols))
        for x in range(cols):
            taps = [(x // 2, 1.0)] if x % 2 == 0 else [(x // 2, 0.5), (min(x // 2 + 1, cw - 1), 0.5)]
            want[i, x] = sum(w for cc, w in taps if cc == j)
        assert np.array_equal(up, want), (i, j)
    # through decode: a grey frame whose one Cr sample is raised lifts red in that row alone
    y = np.full((rows, cols), 128, np.uint8)
    u = np.full((rows, cw), 128, np.uint8)
    v = u.copy()
    v[2, 1] = 200
    rgb = ref.decode((y, u, v), "i422", matrix="bt709", full_range=True)
    changed = np.argwhere(np.abs(rgb[..., 0] - rgb[0, 0, 0]) > 1e-9)
    assert sorted(map(tuple, changed)) == [(2, 1), (2, 2), (2, 3)]
    assert np.isclose(rgb[2, 1, 0] - rgb[0, 0, 0], 0.5 * (rgb[2, 2, 0] - rgb[0, 0, 0]))


@pytest.mark.parametrize("rows,cols", [(8, 10), (7, 9)])
def test_i422_encode_siting_on_impulses(rows, cols):
    """one luma pixel of pure blue on black reaches chroma site (y, j) of its own row with weight (1/4, 1/2, 1/4) over columns 2j-1, 2j, 2j+1, clamped;
    no other row sees it"""
    for (py, px) in [(2, 3), (2, 4), (0, 0), (rows - 1, cols - 1)]:
        rgb = np.zeros((rows, cols, 3))
        rgb[py, px, 2] = 1.0
        yy, u, _ = ref.encode(rgb, "i422", matrix="bt709", full_range=True, bits=10)
        assert u.shape == (rows, (cols + 1) // 2) and yy.shape == (rows, cols)
        got = (u.astype(np.float64) - 512) / 1023 * 2        # Cb' = B / 2: the blue weight the site saw
        want = np.zeros(u.shape)
        for j in range(u.shape[1]):
            want[py, j] = sum(w for c, w in ((max(2 * j - 1, 0), 0.25), (2 * j, 0.5), (min(2 * j + 1, cols - 1), 0.25)) if c == px)
        assert np.abs(got - want).max() <= 1.0 / 1023, (py, px)     # (half a code of rounding)


@pytest.mark.parametrize("bits,full", [(8, False), (10, False), (10, True)])
def test_i444_round_trip_inside_the_cube(bits, full):
    """i444 codes -> RGB -> i444 codes: no resampling either way, so colours that stay inside the RGB cube come back within 1 code (the quantised
    planes decode to RGB that is re-encoded from float64: only the clamp could move them, and it does not act inside the cube)"""
    rgb = 0.1 + 0.8 * np.random.default_rng(5).random((7, 9, 3))
    planes = ref.encode(rgb, "i444", matrix="bt709", full_range=full, bits=bits)
    back = ref.decode(planes, "i444", matrix="bt709", full_range=full, bits=bits)
    assert back.min() > 0.0 and back.max() < 1.0
    again = ref.encode(back, "i444", matrix="bt709", full_range=full, bits=bits)
    for a, b in zip(planes, again):
        assert a.shape == (7, 9) and np.abs(a.astype(int) - b.astype(int)).max() <= 1
    # and the RGB itself within the quantisation of the codes
    assert np.abs(back - rgb).max() < 4.0 / (2 ** bits - 1)


def test_nv12_and_p010_known_answers():
    y = np.arange(12, dtype=np.uint8).reshape(3, 4)
    u = np.array([[10, 11], [12, 13]], np.uint8)
    v = np.array([[20, 21], [22, 23]], np.uint8)
    Y, UV = ref.pack_nv12(y, u, v)
    assert np.array_equal(Y, y) and UV.tolist() == [[10, 20, 11, 21], [12, 22, 13, 23]] and UV.dtype == np.uint8
    assert all(np.array_equal(a, b) for a, b in zip(ref.unpack_nv12(Y, UV), (y, u, v)))
    # P010: the code in the high ten bits; the low six are ignored on reading
    y10, u10, v10 = (y.astype(np.uint16) * 80, u.astype(np.uint16) * 40, v.astype(np.uint16) * 40)
    Y, UV = ref.pack_nv12(y10, u10, v10)
    assert Y.dtype == np.uint16 and np.array_equal(Y, y10 << 6) and UV[1].tolist() == [12 * 40 << 6, 22 * 40 << 6, 13 * 40 << 6, 23 * 40 << 6]
    assert all(np.array_equal(a, b) for a, b in zip(ref.unpack_nv12(Y | 0x3F, UV | 0x15), (y10, u10, v10)))
    # pure white, limited range, 10 bits: Y = 64 + 876 = 940, stored as 940 << 6; chroma at 512 << 6
    Y, UV = ref.encode(np.ones((2, 2, 3)), "nv12", bits=10)
    assert Y.tolist() == [[940 << 6] * 2] * 2 and UV.tolist() == [[512 << 6, 512 << 6]]
    assert ref.encode(np.ones((2, 2, 3)), "i444", bits=10)[0].tolist() == [[940, 940]] * 2
    # decode of an nv12 frame is decode of its i420 samples
    planes = yuv_ref.random_planes(7, 9, 10, 9)
    assert np.array_equal(ref.decode(ref.pack_nv12(*planes), "nv12", bits=10), yuv_ref.decode(*planes, bits=10))
    assert [p.shape for p in ref.pack_nv12(*planes)] == ref.plane_shapes(7, 9, "nv12") == [(7, 9), (4, 10)]


def test_layout_plane_sizes_of_the_c_abi(pkg):
    f = pkg.yuv_layout_plane_sizes
    assert f(1080, 1920, 8, "i420") == ([1080, 540, 540], [1920, 960, 960], [1920 * 1080, 960 * 540, 960 * 540]) == pkg.yuv_plane_sizes(1080, 1920, 8)
    assert f(1080, 1920, 10, "i422") == ([1080, 1080, 1080], [1920, 960, 960], [2 * 1920 * 1080, 2 * 960 * 1080, 2 * 960 * 1080])
    assert f(1080, 1920, 8, "i444") == ([1080] * 3, [1920] * 3, [1920 * 1080] * 3)
    assert f(1080, 1920, 10, "nv12") == ([1080, 540], [1920, 1920], [2 * 1920 * 1080, 2 * 1920 * 540])
    assert f(7, 9, 10, "i420") == ([7, 4, 4], [9, 5, 5], [126, 40, 40])
    assert f(7, 9, 8, "i422") == ([7, 7, 7], [9, 5, 5], [63, 35, 35])
    assert f(7, 9, 8, "i444") == ([7, 7, 7], [9, 9, 9], [63, 63, 63])
    assert f(7, 9, 8, "nv12") == ([7, 4], [9, 10], [63, 40])
    for k, name in enumerate(ref.LAYOUTS):
        assert pkg.YUV_LAYOUTS[name] == k
        rows_, cols_, bytes_ = f(1, 1, 8, name)
        assert (rows_, cols_, bytes_) == (([1, 1], [1, 2], [1, 2]) if name == "nv12" else ([1, 1, 1], [1, 1, 1], [1, 1, 1]))
        for r, c in ((1080, 1920), (7, 9), (1, 1)):
            assert list(zip(*f(r, c, 8, name)[:2])) == ref.plane_shapes(r, c, name) == pkg.yuv_layout_plane_shapes(r, c, name)
    import ctypes as C
    L = pkg.lib()
    n, arr = C.c_int(-7), (C.c_int * 3)(-7, -7, -7)
    for bad in ((0, 4, 8, 0), (4, -1, 8, 2), (4, 4, 9, 1), (4, 4, 16, 3), (4, 4, 8, 4), (4, 4, 8, -1)):
        assert L.w2x_yuv_layout_plane_sizes(*bad, C.byref(n), arr, arr, None) == 0, bad
        assert n.value == -7 and list(arr) == [-7, -7, -7]                       # nothing written
    assert L.w2x_yuv_layout_plane_sizes(4, 4, 8, 3, None, None, None, None) == 1       # every output pointer may be NULL
    with pytest.raises(ValueError):
        f(4, 4, 8, "yuv411p")
    with pytest.raises(pkg.W2xError):
        f(4, 4, 12, "i444")


# ---- the command line: --yuv-in / --yuv-out (parsed in cli/args.cpp; --print-config stops after parsing, no GPU)
W2X = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "waifu2x-tensorrt_amd", "w2x")
BASE = ["--model", "swin_unet/art", "--scale", "4", "--noise", "3", "--batchSize", "4", "--tileSize", "256"]
FORMATS = ["yuv420p", "yuv420p10le", "yuv422p", "yuv422p10le", "yuv444p", "yuv444p10le", "nv12", "p010le"]


def w2x(*args):
    assert os.path.exists(W2X), "w2x was not built"
    return subprocess.run([W2X, *args], capture_output=True, text=True, timeout=120)


def test_cli_yuv_formats_round_trip_in_print_config(pkg, tmp_path):
    clip = tmp_path / "clip.mkv"; clip.write_bytes(b"x")
    cfg = json.loads(w2x(*BASE, "render", "-i", str(clip), "--colorspace", "bt709", "--print-config").stdout)
    assert cfg["yuv_in"] is None and cfg["yuv_out"] is None and cfg["pix_fmt"] == "yuv420p"
    for k, fmt in enumerate(FORMATS):
        other = FORMATS[(k + 3) % len(FORMATS)]
        r = w2x(*BASE, "render", "-i", str(clip), "--colorspace", "bt709", "--yuv-in", fmt, "--yuv-out", other, "--print-config")
        assert r.returncode == 0, r.stderr
        cfg = json.loads(r.stdout)
        assert (cfg["yuv_in"], cfg["yuv_out"], cfg["pix_fmt"]) == (fmt, other, other)          # the encoder's format defaults to --yuv-out
    # --yuv-in alone: the output stays --pix_fmt and its rule
    cfg = json.loads(w2x(*BASE, "render", "-i", str(clip), "--colorspace", "bt709", "--yuv-in=nv12", "--pix_fmt", "yuv420p10le", "--print-config").stdout)
    assert (cfg["yuv_in"], cfg["yuv_out"], cfg["pix_fmt"]) == ("nv12", None, "yuv420p10le")
    # with --yuv-out, --pix_fmt is the encoder's alone and unrestricted
    r = w2x(*BASE, "render", "-i", str(clip), "--colorspace", "bt709", "--pix_fmt", "yuv444p", "--yuv-out", "yuv444p", "--print-config")
    assert r.returncode == 0, r.stderr
    cfg = json.loads(w2x(*BASE, "render", "-i", str(clip), "--colorspace", "bt709", "--pix_fmt", "gbrp", "--yuv-out", "yuv444p10le", "--print-config").stdout)
    assert (cfg["yuv_out"], cfg["pix_fmt"]) == ("yuv444p10le", "gbrp")
    assert cfg["outputs"] == [str(tmp_path / "clip(swin_unet_art)(noise3)(scale4).png")]      # output names unchanged


@pytest.mark.parametrize("opt", ["--yuv-in", "--yuv-out"])
def test_cli_yuv_format_options_are_checked(pkg, tmp_path, opt):
    clip = tmp_path / "clip.mkv"; clip.write_bytes(b"x")
    cases = [
        (["--colorspace", "bt709", opt, "yuv411p"], opt),            # each bad value names the option
        (["--colorspace", "bt709", opt, "NV12"], opt),
        (["--colorspace", "bt709", opt, "yuv420p12le"], opt),
        (["--colorspace", "bt709", opt, "bgr24"], opt),
        ([opt, "nv12"], opt + ": needs --colorspace"),
        (["--colorspace", "bt709", opt, "nv12", "--outsize", "1280x720"], opt),
    ]
    for extra, msg in cases:
        r = w2x(*BASE, "render", "-i", str(clip), *extra, "--print-config")
        assert r.returncode != 0 and msg in r.stderr, (extra, r.returncode, r.stderr)
    r = w2x(*BASE, "build", opt, "nv12", "--print-config")
    assert r.returncode != 0 and opt + ": only with render" in r.stderr, r.stderr
    r = w2x(*BASE, "render", "-i", str(clip), "--colorspace", "bt709", opt, "--print-config")
    assert r.returncode != 0                                                                   # (the value is missing or is not a format)


def test_cli_pix_fmt_rule_without_yuv_out_is_unchanged(pkg, tmp_path):
    clip = tmp_path / "clip.mkv"; clip.write_bytes(b"x")
    r = w2x(*BASE, "render", "-i", str(clip), "--pix_fmt", "yuv444p", "--colorspace", "bt709", "--print-config")
    assert r.returncode != 0 and "--pix_fmt" in r.stderr, r.stderr
    r = w2x(*BASE, "render", "-i", str(clip), "--pix_fmt", "yuv444p", "--colorspace", "bt709", "--yuv-in", "yuv444p", "--print-config")
    assert r.returncode != 0 and "--pix_fmt" in r.stderr, r.stderr
    r = w2x(*BASE, "render", "-i", str(clip), "--pix_fmt", "yuv444p", "--colorspace", "bt709", "--yuv-out", "yuv444p", "--print-config")
    assert r.returncode == 0, r.stderr


def test_cli_help_lists_the_yuv_format_options(pkg):
    r = w2x("--help")
    assert r.returncode == 0 and "--yuv-in" in r.stdout and "--yuv-out" in r.stdout and "p010le" in r.stdout
