"""Host side of the resized renders (no GPU): the tap tables w2x_resize_weights hands the resample kernel against the weight matrix torch's
antialiased interpolate implies, and the command line's --outscale / --resize-filter (sizes, names, keys, rejections)."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_cli import BASE, W2X


def torch_matrix(n_in, n_out, mode):
    """[n_out, n_in]: interpolate one-hot rows (float64) along one axis"""
    x = torch.eye(n_in, dtype=torch.float64).reshape(n_in, 1, 1, n_in)
    return F.interpolate(x, size=(1, n_out), mode=mode, antialias=True, align_corners=False).reshape(n_in, n_out).T.numpy()


@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
@pytest.mark.parametrize("n_out,ratio", [(120, 1), (90, 4 / 3), (80, 1.5), (60, 2), (51, 2.37), (30, 4), (37, 4), (113, 1.5), (7, 2.37), (1, 4)])
def test_resize_weights_match_torch(pkg, mode, n_out, ratio):
    n_in = int(round(n_out * ratio))
    first, w = pkg.resize_weights(n_in, n_out, mode)
    taps = w.shape[1]
    assert taps <= (17 if mode == "bicubic" else 9)
    m = np.zeros((n_out, n_in))
    for i in range(n_out):
        for k in range(taps):
            if first[i] + k < n_in:
                m[i, first[i] + k] += w[i, k]
            else:
                assert w[i, k] == 0                          # nothing past the edge (the kernel stops there)
    t = torch_matrix(n_in, n_out, mode)
    assert np.abs(m - t).max() <= 1e-6
    assert np.abs(w.astype(np.float64).sum(1) - 1).max() <= 1e-6
    for i in range(n_out):                                     # the same first tap
        assert np.nonzero(m[i])[0][0] == np.nonzero(t[i])[0][0], i
    if ratio == 1:                                             # an axis at its own size passes through exactly
        assert np.array_equal(m, np.eye(n_in))


def test_resize_weights_refuse_bad_arguments(pkg):
    with pytest.raises(ValueError):
        pkg.resize_weights(10, 5, "lanczos")
    with pytest.raises(pkg.W2xError):
        pkg.resize_weights(0, 5)


def run(*args):
    return subprocess.run([W2X, *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("f,tag", [("3", "(outscale3)"), ("1.5", "(outscale1.5)"), ("4", "(outscale4)")])
def test_outscale_names_and_keys(pkg, tmp_path, f, tag):
    img = tmp_path / "a.png"
    img.write_bytes(b"x")
    r = run(*BASE, "render", "-i", str(img), "--outscale", f, "--print-config")
    assert r.returncode == 0, r.stderr
    c = json.loads(r.stdout)
    assert c["outscale"] == float(f) and c["resize_filter"] == "bicubic"
    assert c["suffix"] == "(swin_unet_art)(noise3)(scale4)" + tag
    assert c["outputs"] == [str(tmp_path / f"a(swin_unet_art)(noise3)(scale4){tag}.png")]
    r = run(*BASE, "render", "-i", str(img), "--outscale", f, "--resize-filter", "bilinear", "--tta", "--print-config")
    assert r.returncode == 0, r.stderr
    c = json.loads(r.stdout)
    assert c["resize_filter"] == "bilinear" and c["suffix"] == "(swin_unet_art)(noise3)(scale4)" + tag + "(tta)"
    r = run(*BASE, "render", "-i", str(img), "--print-config")        # without --outscale: the names of today
    c = json.loads(r.stdout)
    assert c["outscale"] is None and c["suffix"] == "(swin_unet_art)(noise3)(scale4)"


@pytest.mark.parametrize("extra,msg", [
    (["--outscale", "0.5"], "--outscale"),
    (["--outscale", "5"], "--outscale"),
    (["--outscale", "2", "--resize-filter", "lanczos"], "--resize-filter"),
    (["--resize-filter", "bilinear"], "--resize-filter"),
    (["--outscale", "2", "--devices", "2"], "--outscale"),
])
def test_outscale_rejections(pkg, tmp_path, extra, msg):
    img = tmp_path / "a.png"
    img.write_bytes(b"x")
    r = run(*BASE, "render", "-i", str(img), *extra, "--print-config")
    assert r.returncode != 0 and msg in r.stderr, (r.returncode, r.stderr)


def test_outscale_with_scale_two(pkg, tmp_path):
    img = tmp_path / "b.png"
    img.write_bytes(b"x")
    args = ["--model", "cunet/art", "--scale", "2", "--noise", "0", "--batchSize", "1", "--tileSize", "64", "render", "-i", str(img)]
    assert run(*args, "--outscale", "2", "--print-config").returncode == 0
    r = run(*args, "--outscale", "2.5", "--print-config")
    assert r.returncode != 0 and "--outscale" in r.stderr
