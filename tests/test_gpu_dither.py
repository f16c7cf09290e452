"""Dithered output on the GPU (Img2Img::setDither).  The reference is tests/dither_ref.py: the rule in numpy float32, Bayer by its closed form, the
blue-noise table through dither_table().  Every comparison of RGB, gray and RGBA output is equality on every byte: the dithered kernels quantise the value the
undithered ones round, so a dithered integer frame is the reference quantisation of the float frame (out_bits = 32) of the same call.  Engines: the small
synthetic graphs at tile 64 of test_gpu_gray.CONFIGS; the setting is persistent, so every test puts "none" back (dithered())."""
import contextlib

import numpy as np
import pytest

import dither_ref as ref
import yuv_layout_ref as ylr
import yuv_ref
import yuv_siting_ref as ysr
from test_gpu_gray import CONFIGS, engines, gray_frame, rep  # noqa: F401  (engines: the module-scoped fixture, made again for this module)
from test_gpu_parity import smooth_frame
from test_gpu_planar import bgr_frame, planes_of, same
from test_gpu_rgba import rgba_frame
from test_gpu_yuv_layouts import oracle_canvas
from test_gpu_yuv_siting import SWIN, resized

pytestmark = pytest.mark.gpu

MODES = ("ordered", "bluenoise")
DTYPES = ref.DTYPES


@pytest.fixture(scope="module")
def table(pkg):
    return pkg.dither_table("bluenoise")


@contextlib.contextmanager
def dithered(eng, mode, phase=0, advance=0):
    assert eng.set_dither(mode, phase, advance) is True
    try:
        yield eng
    finally:
        assert eng.set_dither("none") is True


def interleave(planes):
    """R, G, B planes -> the BGR frame"""
    return np.ascontiguousarray(np.stack([planes[2], planes[1], planes[0]], axis=-1))


def differ(a, b):
    return any((x != y).any() for x, y in zip(a, b)) if isinstance(a, tuple) else bool((a != b).any())


# ---- 1. the rule alone, through dither_planes
def crafted(rows, cols, bits, seed):
    """three float32 planes: a ramp over [-0.01, 1.01]; exact codes k / maxcode - k counts up from `seed` and wraps, every code where the plane has room for them;
    those values a hair (one or three float32 steps) either side.  Returns the planes and k."""
    m = (1 << bits) - 1
    n = rows * cols
    ramp = np.linspace(-0.01, 1.01, n).astype(np.float32).reshape(rows, cols)
    k = (np.arange(n) + seed) % (m + 1)
    exact = (k.astype(np.float64) / m).astype(np.float32)
    hair = exact.copy()
    for step in range(3):
        moved = np.where(np.arange(n) % 2 == 0, np.nextafter(hair, np.float32(2)), np.nextafter(hair, np.float32(-1))).astype(np.float32)
        hair = np.where((step == 0) | (np.arange(n) % 4 >= 2), moved, hair)      # a quarter each: +1, -1, +3, -3 steps
    return (ramp, exact.reshape(rows, cols), hair.reshape(rows, cols)), k.reshape(rows, cols)


@pytest.mark.parametrize("bits", [8, 10, 12, 16])
@pytest.mark.parametrize("mode", MODES)
def test_rule_alone(engines, table, mode, bits):
    eng, _ = engines("swin_x4_b2_blend")
    m = (1 << bits) - 1
    for rows, cols in ((37, 70), (16, 64), (256, 256)):                        # (256 x 256: every code of every depth)
        planes, k = crafted(rows, cols, bits, 7)
        assert rows * cols < 65536 or len(np.unique(k)) == m + 1
        for phase in (0, 1, 5) if rows < 256 else (2,):
            with dithered(eng, mode, phase):
                got = eng.dither_planes(planes, bits)
            want = ref.dither_planes(planes, bits, mode, phase, table)
            same(f"{mode} {bits} bits {rows}x{cols} phase {phase}", got, want)
            # Where V is an integer the code is that integer, so exact areas are unchanged - wherever fl32(V + t) is below V + 1 for the largest t, 1 - 1 / (2N):
            # for ordered (1 - 1/128) at every code of every depth; for bluenoise (1 - 1/8192) below code 2048, where fp32 still has 13 fraction bits.  From
            # 2048 on the sum's last bit is 2^-12 or coarser and the rule's one rounded addition takes the top thresholds to V + 1 (at 65535: 8 of 4096
            # positions); the bytes there are the reference's all the same (above).
            V = planes[1] * np.float32(m)
            whole = (V == np.rint(V)) & ((V < 2048) | (mode == "ordered"))
            assert whole.any() and (got[1][whole] == k[whole]).all(), (mode, bits, phase)
            if bits <= 10 or mode == "ordered":
                assert whole.sum() >= 0.5 * whole.size                                # (most codes k / maxcode come back as exactly k from the product)
            assert differ(got, ref.dither_planes(planes, bits, "none")), "dither changed nothing"
        # unaligned destination views with padded steps: three planes cut out of one buffer, plane k starting k + 1 samples into its rows
        block = np.zeros((3, rows, cols + 13), DTYPES[bits])
        views = tuple(block[j, :, j + 1:j + 1 + cols] for j in range(3))
        padded = tuple(np.pad(p, ((0, 0), (3, 9)))[:, 3:3 + cols] for p in planes)
        with dithered(eng, mode, 5):
            eng.dither_planes(padded, bits, dst=views)
        same(f"{mode} {bits} bits views", views, ref.dither_planes(planes, bits, mode, 5, table))
        for j in range(3):
            assert not block[j, :, :j + 1].any() and not block[j, :, j + 1 + cols:].any()
    # mode none through the hook is the undithered quantisation
    planes, _ = crafted(37, 70, bits, 9)
    same(f"none {bits} bits", eng.dither_planes(planes, bits), ref.dither_planes(planes, bits, "none"))


# ---- 2. what it is for: the mean over a period of the pattern is the value
@pytest.mark.parametrize("bits", [8, 10])
def test_block_means_carry_the_value(engines, bits):
    """Ordered: a plane constant over each aligned 8 x 8 block gives a block mean within 1/64 code of v * maxcode; BlueNoise: constant over a 64 x 64 tile, within
    1/4096 code.  The thresholds (i + 0.5) / N are equally spaced, so the mean of floor(V + t) over one period is V to within 1 / (2N); the fp32 rounding of V and
    of V + t (at most 2^-14 code below 1024) moves a sample across its threshold only where V + t is that close to an integer, which costs less than the other
    1 / (2N).  rint alone is up to 1/2 off on the same planes."""
    eng, _ = engines("swin_x4_b2_blend")
    m = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    for mode, side, shape, bound in (("ordered", 8, (64, 64), 1 / 64), ("bluenoise", 64, (64, 128), 1 / 4096)):
        by, bx = shape[0] // side, shape[1] // side
        planes, values = [], []
        for c in range(3):
            v = rng.uniform(0.02, 0.98, (by, bx))
            v[0, 0] = (37 + 0.49) / m                                # a value rint alone gets almost half a code wrong
            v = v.astype(np.float32)
            values.append(v.astype(np.float64) * m)
            planes.append(np.ascontiguousarray(np.kron(v, np.ones((side, side), np.float32))))
        for phase in (0, 3):
            with dithered(eng, mode, phase):
                got = eng.dither_planes(planes, bits)
            worst = 0.0
            for c in range(3):
                means = got[c].astype(np.float64).reshape(by, side, bx, side).mean(axis=(1, 3))
                worst = max(worst, float(np.abs(means - values[c]).max()))
            print(f"DITHER means {mode} {bits} bits phase {phase}: worst |block mean - v * maxcode| = {worst:.6f} code (bound {bound:.6f})")
            assert worst <= bound, (mode, bits, phase, worst)
        plain = eng.dither_planes(planes, bits)
        off = max(float(np.abs(plain[c].astype(np.float64).reshape(by, side, bx, side).mean(axis=(1, 3)) - values[c]).max()) for c in range(3))
        assert off > 0.45, off                                       # rint alone: the whole block is one code


# ---- 3. frames are the rule applied to the canvas
FRAME_CASES = [("swin_x4_b2_blend", 45, 57), ("cunet_x2_b3_noblend_tta", 61, 83), ("cunet_x2_b1_fp32", 57, 70)]


@pytest.mark.parametrize("name,rows,cols", FRAME_CASES)
def test_frames_are_the_rule_on_the_canvas(engines, table, name, rows, cols):
    """the dithered twin of test_gpu_planar.test_output_depths_quantise_one_canvas"""
    eng, scale = engines(name)
    src = planes_of(bgr_frame(rows, cols, 5, "noise"))
    f = eng.render_planar(src, out_bits=32)
    for mode in MODES:
        other = MODES[1 - MODES.index(mode)]
        for bits, phase in ((8, 0), (10, 2), (16, 0)):
            with dithered(eng, mode, phase):
                got = eng.render_planar(src, out_bits=bits)
                again_float = eng.render_planar(src, out_bits=32)
            same(f"{name} {mode} out_bits {bits} phase {phase}", got, ref.dither_planes(f, bits, mode, phase, table))
            same(f"{name} {mode}: float output untouched", again_float, f)
            assert differ(got, eng.render_planar(src, out_bits=bits)), "the dithered bytes are the undithered ones"
            # mutants: a reference without the plane offsets, and the other mode, must not match
            dropped = ref.dither_planes(f, bits, mode, phase, table, offsets_dropped=True)
            assert (got[1] != dropped[1]).any() and (got[2] != dropped[2]).any()
            assert differ(got, ref.dither_planes(f, bits, other, phase, table))
            if phase:
                assert differ(got, ref.dither_planes(f, bits, mode, 0, table))


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
def test_resized_frames_are_the_rule_on_the_resized_canvas(engines, table, filt):
    eng, scale = engines("swin_x4_b2_blend")
    src = planes_of(bgr_frame(45, 57, 50, "noise"))
    for size in ((71, 103), (150, 200), (100, 201), (113, 150)):                 # widths of every residue mod 4
        f = eng.render_planar_resized(src, size, out_bits=32, filter=filt)
        for mode, bits, phase in (("ordered", 8, 1), ("bluenoise", 8, 0), ("bluenoise", 10, 4), ("ordered", 16, 0)):
            with dithered(eng, mode, phase):
                got = eng.render_planar_resized(src, size, out_bits=bits, filter=filt)
            same(f"resized {size} {filt} {mode} {bits}", got, ref.dither_planes(f, bits, mode, phase, table))
            assert differ(got, eng.render_planar_resized(src, size, out_bits=bits, filter=filt))
            dropped = ref.dither_planes(f, bits, mode, phase, table, offsets_dropped=True)
            assert (got[1] != dropped[1]).any() and (got[2] != dropped[2]).any()


# ---- 4. the project's equalities survive, with one setting on both sides
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,rows,cols", [("swin_x4_b2_blend", 40, 141), ("cunet_x2_b3_noblend_tta", 61, 83)])
def test_equalities_survive(pkg, engines, table, mode, name, rows, cols):
    eng, scale = engines(name)
    bgr, bgr16 = bgr_frame(rows, cols, 11, "smooth"), bgr_frame(rows, cols, 12, "noise", np.uint16)
    g = gray_frame(rows, cols, 13, "smooth")
    bgra = rgba_frame(rows, cols, 14)
    plain_rgba = eng.render_rgba(bgra, bleed=2)
    planes4 = tuple(np.ascontiguousarray(bgra[..., k]) for k in (2, 1, 0, 3))
    plain_rgbap = eng.render_planar_rgba(planes4, bleed=2, out_bits=10)
    opaque = bgra.copy()
    opaque[..., 3] = 255
    plain_opaque = eng.render_rgba(opaque)
    size = (rows * scale - 17, cols * scale - 6)
    plain_rgba_resized = eng.render_rgba_resized(bgra, size)
    with dithered(eng, mode, 3):
        out = eng.render(bgr)
        f = eng.render_planar(planes_of(bgr), out_bits=32)
        same("render() is the rule on the canvas", planes_of(out), ref.dither_planes(f, 8, mode, 3, table))
        same("render() is the interleaved 8 / 8 planes", out, interleave(eng.render_planar(planes_of(bgr))))
        same("16-bit render() is the 16 / 16 planes", eng.render(bgr16), interleave(eng.render_planar(planes_of(bgr16))))
        same("render_gray is plane G of render(rep(g))", eng.render_gray(g), eng.render(rep(g))[..., 1])
        same("render_gray is the rule at plane index 1", eng.render_gray(g),
             ref.dither_plane(eng.render_planar(planes_of(rep(g)), out_bits=32)[1], 8, mode, 1, 3, table))
        # RGBA: colour is render() of the bled colour, alpha the undithered call's bytes
        rgba = eng.render_rgba(bgra, bleed=2)
        bled = pkg.alpha_bleed(np.ascontiguousarray(bgra[..., :3]), np.ascontiguousarray(bgra[..., 3]), 2)
        same("render_rgba colour", rgba[..., :3], eng.render(bled))
        same("render_rgba alpha is undithered", rgba[..., 3], plain_rgba[..., 3])
        assert differ(rgba[..., :3], plain_rgba[..., :3])
        rgbap = eng.render_planar_rgba(planes4, bleed=2, out_bits=10)
        same("render_planar_rgba colour", rgbap[:3], eng.render_planar(planes_of(bled), out_bits=10))
        same("render_planar_rgba alpha is undithered", rgbap[3], plain_rgbap[3])
        # an opaque cut-out stays opaque, with and without the uniform-alpha shortcut
        for skip in (False, True):
            o = eng.render_rgba(opaque, skip_uniform_alpha=skip)
            op = eng.render_planar_rgba(tuple(np.ascontiguousarray(opaque[..., k]) for k in (2, 1, 0, 3)), skip_uniform_alpha=skip, out_bits=12)
            if skip:                                                  # the shortcut: the plane keeps its value, no 254 sprinkled in
                assert (o[..., 3] == 255).all() and (op[3] == 4095).all()
            else:                                                     # through the network (these synthetic weights do not keep 255): the undithered bytes
                same("opaque alpha is undithered", o[..., 3], plain_opaque[..., 3])
            same(f"opaque colour, skip {skip}", o[..., :3], eng.render(np.ascontiguousarray(opaque[..., :3])))
        # resized calls: at the scaled size they are the plain calls, elsewhere colour follows render_resized and alpha stays undithered
        full = (rows * scale, cols * scale)
        same("render_resized at the scaled size", eng.render_resized(bgr, full), out)
        same("render_planar_resized at the scaled size", eng.render_planar_resized(planes_of(bgr), full, out_bits=10), eng.render_planar(planes_of(bgr), out_bits=10))
        same("render_gray_resized at the scaled size", eng.render_gray_resized(g, full), eng.render_gray(g))
        same("render_rgba_resized at the scaled size", eng.render_rgba_resized(bgra, full, bleed=2), rgba)
        rr = eng.render_rgba_resized(bgra, size)
        same("render_rgba_resized colour", rr[..., :3], eng.render_resized(np.ascontiguousarray(bgra[..., :3]), size))
        same("render_rgba_resized alpha is undithered", rr[..., 3], plain_rgba_resized[..., 3])
        same("render_resized is the interleaved planes", eng.render_resized(bgr, size), interleave(eng.render_planar_resized(planes_of(bgr), size)))
        same("render_gray_resized is plane G", eng.render_gray_resized(g, size), eng.render_resized(rep(g), size)[..., 1])
        # strips: the thresholds are those of the absolute position
        if not CONFIGS[name][6].get("tta"):
            strips = np.full_like(out, 77)
            for part in range(2):
                assert eng.render_strip(bgr, strips, part, 2)
            same("render_strip parts 0 / 2 and 1 / 2 are render()'s columns", strips, out)
    same("the setting is gone", eng.render(bgr), interleave(eng.render_planar(planes_of(bgr))))
    assert differ(eng.render(bgr), out)


# ---- 5. sequences: frame i is the single call at phase + i * advance
@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_sequences_follow_phase_and_advance(engines, mode, pinned):
    eng, scale = engines("swin_x4_b2_tta")                                # (90 x 130 frames with TTA: 48 slots of one pass, the sequence rolls)
    frames = [bgr_frame(90, 130, 60 + k, "noise" if k % 2 else "smooth") for k in range(3)]
    size = (270, 391)
    for advance in (0, 1):
        want, want_planar, want_resized = [], [], []
        for i, fr in enumerate(frames):
            with dithered(eng, mode, 7 + i * advance):
                want.append(eng.render(fr))
                want_planar.append(eng.render_planar(planes_of(fr), out_bits=10))
                want_resized.append(eng.render_resized(fr, size))
        with dithered(eng, mode, 7, advance):
            got = eng.render_sequence(frames, pinned=pinned)
            got_planar = eng.render_sequence_planar([planes_of(fr) for fr in frames], out_bits=10, pinned=pinned)
            got_resized = eng.render_sequence_resized(frames, size, pinned=pinned)
            still = eng.render_sequence([frames[0]] * 3, pinned=pinned)
        for i in range(3):
            same(f"{mode} advance {advance} BGR frame {i}", got[i], want[i])
            same(f"{mode} advance {advance} planar frame {i}", got_planar[i], want_planar[i])
            same(f"{mode} advance {advance} resized frame {i}", got_resized[i], want_resized[i])
        if advance:
            assert differ(still[0], still[1]) and differ(still[1], still[2]), "temporal dither repeats its pattern"
        else:
            same("a still pattern", still[1], still[0])
            same("a still pattern", still[2], still[0])


# ---- 6. YUV: no exact oracle exists - the project's bound is 1 code against the float64 reference
def yuv_unrounded(rgb, layout, siting, bits):
    """the unrounded float64 code values c of the planes Y, U, V that yuv_siting_ref.encode rounds: its statements (levels, MATRICES, site_rgb) without the rint"""
    kr, kb = yuv_ref.MATRICES["bt709"]
    kg = 1.0 - kr - kb
    yo, ys, co, cs = yuv_ref.levels(bits, False)
    x = np.clip(np.asarray(rgb, np.float64), 0.0, 1.0)
    f = ysr.site_rgb(x, "i420" if layout == "nv12" else layout, siting)
    fy = kr * f[..., 0] + kg * f[..., 1] + kb * f[..., 2]
    return (yo + ys * (kr * x[..., 0] + kg * x[..., 1] + kb * x[..., 2]), co + cs * (f[..., 2] - fy) / (2 * (1 - kb)), co + cs * (f[..., 0] - fy) / (2 * (1 - kr)))


def yuv_shares(tag, eng, call, c, bits, layout, mode, phase, table):
    """the dithered planes of call() against floor(c + t), the undithered ones against rint(c): every sample within 1; the share of dithered samples that are not
    exactly floor(c + t) at most twice the share of undithered ones that are not rint(c), plus 0.1 % - the yardstick is the undithered kernels' own share on the
    same frame, the factor is for fp32 boundary cases (a threshold moves every sample's boundary, rint has its boundaries at the half codes only)"""
    top = (1 << bits) - 1
    plain = call()
    with dithered(eng, mode, phase):
        got = call()
    if layout == "nv12":
        plain, got = ylr.unpack_nv12(*plain, bits), ylr.unpack_nv12(*got, bits)
    miss_d = miss_p = total = 0
    for k, name in enumerate("YUV"):
        t = ref.thresholds(mode, c[k].shape, k, phase, table).astype(np.float64)
        want = np.clip(np.floor(c[k] + t), 0, top)
        want_plain = np.clip(np.rint(c[k]), 0, top)
        assert got[k].shape == want.shape, (tag, name, got[k].shape, want.shape)
        dd, dp = np.abs(got[k].astype(np.float64) - want), np.abs(plain[k].astype(np.float64) - want_plain)
        print(f"DITHER YUV {tag} {mode} phase {phase} {name}: dithered max {int(dd.max())} not exact {float((dd != 0).mean()):.6f}; undithered max {int(dp.max())} not exact {float((dp != 0).mean()):.6f} of {dd.size}")
        assert dd.max() <= 1 and dp.max() <= 1, (tag, name, dd.max(), dp.max())
        miss_d += int((dd != 0).sum()); miss_p += int((dp != 0).sum()); total += dd.size
        assert (got[k] != plain[k]).any(), (tag, name, "the dithered plane is the undithered one")
    share_d, share_p = miss_d / total, miss_p / total
    print(f"DITHER YUV {tag} {mode} phase {phase}: share not exact dithered {share_d:.6f}, undithered {share_p:.6f}, bound {2 * share_p + 0.001:.6f}")
    assert share_d <= 2 * share_p + 0.001, (tag, mode, share_d, share_p)
    return got


def test_yuv_frames_follow_the_rule_within_a_code(engines, table, monkeypatch):
    eng, scale = engines("swin_x4_b2_blend")
    rows, cols = 45, 67
    planes = ysr.gpu_noise(rows, cols)
    canvas = oracle_canvas(eng, ysr.decode(planes, "i420", "left"), monkeypatch, **SWIN)
    # yuv420p 8 / 8, both modes
    c8 = yuv_unrounded(canvas, "i420", "left", 8)
    got420 = {m: yuv_shares("yuv420p 8/8", eng, lambda: eng.render_yuv(*planes), c8, 8, "i420", m, 2, table) for m in MODES}
    # nv12 is the yuv420p samples; Y bytes stay equal across output layouts and sitings
    with dithered(eng, "ordered", 2):
        nv = eng.render_yuv(planes, layout="i420", out_layout="nv12")
        for a, b in zip(nv, ylr.pack_nv12(*got420["ordered"])):
            same("nv12 holds the yuv420p samples", a, b)
        for kw in (dict(out_layout="i422"), dict(out_layout="i444"), dict(out_siting="center"), dict(out_siting="topleft")):
            same(f"Y plane {kw}", eng.render_yuv(planes, layout="i420", **kw)[0], got420["ordered"][0])
    # yuv444p10le out
    yuv_shares("yuv444p10le out", eng, lambda: eng.render_yuv(planes, layout="i420", out_layout="i444", out_bits=10), yuv_unrounded(canvas, "i444", "left", 10), 10, "i444",
               "bluenoise", 0, table)
    # siting = "center", both sides
    pc = ysr.gpu_noise(rows, cols)
    canvas_c = oracle_canvas(eng, ysr.decode(pc, "i420", "center"), monkeypatch, **SWIN)
    yuv_shares("center 8/8", eng, lambda: eng.render_yuv(pc, layout="i420", siting="center"), yuv_unrounded(canvas_c, "i420", "center", 8), 8, "i420", "bluenoise", 1, table)
    # one resized target, nv12 out
    size = (150, 198)
    rgb = resized(canvas, size, "bicubic")
    yuv_shares("resized 150x198 nv12", eng, lambda: eng.render_yuv_layout_resized(planes, size, layout="i420", out_layout="nv12"), yuv_unrounded(rgb, "nv12", "left", 8), 8, "nv12",
               "ordered", 3, table)
    got_r = yuv_shares("resized 150x198 i420", eng, lambda: eng.render_yuv_layout_resized(planes, size, layout="i420"), yuv_unrounded(rgb, "i420", "left", 8), 8, "i420", "bluenoise", 3, table)
    with dithered(eng, "bluenoise", 3):
        for a, b in zip(eng.render_yuv_layout_resized(planes, size, layout="i420", out_layout="nv12"), ylr.pack_nv12(*got_r)):
            same("resized nv12 holds the yuv420p samples", a, b)
        same("resized Y plane i444", eng.render_yuv_layout_resized(planes, size, layout="i420", out_layout="i444")[0], got_r[0])
        full = eng.render_yuv_layout_resized(planes, (rows * scale, cols * scale), layout="i420")
        for a, b in zip(full, eng.render_yuv(*planes)):
            same("resized at the scaled size is the plain call", a, b)


@pytest.mark.parametrize("pinned", [False, True])
def test_yuv_sequences_follow_phase_and_advance(engines, pinned):
    eng, scale = engines("swin_x4_b2_tta")
    frames = [yuv_ref.random_planes(90, 130, 8, 200 + k) for k in range(3)]
    for mode, advance in (("ordered", 1), ("bluenoise", 0), ("bluenoise", 1)):
        want = []
        for i, fr in enumerate(frames):
            with dithered(eng, mode, 4 + i * advance):
                want.append((eng.render_yuv(*fr), eng.render_yuv_layout_resized(fr, (270, 390), layout="i420", out_layout="nv12")))
        with dithered(eng, mode, 4, advance):
            got = eng.render_sequence_yuv(frames, pinned=pinned)
            got_r = eng.render_sequence_yuv_layout_resized(frames, (270, 390), layout="i420", out_layout="nv12", pinned=pinned)
        for i in range(3):
            for a, b in zip(got[i], want[i][0]):
                same(f"{mode} advance {advance} YUV frame {i}", a, b)
            for a, b in zip(got_r[i], want[i][1]):
                same(f"{mode} advance {advance} resized nv12 frame {i}", a, b)


# ---- 7. hygiene
def test_none_restores_and_refusals_leave_the_setting(engines):
    eng, scale = engines("swin_x4_b2_blend")
    r, c = 48, 64
    bgr, g, bgra = smooth_frame(r, c, 30), gray_frame(r, c, 31, "noise"), rgba_frame(r, c, 33)
    p10 = planes_of(bgr)
    yuv = yuv_ref.random_planes(r, c, 8, 34)

    def calls():
        return [eng.render(bgr), eng.render_gray(g), eng.render_rgba(bgra), interleave(eng.render_planar(p10, out_bits=10)), eng.render_resized(bgr, (100, 201)), eng.render(bgr),
                np.concatenate([p.ravel() for p in eng.render_yuv(*yuv)])]
    before = calls()
    assert eng.dither() == ("none", 0, 0)
    seen = {}
    for mode in MODES:
        assert eng.set_dither(mode, 2, 1) and eng.dither() == (mode, 2, 1)
        seen[mode] = calls()
        for k in (0, 1, 3, 4, 6):
            assert differ(seen[mode][k], before[k]), (mode, k)
        same(f"{mode}: the setting holds from call to call", seen[mode][0], seen[mode][5])      # (and does not leak between kinds: BGR after gray, RGBA, planar)
        # a refused mode leaves the previous setting and a usable engine
        del eng.messages[:]
        assert eng.set_dither(7) is False and "Unknown dither mode 7" in eng.last_error()
        assert eng.dither() == (mode, 2, 1)
        same(f"{mode}: still set after a refusal", eng.render(bgr), seen[mode][0])
        with pytest.raises(ValueError):
            eng.set_dither("floyd")
        assert eng.dither() == (mode, 2, 1)
    assert differ(seen["ordered"][0], seen["bluenoise"][0])
    assert eng.set_dither("none") and eng.dither() == ("none", 0, 0)
    for k, (a, b) in enumerate(zip(calls(), before)):
        same(f"none restores call {k}", a, b)
