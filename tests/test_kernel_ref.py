"""CPU checks of the float64 references in tests/kernel_ref.py and of the host side of tools/kernel_check/transformer_check.cpp: the references
against an independent torch formulation, the packed attention bias table (fragorder.h swin_bias32, the one function lower.cpp and the harness
share) against the logical table, and the large-input formula of the C++ harness against its Python twin."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import kernel_ref as kr


def _weights(rng, n, k, s=None):
    return kr.f16(rng.normal(0, s if s is not None else 1 / np.sqrt(k), (n, k)))


def test_attention_reference_matches_torch_float64():
    rng = np.random.default_rng(1)
    for C, H, W, ry in ((96, 12, 18, 3), (192, 6, 12, 0)):
        B, hd = 2, C // 6
        x = kr.f16(rng.normal(0, 1, (B, H, W, C)))
        wqkv, wproj = _weights(rng, 3 * C, C), _weights(rng, C, C)
        bqkv, bproj = rng.normal(0, 0.1, 3 * C), rng.normal(0, 0.1, C)
        masks, maskid = kr.swin_shift_masks(H, W) if ry else (np.zeros((1, 36, 36)), np.zeros(H * W // 36, np.int32))
        bias = kr.f16(rng.normal(0, 1, (len(masks), 6, 36, 36)) + masks[:, None])
        table = kr.window_table(H, W, ry, ry)
        scale = hd ** -0.5
        got = kr.attention(x, wqkv, bqkv, wproj, bproj, bias, maskid, table, scale, 1e-5)
        # torch: roll + window partition as the ONNX graph spells it, per-window loops over heads
        t = torch.from_numpy(x).roll((-ry, -ry), dims=(1, 2))
        win = t.reshape(B, H // 6, 6, W // 6, 6, C).permute(0, 1, 3, 2, 4, 5).reshape(B, -1, 36, C)
        xn = F.layer_norm(win, (C,), eps=1e-5)
        qkv = xn @ torch.from_numpy(wqkv).T + torch.from_numpy(bqkv)
        q, k, v = (qkv[..., i * C:(i + 1) * C].reshape(B, -1, 36, 6, hd).transpose(2, 3) for i in range(3))
        a = torch.softmax(q @ k.transpose(-1, -2) * scale + torch.from_numpy(bias)[torch.from_numpy(maskid).long()], dim=-1)
        o = (a @ v).transpose(2, 3).reshape(B, -1, 36, C) @ torch.from_numpy(wproj).T + torch.from_numpy(bproj) + win
        o = o.reshape(B, H // 6, W // 6, 6, 6, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C).roll((ry, ry), dims=(1, 2))
        assert np.abs(got - o.numpy()).max() <= 1e-12
        # the ideal fp16 kernel is an fp16 evaluation of the same function: within a few fp16 ULP
        ideal = kr.attention(x, wqkv, bqkv, wproj, bproj, bias, maskid, table, scale, 1e-5, f16_model=True)
        assert kr.error_metrics(ideal, got)["max_ulp"] < 8


def test_mlp_and_head_reference_match_torch_float64():
    rng = np.random.default_rng(2)
    for C in (96, 192):
        x = kr.f16(rng.normal(0, 1, (300, C)))
        w1, w2 = _weights(rng, 2 * C, C, 3.0 / np.sqrt(C)), _weights(rng, C, 2 * C)
        b1, b2 = rng.normal(0, 0.1, 2 * C), rng.normal(0, 0.1, C)
        got = kr.mlp(x, w1, b1, w2, b2, 1e-5)
        t = torch.from_numpy(x)
        h = F.linear(F.layer_norm(t, (C,), eps=1e-5), torch.from_numpy(w1), torch.from_numpy(b1))
        ref = t + F.linear(F.gelu(h, approximate="none"), torch.from_numpy(w2), torch.from_numpy(b2))
        assert np.abs(got - ref.numpy()).max() <= 1e-12
        assert np.abs(h.numpy()).max() > 6.5      # the GELU clamp region is reached
    tiw, tib = _weights(rng, 64, 96), rng.normal(0, 0.1, 64)
    y = kr.f16(rng.normal(0, 1, (2 * 64 * 8, 96)))
    got = kr.image_head(y, tiw, tib, 2, 64 * 8, 64, clip=(0.0, 1.0))
    # DepthToSpace(4), DCR order: output column 16 dy + 4 dx + ch of row (oy, ox) -> pixel (4 oy + dy, 4 ox + dx), channel ch
    h = torch.clamp(F.linear(torch.from_numpy(y), torch.from_numpy(tiw), torch.from_numpy(tib)), 0, 1).reshape(2, 8, 64, 4, 4, 4)
    ref = h.permute(0, 1, 3, 2, 4, 5).reshape(2, 32, 256, 4)
    assert np.abs(got - ref.numpy()).max() <= 1e-12


def test_stats_reference():
    rng = np.random.default_rng(3)
    y = kr.f16(rng.normal(5, 2, (50, 96)))
    s = kr.row_stats(y, 1e-5)
    t = torch.from_numpy(y)
    assert np.abs(s[:, 0] - t.mean(-1).numpy()).max() <= 1e-12
    assert np.abs(s[:, 1] - torch.rsqrt(t.var(-1, unbiased=False) + 1e-5).numpy()).max() <= 1e-12


def test_window_table_and_shift_masks():
    t = kr.window_table(12, 18, 3, 3)
    assert sorted(t.tolist()) == list(range(12 * 18))
    masks, maskid = kr.swin_shift_masks(12, 18)
    # 2 x 3 windows: interior (unmasked) | last column | last row | corner
    m = maskid.tolist()
    assert len(masks) == 4 and m[0] == m[1] and m[3] == m[4] and len({m[0], m[2], m[3], m[5]}) == 4
    assert (masks[m[0]] == 0).all() and (masks[m[5]] == -100).sum() == 36 * 36 - 4 * 9 * 9   # the corner: four regions of 3 x 3 tokens


def test_packed_bias_table_round_trips(tmp_path):
    """fragorder.h swin_bias32 (built into the harness; lower.cpp calls the same function) against the logical table: every packed entry is
    logical * log2(e) at the (query, key) its lane order names, and the numpy restatement gives the same bits."""
    exe = kr.build_harness(tmp_path / "transformer_check")
    rng = np.random.default_rng(4)
    nmh = 4 * 6
    bias = rng.normal(0, 2, (nmh, 36, 36)).astype(np.float16)
    bias.tofile(tmp_path / "bias.bin")
    import subprocess
    subprocess.run([exe, "--pack-bias", str(tmp_path), str(nmh)], check=True, timeout=60)
    packed = np.fromfile(tmp_path / "bias32.bin", dtype=np.float32)
    assert packed.tobytes() == kr.pack_bias32(bias).tobytes()
    p = packed.reshape(nmh, 3, 576)
    lane = np.arange(64)
    fr, g = lane & 15, lane >> 4
    logical = np.full((nmh, 36, 36), np.nan, dtype=np.float32)
    for qt in range(3):
        for kt in range(2):
            for j in range(4):
                q, k = qt * 16 + fr, kt * 16 + 4 * g + j
                ok = q < 36
                logical[:, q[ok], k[ok]] = p[:, qt, kt * 256 + lane[ok] * 4 + j]
        q = qt * 16 + fr
        ok = q < 36
        logical[:, q[ok], 32 + g[ok]] = p[:, qt, 512 + lane[ok]]
    assert not np.isnan(logical).any()
    assert np.array_equal(logical, bias.astype(np.float32) * np.float32(kr.LOG2E))


def test_large_input_formula_matches_the_harness(tmp_path):
    exe = kr.build_harness(tmp_path / "transformer_check")
    rng = np.random.default_rng(5)
    for C in (96, 192):
        rows = np.concatenate([np.arange(8), rng.integers(0, 1 << 31, 500), [(1 << 30) - 1, 11_184_810, 22_369_619]]).astype(np.int64)
        rows.tofile(tmp_path / "gen.rows")
        (tmp_path / "gen.json").write_text(json.dumps({"C": C, "seed": 77, "nrows": len(rows)}))
        import subprocess
        subprocess.run([exe, "--gen-only", str(tmp_path)], check=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
        got = np.fromfile(tmp_path / "gen.bin", dtype=np.float16).reshape(-1, C)
        want = kr.gen_rows(rows, C, 77)
        assert got.tobytes() == want.tobytes()
        assert len({r.tobytes() for r in want}) == len(set(rows.tolist()))     # distinct rows stay distinct


# ---- gemm_ref (GemmParams in float64) against torch float64
def test_gemm_ref_convolutions_match_torch_conv2d():
    rng = np.random.default_rng(6)
    for (kh, stride, Cin, N, y0, x0, act) in ((3, 1, 48, 96, 1, 2, 1), (3, 1, 4, 32, 0, 0, 0), (2, 2, 96, 192, 0, 0, 0), (2, 2, 8, 16, 2, 4, 3)):
        B, Ho, Wo = 2, 5, 7
        Hs, Ws = y0 + (Ho - 1) * stride + kh + 1, x0 + (Wo - 1) * stride + kh + 2
        a = kr.f16(rng.normal(0, 1, (B, Hs, Ws, Cin)))
        w = kr.f16(rng.normal(0, 0.1, (N, Cin, kh, kh)))            # torch layout [N][C][ky][kx]
        bias = rng.normal(0, 0.1, N)
        K = kh * kh * Cin
        wt = np.zeros((N, (K + 7) // 8 * 8))
        wt[:, :K] = w.transpose(0, 2, 3, 1).reshape(N, K)           # k = (ky * kw + kx) * Cin + c
        got = kr.gemm_ref(dict(a=a, a_y0=y0, a_x0=x0, amode=2, kh=kh, kw=kh, stride=stride, Mrows=Ho * Wo, aW=Wo, K=K, N=N, wt=wt, bias=bias, act=act, alpha=0.1,
                               out_shape=(Ho + 1, Wo + 2, N)))["out"]
        t = torch.from_numpy(a).permute(0, 3, 1, 2)[:, :, y0:, x0:]
        ref = F.conv2d(t, torch.from_numpy(w), torch.from_numpy(bias), stride=stride)[:, :, :Ho, :Wo]
        ref = {0: ref, 1: F.leaky_relu(ref, 0.1), 3: F.relu(ref)}[act].permute(0, 2, 3, 1).numpy()
        assert np.abs(got[:, :Ho, :Wo] - ref).max() <= 1e-12
        assert np.isnan(got[:, Ho:]).all() and np.isnan(got[:, :, Wo:]).all()      # the rest of the view is not stored


def test_gemm_ref_pixel_shuffle_matches_torch():
    """omode 2 puts column (dy * r + dx) * Cs + c at sub-pixel (dy, dx), channel c; torch's pixel_shuffle reads channel c * r * r + dy * r + dx."""
    rng = np.random.default_rng(7)
    for r, Cs, K in ((2, 96, 192), (4, 4, 96)):
        B, H, W, N = 2, 3, 5, r * r * Cs
        a = kr.f16(rng.normal(0, 1, (B, H, W, K)))
        wt, bias = _weights(rng, N, K), rng.normal(0, 0.1, N)
        res = kr.f16(rng.normal(0, 1, (B, r * H + 2, r * W + 3, Cs)))
        got = kr.gemm_ref(dict(a=a, Mrows=H * W, aW=W, K=K, N=N, wt=wt, bias=bias, omode=2, r=r, out_shape=(r * H, r * W, Cs), res=res, res_y0=1, res_x0=2,
                               clip=(-1.0, 1.5)))["out"]
        lin = F.linear(torch.from_numpy(a), torch.from_numpy(wt), torch.from_numpy(bias))                     # [B][H][W][(dy dx c)]
        chan_major = lin.reshape(B, H, W, r * r, Cs).permute(0, 4, 3, 1, 2).reshape(B, Cs * r * r, H, W)       # [B][(c dy dx)][H][W]
        ref = F.pixel_shuffle(chan_major, r).permute(0, 2, 3, 1) + torch.from_numpy(res)[:, 1:1 + r * H, 2:2 + r * W]
        assert np.abs(got - torch.clamp(ref, -1.0, 1.5).numpy()).max() <= 1e-12


def test_gemm_ref_folded_layer_norm_matches_torch():
    """LayerNorm folded as lower.cpp does it: W' = W * gamma, csum = row sums of W', bias' = bias + W beta; the kernel gets the rows' (mean, rstd)."""
    rng = np.random.default_rng(8)
    B, H, W, C, N = 2, 4, 6, 96, 192
    a = kr.f16(rng.normal(3, 2, (B, H, W, C)))
    w, bias, gamma, beta = rng.normal(0, 0.1, (N, C)), rng.normal(0, 0.1, N), rng.normal(1, 0.1, C), rng.normal(0, 0.1, C)
    wt = w * gamma
    for act in (0, 2, 4):
        got = kr.gemm_ref(dict(a=a, Mrows=H * W, aW=W, K=C, N=N, wt=wt, bias=bias + w @ beta, ln=1, csum=wt.sum(axis=1), stats_in=kr.row_stats(a, 1e-5),
                               act=act, out_shape=(H, W, N), stats=True, Cout=N, ln_eps=1e-5))
        t = F.linear(F.layer_norm(torch.from_numpy(a), (C,), torch.from_numpy(gamma), torch.from_numpy(beta), eps=1e-5), torch.from_numpy(w), torch.from_numpy(bias))
        ref = {0: t, 2: F.gelu(t, approximate="none"), 4: torch.sigmoid(t)}[act]
        assert np.abs(got["out"] - ref.numpy()).max() <= 1e-12
        assert np.abs(got["stats"][..., 0] - ref.mean(-1).numpy()).max() <= 1e-12
        assert np.abs(got["stats"][..., 1] / torch.rsqrt(ref.var(-1, unbiased=False) + 1e-5).numpy() - 1).max() <= 1e-12


def test_gemm_ref_window_modes_match_roll_and_partition():
    rng = np.random.default_rng(9)
    B, H, W, C = 2, 12, 18, 96
    a = kr.f16(rng.normal(0, 1, (B, H, W, C)))
    wt, bias = _weights(rng, C, C), rng.normal(0, 0.1, C)
    table = kr.window_table(H, W, 3, 3)
    lin = F.linear(torch.from_numpy(a), torch.from_numpy(wt), torch.from_numpy(bias))
    # amode 1: rows come out in window order of the rolled map
    got = kr.gemm_ref(dict(a=a, amode=1, win_table=table, Mrows=H * W, aW=W, K=C, N=C, wt=wt, bias=bias, out_shape=(H, W, C)))["out"]
    win = lin.roll((-3, -3), dims=(1, 2)).reshape(B, H // 6, 6, W // 6, 6, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    assert np.abs(got - win.numpy()).max() <= 1e-12
    # omode 1: window-order rows go back to their pixels, plus a skip connection read at the OUTPUT pixel
    res = kr.f16(rng.normal(0, 1, (B, H, W, C)))
    got = kr.gemm_ref(dict(a=win.numpy(), omode=1, win_table=table, Mrows=H * W, aW=W, K=C, N=C, wt=np.eye(C), out_shape=(H, W, C), res=res))["out"]
    assert np.abs(got - (lin.numpy() + res)).max() <= 1e-12


def test_gemm_ref_fp16_model_rounds_before_and_after_the_skip_adds():
    a = np.array([[[[1.0, 0, 0, 0, 0, 0, 0, 0]]]])
    wt = np.zeros((8, 8)); wt[0, 0] = 1.0 + 2.0 ** -11 + 2.0 ** -20            # just above a tie: fp16 rounds it up to 1 + 2^-10, and the skip add makes the next tie
    res = np.full((1, 1, 1, 8), 2.0 ** -11)
    p = dict(a=a, Mrows=1, aW=1, K=8, N=8, wt=wt, out_shape=(1, 1, 8), res=res)
    exact, model = kr.gemm_ref(p)["out"][0, 0, 0, 0], kr.gemm_ref(p, f16_model=True)["out"][0, 0, 0, 0]
    assert exact == 1.0 + 2.0 ** -10 + 2.0 ** -20
    assert model == float(np.float16(np.float64(np.float16(wt[0, 0])) + 2.0 ** -11)) == 1.0 + 2.0 ** -9
    assert float(np.float16(exact)) == 1.0 + 2.0 ** -10                         # a single rounding of the exact sum lands elsewhere


# ---- cunet's additions to gemm_ref, the squeeze-excite reference
def test_gemm_ref_round_once_rounds_the_skip_sum_alone():
    """conv3h_kernel adds the skip and clips in fp32 and rounds once: the same tie as above lands on the exact sum's rounding, not on gemm_kernel's."""
    a = np.array([[[[1.0, 0, 0, 0, 0, 0, 0, 0]]]])
    wt = np.zeros((8, 8)); wt[0, 0] = 1.0 + 2.0 ** -11 + 2.0 ** -20
    res = np.full((1, 1, 1, 8), 2.0 ** -11)
    p = dict(a=a, Mrows=1, aW=1, K=8, N=8, wt=wt, out_shape=(1, 1, 8), res=res)
    twice, once = kr.gemm_ref(p, f16_model=True)["out"][0, 0, 0, 0], kr.gemm_ref(dict(p, round_once=True), f16_model=True)["out"][0, 0, 0, 0]
    assert twice == 1.0 + 2.0 ** -9 and once == 1.0 + 2.0 ** -10 == float(np.float16(kr.gemm_ref(p)["out"][0, 0, 0, 0]))
    assert kr.gemm_ref(dict(p, round_once=True))["out"][0, 0, 0, 0] == kr.gemm_ref(p)["out"][0, 0, 0, 0]      # the exact form has no rounding to move
    # the clip runs on the unrounded sum
    c = kr.gemm_ref(dict(p, round_once=True, clip=(0.0, 1.0)), f16_model=True)["out"][0, 0, 0, 0]
    assert c == 1.0


def test_gemm_ref_gates_against_an_explicit_loop():
    """a_scale / res_scale [B][C]: exact x * s unrounded; the fp16 model rounds fp16(x * s) once per element (gate8) - held against a per-element loop, for the
    rows mode, the 3x3 taps (channel = k mod Cs) and the 2x2 stride-2 taps."""
    rng = np.random.default_rng(11)
    for amode, kh, stride, Cs in ((0, 1, 1, 16), (2, 3, 1, 8), (2, 2, 2, 8)):
        B, Ho, Wo, N = 2, 2, 3, 8
        K = kh * kh * Cs
        Hs, Ws = (Ho - 1) * stride + kh + 1, (Wo - 1) * stride + kh
        a = kr.f16(rng.normal(0, 1, (B, Hs, Ws, Cs)))
        wt, bias = _weights(rng, N, K), rng.normal(0, 0.1, N)
        s, rs = rng.uniform(0.1, 0.9, (B, Cs)).astype(np.float32), rng.uniform(0.1, 0.9, (B, N)).astype(np.float32)
        res = kr.f16(rng.normal(0, 1, (B, Ho + 1, Wo + 1, N)))
        p = dict(a=a, a_y0=1, amode=amode, kh=kh, kw=kh, stride=stride, Mrows=Ho * Wo, aW=Wo, K=K, N=N, wt=wt, bias=bias, out_shape=(Ho, Wo, N), a_scale=s, res=res, res_y0=1,
                 res_x0=1, res_scale=rs)
        for model in (False, True):
            got = kr.gemm_ref(p, model)["out"]
            r = kr.f16 if model else (lambda v: v)
            for b in range(B):
                for oy in range(Ho):
                    for ox in range(Wo):
                        for n in range(N):
                            acc = 0.0
                            for ky in range(kh):
                                for kx in range(kh):
                                    for c in range(Cs):
                                        x = float(r(a[b, oy * stride + 1 + ky, ox * stride + kx, c] * np.float64(s[b, c])))
                                        acc += x * wt[n, (ky * kh + kx) * Cs + c]
                            v = float(r(acc + bias[n]))
                            v = float(r(v + float(r(res[b, oy + 1, ox + 1, n] * np.float64(rs[b, n])))))
                            assert abs(got[b, oy, ox, n] - v) <= 1e-12, (amode, model)
        # the gate's rounding is visible: the model differs from the exact form by more than the two output roundings alone would allow somewhere
        assert np.abs(kr.gemm_ref(p, True)["out"] - kr.gemm_ref(p)["out"]).max() > 0


def test_gemm_ref_short_head_counts_missing_rows_as_zero():
    rng = np.random.default_rng(12)
    B, Ho, Wo, Cin = 2, 3, 4, 8
    a = kr.f16(rng.normal(0, 1, (B, Ho + 2, Wo + 2, Cin)))
    wt, bias = _weights(rng, 3, 9 * Cin), rng.normal(0.5, 0.1, 3)
    res = kr.f16(rng.normal(0.5, 1.0, (B, Ho, Wo, 4)))
    p = dict(a=a, amode=2, kh=3, kw=3, Mrows=Ho * Wo, aW=Wo, K=9 * Cin, N=3, wt=wt, bias=bias, out_shape=(Ho, Wo, 4), res=res, clip=(0.0, 1.0), round_once=True)
    full = dict(p, N=4, wt=np.concatenate([wt, np.zeros((1, wt.shape[1]))]), bias=np.concatenate([bias, [0.0]]))
    for model in (False, True):
        got = kr.gemm_ref(p, model)["out"]
        assert np.array_equal(got, kr.gemm_ref(full, model)["out"])
        assert np.array_equal(got[..., 3], np.clip(res[..., 3], 0.0, 1.0))
    assert np.array_equal(kr.gemm_ref(dict(p, res=None, clip=None))["out"][..., 3], np.zeros((B, Ho, Wo)))


def test_pool_sums_tile_orders():
    rng = np.random.default_rng(13)
    B, Ho, Wo, C = 2, 9, 65, 8
    out = np.full((B, Ho + 1, Wo + 2, C), np.nan)
    out[:, :Ho, :Wo] = rng.normal(0, 1, (B, Ho, Wo, C))
    rows = kr.pool_sums(out, Ho * Wo, Wo, ("rows", 128))
    assert rows.shape == (B, 5, C)
    flat = out[:, :Ho, :Wo].reshape(B, -1, C)
    for t in range(5):
        assert np.allclose(rows[:, t], flat[:, 128 * t:128 * (t + 1)].sum(axis=1), rtol=0, atol=1e-12)
    tiles = kr.pool_sums(out, Ho * Wo, Wo, ("tiles", 8, 64))
    assert tiles.shape == (B, 4, C)
    want = [out[:, :8, :64], out[:, :8, 64:65], out[:, 8:9, :64], out[:, 8:9, 64:65]]          # row-major tile order, the ragged tiles hold 8, 64 and 1 pixels
    for t in range(4):
        assert np.allclose(tiles[:, t], want[t].sum(axis=(1, 2)), rtol=0, atol=1e-12)
    assert np.allclose(rows.sum(axis=1), tiles.sum(axis=1), rtol=0, atol=1e-10)
    mag, n = kr.pool_abs_counts(out, Ho * Wo, Wo, ("tiles", 8, 64))
    assert np.array_equal(n[0, :, 0], [512, 8, 64, 1]) and (mag >= np.abs(tiles)).all()
    got = kr.gemm_ref(dict(a=np.ones((1, 1, 130, 8)), Mrows=130, aW=130, K=8, N=8, wt=np.eye(8), out_shape=(1, 130, 8), pool=("rows", 128)))["pool"]
    assert np.array_equal(got[0, :, 0], [128.0, 2.0])


def test_cells_read_is_the_reference_gather():
    """Whatever cells_read leaves out may hold NaN without touching gemm_ref's stored outputs; and every cell it keeps reaches one."""
    rng = np.random.default_rng(14)
    a = kr.f16(rng.normal(0, 1, (2, 9, 11, 8)))
    wt = _weights(rng, 8, 72)
    res = kr.f16(rng.normal(0, 1, (2, 6, 8, 8)))
    p = dict(a=a, a_y0=1, a_x0=2, amode=2, kh=3, kw=3, Mrows=4 * 5, aW=5, K=72, N=8, wt=wt, out_shape=(5, 6, 8), res=res, res_y0=1, res_x0=2)
    mask, skips = kr.cells_read(p)
    assert mask.sum() == 6 * 7 and mask[1:7, 2:9].all() and skips["res"].sum() == 20 and skips["res"][1:5, 2:7].all()
    q = dict(p, a=a.copy(), res=res.copy())
    q["a"][:, ~mask] = np.nan
    q["res"][:, ~skips["res"]] = np.nan
    want, got = kr.gemm_ref(p)["out"], kr.gemm_ref(q)["out"]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    q["a"][0, 1, 2, 0] = np.nan                                   # a cell it keeps
    assert np.isnan(kr.gemm_ref(q)["out"][0, 0, 0]).all()
    m2, _ = kr.cells_read(dict(a=a, amode=2, kh=2, kw=2, stride=2, Mrows=6, aW=3, K=32, N=8, wt=wt, out_shape=(2, 3, 8)))
    assert m2.sum() == 24 and m2[:4, :6].all()


def test_two_launches_is_conv_of_conv():
    rng = np.random.default_rng(15)
    a = kr.f16(rng.normal(0, 1, (1, 9, 9, 4)))
    w1, w2 = kr.f16(rng.normal(0, 0.3, (8, 4, 3, 3))), kr.f16(rng.normal(0, 0.2, (8, 8, 3, 3)))
    flat = lambda w: w.transpose(0, 2, 3, 1).reshape(w.shape[0], -1)
    wt1 = np.zeros((8, 40)); wt1[:, :36] = flat(w1)
    P1 = dict(a=a, amode=2, kh=3, kw=3, Mrows=49, aW=7, K=36, N=8, wt=wt1, act=1, alpha=0.1, out_shape=(7, 7, 8))
    P2 = dict(a=None, a_y0=1, a_x0=1, amode=2, kh=3, kw=3, Mrows=16, aW=4, K=72, N=8, wt=flat(w2), out_shape=(4, 4, 8))
    mid, out = kr.two_launches(P1, P2)
    t = F.leaky_relu(F.conv2d(torch.from_numpy(a).permute(0, 3, 1, 2), torch.from_numpy(w1)), 0.1)
    ref = F.conv2d(t[:, :, 1:, 1:], torch.from_numpy(w2))[:, :, :4, :4].permute(0, 2, 3, 1).numpy()
    assert np.abs(mid - t.permute(0, 2, 3, 1).numpy()).max() <= 1e-12 and np.abs(out - ref).max() <= 1e-12
    mid16, out16 = kr.two_launches(P1, P2, True)
    assert np.array_equal(mid16, kr.f16(mid16)) and np.array_equal(out16, kr.f16(out16)) and np.abs(mid16 - mid).max() > 0


def test_se_ref_matches_torch_float64():
    rng = np.random.default_rng(16)
    B, nb, C, Cm = 3, 5, 64, 8
    pp = rng.normal(0, 30, (B, nb, C + 8))                       # (columns past C are ignored)
    w1, b1, w2, b2 = rng.normal(0, 0.2, (Cm, C)), rng.normal(0, 0.2, Cm), rng.normal(0, 0.5, (C, Cm)), rng.normal(0, 0.5, C)
    inv = 1.0 / 585
    got = kr.se_ref(pp, inv, w1, b1, w2, b2)
    mean = torch.from_numpy(pp[:, :, :C]).sum(dim=1) * inv
    ref = torch.sigmoid(F.linear(F.relu(F.linear(mean, torch.from_numpy(w1), torch.from_numpy(b1))), torch.from_numpy(w2), torch.from_numpy(b2)))
    assert got.dtype == np.float64 and np.abs(got - ref.numpy()).max() <= 1e-14
    f32 = kr.se_ref(pp, inv, w1, b1, w2, b2, dtype=np.float32)
    assert f32.dtype == np.float32
    d = np.abs(f32.astype(np.float64) - got)
    assert 0 < d.max() <= (0.25 * kr.se_bound(pp, inv, w1, b1, w2, b2) + 4 * 2.0 ** -24 * got).max()       # an fp32 evaluation sits inside the derived bound
    # the bound sees a partial that is off by one part in 100 (these partials cancel: the worst-case bound is a few 1e-5)
    pp2 = pp.copy(); pp2[:, 0, :C] *= 1.01
    assert (np.abs(kr.se_ref(pp2, inv, w1, b1, w2, b2) - got) > 0.25 * kr.se_bound(pp, inv, w1, b1, w2, b2) + 16 * 2.0 ** -24 * got).any()
