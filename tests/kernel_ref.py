"""Float64 references of the fused fp16 transformer kernels (k_swinattn96.hip, k_swinattn192u.hip, k_mlp96q.hip, mlp2_kernel<192,2,4> of
k_mlp2.hip), for tests/test_gpu_transformer_kernels.py.

Every operation comes in two forms:
  * exact (`f16_model=False`): float64 throughout, no intermediate rounding - the function the kernel approximates;
  * ideal fp16 kernel (`f16_model=True`): float64 arithmetic, rounded to fp16 at the storage points the kernels document - the LayerNorm output,
    q / k / v, the probabilities, the head outputs, the projection / second-layer output, the GELU output and y.
A kernel is held to "no worse than the ideal fp16 kernel, against the exact one" (the pattern of parity_util.assert_as_accurate_as_ideal_fp16).

The LayerNorm gamma / beta are folded into the first matrix and bias, as lower.cpp does: LN here is the bare normalisation.  GELU is the exact
erf form, so the kernels' degree-4 fit (W2X_GELU_DEG) is measured, not assumed.  Inputs (rows, weights, the logical bias table) are fp16 values;
the q scale and the fp32 biases are taken as they are handed to the kernel."""
import numpy as np
from scipy.special import erf

NTOK, WS, HEADS = 36, 6, 6
LOG2E = 1.4426950408889634


def f16(a):
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def layer_norm(x, eps):
    m = x.mean(axis=-1, keepdims=True)
    v = ((x - m) ** 2).mean(axis=-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps)


def gelu(h):
    return 0.5 * h * (1.0 + erf(h / np.sqrt(2.0)))


def row_stats(y, eps):
    """LayerNorm statistics of rows (mean, rstd) as the kernels' stats_out holds them."""
    y = np.asarray(y, dtype=np.float64)
    m = y.mean(axis=-1)
    return np.stack([m, 1.0 / np.sqrt(((y - m[..., None]) ** 2).mean(axis=-1) + eps)], axis=-1)


# ---- windows
def window_table(H, W, ry, rx):
    """int32 [H*W]: window-order row (window wl = wy * W/6 + wx, token t = ty * 6 + tx) -> pixel ((wy*6+ty+ry) % H) * W + (wx*6+tx+rx) % W -
    the closed form k_swinattn*.hip evaluate for ry >= 0, and what lower.cpp stores as the explicit table."""
    nwy, nwx = H // WS, W // WS
    wy, wx, ty, tx = np.meshgrid(np.arange(nwy), np.arange(nwx), np.arange(WS), np.arange(WS), indexing="ij")
    return ((((wy * WS + ty + ry) % H) * W + (wx * WS + tx + rx) % W).reshape(-1)).astype(np.int32)


def swin_shift_masks(H, W, shift=3):
    """The Swin shift mask (-100 between tokens of different regions of the rolled map) as mask classes: (masks [nmask][36][36], maskid [nwin])."""
    def region(n):
        r = np.zeros(n, dtype=np.int64)
        r[n - WS:n - shift] = 1
        r[n - shift:] = 2
        return r
    lab = region(H)[:, None] * 3 + region(W)[None, :]
    nwy, nwx = H // WS, W // WS
    win = lab.reshape(nwy, WS, nwx, WS).transpose(0, 2, 1, 3).reshape(nwy * nwx, NTOK)
    masks = np.where(win[:, :, None] != win[:, None, :], -100.0, 0.0)
    uniq, maskid = np.unique(masks.reshape(len(masks), -1), axis=0, return_inverse=True)
    return uniq.reshape(-1, NTOK, NTOK), maskid.reshape(-1).astype(np.int32)


def pack_bias32(bias):
    """numpy restatement of fragorder.h swin_bias32: logical [nmh][36][36] (fp16 values) -> fp32 * log2(e) in the kernels' load order
    [nmh][query tile 3][key tile 0: 64 lanes x 4 | key tile 1: 64 lanes x 4 | keys 32..35: 64 lanes]."""
    b = np.asarray(bias, dtype=np.float32).reshape(-1, NTOK, NTOK) * np.float32(LOG2E)
    nmh = b.shape[0]
    lane = np.arange(64)
    fr, g = lane & 15, lane >> 4
    out = np.zeros((nmh, 3, 576), dtype=np.float32)
    for qt in range(3):
        q = np.minimum(qt * 16 + fr, NTOK - 1)
        for kt in range(2):
            keys = kt * 16 + g[:, None] * 4 + np.arange(4)[None, :]
            out[:, qt, kt * 256:(kt + 1) * 256] = b[:, q[:, None], keys].reshape(nmh, 256)
        out[:, qt, 512:576] = b[:, q, 32 + g]
    return out.reshape(-1)


def attention(x, wqkv, bqkv, wproj, bproj, bias, maskid, table, scale, eps, f16_model=False):
    """y = x + proj(W-MSA(LN(x))) on token maps x [B][H][W][C] (window-order row -> pixel: table), per-head rel-pos bias + mask
    bias [nmask][heads][36][36] selected per window by maskid [nwin]."""
    B, H, W, C = x.shape
    nwin = H * W // NTOK
    X = np.asarray(x, dtype=np.float64).reshape(B, H * W, C)[:, table].reshape(B * nwin, NTOK, C)
    bw = np.broadcast_to(np.asarray(bias, dtype=np.float64)[np.asarray(maskid)][None], (B, nwin, HEADS, NTOK, NTOK)).reshape(B * nwin, HEADS, NTOK, NTOK)
    yt = attention_windows(X, wqkv, bqkv, wproj, bproj, bw, scale, eps, f16_model).reshape(B, H * W, C)
    y = np.empty_like(yt)
    y[:, table] = yt
    return y.reshape(B, H, W, C)


def attention_windows(X, wqkv, bqkv, wproj, bproj, bw, scale, eps, f16_model=False):
    """The same on windows: X [n][36][C] tokens in window order, bw [n][heads][36][36] the bias of each window's class -> y tokens."""
    r = f16 if f16_model else (lambda a: a)
    n, _, C = X.shape
    hd = C // HEADS
    xn = r(layer_norm(X, eps))
    wq, wk, wv = (np.asarray(wqkv, dtype=np.float64)[i * C:(i + 1) * C] for i in range(3))
    bq, bk, bv = (np.asarray(bqkv, dtype=np.float64)[i * C:(i + 1) * C] for i in range(3))
    heads = lambda a: a.reshape(n, NTOK, HEADS, hd).transpose(0, 2, 1, 3)     # [n][heads][36][hd]
    if f16_model:
        # the kernels: q rounded after the scale, k without its bias (it adds the same q.bk to every key of a query: the softmax drops it),
        # v without its bias (added to the normalised output: the weighted mean commutes with it)
        q, k, v = heads(r((xn @ wq.T + bq) * scale)), heads(r(xn @ wk.T)), heads(r(xn @ wv.T))
    else:
        q, k, v = heads((xn @ wq.T + bq) * scale), heads(xn @ wk.T + bk), heads(xn @ wv.T + bv)
    s = q @ k.transpose(0, 1, 3, 2) + bw
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    if f16_model:
        e = r(e)
        o = r(e @ v / e.sum(axis=-1, keepdims=True) + bv.reshape(HEADS, 1, hd))
    else:
        o = e @ v / e.sum(axis=-1, keepdims=True)
    o = o.transpose(0, 2, 1, 3).reshape(n, NTOK, C)
    pr = r(o @ np.asarray(wproj, dtype=np.float64).T + bproj)
    return r(X + pr)


def mlp(x, w1, b1, w2, b2, eps, f16_model=False):
    """y = x + W2 gelu(W1 LN(x) + b1) + b2 on rows x [M][C] (exact erf GELU)."""
    r = f16 if f16_model else (lambda a: a)
    x = np.asarray(x, dtype=np.float64)
    h = r(layer_norm(x, eps)) @ np.asarray(w1, dtype=np.float64).T + b1
    o = r(r(gelu(h)) @ np.asarray(w2, dtype=np.float64).T + b2)
    return r(x + o)


def image_head(y, tiw, tib, B, Mrows, aW, clip=None, f16_model=False):
    """The image head folded into the C = 96 MLP: Linear 96 -> 64 per row, optional Clip, DepthToSpace(4): out[b][4 oy + dy][4 ox + dx][ch]
    = head[row b * Mrows + oy * aW + ox][16 dy + 4 dx + ch]."""
    r = f16 if f16_model else (lambda a: a)
    h = r(np.asarray(y, dtype=np.float64) @ np.asarray(tiw, dtype=np.float64).T + tib)
    if clip is not None:
        h = np.clip(h, clip[0], clip[1])
    Hr = Mrows // aW
    return h.reshape(B, Hr, aW, 4, 4, 4).transpose(0, 1, 3, 2, 4, 5).reshape(B, 4 * Hr, 4 * aW, 4)


# ---- the general implicit GEMM (kernels.h GemmParams; k_gemm.hip and the kernels specialised from it: k_stem.hip, k_conv48.hip, k_pixgemm.hip; cunet's k_conv3.hip,
# k_conv3h.hip and gated operands, for tests/test_gpu_cunet_kernels.py)
def activation(v, act, alpha=0.0):
    """GemmParams::act: 0 none, 1 LeakyReLU(alpha), 2 GELU (exact erf), 3 ReLU, 4 sigmoid."""
    if act == 1:
        return np.where(v > 0, v, v * alpha)
    if act == 2:
        return gelu(v)
    if act == 3:
        return np.maximum(v, 0.0)
    if act == 4:
        return 1.0 / (1.0 + np.exp(-v))
    return v


def gemm_ref(params, f16_model=False):
    """GemmParams restated in float64.  `params` (a dict; absent keys take the struct's defaults):
      a [B][Hs][Ws][Cs] with origin a_y0 / a_x0; amode 0 rows, 1 rows through win_table, 2 kh x kw taps at `stride` (k = (ky * kw + kx) * Cs + c);
      Mrows rows per image, row m at pixel (m // aW, m % aW) (amode 1: win_table[m] instead of m); wt [N][>= K] (columns past K ignored), bias [N];
      ln: rstd * (acc - mean * csum) with (mean, rstd) = stats_in [B][Hs][Ws][2] at the row's input pixel; act / alpha; res, res2 (maps with origins
      res_y0 / res_x0, res2_y0 / res2_x0, indexed by the OUTPUT pixel); clip (lo, hi) or None; out_shape (Hs, Ws, Cs); omode 0 rows, 1 scatter
      through win_table (pixel = divmod(table, out Ws)), 2 pixel shuffle by r with column (dy * r + dx) * Cs + c; stats (bool): (mean, rstd) over the
      Cout stored channels with ln_eps.
    Returns {"out": [B][Hs][Ws][Cs] (NaN where nothing is stored), "stats": [B][Hs][Ws][2] (likewise) or None}.
    f16_model=True rounds to fp16 where gemm_kernel stores: the activated value (its LDS tile) and the final one after the skip adds and the clip.  The
    kernels with a single store (stem_kernel, conv48_kernel, merge_kernel, toimage_kernel, pixgemm_kernel without res) round once, which is the same
    thing: with no skip add in between, the second rounding (and the clip between fp16 bounds) finds an fp16 value.
    cunet's additions:
      a_scale [B][a Cs], res_scale [B][res Cs]: squeeze-excite gates of the input map / the first skip map.  Exact: x * s unrounded; f16_model: fp16(x * s), the one
        rounding of kernels.h gate8 (and of the in-place pass scale_kernel);
      round_once=True: the activated value is NOT rounded, the skip add and the clip run on it and the result is rounded once (conv3h_kernel; f16_model only);
      N smaller than the stored channels (rows mode onto 4 stored channels, N = 3): the missing rows count as zero weights with zero bias, so a missing channel holds
        clip(act(0) + res) = clip(res);
      pool = ("rows", R) or ("tiles", TH, TW): also returns "pool" [B][tiles][N], the column sums of the stored values per workgroup (pool_sums below)."""
    g = lambda k, d=None: params.get(k, d)
    r16 = f16 if f16_model else (lambda v: v)
    a = np.asarray(params["a"], dtype=np.float64)
    B, Hs, Ws, Cs = a.shape
    once = bool(g("round_once", False))
    if g("a_scale") is not None:
        with np.errstate(invalid="ignore"):
            a = r16(a * np.asarray(params["a_scale"], dtype=np.float64).reshape(B, 1, 1, Cs))
    amode, kh, kw, stride = g("amode", 0), g("kh", 1), g("kw", 1), g("stride", 1)
    Mrows, aW, K, N = params["Mrows"], params["aW"], params["K"], params["N"]
    m = np.arange(Mrows)
    src = np.asarray(params["win_table"], dtype=np.int64)[:Mrows] if amode == 1 else m
    py, px = (src // aW) * stride + g("a_y0", 0), (src % aW) * stride + g("a_x0", 0)
    if amode == 2:
        ky, kx = np.meshgrid(np.arange(kh), np.arange(kw), indexing="ij")
        A = a[:, py[:, None, None] + ky[None], px[:, None, None] + kx[None], :].reshape(B, Mrows, kh * kw * Cs)[..., :K]
    else:
        A = a[:, py, px, :K]
    wt, bias = np.asarray(params["wt"], dtype=np.float64)[:, :K], g("bias")
    if g("omode", 0) != 2 and params["out_shape"][2] == 4 and N < 4:                  # a head of fewer than 4 channels stores 4: zero weights, zero bias
        wt = np.concatenate([wt[:N], np.zeros((4 - N, K))])
        bias = None if bias is None else np.concatenate([np.asarray(bias, dtype=np.float64)[:N], np.zeros(4 - N)])
        N = 4
    v = A @ wt.T                                                                     # [B][Mrows][N]
    if g("ln", 0):
        st = np.asarray(params["stats_in"], dtype=np.float64)[:, py, px]             # [B][Mrows][2]
        v = st[..., 1:2] * (v - st[..., 0:1] * np.asarray(params["csum"], dtype=np.float64))
    if bias is not None:
        v = v + np.asarray(bias, dtype=np.float64)
    v = activation(v, g("act", 0), g("alpha", 0.0))
    if not once:
        v = r16(v)
    oHs, oWs, oCs = params["out_shape"]
    omode, r = g("omode", 0), g("r", 1) if g("omode", 0) == 2 else 1
    dst = np.asarray(params["win_table"], dtype=np.int64)[:Mrows] if omode == 1 else m
    oy, ox = (dst // oWs, dst % oWs) if omode == 1 else (m // aW, m % aW)
    out = np.full((B, oHs, oWs, oCs), np.nan)
    stats = np.full((B, oHs, oWs, 2), np.nan) if g("stats", False) else None
    ncol = oCs if omode == 2 else N
    for sg in range(r * r):
        dy, dx = sg // r, sg % r
        Y, X = oy * r + dy, ox * r + dx
        t = v[..., sg * ncol:(sg + 1) * ncol]
        for key in ("res", "res2"):
            if g(key) is not None:
                rm = np.asarray(params[key], dtype=np.float64)[:, Y + g(key + "_y0", 0), X + g(key + "_x0", 0), :ncol]
                if key == "res" and g("res_scale") is not None:
                    rm = r16(rm * np.asarray(params["res_scale"], dtype=np.float64)[:, None, :ncol])
                t = t + rm
        if g("clip") is not None:
            t = np.clip(t, g("clip")[0], g("clip")[1])
        t = r16(t)
        out[:, Y, X, :ncol] = t
        if stats is not None:
            stats[:, Y, X] = row_stats(t[..., :g("Cout", ncol)], g("ln_eps", 1e-5))
    pool = pool_sums(out, Mrows, aW, g("pool"))[..., :N] if g("pool") is not None else None
    return {"out": out, "stats": stats, "pool": pool}


def pool_sums(out, Mrows, aW, tiling):
    """Squeeze-excite pooling partials of a rows-mode output map [B][Hs][Ws][C] whose rows m < Mrows sit at (m // aW, m % aW): float64 column sums per workgroup in
    tile order.  ("rows", R): gemm_kernel, R consecutive rows of an image; ("tiles", TH, TW): conv3_kernel, TH x TW pixel tiles in row-major tile order - the
    pixels of a ragged tile past Ho x Wo are left out."""
    out = np.asarray(out, dtype=np.float64)
    B, C = out.shape[0], out.shape[3]
    Ho, Wo = Mrows // aW, aW
    v = out[:, :Ho, :Wo]
    if tiling[0] == "rows":
        R = tiling[1]
        flat = v.reshape(B, Ho * Wo, C)
        return np.stack([flat[:, t:t + R].sum(axis=1) for t in range(0, Mrows, R)], axis=1)
    TH, TW = tiling[1], tiling[2]
    return np.stack([v[:, y:y + TH, x:x + TW].sum(axis=(1, 2)) for y in range(0, Ho, TH) for x in range(0, Wo, TW)], axis=1)


def pool_abs_counts(out, Mrows, aW, tiling):
    """For pool_sums' derived bound (n - 1) 2^-24 sum |v|: (sum |v|, n) per partial."""
    o = np.asarray(out, dtype=np.float64)
    return pool_sums(np.abs(o), Mrows, aW, tiling), pool_sums(np.ones_like(o), Mrows, aW, tiling)


def cells_read(params):
    """The reference's own index arithmetic: bool [Hs][Ws] of the input map's pixels that a stored output depends on (the same for every image), and for each skip map
    present {"res": mask, ...}.  Everything else may hold NaN."""
    g = lambda k, d=None: params.get(k, d)
    Hs, Ws = np.asarray(params["a"]).shape[1:3]
    amode, kh, kw, stride = g("amode", 0), g("kh", 1), g("kw", 1), g("stride", 1)
    Mrows, aW = params["Mrows"], params["aW"]
    m = np.arange(Mrows)
    src = np.asarray(params["win_table"], dtype=np.int64)[:Mrows] if amode == 1 else m
    py, px = (src // aW) * stride + g("a_y0", 0), (src % aW) * stride + g("a_x0", 0)
    mask = np.zeros((Hs, Ws), dtype=bool)
    for ky in range(kh if amode == 2 else 1):
        for kx in range(kw if amode == 2 else 1):
            mask[py + ky, px + kx] = True
    r = g("r", 1) if g("omode", 0) == 2 else 1
    oy, ox = m // aW, m % aW
    skips = {}
    for key in ("res", "res2"):
        if g(key) is not None:
            rm = np.zeros(np.asarray(params[key]).shape[1:3], dtype=bool)
            for dy in range(r):
                for dx in range(r):
                    rm[oy * r + dy + g(key + "_y0", 0), ox * r + dx + g(key + "_x0", 0)] = True
            skips[key] = rm
    return mask, skips


def two_launches(P1, P2, f16_model=False):
    """A fused launch as its two launches: P2 reads P1's output map (P2["a"] is ignored).  Exact: no rounding in between; f16_model: fp16 where each launch stores.
    STEM: stem -> fp16 -> conv.  UP: fp16(leaky(proj(fp16(x s)))) -> fp16(+ skip) -> conv (gemm_ref's two roundings of a launch with a skip add)."""
    mid = gemm_ref(P1, f16_model)["out"]
    return mid, gemm_ref(dict(P2, a=np.nan_to_num(mid)), f16_model)["out"]


# ---- squeeze-excite gates (k_prepost.hip se_kernel)
def se_ref(pool_partials, inv_count, w1, b1, w2, b2, dtype=np.float64):
    """gate[b][c] = sigmoid(W2 relu(W1 mean + b1) + b2), mean = inv_count * (sum of the image's partials); pool_partials [B][nblocks][>= C] (columns past C ignored),
    w1 [Cmid][C], w2 [C][Cmid].  dtype=np.float32 restates the same formula in float32 - the "ideal fp32 kernel" se_kernel is measured beside."""
    w1, b1, w2, b2 = (np.asarray(v, dtype=dtype) for v in (w1, b1, w2, b2))
    C = w1.shape[1]
    mean = np.asarray(pool_partials, dtype=dtype)[:, :, :C].sum(axis=1, dtype=dtype) * dtype(inv_count)
    mid = np.maximum(mean @ w1.T + b1, dtype(0))
    return (dtype(1) / (dtype(1) + np.exp(-(mid @ w2.T + b2)))).astype(dtype)


def se_bound(pool_partials, inv_count, w1, b1, w2, b2):
    """Derived fp32 bound Delta a on the sigmoid's argument: the partial-sum tree (n - 1 additions), the product with inv_count and the two dot products, each of L
    terms at (L + 1) 2^-24 of its sum of magnitudes, the first layer's error carried through |W2|.  [B][C]."""
    u = 2.0 ** -24
    w1, b1, w2, b2 = (np.asarray(v, dtype=np.float64) for v in (w1, b1, w2, b2))
    C, Cmid = w1.shape[1], w1.shape[0]
    pp = np.asarray(pool_partials, dtype=np.float64)[:, :, :C]
    n = pp.shape[1]
    amean = np.abs(pp).sum(axis=1) * inv_count
    dmean = (n + 1) * u * amean
    mag1 = amean @ np.abs(w1).T + np.abs(b1)
    dmid = dmean @ np.abs(w1).T + (C + 1) * u * mag1
    mid = np.maximum((pp.sum(axis=1) * inv_count) @ w1.T + b1, 0)
    mag2 = np.abs(mid) @ np.abs(w2).T + np.abs(b2)
    return dmid @ np.abs(w2).T + (Cmid + 1) * u * mag2


# ---- the large-input formula (tools/kernel_check/transformer_check.cpp gen_x16)
_M64 = (1 << 64) - 1


def gen_rows(rows, C, seed):
    """fp16 rows of the run-splitting cases at global row indices `rows`: k / 256 - 2, channels 0..2 the row index in 10-bit digits, the
    others a splitmix64 hash of (row, channel, seed) - identical to transformer_check.cpp gen_x16."""
    rows = np.asarray(rows, dtype=np.uint64)
    k = np.empty((len(rows), C), dtype=np.uint64)
    for c in range(3):
        k[:, c] = (rows >> np.uint64(10 * c)) & np.uint64(1023)
    with np.errstate(over="ignore"):
        z = rows[:, None] * np.uint64(C) + np.arange(3, C, dtype=np.uint64)[None, :] + np.uint64((seed * 0x9E3779B97F4A7C15) & _M64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    k[:, 3:] = z >> np.uint64(54)
    return (k.astype(np.float64) / 256.0 - 2.0).astype(np.float16)


# ---- metrics
def ulp16(a):
    """ULP of fp16 at |a| (normal range; subnormal spacing below 2^-14)."""
    return np.exp2(np.floor(np.log2(np.maximum(np.abs(a), 2.0 ** -14))) - 10)


def error_metrics(got, exact):
    """Error of `got` against the exact reference in units of ulp16(|exact|): max, rms, fraction within 1 ULP16, mean signed error.  |exact| is
    floored at a quarter of the tensor's rms: the outputs are sums (x + branch) whose rounding does not shrink where the sum cancels."""
    exact = np.asarray(exact, dtype=np.float64)
    floor = 0.25 * np.sqrt(np.mean(exact * exact))
    d = (np.asarray(got, dtype=np.float64) - exact) / ulp16(np.maximum(np.abs(exact), floor))
    if not np.isfinite(d).all():
        return {"max_ulp": float("inf"), "rms_ulp": float("inf"), "frac_1ulp": 0.0, "mean_ulp": float("nan"), "n": int(d.size)}
    return {"max_ulp": float(np.abs(d).max()), "rms_ulp": float(np.sqrt(np.mean(d * d))), "frac_1ulp": float((np.abs(d) <= 1.0).mean()),
            "mean_ulp": float(d.mean()), "n": int(d.size)}


# ---- the harnesses (tools/kernel_check/transformer_check.cpp, conv_check.cpp): host code only, built like the w2x command line
def build_harness(exe, source="transformer_check.cpp"):   # (cunet_check.cpp too)
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["g++", "-std=c++17", "-O2", "-fopenmp", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.join(root, "waifu2x-tensorrt_amd", "csrc"), os.path.join(root, "tools", "kernel_check", source),
                    "-o", str(exe), "-L/opt/rocm/lib", "-lamdhip64", "-ldl", "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=300)
    return str(exe)
