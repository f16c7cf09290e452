"""The convolution and projection kernels of swin_unet's path alone - gemm_kernel (k_gemm.hip, every instantiation these cases select), stem_kernel,
conv48_kernel<false> / <true>, pixgemm_kernel, merge_kernel and toimage_kernel - against the float64 reference kernel_ref.gemm_ref, through the library as
built (tools/kernel_check/conv_check.cpp finds w2x::launch_* and *_supported of libw2x.so by name, so the code objects are the shipped ones).

Every case prints one KERNEL {json} line (errors in ULP16 of the exact reference; the same for the ideal fp16 kernel, gemm_ref(f16_model=True)) and is held
to the scheme of tests/test_gpu_transformer_kernels.py, with tighter constants (that file's are the ceilings):
  * max <= the ideal fp16 kernel's max + REL_MAX_ALLOW, rms <= REL_RMS_FACTOR x its rms, |mean signed error| <= |its| + MEAN_ALLOW;
  * the fraction within 1 ULP16 >= FRAC_FLOOR_MARGIN under the measured one (tests/golden/conv_kernel_frac.json, profiles/kernel_check/);
  * single-store kernels (everything but a launch with a skip add): per element |err| <= 0.5 ULP16(result) + K 2^-23 sum |a w|, K the reduction length
    (twice the worst case of K fp32 roundings; the bias is the initial accumulator and counts as a term);
  * statistics outputs against float64 statistics of the kernel's own stored rows;
  * cells of the output view that no row maps to, and the guard bands, unchanged; two runs bit-identical; the first image alone bit-identical.
Every specialised case also runs on launch_gemm ("@gemm" records; the two outputs' difference in ULP16 is recorded).  Mutants (one value handed to the
kernel changed, the reference keeping the true one) must fail those bounds.  The four run-splitting / 32-bit-offset cases put a map just under each
specialised predicate's limit, and a Linear just past launch_gemm's 2^31 halves, and check sampled pixels."""
import json
import os
import subprocess
import time

import numpy as np
import pytest

import kernel_ref as kr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "waifu2x-tensorrt_amd", "libw2x.so")
_OUT = os.environ.get("W2X_KERNEL_CHECK_OUT")      # the KERNEL records are appended there as JSON lines (profiles/kernel_check/conv_check.jsonl)

# Bounds (profiles/kernel_check/record.txt, conv_check.jsonl).  The transformer file's constants (2.0, 1.10, 0.03) are ceilings; these kernels have no fitted
# function and no intermediate store the ideal kernel lacks, so they part from it by their fp32 accumulation alone: largest measured excess of max 0.015 ULP16
# (gemm_ln_offset, the cancellation case; 0.0013 elsewhere), rms ratio <= 1.001, |mean| excess <= 0.001.  The margins leave about ten times that.
REL_MAX_ALLOW = 0.25     # ULP16 over the ideal fp16 kernel's max
REL_RMS_FACTOR = 1.02    # on its rms
MEAN_ALLOW = 0.01        # ULP16 over the ideal kernel's |mean signed error|, plus 4 standard errors of the mean
FRAC_FLOOR_MARGIN = 0.005
STATS_RSTD_REL = 2.0e-6
STATS_MEAN_REL = 2.0e-7
EPS = 1e-5
with open(os.path.join(ROOT, "tests", "golden", "conv_kernel_frac.json")) as _f:
    FRAC_MEASURED = json.load(_f)                 # measured fraction within 1 ULP16 per record (seeded inputs, deterministic kernels)

PIX_MAX = 0xFFFF0000                              # pixgemm_supported: bytes of any map of pixgemm_kernel / merge_kernel
CONV48_MAX = (1 << 32) - 65536                    # conv48_supported: bytes of the input map
GEMM_MAX = (1 << 31) - 1                          # launch_gemm: halves of a (pixels of the other maps) per run


def f16a(a):
    return np.asarray(a, dtype=np.float64).astype(np.float16)


def data(rng, shape, kind="normal"):
    if kind == "normal":
        return f16a(rng.normal(0, 1, shape))
    if kind == "offset":        # |mean| / std ~ 30 per row: cancellation in rstd * (acc - mean * csum)
        return f16a(rng.choice([-30.0, 30.0], shape[:-1] + (1,)) + rng.normal(0, 1, shape))
    if kind == "wide":          # |x| up to 64
        return f16a(np.clip(rng.normal(0, 16, shape), -64, 64))
    raise ValueError(kind)


def weights(rng, N, K):
    """[N][Kw] fp16 values, Kw = K rounded up to 8 and zero padded, and an fp32 bias."""
    Kw = (K + 7) // 8 * 8
    w = np.zeros((N, Kw))
    w[:, :K] = rng.normal(0, K ** -0.5, (N, K))
    return f16a(w), rng.normal(0, 0.2, N).astype(np.float32)


class Suite:
    def __init__(self, d):
        self.dir, self.cases, self.meta = d, [], {}

    def put(self, name, arr):
        np.ascontiguousarray(arr).tofile(os.path.join(self.dir, name))
        return name

    def read(self, name, dtype, shape):
        return np.fromfile(os.path.join(self.dir, name), dtype=dtype).reshape(shape)


def spec_numbers(P, pre=""):
    a = P["a"]
    s = {"B": a.shape[0], "aHs": a.shape[1], "aWs": a.shape[2], "aCs": a.shape[3], "ay0": P.get("a_y0", 0), "ax0": P.get("a_x0", 0),
         "amode": P.get("amode", 0), "kh": P.get("kh", 1), "kw": P.get("kw", 1), "stride": P.get("stride", 1), "Mrows": P["Mrows"], "aW": P["aW"],
         "K": P["K"], "N": P["N"], "Kw": P["wt"].shape[1], "ln": P.get("ln", 0), "act": P.get("act", 0), "alpha": P.get("alpha", 0.0),
         "oHs": P["out_shape"][0], "oWs": P["out_shape"][1], "oCs": P["out_shape"][2], "omode": P.get("omode", 0), "r": P.get("r", 1),
         "Cout": P.get("Cout", P["out_shape"][2]), "ln_eps": P.get("ln_eps", EPS)}
    if P.get("clip") is not None:
        s.update(has_clip=1, clip_lo=P["clip"][0], clip_hi=P["clip"][1])
    for key, k in (("res", "r"), ("res2", "r2")):
        if P.get(key) is not None:
            m = P[key]
            s.update({k + "Hs": m.shape[1], k + "Ws": m.shape[2], k + "Cs": m.shape[3], k + "y0": P.get(key + "_y0", 0), k + "x0": P.get(key + "_x0", 0)})
    return {pre + k: v for k, v in s.items()}


def spec_files(S, name, P, pre=""):
    s = {"wt": S.put(name + f".{pre}wt", f16a(P["wt"])), "bias": S.put(name + f".{pre}bias", np.asarray(P["bias"], np.float32))}
    if "a" in P and not P.get("a_is_mid"):
        s["a"] = S.put(name + f".{pre}a", f16a(P["a"]))
    if P.get("ln"):
        s["csum"] = S.put(name + ".csum", np.asarray(P["csum"], np.float32))
        s["stats_in"] = S.put(name + ".stats_in", np.asarray(P["stats_in"], np.float32))
    if P.get("win_table") is not None:
        s["win_table"] = S.put(name + ".win_table", np.asarray(P["win_table"], np.int32))
    for key in ("res", "res2"):
        if P.get(key) is not None:
            s[key] = S.put(name + "." + key, f16a(P[key]))
    return {pre + k: v for k, v in s.items()}


def gcase(S, name, launcher, P, also_gemm=None, mutate="", single_store=None):
    """One parameter set P (gemm_ref's dict; "stats": statistics wanted) on `launcher`, and on launch_gemm too unless it IS launch_gemm."""
    also = launcher != "gemm" if also_gemm is None else also_gemm
    spec = dict(kind="gemm", name=name, launcher=launcher, also_gemm=int(also), stats=int(bool(P.get("stats"))), mutate=mutate)
    spec.update(spec_numbers(P))
    spec.update(spec_files(S, name, P))
    S.cases.append(spec)
    if single_store is None:
        single_store = P.get("res") is None and P.get("res2") is None and P.get("act", 0) in (0, 1) and not P.get("ln")
    S.meta[name] = dict(P=P, launcher=launcher, also=also, single_store=single_store, mutate=mutate)


# ---------------------------------------------------------------- parameter sets
def linear(rng, K, N, B, H, W, kind="normal", **extra):
    wt, bias = weights(rng, N, K)
    P = dict(a=data(rng, (B, H, W, K), kind), Mrows=H * W, aW=W, K=K, N=N, wt=wt, bias=bias, out_shape=(H, W, N))
    P.update(extra)
    return P


def with_ln(P):
    a = P["a"].astype(np.float64)
    P.update(ln=1, csum=P["wt"].astype(np.float64).sum(axis=1).astype(np.float32), stats_in=kr.row_stats(a, EPS).astype(np.float32))
    return P


def conv(rng, kh, stride, Cin, N, B, Ho, Wo, y0=0, x0=0, pad=(0, 0), opad=(0, 0), act=0, alpha=0.1, kind="normal"):
    """kh x kh taps at `stride`; the input view `pad` larger than needed behind the origin, the output view `opad` larger than Ho x Wo."""
    K = kh * kh * Cin
    wt, bias = weights(rng, N, K)
    a = data(rng, (B, y0 + (Ho - 1) * stride + kh + pad[0], x0 + (Wo - 1) * stride + kh + pad[1], Cin), kind)
    return dict(a=a, a_y0=y0, a_x0=x0, amode=2, kh=kh, kw=kh, stride=stride, Mrows=Ho * Wo, aW=Wo, K=K, N=N, wt=wt, bias=bias, act=act, alpha=alpha,
                out_shape=(Ho + opad[0], Wo + opad[1], N))


def shuffle(rng, K, Cso, r, B, H, W, res=None, act=0, clip=None, kind="normal", stats=False, opad=(0, 0)):
    """Linear K -> r r Cso + pixel shuffle; res = (y0, x0): a skip map with that origin and one spare row / column behind it."""
    N = r * r * Cso
    wt, bias = weights(rng, N, K)
    P = dict(a=data(rng, (B, H, W, K), kind), Mrows=H * W, aW=W, K=K, N=N, wt=wt, bias=bias, act=act, alpha=0.1, omode=2, r=r,
             out_shape=(r * H + opad[0], r * W + opad[1], Cso), Cout=Cso, stats=stats)
    if res is not None:
        P.update(res=data(rng, (B, r * H + res[0] + 1, r * W + res[1] + 1, Cso)), res_y0=res[0], res_x0=res[1])
    if clip is not None:
        P["clip"] = clip
    return P


def pair_case(S, rng, name, Ho, Wo, act):
    """stem (4 -> 48, origin (2, 3)) -> conv48 (origin (1, 2) of the stem's map, one spare row / column) - as two launches and as conv48_kernel<true>."""
    sHo, sWo = 1 + Ho + 2 + 1, 2 + Wo + 2 + 1
    Ps = conv(rng, 3, 1, 4, 48, 2, sHo, sWo, y0=2, x0=3, act=1, alpha=0.1)
    Ps["a"][..., 3] = data(rng, Ps["a"].shape[:-1])          # the fourth stored channel is not zero here, nor are its weights
    Pc = conv(rng, 3, 1, 48, 96, 2, Ho, Wo, y0=1, x0=2, pad=(1, 1), opad=(1, 2), act=act, alpha=0.2)
    assert Pc["a"].shape[1:3] == (sHo, sWo)
    Pc["a_is_mid"] = True
    spec = dict(kind="pair", name=name)
    spec.update(spec_numbers(Pc)); spec.update(spec_files(S, name, Pc))
    spec.update(spec_numbers(Ps, "s_")); spec.update(spec_files(S, name, Ps, "s_"))
    S.cases.append(spec)
    S.meta[name] = dict(pair=(Ps, Pc))


def build_suite(d):
    S = Suite(d)
    rng = np.random.default_rng(1019)
    g = lambda name, P, **k: gcase(S, "gemm_" + name, "gemm", P, **k)
    # ---- gemm_kernel: rows around the 128-row tile, images never sharing a tile
    for B in (1, 3):
        for rows in (1, 127, 128, 129):
            g(f"lin96_r{rows}_B{B}", linear(rng, 96, 96, B, 1, rows))
    g("lin192x384", linear(rng, 192, 384, 3, 1, 129))                   # two column tiles
    g("lin72x48", linear(rng, 72, 48, 3, 1, 129))                       # KB 64, ragged last k-chunk
    g("lin64x32", linear(rng, 64, 32, 3, 1, 129))
    g("lin96_wide", linear(rng, 96, 96, 3, 1, 129, kind="wide"))
    g("ln_normal", with_ln(linear(rng, 96, 96, 3, 1, 129)))
    g("ln_offset", with_ln(linear(rng, 96, 96, 3, 1, 129, kind="offset")))
    for act in (1, 2, 3, 4):
        g(f"act{act}", linear(rng, 96, 96, 1, 1, 129, act=act, alpha=0.1))
    r1, r2 = data(rng, (3, 8, 11, 96)), data(rng, (3, 6, 9, 96))
    g("res_res2", linear(rng, 96, 96, 3, 5, 7, res=r1, res_y0=1, res_x0=2, res2=r2, res2_y0=1, res2_x0=1))
    g("res_clip", linear(rng, 96, 96, 3, 5, 7, res=r1, res_y0=2, res_x0=3, clip=(-0.5, 0.75)))
    tab = kr.window_table(12, 18, 3, 3)
    g("amode1_ln", with_ln(linear(rng, 96, 96, 3, 12, 18, amode=1, win_table=tab)))
    g("omode1_res", linear(rng, 96, 96, 3, 12, 18, omode=1, win_table=tab, res=data(rng, (3, 12, 18, 96))))
    g("conv3x3_48", conv(rng, 3, 1, 48, 96, 3, 5, 7, y0=1, x0=2, pad=(1, 1), act=1))      # K = 432, KB 64
    for N in (32, 48, 64):
        g(f"conv3x3_4ch_N{N}", conv(rng, 3, 1, 4, N, 3, 3, 17, y0=2, x0=3, act=1), single_store=True)   # K = 36, Kw = 40
    g("conv2x2s2_96", conv(rng, 2, 2, 96, 192, 3, 3, 5))
    g("shuf96", shuffle(rng, 192, 96, 2, 3, 5, 7))                       # bn = 96
    g("shuf96_res", shuffle(rng, 192, 96, 2, 3, 5, 7, res=(1, 2)))
    g("shuf192_stats", shuffle(rng, 192, 192, 2, 3, 5, 7, stats=True))   # bn = 192
    g("shuf4_clip", shuffle(rng, 96, 4, 4, 3, 5, 7, clip=(0.0, 1.0)))    # OP = 4
    g("stats96", linear(rng, 96, 96, 3, 1, 129, stats=True, Cout=96))
    g("stats192", linear(rng, 96, 192, 3, 1, 129, stats=True, Cout=192))
    # ---- stem_kernel: a workgroup per output row, 16-pixel groups; the output view wider and taller than Ho x Wo
    i = 0
    for N in (32, 48, 64):
        for Wo in (1, 15, 16, 17, 65):
            for Ho in (1, 3):
                P = conv(rng, 3, 1, 4, N, 2, Ho, Wo, y0=(0, 2)[i % 2], x0=(0, 3)[i % 2], pad=(0, 1), opad=(1, 2), act=(i // 2) % 2, kind="wide" if i % 7 == 3 else "normal")
                P["a"][..., 3] = data(rng, P["a"].shape[:-1])            # a non-zero fourth input channel, with non-zero weights
                gcase(S, f"stem_N{N}_{Ho}x{Wo}", "stem", P)
                i += 1
    # ---- conv48_kernel: 4 x 64 tiles; alone on a random map, and behind the stem (two launches / fused)
    for Ho, Wo in ((1, 1), (3, 63), (4, 64), (5, 65), (9, 130)):
        for act in (0, 1):
            gcase(S, f"conv48_{Ho}x{Wo}_act{act}", "conv48", conv(rng, 3, 1, 48, 96, 2, Ho, Wo, y0=1, x0=2, pad=(1, 1), opad=(1, 2), act=act, alpha=0.2,
                                                               kind="wide" if (Ho, act) == (5, 1) else "normal"))
            pair_case(S, rng, f"pair_{Ho}x{Wo}_act{act}", Ho, Wo, act)
    # ---- merge_kernel: 128 output pixels per workgroup straddle output rows and images
    i = 0
    for Cin in (96, 192):
        for Ho, Wo in ((1, 1), (3, 5), (8, 16), (9, 15)):
            for B in (1, 3):
                P = conv(rng, 2, 2, Cin, 192, B, Ho, Wo, y0=i % 2, x0=i % 2, pad=(i % 2, i % 2), act=(i // 2) % 2, kind="wide" if i == 3 else "normal")
                gcase(S, f"merge{Cin}_{Ho}x{Wo}_B{B}", "pixgemm", P)
                i += 1
    # ---- pixgemm_kernel: 192 -> 4 x 96 (128 rows per workgroup), 192 -> 4 x 192 (64)
    for Cso, BM in ((96, 128), (192, 64)):
        for M in (1, BM - 1, BM, BM + 1):
            gcase(S, f"pix{Cso}_M{M}", "pixgemm", shuffle(rng, 192, Cso, 2, 1, 1, M, act=M % 2))
        gcase(S, f"pix{Cso}_5x7_B3", "pixgemm", shuffle(rng, 192, Cso, 2, 3, 5, 7))
        gcase(S, f"pix{Cso}_5x7_B3_res", "pixgemm", shuffle(rng, 192, Cso, 2, 3, 5, 7, res=(1, 2), act=1, opad=(1, 1)))
        gcase(S, f"pix{Cso}_5x7_B3_wide", "pixgemm", shuffle(rng, 192, Cso, 2, 3, 5, 7, res=(0, 0), kind="wide"))
    # ---- toimage_kernel: 256 rows per workgroup
    for M in (1, 255, 256, 257):
        gcase(S, f"toimage_M{M}", "pixgemm", shuffle(rng, 96, 4, 4, 1, 1, M, clip=(0.0, 1.0) if M % 2 else None))
    gcase(S, "toimage_5x7_B9_clip", "pixgemm", shuffle(rng, 96, 4, 4, 9, 5, 7, clip=(0.0, 1.0)))     # image boundaries inside a workgroup
    gcase(S, "toimage_5x7_B9_wide", "pixgemm", shuffle(rng, 96, 4, 4, 9, 5, 7, kind="wide"))
    # the folded head of launch_mlp against launch_mlp + toimage_kernel (the transformer file's shape and weight recipe)
    C = 96
    mw = {"w1": f16a(rng.normal(0, C ** -0.5, (2 * C, C))), "b1": rng.normal(0, 0.2, 2 * C).astype(np.float32), "w2": f16a(rng.normal(0, (2 * C) ** -0.5, (C, 2 * C))),
          "b2": rng.normal(0, 0.2, C).astype(np.float32), "tiw": f16a(rng.normal(0, C ** -0.5, (64, C))), "tib": rng.normal(0.5, 0.2, 64).astype(np.float32)}
    for k, v in mw.items():
        S.put("m96." + k, v)
    for clip in (0, 1):
        name = f"tihead_clip{clip}"
        S.cases.append(dict(kind="tihead", name=name, w="m96", B=2, Mrows=192, aW=48, has_clip=clip, clip_lo=0.0, clip_hi=1.0, x=S.put(name + ".x", data(rng, (384, C)))))
        S.meta[name] = dict(tihead=True)
    # ---- mutants: the kernel is handed one changed value
    mut = lambda base, m: gcase(S, f"{base}~{m}", S.meta[base]["launcher"], S.meta[base]["P"], mutate=m, single_store=S.meta[base]["single_store"])
    for base in ("conv48_5x65_act1", "stem_N48_3x65", "gemm_conv3x3_48"):
        mut(base, "wt_transpose_taps")
        mut(base, "ax0+1")
    mut("pix96_5x7_B3", "subpixel_swap"); mut("gemm_shuf96", "subpixel_swap"); mut("toimage_5x7_B9_clip", "subpixel_swap")
    mut("pix96_5x7_B3_res", "res_origin+1"); mut("gemm_res_clip", "res_origin+1")
    for delta in (0.03125, 0.00390625, 0.00048828125):
        mut("merge96_8x16_B3", f"bias_delta={delta}")
    mut("stem_N48_3x65", "alpha"); mut("conv48_5x65_act1", "alpha"); mut("pix96_5x7_B3_res", "alpha")
    mut("toimage_5x7_B9_clip", "clip_hi"); mut("gemm_res_clip", "clip_hi")
    mut("gemm_ln_offset", "csum")
    mut("gemm_stats96", "ln_eps"); mut("gemm_shuf192_stats", "ln_eps")
    mut("gemm_amode1_ln", "table_swap"); mut("gemm_omode1_res", "table_swap")
    # ---- refusals (launch_gemm answers from the sizes alone) and the predicate audit (no launch)
    tiny = dict(B=1, aHs=1, aWs=1, aCs=8, Mrows=1, aW=1, K=8, Kw=8, oHs=1, oWs=1)

    def ref(name, **k):
        S.cases.append(dict(dict(tiny, kind="refuse", name="refuse_" + name), **k))
        S.meta["refuse_" + name] = dict(refuse=True)
    ref("N80", N=80, oCs=80)
    ref("stats_N384", N=384, oCs=384, stats=1)
    ref("aCs4_N96", aCs=4, amode=2, kh=3, kw=3, aHs=3, aWs=3, K=36, Kw=40, N=96, oCs=96)
    ref("one_image_past_2G_halves", aHs=3345, aWs=3345, aCs=192, Mrows=3345 * 3345, aW=3345, K=192, Kw=192, N=192, oHs=3345, oWs=3345, oCs=192)   # 2 148 244 800 halves
    merge_ok = dict(B=2, aHs=10, aWs=12, aCs=96, amode=2, kh=2, kw=2, stride=2, Mrows=30, aW=6, K=384, Kw=384, N=192, oHs=5, oWs=6, oCs=192)
    pix_ok = dict(B=2, aHs=5, aWs=7, aCs=192, Mrows=35, aW=7, K=192, Kw=192, N=384, oHs=10, oWs=14, oCs=96, omode=2, r=2, rHs=11, rWs=16, rCs=96, ry0=1, rx0=2)
    head_ok = dict(B=2, aHs=5, aWs=7, aCs=96, Mrows=35, aW=7, K=96, Kw=96, N=64, oHs=20, oWs=28, oCs=4, omode=2, r=4)
    conv48_ok = dict(B=2, aHs=8, aWs=12, aCs=48, ay0=1, ax0=2, amode=2, kh=3, kw=3, Mrows=5 * 8, aW=8, K=432, Kw=432, N=96, oHs=5, oWs=8, oCs=96)
    stem_ok = dict(B=2, aHs=10, aWs=14, aCs=4, amode=2, kh=3, kw=3, Mrows=8 * 12, aW=12, K=36, Kw=40, N=48, oHs=8, oWs=12, oCs=48, act=1, alpha=0.1)

    def pred(name, which, want, base, **k):
        S.cases.append(dict(dict(base, kind="predicate", name="pred_" + name, pred=which), **k))
        S.meta["pred_" + name] = dict(predicate=want)
    pred("merge_ok", "pixgemm", True, merge_ok)
    pred("merge_rows_past_view", "pixgemm", False, merge_ok, aHs=9)               # a.y0 + 2 Ho > a.Hs
    pred("merge_cols_past_view", "pixgemm", False, merge_ok, aWs=11)
    pred("merge_origin_past_view", "pixgemm", False, merge_ok, ay0=1)
    pred("merge_negative_origin", "pixgemm", False, merge_ok, ax0=-1)
    pred("merge_map_at_limit", "pixgemm", False, merge_ok, B=1, aHs=4730, aWs=4730, Mrows=2365 * 2365, aW=2365, oHs=2365, oWs=2365)   # 4 295 596 800 B
    pred("pix_ok", "pixgemm", True, pix_ok)
    pred("pix_out_too_narrow", "pixgemm", False, pix_ok, oWs=13)
    pred("pix_out_too_short", "pixgemm", False, pix_ok, oHs=9)
    pred("pix_res_rows_past_view", "pixgemm", False, pix_ok, rHs=10)              # res.y0 + 2 H > res.Hs
    pred("pix_res_cols_past_view", "pixgemm", False, pix_ok, rx0=3)
    pred("pix_res_negative_origin", "pixgemm", False, pix_ok, ry0=-1)
    pred("pix_out_at_limit", "pixgemm", False, dict(pix_ok, rCs=0), B=1, aHs=2365, aWs=2365, Mrows=2365 * 2365, aW=2365, oHs=4730, oWs=4730)
    pred("head_ok", "pixgemm", True, head_ok)
    pred("head_out_too_narrow", "pixgemm", False, head_ok, oWs=27)
    pred("head_out_too_short", "pixgemm", False, head_ok, oHs=19)
    pred("conv48_ok", "conv48", True, conv48_ok)
    pred("conv48_rows_past_view", "conv48", False, conv48_ok, ay0=2)
    pred("conv48_cols_past_view", "conv48", False, conv48_ok, aWs=11)
    pred("conv48_negative_origin", "conv48", False, conv48_ok, ay0=-1)
    pred("conv48_out_too_small", "conv48", False, conv48_ok, oWs=7)
    pred("conv48_map_at_limit", "conv48", False, conv48_ok, B=1, aHs=6689, aWs=6689, Mrows=6686 * 6685, aW=6685, oHs=6686, oWs=6685)   # 4 295 381 056 B
    pred("conv48_alpha_above_1", "conv48", False, conv48_ok, act=1, alpha=1.5)
    pred("stem_ok", "stem", True, stem_ok)
    pred("stem_rows_past_view", "stem", False, stem_ok, aHs=9)
    pred("stem_cols_past_view", "stem", False, stem_ok, ax0=1)
    pred("stem_negative_origin", "stem", False, stem_ok, ay0=-1)
    pred("stem_out_too_small", "stem", False, stem_ok, oHs=7)
    pair_ok = dict(dict(conv48_ok, aHs=8, aWs=12), **{"s_" + k: v for k, v in stem_ok.items()})
    pred("pair_ok", "conv48_stem", True, pair_ok)
    pred("pair_conv_past_stem_rows", "conv48_stem", False, pair_ok, **{"s_Mrows": 7 * 12})      # the stem computes 7 rows, the convolution reads 8
    pred("pair_batch_differs", "conv48_stem", False, pair_ok, **{"s_B": 3})
    large_cases(S, rng)
    with open(os.path.join(d, "cases.json"), "w") as f:
        json.dump(S.cases, f)
    return S


# ---------------------------------------------------------------- 32-bit offsets: maps of 4 GB from the shared formula, sampled pixels
def sample(rng, total, around, n_random=2048):
    s = {0, total - 1}
    for c in around:
        s.update(range(max(0, c - 4), min(total, c + 4)))
    s.update(rng.integers(0, total, n_random).tolist())
    return np.array(sorted(s), dtype=np.int64)


def large_cases(S, rng):
    seed = 20261019

    def add(name, launcher, numbers, wt, bias, opix, patch, P1):
        """opix: sampled output pixel indices; patch: their input pixels [n][ph][pw]; P1: gemm_ref parameters of ONE output pixel's patch (B = n, a filled in later)."""
        spec = dict(kind="gemm", name=name, launcher=launcher, also_gemm=0, gen=1, seed=seed, rows=S.put(name + ".rows", opix), nrows=len(opix),
                    wt=S.put(name + ".wt", wt), bias=S.put(name + ".bias", bias))
        spec.update(numbers)
        S.cases.append(spec)
        S.meta[name] = dict(large=dict(patch=patch, P1=P1, C=numbers["aCs"], seed=seed, oCs=numbers["oCs"]), launcher=launcher)

    # launch_gemm: Linear 192 -> 192 on images of 240 x 240 tokens, one image more than a run of 2^31 - 1 halves holds
    Mrows, C = 240 * 240, 192
    per_run = GEMM_MAX // (Mrows * C)
    B = per_run + 1
    assert B * Mrows * C > 1 << 31
    wt, bias = weights(rng, C, C)
    opix = sample(rng, B * Mrows, [per_run * Mrows, (1 << 31) // C])
    add("split_gemm_lin192", "gemm", dict(B=B, aHs=240, aWs=240, aCs=C, Mrows=Mrows, aW=240, K=C, Kw=C, N=C, oHs=240, oWs=240, oCs=C), wt, bias, opix,
        opix[:, None, None], dict(Mrows=1, aW=1, K=C, N=C, wt=wt, bias=bias, out_shape=(1, 1, C)))
    # merge_kernel: 96 -> 192, the input map just under pixgemm_supported's limit
    Cin, Wm = 96, 2112
    Hm = PIX_MAX // (3 * Wm * Cin * 2) // 2 * 2
    B = 3
    while B * Hm * Wm * Cin * 2 >= PIX_MAX:
        Hm -= 2
    wt, bias = weights(rng, 192, 4 * Cin)
    Ho, Wo = Hm // 2, Wm // 2
    opix = sample(rng, B * Ho * Wo, [Ho * Wo, 2 * Ho * Wo, (1 << 31) // (4 * Cin)])
    b, oy, ox = opix // (Ho * Wo), opix % (Ho * Wo) // Wo, opix % Wo
    patch = (b[:, None, None] * Hm + 2 * oy[:, None, None] + np.arange(2)[None, :, None]) * Wm + 2 * ox[:, None, None] + np.arange(2)[None, None, :]
    add("limit_merge96", "pixgemm", dict(B=B, aHs=Hm, aWs=Wm, aCs=Cin, amode=2, kh=2, kw=2, stride=2, Mrows=Ho * Wo, aW=Wo, K=4 * Cin, Kw=4 * Cin, N=192, oHs=Ho, oWs=Wo, oCs=192),
        wt, bias, opix, patch, dict(amode=2, kh=2, kw=2, stride=2, Mrows=1, aW=1, K=4 * Cin, N=192, wt=wt, bias=bias, out_shape=(1, 1, 192)))
    # pixgemm_kernel: 192 -> 4 x 96, the output map just under the limit
    W, B = 1056, 3
    H = PIX_MAX // (B * 4 * W * 96 * 2)
    while B * 4 * H * W * 96 * 2 >= PIX_MAX:
        H -= 1
    wt, bias = weights(rng, 384, 192)
    rows = sample(rng, B * H * W, [H * W, 2 * H * W], n_random=1024)
    b, y, x = rows // (H * W), rows % (H * W) // W, rows % W
    opix = (((b * 2 * H + 2 * y)[:, None] + np.array([0, 0, 1, 1])[None]) * (2 * W) + 2 * x[:, None] + np.array([0, 1, 0, 1])[None]).reshape(-1)
    add("limit_pix96", "pixgemm", dict(B=B, aHs=H, aWs=W, aCs=192, Mrows=H * W, aW=W, K=192, Kw=192, N=384, oHs=2 * H, oWs=2 * W, oCs=96, omode=2, r=2), wt, bias, opix,
        rows[:, None, None], dict(Mrows=1, aW=1, K=192, N=384, wt=wt, bias=bias, omode=2, r=2, out_shape=(2, 2, 96)))
    # conv48_kernel: the input map just under conv48_supported's limit
    Wc, B = 2114, 3
    Hc = CONV48_MAX // (B * Wc * 48 * 2)
    while B * Hc * Wc * 48 * 2 >= CONV48_MAX:
        Hc -= 1
    wt, bias = weights(rng, 96, 432)
    Ho, Wo = Hc - 2, Wc - 2
    opix = sample(rng, B * Ho * Wo, [Ho * Wo, 2 * Ho * Wo], n_random=1024)
    b, oy, ox = opix // (Ho * Wo), opix % (Ho * Wo) // Wo, opix % Wo
    patch = (b[:, None, None] * Hc + oy[:, None, None] + np.arange(3)[None, :, None]) * Wc + ox[:, None, None] + np.arange(3)[None, None, :]
    add("limit_conv48", "conv48", dict(B=B, aHs=Hc, aWs=Wc, aCs=48, amode=2, kh=3, kw=3, Mrows=Ho * Wo, aW=Wo, K=432, Kw=432, N=96, oHs=Ho, oWs=Wo, oCs=96, act=1, alpha=0.2),
        wt, bias, opix, patch, dict(amode=2, kh=3, kw=3, Mrows=1, aW=1, K=432, N=96, wt=wt, bias=bias, act=1, alpha=0.2, out_shape=(1, 1, 96)))


# ---------------------------------------------------------------- the run
@pytest.fixture(scope="module")
def run(tmp_path_factory, pkg):
    t0 = time.time()
    d = str(tmp_path_factory.mktemp("conv_check"))
    exe = kr.build_harness(os.path.join(d, "conv_check"), "conv_check.cpp")
    S = build_suite(d)
    t1 = time.time()
    p = subprocess.run([exe, LIB, d], capture_output=True, text=True, timeout=400)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = {}
    for line in p.stdout.splitlines():
        if line.startswith("CASE "):
            f = line.split()
            res[f[1]] = {k: float(v) for k, v in (t.split("=") for t in f[2:])}
    assert set(res) == set(S.meta), set(S.meta) - set(res)
    print(f"conv_check: build + inputs {t1 - t0:.1f} s, harness {time.time() - t1:.1f} s")
    yield S, res
    print(f"conv_check: the file took {time.time() - t0:.1f} s")


def _record(rec):
    if _OUT:
        with open(_OUT, "a") as f:
            f.write(json.dumps(rec) + "\n")
    print("KERNEL " + json.dumps(rec), flush=True)


# ---------------------------------------------------------------- evaluation
def judge(rec_name, got, exact, ideal, frac_key, P=None, single_store=False, stats=None, eps=EPS):
    """The bounds of one output -> (record, violated bounds).  got: fp16 array; exact / ideal: float64, NaN where nothing is stored."""
    mask = ~np.isnan(exact)
    bad = []
    if not (got.view(np.uint16)[~mask] == 0xA5A5).all():
        bad.append("cells_outside_written")
    g64 = got.astype(np.float64)
    k, i = kr.error_metrics(g64[mask], exact[mask]), kr.error_metrics(ideal[mask], exact[mask])
    rec = {"case": rec_name, "kernel": k, "ideal_fp16": i}
    if not k["max_ulp"] <= i["max_ulp"] + REL_MAX_ALLOW:
        bad.append("max")
    if not k["rms_ulp"] <= REL_RMS_FACTOR * i["rms_ulp"]:
        bad.append("rms")
    if FRAC_MEASURED.get(frac_key) is None or not k["frac_1ulp"] >= FRAC_MEASURED[frac_key] - FRAC_FLOOR_MARGIN:
        bad.append("frac_1ulp")
    if not abs(k["mean_ulp"]) <= abs(i["mean_ulp"]) + MEAN_ALLOW + 4 * k["rms_ulp"] / np.sqrt(k["n"]):
        bad.append("mean_signed")
    if single_store and P is not None:
        q = dict(P, a=np.abs(P["a"].astype(np.float64)), wt=np.abs(P["wt"].astype(np.float64)), bias=np.abs(np.asarray(P["bias"], np.float64)), act=0, clip=None, stats=False)
        mag = kr.gemm_ref(q)["out"]
        with np.errstate(invalid="ignore"):
            bound = 0.5 * kr.ulp16(np.maximum(np.abs(exact), np.abs(g64))) + (P["K"] + 1) * 2.0 ** -23 * mag
            excess = (np.abs(g64 - exact) - bound)[mask]
        rec["derived_bound_worst_margin"] = float((np.abs(g64 - exact) / bound)[mask].max())
        if not (excess <= 0).all():
            bad.append("derived_elementwise")
    if stats is not None:
        st, Cout = stats
        pm = mask[..., 0]
        ref = kr.row_stats(g64[pm][:, :Cout], eps)
        st = st.astype(np.float64)[pm]
        var = 1.0 / ref[:, 1] ** 2 - eps
        rs = float((np.abs(st[:, 1] / ref[:, 1] - 1) / (1 + ref[:, 0] ** 2 / var)).max())
        ms = float((np.abs(st[:, 0] - ref[:, 0]) / np.sqrt(ref[:, 0] ** 2 + var)).max())
        rec["stats"] = {"rstd_rel": rs, "mean_rel": ms}
        if not rs <= STATS_RSTD_REL:
            bad.append("stats_rstd")
        if not ms <= STATS_MEAN_REL:
            bad.append("stats_mean")
    rec["violations"] = bad
    return rec, bad


def evaluate(S, res, name):
    """All records of one case: [(record, violations)]."""
    m = S.meta[name]
    base = name.split("~")[0]
    out = []
    if "pair" in m:
        Ps, Pc = m["pair"]
        for f in (False, True):
            mid = kr.gemm_ref(Ps, f)["out"]
            conv_out = kr.gemm_ref(dict(Pc, a=np.nan_to_num(mid)), f)["out"]
            if not f:
                exact_mid, exact = mid, conv_out
            else:
                ideal_mid, ideal = mid, conv_out
        oshape = (Pc["a"].shape[0],) + tuple(Pc["out_shape"])
        out.append(judge(name + ":stem", S.read(name + ".mid", np.float16, exact_mid.shape), exact_mid, ideal_mid, base + ":stem", Ps, True))
        out.append(judge(name, S.read(name + ".y", np.float16, oshape), exact, ideal, base))
        return out
    if "large" in m:
        L = m["large"]
        a = kr.gen_rows(L["patch"].reshape(-1), L["C"], L["seed"]).reshape(L["patch"].shape + (L["C"],))
        P = dict(L["P1"], a=a)
        exact, ideal = kr.gemm_ref(P)["out"], kr.gemm_ref(P, True)["out"]
        got = S.read(name + ".y", np.float16, (-1, L["oCs"])).reshape(exact.shape)
        out.append(judge(name, got, exact, ideal, base, P, True))
        return out
    P = m["P"]
    exact, ideal = kr.gemm_ref(P), kr.gemm_ref(P, True)
    shape = exact["out"].shape
    for ext, sext, tag in [(".y", ".stats", "")] + ([(".gy", ".gstats", "@gemm")] if m["also"] else []):
        st = (S.read(name + sext, np.float32, shape[:3] + (2,)), P.get("Cout", shape[3])) if P.get("stats") else None      # (judged with the true ln_eps)
        out.append(judge(name + tag, S.read(name + ext, np.float16, shape), exact["out"], ideal["out"], base + tag, P, m["single_store"], st))
    if len(out) == 2:
        mask = ~np.isnan(exact["out"])       # (ULP16 of the exact value with error_metrics' floor: the two kernels add in different orders)
        out[0][0]["against_gemm_kernel_ulp16"] = kr.error_metrics(S.read(name + ".y", np.float16, shape)[mask], S.read(name + ".gy", np.float16, shape).astype(np.float64)[mask])["max_ulp"]
    return out


def names(S, pred):
    return [n for n in S.meta if pred(n, S.meta[n])]


def test_every_case_ran_clean(run):
    S, res = run
    for n, m in S.meta.items():
        r = res[n]
        if m.get("refuse") or "predicate" in m:
            continue
        assert r["err"] == 0 and r["gerr"] == 0 and r["guards"] == 1, (n, r)
        assert r["det"] == 1, (n, "two runs differ")
        assert r["first"] == 1, (n, "the first image alone differs from the same image in the batch")
        assert r["untouched"] == 1, (n, "a fused launch wrote the map it replaces")


def test_refusals_and_predicate_audit(run):
    """launch_gemm refuses from the sizes alone (hipErrorInvalidValue, the output untouched); every predicate refuses views that do not hold what its kernel
    would touch, and still takes the engine's shapes."""
    S, res = run
    for n in names(S, lambda n, m: m.get("refuse")):
        assert res[n]["err"] == 1 and res[n]["untouched"] == 1, (n, res[n])
    for n in names(S, lambda n, m: "predicate" in m):
        assert (res[n]["err"] == 0) == S.meta[n]["predicate"] and res[n]["untouched"] == 1, (n, res[n])


FAMILIES = ["gemm", "stem", "conv48", "pair", "merge", "pix", "toimage", "split", "limit"]


@pytest.mark.parametrize("family", FAMILIES)
def test_kernels_against_float64(run, family):
    S, res = run
    failed = []
    cases = names(S, lambda n, m: "~" not in n and n.startswith(family) and not (m.get("refuse") or "predicate" in m or m.get("tihead")))
    assert cases
    for n in cases:
        for rec, bad in evaluate(S, res, n):
            rec["harness"] = res[n]
            _record(rec)
            if bad:
                failed.append((rec["case"], bad, rec))
    assert not failed, failed


def test_mutants_fail_their_bounds(run):
    S, res = run
    caught, smallest = {}, None
    for n in names(S, lambda n, m: "~" in n):
        for rec, bad in evaluate(S, res, n):
            rec["mutant"] = True
            _record(rec)
            caught[rec["case"]] = bad
            if "bias_delta=" in n and bad and "@gemm" not in rec["case"]:
                d = float(n.split("=")[1])
                smallest = d if smallest is None else min(smallest, d)
    _record({"mutants": caught, "smallest_failing_bias_delta": smallest})
    for n, bad in caught.items():
        if "bias_delta=" in n:
            continue        # (the perturbation scan: recorded, the largest must fail)
        assert bad, (n, "mutant passed every bound")
    assert smallest is not None and smallest <= 0.00390625      # 4 ULP16 of the typical output on one of 192 channels


def test_byte_identities(run):
    """conv48_kernel<true> against launch_stem then launch_conv48; the folded head of launch_mlp against launch_mlp then toimage_kernel."""
    S, _ = run
    for n in names(S, lambda n, m: "pair" in m or m.get("tihead")):
        a, b = np.fromfile(os.path.join(S.dir, n + ".y"), np.uint16), np.fromfile(os.path.join(S.dir, n + ".fy"), np.uint16)
        assert len(a) and np.array_equal(a, b), (n, int((a != b).sum()))
