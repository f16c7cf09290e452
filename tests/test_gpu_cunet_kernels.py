"""cunet's convolution, gate and head kernels alone - conv3_kernel<POOL, MODE> (k_conv3.hip: plain, pooling, STEM, UP), conv3h_walk_kernel / conv3h_kernel (k_conv3h.hip),
merge_slab_kernel and pixgemm_kernel at K = 64 / 128 with their gates (k_pixgemm.hip), se_kernel / scale_kernel (k_prepost.hip) and gemm_kernel's a_scale / res_scale /
pool_out branches - against the float64 references of kernel_ref (gemm_ref, two_launches, se_ref), through the library as built (tools/kernel_check/cunet_check.cpp
finds w2x::launch_* and *_supported of libw2x.so by name).

The scheme is that of tests/test_gpu_conv_kernels.py (its helpers are imported, not copied), with the same constants:
  * max <= the ideal fp16 kernel's max + 0.25 ULP16, rms <= 1.02 x its rms, |mean signed error| <= |its| + 0.01 + 4 sigma;
  * the fraction within 1 ULP16 >= the IDEAL fp16 model's fraction for the same case (computed here, on the CPU) - FRAC_MARGIN; tests/golden/cunet_kernel_frac.json
    records both per case (profiles/kernel_check/cunet_check.jsonl);
  * single-store launches: per element |err| <= 0.5 ULP16(result) + (K + 1) 2^-23 sum |a w| (gated operands: a = fp16(x s));
  * pooling partials against float64 column sums of the kernel's OWN stored outputs, per tile in tile order: |err| <= (n - 1) 2^-24 sum |v|;
  * se_kernel's gates against se_ref of the dumped partials: |ds| <= 1/4 da + SE_C 2^-24 s (da: kernel_ref.se_bound);
  * a specialised kernel against gemm_kernel on the same parameters: at most 2 ULP16 apart (conv3h with a skip add rounds once, gemm_kernel twice: through their models only);
  * byte identities exact: STEM / UP against their two launches, <PIX, true> against the walk, a folded gate against launch_scale + the ungated launch;
  * outputs pre-filled with 0xA5A5 between guard bands, two runs bit-identical, the first image alone bit-identical;
  * input cells no stored output depends on (kernel_ref.cells_read: behind the origin, past y0 + Ho + 2 / x0 + Wo + 2, the spare rows of skip maps) hold fp16 NaN.
Mutants (one value handed to the kernel changed, the reference keeping the true one) must fail those bounds.  Nothing past a limit is launched: the over-limit shapes go
through the predicates, or launch_se's refusal."""
import json
import os
import subprocess
import time

import numpy as np
import pytest

import kernel_ref as kr
import test_gpu_conv_kernels as ck      # data, weights, Suite, spec_numbers, conv, shuffle, sample and the bounds' constants

pytestmark = pytest.mark.gpu

ROOT, LIB = ck.ROOT, ck.LIB
_OUT = os.environ.get("W2X_KERNEL_CHECK_OUT")      # the KERNEL records are appended there as JSON lines (profiles/kernel_check/cunet_check.jsonl)

REL_MAX_ALLOW, REL_RMS_FACTOR, MEAN_ALLOW = ck.REL_MAX_ALLOW, ck.REL_RMS_FACTOR, ck.MEAN_ALLOW      # 0.25, 1.02, 0.01: the same class of kernel
# Fraction within 1 ULP16, against the ideal fp16 model's fraction of the same case: largest shortfall of the first run 0.00011 (head64_res_clip_17x130@gemm; 0.00006
# on a specialised kernel, uppair_17x130_o01_g1; profiles/kernel_check/record.txt), the margin about ten times that.
FRAC_MARGIN = 0.001
AGAINST_GEMM_MAX = 2.0   # ULP16: the project's recorded figure
# se_kernel: allowance for the hardware exponential and division in units of 2^-24 s, which cannot be derived.  Measured against se_ref: the kernel's largest error 11.9
# units where the float32 numpy restatement has 7.0 (chain64_se_gemm), its largest excess over the restatement 5.95 units (chain64_se_conv3: 9.97 against 4.02) - ten
# times that.  (The derived part 1/4 da is 119 units and more on these partials: the worst gate uses 0.013 of the bound.)
SE_C = 60.0
PIX_MAX = ck.PIX_MAX
with open(os.path.join(ROOT, "tests", "golden", "cunet_kernel_frac.json")) as _f:
    FRAC_RECORDED = json.load(_f)                  # {record: {"kernel": measured, "ideal": the model's}} - a record of the first run, not a bound

NAN16 = np.float16(np.nan)
f16a, data, weights = ck.f16a, ck.data, ck.weights


# ---------------------------------------------------------------- cases
def poison(P):
    """fp16 NaN into every cell of the input and skip maps that no stored output depends on (the reference's own index arithmetic: kernel_ref.cells_read)."""
    mask, skips = kr.cells_read(P)
    P["a"] = P["a"].copy()
    P["a"][:, ~mask] = NAN16
    for key, m in skips.items():
        P[key] = P[key].copy()
        P[key][:, ~m] = NAN16
    P["poisoned"] = int((~mask).sum() + sum(int((~m).sum()) for m in skips.values()))
    return P


def spec_files(S, name, P, pre=""):
    """ck.spec_files plus the gates; a value that is a string names a file an earlier case of the run writes."""
    s = {}
    for key, dt in (("wt", np.float16), ("bias", np.float32), ("a", np.float16), ("res", np.float16), ("a_scale", np.float32), ("res_scale", np.float32)):
        v = P.get(key)
        if v is None or (key == "a" and P.get("a_is_mid")):
            continue
        s[key] = v if isinstance(v, str) else S.put(f"{name}.{pre}{key}", np.asarray(v).astype(dt))
    return {pre + k: v for k, v in s.items()}


def spec_numbers(P, pre=""):
    Q = dict(P)
    for key, shp in (P.get("shapes") or {}).items():      # maps that come from an earlier case's file: only their shape is known here
        Q[key] = np.zeros(shp, np.float16)
    return ck.spec_numbers(Q, pre)


def gcase(S, name, launcher, P, also_gemm=None, mutate="", single_store=None, pool=False, scale_ident=False, switch=""):
    also = launcher != "gemm" if also_gemm is None else also_gemm
    spec = dict(kind="gemm", name=name, launcher=launcher, also_gemm=int(also), mutate=mutate, pool=int(pool), scale_ident=int(scale_ident), switch=switch)
    spec.update(spec_numbers(P))
    spec.update(spec_files(S, name, P))
    S.cases.append(spec)
    if single_store is None:
        single_store = P.get("res") is None
    S.meta[name] = dict(P=P, launcher=launcher, also=also, single_store=single_store, mutate=mutate, pool=pool)


def conv3(rng, Cin, N, B, Ho, Wo, act, kind="normal"):
    """3x3 onto N channels: origin (1, 2), a spare row and column behind the view, an output view larger than Ho x Wo."""
    return poison(ck.conv(rng, 3, 1, Cin, N, B, Ho, Wo, y0=1, x0=2, pad=(1, 1), opad=(1, 2), act=act, alpha=0.2, kind=kind))


def head(rng, Cin, B, Ho, Wo, variant):
    """cunet's image heads: rows mode N = 3 onto 4 stored channels (res + clip, clip alone, res alone) or N = 16 with a 2x pixel shuffle."""
    K = 9 * Cin
    pix = variant == "pix"
    N = 16 if pix else 3
    wt, bias = weights(rng, N, K)
    bias = (bias + (0.0 if pix else 0.5)).astype(np.float32)
    P = dict(a=data(rng, (B, 1 + Ho + 2 + 1, 2 + Wo + 2 + 1, Cin)), a_y0=1, a_x0=2, amode=2, kh=3, kw=3, Mrows=Ho * Wo, aW=Wo, K=K, N=N, wt=wt, bias=bias,
             act=1 if pix else 0, alpha=0.1, round_once=True)
    if pix:
        P.update(omode=2, r=2, out_shape=(2 * Ho + 1, 2 * Wo + 2, 4), Cout=4)
    else:
        P.update(out_shape=(Ho + 1, Wo + 2, 4), Cout=4)
        if variant in ("res_clip", "res"):
            P.update(res=f16a(rng.normal(0.3, 0.3, (B, Ho + 2, Wo + 3, 4))), res_y0=1, res_x0=2)      # (all four stored channels non-zero)
        if variant in ("res_clip", "clip"):
            P["clip"] = (0.0, 1.0)
    return poison(P)


def gates(rng, B, C):
    return rng.uniform(0.05, 0.95, (B, C)).astype(np.float32)      # distinct rows per image


def pair_case(S, rng, name, fuse, Ho, Wo, y0=1, x0=2, gated=False, s_mutate="", mutate=""):
    B = 2
    if fuse == "stem":     # stem 4 -> 32 (origin (2, 3)) -> conv 32 -> 64 at origin (y0, x0) of the stem's map, one spare row / column
        sHo, sWo = y0 + Ho + 2 + 1, x0 + Wo + 2 + 1
        P1 = ck.conv(rng, 3, 1, 4, 32, B, sHo, sWo, y0=2, x0=3, pad=(1, 1), act=1, alpha=0.1)
        P1["a"][..., 3] = data(rng, P1["a"].shape[:-1])          # the fourth stored channel is not zero, nor are its weights
        Cm = 32
    else:                  # projection 64 -> 4 x 64 (LeakyReLU, gate, skip map at (1, 2) with a spare row / column), larger than what the convolution reads
        Hl, Wl = (y0 + Ho + 2 + 1) // 2 + 1, (x0 + Wo + 2 + 1) // 2 + 1
        sHo, sWo = 2 * Hl, 2 * Wl
        P1 = ck.shuffle(rng, 64, 64, 2, B, Hl, Wl, res=(1, 2), act=1)
        if gated:
            P1["a_scale"] = gates(rng, B, 64)
        Cm = 64
    P1 = poison(P1)
    P2 = ck.conv(rng, 3, 1, Cm, 64, B, Ho, Wo, y0=y0, x0=x0, pad=(sHo - (y0 + Ho + 2), sWo - (x0 + Wo + 2)), opad=(1, 2), act=1, alpha=0.2)
    assert P2["a"].shape[1:3] == (sHo, sWo)
    P2["a_is_mid"] = True
    spec = dict(kind="pair", name=name, fuse=fuse, s_mutate=s_mutate, mutate=mutate)
    spec.update(spec_numbers(P2)); spec.update(spec_files(S, name, P2))
    spec.update(spec_numbers(P1, "s_")); spec.update(spec_files(S, name, P1, "s_"))
    S.cases.append(spec)
    S.meta[name] = dict(pair=(P1, P2), mutate=s_mutate or mutate)


def se_weights(rng, C):
    Cm = C // 8
    return dict(w1=rng.normal(0, C ** -0.5, (Cm, C)).astype(np.float32), b1=rng.normal(0.1, 0.2, Cm).astype(np.float32),
                w2=rng.normal(0, 2.0 * Cm ** -0.5, (C, Cm)).astype(np.float32), b2=rng.normal(0, 0.5, C).astype(np.float32))


def se_case(S, name, pool, B, C, nblocks, inv_count, W, handed=None, mutate=""):
    """launch_se on the partials `pool` (an array, or the file of an earlier case); `handed`: what the kernel gets where it differs from the truth (mutants)."""
    h = dict(W, inv_count=inv_count)
    h.update(handed or {})
    spec = dict(kind="se", name=name, B=B, C=C, Cs=C, Cmid=C // 8, nblocks=nblocks, Mrows=0, inv_count=float(h["inv_count"]),
                pool=pool if isinstance(pool, str) else S.put(name + ".poolin", np.asarray(pool, np.float32)))
    for k in ("w1", "b1", "w2", "b2"):
        spec[k] = S.put(f"{name}.{k}", np.asarray(h[k], np.float32))
    S.cases.append(spec)
    S.meta[name] = dict(se=dict(W, inv_count=inv_count, pool=pool, shape=(B, nblocks, C)), mutate=mutate)


def build_suite(d):
    S = ck.Suite(d)
    rng = np.random.default_rng(1021)
    # ---- conv3_kernel<false, 0> / <true, 0>: 8 x 64 tiles, 32-channel chunks (nchunk 2 / 4 / 8), 64-channel blocks (nblk 1 / 2 / 4: the XCD-grouped grid from 2 on)
    i = 0
    for Cin, N in ((64, 64), (64, 128), (128, 64), (128, 256), (256, 128)):
        for Ho, Wo in ((1, 1), (7, 63), (8, 64), (9, 65), (17, 130)):
            B = 3 if (N, Ho) == (128, 9) else 2            # 3 x 4 tiles = 12, rounded up to 16 workgroup rounds with nblk = 2: the early return
            P = conv3(rng, Cin, N, B, Ho, Wo, act=i % 2, kind="wide" if i == 7 else "normal")
            gcase(S, f"conv3_{Cin}x{N}_{Ho}x{Wo}", "conv3", P, pool=(Ho, Wo) != (8, 64))      # pooling on every ragged shape
            if (Cin, N) == (64, 64) and (Ho, Wo) != (8, 64):
                gcase(S, f"conv3_{Cin}x{N}_{Ho}x{Wo}_nopool", "conv3", P, also_gemm=False)    # <false, 0> on the ragged shapes too
            i += 1
    # ---- STEM and UP against their two launches
    for Ho, Wo in ((1, 1), (8, 64), (9, 65), (17, 130)):
        pair_case(S, rng, f"stempair_{Ho}x{Wo}", "stem", Ho, Wo)
    for Ho, Wo in ((1, 1), (9, 65), (17, 130)):
        for y0, x0 in ((0, 0), (0, 1), (1, 0), (1, 1)) if Ho > 1 else ((1, 0),):
            for gated in (False, True) if Ho < 17 else ((y0 + x0) % 2 == 1,):
                pair_case(S, rng, f"uppair_{Ho}x{Wo}_o{y0}{x0}_g{int(gated)}", "up", Ho, Wo, y0, x0, gated)
    # ---- conv3h: Cin = 64 the walk (and <PIX, true> under the debug switch), 32 / 128 conv3h_kernel<PIX, false>; 17 x 130: three row blocks of eight rows
    for Cin in (64, 32, 128):
        for Ho, Wo in ((1, 1), (3, 63), (4, 64), (5, 65), (17, 130)):
            for variant in ("res_clip", "clip", "res", "pix"):
                P = head(rng, Cin, 2, Ho, Wo, variant)
                gcase(S, f"head{Cin}_{variant}_{Ho}x{Wo}", "conv3h", P, single_store=variant in ("clip", "pix"))
                if Cin == 64:
                    gcase(S, f"head{Cin}_{variant}_{Ho}x{Wo}_tile", "conv3h", P, also_gemm=False, single_store=variant in ("clip", "pix"), switch="no_conv3h_walk")
    # ---- merge_slab_kernel: 128 output pixels per workgroup, 32 per wave, straddling output rows and images
    i = 0
    for C in (64, 128):
        S.cases.append(dict(kind="rows", name=f"rows_slab{C}", expect=128, B=1, aHs=2, aWs=2, aCs=C, amode=2, kh=2, kw=2, stride=2, Mrows=1, aW=1, K=4 * C, Kw=4 * C, N=C, oHs=1, oWs=1, oCs=C))
        S.meta[f"rows_slab{C}"] = dict(rows=True)
        for Ho, Wo in ((1, 1), (3, 5), (8, 16), (9, 15)):
            for B in (1, 3):
                P = ck.conv(rng, 2, 2, C, C, B, Ho, Wo, y0=i % 2, x0=i % 2, pad=(i % 2, i % 2), act=(i // 2) % 2, kind="wide" if i == 3 else "normal")
                gated = i % 4 in (1, 2)
                if gated:
                    P["a_scale"] = gates(rng, B, C)
                gcase(S, f"slab{C}_{Ho}x{Wo}_B{B}", "pixgemm", poison(P), scale_ident=gated)
                i += 1
    # ---- pixgemm_kernel at K = 64 (PixCfg TT = 2: 128 rows per workgroup) and K = 128 (TT = 1: 64)
    for C, BM in ((64, 128), (128, 64)):
        # (BM is asked of the library, pixgemm_rows_per_workgroup: a "rows" case fails the run-clean test if a workgroup no longer owns BM rows)
        S.cases.append(dict(kind="rows", name=f"rows_pix{C}", expect=BM, B=1, aHs=1, aWs=BM, aCs=C, Mrows=BM, aW=BM, K=C, Kw=C, N=4 * C, oHs=2, oWs=2 * BM, oCs=C, omode=2, r=2))
        S.meta[f"rows_pix{C}"] = dict(rows=True)
        for M in (1, BM - 1, BM, BM + 1):
            gcase(S, f"pix{C}_M{M}", "pixgemm", ck.shuffle(rng, C, C, 2, 1, 1, M, act=M % 2))
        gcase(S, f"pix{C}_5x7_B3_res", "pixgemm", poison(ck.shuffle(rng, C, C, 2, 3, 5, 7, res=(1, 2), act=1, opad=(1, 1))))
        P = ck.shuffle(rng, C, C, 2, 3, 5, 7, res=(1, 2), act=1)
        P["res_scale"] = gates(rng, 3, C)
        gcase(S, f"pix{C}_5x7_B3_resscale", "pixgemm", poison(P), scale_ident=True)
        P = ck.shuffle(rng, C, C, 2, 3, 5, 7, res=(0, 0))
        P["a_scale"] = gates(rng, 3, C)
        gcase(S, f"pix{C}_5x7_B3_ascale", "pixgemm", poison(P), scale_ident=True)
    # ---- gemm_kernel alone: the branches the engine takes under the debug switches and for every shape a predicate refuses
    P = ck.conv(rng, 3, 1, 64, 64, 3, 5, 7, y0=1, x0=2, pad=(1, 1), act=1)
    P["a_scale"] = gates(rng, 3, 64)
    gcase(S, "gemm_conv3x3_ascale", "gemm", poison(P), scale_ident=True)
    P = ck.linear(rng, 64, 64, 3, 5, 7, res=data(rng, (3, 7, 10, 64)), res_y0=1, res_x0=2)
    P["res_scale"] = gates(rng, 3, 64)
    gcase(S, "gemm_lin_resscale", "gemm", poison(P), scale_ident=True)
    for rows in (127, 128, 129):
        gcase(S, f"gemm_pool_r{rows}", "gemm", ck.linear(rng, 64, 64, 3, 1, rows), pool=True)
    # ---- the gate chain: producer with pool_out (conv3_kernel<true, 0>, and gemm_kernel on the same parameters) -> launch_se -> gated consumers, on a 9 x 65 map
    for C in (64, 128):
        Pp = ck.conv(rng, 3, 1, C, C, 3, 9, 65, act=1, alpha=0.2)
        prod = f"chain{C}_prod"
        gcase(S, prod, "conv3", Pp, pool=True)
        W = se_weights(rng, C)
        inv = 1.0 / (9 * 65)
        se_case(S, f"chain{C}_se_conv3", prod + ".pool", 3, C, 4, inv, W)       # conv3_tiles: 2 x 2 tiles of 8 x 64
        se_case(S, f"chain{C}_se_gemm", prod + ".gpool", 3, C, 5, inv, W)       # ceil(585 / 128) row tiles
        gate_file, shp = f"chain{C}_se_conv3.gates", dict(a=(3, 9, 65, C))
        wt, bias = weights(rng, 4 * C, C)
        gcase(S, f"chain{C}_pix", "pixgemm", dict(a=prod + ".y", a_scale=gate_file, shapes=shp, Mrows=585, aW=65, K=C, N=4 * C, wt=wt, bias=bias, act=1, alpha=0.1, omode=2, r=2,
                                                out_shape=(18, 130, C), Cout=C), scale_ident=True)
        wt, bias = weights(rng, C, 4 * C)
        gcase(S, f"chain{C}_slab", "pixgemm", dict(a=prod + ".y", a_scale=gate_file, shapes=shp, amode=2, kh=2, kw=2, stride=2, Mrows=4 * 32, aW=32, K=4 * C, N=C, wt=wt, bias=bias,
                                                 out_shape=(4, 32, C)), scale_ident=True)
        wt, bias = weights(rng, C, C)
        gcase(S, f"chain{C}_gemm_ascale", "gemm", dict(a=prod + ".y", a_scale=gate_file, shapes=shp, Mrows=585, aW=65, K=C, N=C, wt=wt, bias=bias, out_shape=(9, 65, C)), scale_ident=True)
        gcase(S, f"chain{C}_gemm_resscale", "gemm", dict(a=data(rng, (3, 9, 65, C)), res=prod + ".y", res_scale=gate_file, shapes=dict(res=(3, 9, 65, C)), Mrows=585, aW=65, K=C, N=C,
                                                        wt=wt, bias=bias, out_shape=(9, 65, C)), scale_ident=True)
    # ---- mutants
    def mut(base, m):
        M = S.meta[base]
        assert not m.startswith("gate_") or M["P"].get("a_scale") is not None, base
        gcase(S, f"{base}~{m}", M["launcher"], M["P"], also_gemm=M["also"], mutate=m, single_store=M["single_store"], pool=M["pool"])
    for m in ("wt_transpose_taps", "ax0+1", "alpha", "perm_row_swap"):
        mut("conv3_64x64_9x65", m)            # (act 1)
    for delta in (0.03125, 0.00390625, 0.00048828125):
        mut("conv3_128x256_9x65", f"bias_delta={delta}")
    for m in ("subpixel_swap", "res_origin+1", "gate_next_image"):
        pair_case(S, np.random.default_rng(7), f"uppair_9x65_o10_g1~{m}", "up", 9, 65, 1, 0, True, s_mutate=m)
    pair_case(S, np.random.default_rng(8), "stempair_9x65~alpha", "stem", 9, 65, s_mutate="alpha")
    mut("head64_pix_5x65", "subpixel_swap"); mut("head64_res_clip_5x65", "res_origin+1"); mut("head64_res_clip_5x65", "clip_hi")
    mut("slab64_8x16_B3", "gate_shift_channel"); mut("pix64_5x7_B3_ascale", "gate_shift_channel"); mut("gemm_conv3x3_ascale", "gate_shift_channel")
    # SE mutants on partials of a known shape: 3 images x 4 tiles, as conv3_kernel<true, 0> writes them for 9 x 65
    W = se_weights(rng, 64)
    pp = rng.normal(0.2, 0.6, (3, 4, 64)) * np.array([512, 8, 64, 1])[None, :, None]
    inv = 1.0 / (9 * 65)
    se_case(S, "se_alone", pp, 3, 64, 4, inv, W)
    se_case(S, "se_alone~inv_count_padded", pp, 3, 64, 4, inv, W, handed=dict(inv_count=1.0 / (16 * 128)), mutate="inv_count")      # the padded tile area instead of Ho Wo
    se_case(S, "se_alone~w1_transposed", pp, 3, 64, 4, inv, W, handed=dict(w1=np.ascontiguousarray(W["w1"].T).reshape(8, 64)), mutate="w1")
    j = int(np.argmax(np.maximum((pp.sum(axis=1) * inv) @ W["w1"].T.astype(np.float64) + W["b1"], 0).min(axis=0)))      # a hidden unit that is active in every image
    w2 = W["w2"].copy(); w2[5, j] += 0.01
    se_case(S, "se_alone~w2_entry", pp, 3, 64, 4, inv, W, handed=dict(w2=w2), mutate="w2")
    for name, k in (("C0", dict(C=0)), ("C300", dict(C=300, Cs=304)), ("Cmid0", dict(Cmid=0)), ("nblocks0", dict(nblocks=0))):
        S.cases.append(dict(dict(kind="se_refuse", name="se_refuse_" + name, B=3, C=64, Cs=64, Cmid=8, nblocks=4, inv_count=inv), **k))
        S.meta["se_refuse_" + name] = dict(refuse=True)
    predicate_cases(S)
    large_cases(S, rng)
    with open(os.path.join(d, "cases.json"), "w") as f:
        json.dump(S.cases, f)
    return S


def predicate_cases(S):
    """No launch: each refusal beside an acceptance of an engine-like shape."""
    def pred(name, which, want, base, **k):
        S.cases.append(dict(dict(base, kind="predicate", name="pred_" + name, pred=which), **k))
        S.meta["pred_" + name] = dict(predicate=want)
    conv3_ok = dict(B=2, aHs=20, aWs=70, aCs=64, ay0=1, ax0=2, amode=2, kh=3, kw=3, Mrows=16 * 64, aW=64, K=576, Kw=576, N=64, oHs=16, oWs=64, oCs=64, act=1, alpha=0.1)
    pred("conv3_ok", "conv3", True, conv3_ok)
    pred("conv3_ok_pooled", "conv3", True, conv3_ok, pooled=1)
    pred("conv3_rows_past_view", "conv3", False, conv3_ok, ay0=3)
    pred("conv3_cols_past_view", "conv3", False, conv3_ok, aWs=67)
    pred("conv3_negative_y0", "conv3", False, conv3_ok, ay0=-1)
    pred("conv3_negative_x0", "conv3", False, conv3_ok, ax0=-1)
    pred("conv3_out_too_small", "conv3", False, conv3_ok, oWs=63)
    pred("conv3_out_origin", "conv3", False, conv3_ok, oHs=17, oy0=1)              # the epilogue ignores out.y0 / out.x0
    pred("conv3_out_origin_x", "conv3", False, conv3_ok, oWs=65, ox0=1)
    pred("conv3_B0", "conv3", False, conv3_ok, B=0)
    pred("conv3_alpha_above_1", "conv3", False, conv3_ok, alpha=1.5)
    pred("conv3_gated", "conv3", False, conv3_ok, gated=1)
    pred("conv3_out_image_at_limit", "conv3", False, conv3_ok, B=1, aHs=4100, aWs=4100, ay0=0, ax0=0, Mrows=4098 * 4098, aW=4098, oHs=4098, oWs=4098)   # 2 149 576 192 B > 2^31 - 1
    pred("conv3_out_image_under_limit", "conv3", True, conv3_ok, B=1, aHs=4097, aWs=4097, ay0=0, ax0=0, Mrows=4095 * 4095, aW=4095, oHs=4095, oWs=4095)  # 2 146 435 200 B
    pred("conv3_halo_rows_at_limit", "conv3", False, conv3_ok, B=1, aHs=3, aWs=1525204, ay0=0, ax0=0, Mrows=1525202, aW=1525202, oHs=1, oWs=1525202)   # 11 rows: 2 147 487 232 B
    pred("conv3_pool_more_tiles_than_planned", "conv3", False, conv3_ok, pooled=1, aHs=11, aWs=4, ay0=0, ax0=0, Mrows=9 * 2, aW=2, oHs=9, oWs=2)      # 2 tiles, one row tile of 128
    stem_ok = dict(B=2, aHs=24, aWs=74, aCs=4, ay0=1, ax0=1, amode=2, kh=3, kw=3, Mrows=20 * 70, aW=70, K=36, Kw=40, N=32, oHs=20, oWs=70, oCs=32, act=1, alpha=0.1)
    spair_ok = dict(dict(conv3_ok, aCs=32, K=288, Kw=288), **{"s_" + k: v for k, v in stem_ok.items()})
    pred("stempair_ok", "conv3_stem", True, spair_ok)
    pred("stempair_conv_past_stem_rows", "conv3_stem", False, spair_ok, **{"s_Mrows": 18 * 70})     # the stem computes 18 rows, the convolution reads rows 1 .. 18
    pred("stempair_conv_past_stem_cols", "conv3_stem", False, spair_ok, ax0=5)
    pred("stempair_negative_origin", "conv3_stem", False, spair_ok, ay0=-1)
    pred("stempair_batch_differs", "conv3_stem", False, spair_ok, **{"s_B": 3})
    pred("stempair_B0", "conv3_stem", False, spair_ok, B=0, **{"s_B": 0})
    pred("stempair_stem_alpha_above_1", "conv3_stem", True, spair_ok, **{"s_alpha": 1.5})          # (the stem selects v > 0 ? v : v alpha: any slope)
    pred("stempair_conv_alpha_above_1", "conv3_stem", False, spair_ok, alpha=1.5)
    pred("stempair_pooled", "conv3_stem", False, spair_ok, pooled=1)
    pred("stempair_input_image_at_limit", "conv3_stem", False, dict(spair_ok, B=1, **{"s_B": 1, "s_aHs": 16400, "s_aWs": 16400}))    # 2 151 680 000 B of input per image
    proj_ok = dict(B=2, aHs=12, aWs=40, aCs=64, Mrows=480, aW=40, K=64, Kw=64, N=256, oHs=24, oWs=80, oCs=64, omode=2, r=2, Cout=64, act=1, alpha=0.1, rHs=26, rWs=83, rCs=64, ry0=1, rx0=2)
    upc_ok = dict(conv3_ok, aHs=24, aWs=80, ay0=1, ax0=1)
    up_ok = dict(upc_ok, **{"s_" + k: v for k, v in proj_ok.items()})
    pred("uppair_ok", "conv3_up", True, up_ok)
    pred("uppair_ok_gated", "conv3_up", True, up_ok, s_gated=1)
    pred("uppair_conv_past_projection_rows", "conv3_up", False, up_ok, ay0=7)                       # 7 + 16 + 2 > 24
    pred("uppair_conv_past_projection_cols", "conv3_up", False, up_ok, ax0=15)
    pred("uppair_negative_origin", "conv3_up", False, up_ok, ax0=-1)
    pred("uppair_skip_rows_past_view", "conv3_up", False, up_ok, **{"s_rHs": 25, "s_ry0": 2})       # the projection's own skip rows end at the view's edge... and past it
    pred("uppair_skip_negative_origin", "conv3_up", False, up_ok, **{"s_ry0": -1})
    pred("uppair_projection_out_too_small", "conv3_up", False, up_ok, aHs=23, **{"s_oHs": 23})
    pred("uppair_batch_differs", "conv3_up", False, up_ok, **{"s_B": 3})
    pred("uppair_B0", "conv3_up", False, up_ok, B=0, **{"s_B": 0})
    pred("uppair_projection_alpha_above_1", "conv3_up", False, up_ok, **{"s_alpha": 1.5})
    pred("uppair_no_skip", "conv3_up", False, up_ok, **{"s_rCs": 0})
    pred("uppair_rows_at_limit", "conv3_up", False, dict(up_ok, B=1, aHs=11600, aWs=11600, Mrows=16 * 64, **{"s_B": 1, "s_aHs": 5800, "s_aWs": 5800, "s_Mrows": 5800 * 5800, "s_aW": 5800,
                                                         "s_oHs": 11600, "s_oWs": 11600, "s_rHs": 11602, "s_rWs": 11603}))   # 4 305 920 000 B of rows
    head_ok = dict(B=2, aHs=20, aWs=70, aCs=64, ay0=1, ax0=2, amode=2, kh=3, kw=3, Mrows=16 * 64, aW=64, K=576, Kw=576, N=3, oHs=16, oWs=64, oCs=4, has_clip=1, clip_lo=0.0, clip_hi=1.0,
                   rHs=18, rWs=68, rCs=4, ry0=1, rx0=2)
    headpix_ok = dict(B=2, aHs=20, aWs=70, aCs=64, ay0=1, ax0=2, amode=2, kh=3, kw=3, Mrows=16 * 64, aW=64, K=576, Kw=576, N=16, oHs=32, oWs=128, oCs=4, omode=2, r=2, act=1, alpha=0.1)
    pred("head_ok", "conv3h", True, head_ok)
    pred("head_rows_past_view", "conv3h", False, head_ok, aHs=18)
    pred("head_cols_past_view", "conv3h", False, head_ok, ax0=5)
    pred("head_negative_origin", "conv3h", False, head_ok, ay0=-1)
    pred("head_out_too_small", "conv3h", False, head_ok, oHs=15)
    pred("head_B0", "conv3h", False, head_ok, B=0)
    pred("head_res_rows_past_view", "conv3h", False, head_ok, rHs=16)
    pred("head_res_negative_origin", "conv3h", False, head_ok, rx0=-1)
    pred("head_N5", "conv3h", False, head_ok, N=5)
    pred("headpix_ok", "conv3h", True, headpix_ok)
    pred("headpix_out_too_narrow", "conv3h", False, headpix_ok, oWs=127)
    pred("headpix_out_too_short", "conv3h", False, headpix_ok, oHs=31)
    pred("headpix_cols_past_view", "conv3h", False, headpix_ok, aWs=67)
    pred("headpix_B0", "conv3h", False, headpix_ok, B=0)
    pred("headpix_alpha_above_1", "conv3h", True, headpix_ok, alpha=1.5)                            # (both conv3h kernels select v > 0 ? v : v alpha: any slope)
    # conv3h_supported has no 32-bit limit and needs none: conv3h_kernel forms every address in size_t, and the walk's 32-bit row offsets are guarded in launch_conv3h,
    # which falls back to conv3h_kernel.  One image past 4 GiB, and three images of 1.48 GB, are taken.
    nores = dict(rCs=0, rHs=0, rWs=0)
    pred("head_image_past_4G", "conv3h", True, dict(head_ok, **nores), B=1, aHs=6000, aWs=6000, ay0=0, ax0=0, Mrows=5998 * 5998, aW=5998, oHs=5998, oWs=5998)   # 4 608 000 000 B
    pred("head_images_past_4G_together", "conv3h", True, dict(head_ok, **nores), B=3, aHs=3400, aWs=3400, ay0=0, ax0=0, Mrows=3398 * 3398, aW=3398, oHs=3398, oWs=3398)
    for C, side_at, side_under in ((64, 5800, 5792), (128, 4096, 4094)):
        slab_ok = dict(B=2, aHs=18, aWs=66, aCs=C, amode=2, kh=2, kw=2, stride=2, Mrows=9 * 33, aW=33, K=4 * C, Kw=4 * C, N=C, oHs=9, oWs=33, oCs=C)
        pred(f"slab{C}_ok", "pixgemm", True, slab_ok)
        pred(f"slab{C}_ok_gated", "pixgemm", True, slab_ok, gated=1)
        pred(f"slab{C}_rows_past_view", "pixgemm", False, slab_ok, aHs=17)
        pred(f"slab{C}_cols_past_view", "pixgemm", False, slab_ok, ax0=1)
        pred(f"slab{C}_negative_origin", "pixgemm", False, slab_ok, ay0=-1)
        big = lambda s: dict(B=1, aHs=s, aWs=s, Mrows=(s // 2) ** 2, aW=s // 2, oHs=s // 2, oWs=s // 2)
        pred(f"slab{C}_map_at_limit", "pixgemm", False, slab_ok, **big(side_at))          # 64: 4 305 920 000 B; 128: 4 294 967 296 B >= 0xFFFF0000
        pred(f"slab{C}_map_under_limit", "pixgemm", True, slab_ok, **big(side_under))     # 64: 4 294 049 792 B; 128: 4 290 774 016 B
        pred(f"slab{C}_batch_at_limit", "pixgemm", False, slab_ok, B=32 if C == 64 else 16, aHs=1024, aWs=1024, Mrows=512 * 512, aW=512, oHs=512, oWs=512)   # images of 128 / 256 MB: 4 GiB together
        pcx_ok = dict(B=2, aHs=5, aWs=7, aCs=C, Mrows=35, aW=7, K=C, Kw=C, N=4 * C, oHs=10, oWs=14, oCs=C, omode=2, r=2, Cout=C, act=1, alpha=0.1, rHs=11, rWs=16, rCs=C, ry0=1, rx0=2)
        pred(f"pix{C}_ok", "pixgemm", True, pcx_ok)
        pred(f"pix{C}_ok_gated", "pixgemm", True, pcx_ok, gated=1)
        pred(f"pix{C}_out_too_narrow", "pixgemm", False, pcx_ok, oWs=13)
        pred(f"pix{C}_res_rows_past_view", "pixgemm", False, pcx_ok, rHs=10)
        pred(f"pix{C}_res_negative_origin", "pixgemm", False, pcx_ok, ry0=-1)
        pred(f"slab{C}_B0", "pixgemm", False, slab_ok, B=0)
        pred(f"pix{C}_B0", "pixgemm", False, pcx_ok, B=0)
        pred(f"slab{C}_alpha_above_1", "pixgemm", True, slab_ok, act=1, alpha=1.5)                 # (merge_slab_kernel and pixgemm_kernel select v > 0 ? v : v alpha: any slope)
        pred(f"pix{C}_alpha_above_1", "pixgemm", True, pcx_ok, alpha=1.5)
        # pixgemm_kernel's three maps against 0xFFFF0000 bytes.  The output is four times the rows (out.Cs = K, r = 2), so its limit is the one a pass meets first
        at, under = (2897, 2896) if C == 64 else (2048, 2047)
        pshape = lambda s: dict(B=1, aHs=s, aWs=s, Mrows=s * s, aW=s, oHs=2 * s, oWs=2 * s, rCs=0, rHs=0, rWs=0)
        pred(f"pix{C}_out_at_limit", "pixgemm", False, pcx_ok, **pshape(at))                       # 64: 4 297 015 808 B; 128: 4 294 967 296 B
        pred(f"pix{C}_out_under_limit", "pixgemm", True, pcx_ok, **pshape(under))                  # 64: 4 294 049 792 B; 128: 4 290 774 016 B
        rs = (5793, 5794, 1, 2) if C == 64 else (4096, 4096, 1, 1)                                # a skip map at the limit behind an output under it
        pred(f"pix{C}_res_at_limit", "pixgemm", False, pcx_ok, **dict(pshape(under), rCs=C, rHs=rs[0], rWs=rs[1], ry0=rs[2], rx0=rs[3]))      # 64: 4 296 274 176 B; 128: 4 294 967 296 B
        pred(f"pix{C}_res_under_limit", "pixgemm", True, pcx_ok, **dict(pshape(under), rCs=C, rHs=2 * under, rWs=2 * under, ry0=0, rx0=0))
        pred(f"pix{C}_rows_at_limit", "pixgemm", False, pcx_ok, **pshape(5793 if C == 64 else 4096))   # rows 4 295 596 672 / 4 294 967 296 B (the output with them)
    pred("slab_gated_96", "pixgemm", False, dict(B=2, aHs=10, aWs=12, aCs=96, amode=2, kh=2, kw=2, stride=2, Mrows=30, aW=6, K=384, Kw=384, N=192, oHs=5, oWs=6, oCs=192), gated=1)


def large_cases(S, rng):
    """32-bit offsets: maps from the shared formula (kernel_ref.gen_rows), sampled pixels."""
    seed = 20261021

    def add(name, launcher, numbers, wt, bias, opix, patch, P1):
        spec = dict(kind="gemm", name=name, launcher=launcher, also_gemm=0, gen=1, seed=seed, rows=S.put(name + ".rows", opix), nrows=len(opix),
                    wt=S.put(name + ".wt", wt), bias=S.put(name + ".bias", bias))
        spec.update(numbers)
        S.cases.append(spec)
        S.meta[name] = dict(large=dict(patch=patch, P1=P1, C=numbers["aCs"], seed=seed, oCs=numbers["oCs"]), launcher=launcher)

    # merge_slab_kernel 64 -> 64: the input map just under pixgemm_supported's limit (its int row offset, counted in halves, just under 2^31)
    Cin, Wm, B = 64, 2112, 3
    Hm = PIX_MAX // (B * Wm * Cin * 2) // 2 * 2
    while B * Hm * Wm * Cin * 2 >= PIX_MAX:
        Hm -= 2
    wt, bias = weights(rng, 64, 4 * Cin)
    Ho, Wo = Hm // 2, Wm // 2
    opix = ck.sample(rng, B * Ho * Wo, [Ho * Wo, 2 * Ho * Wo, B * Ho * Wo - Wo], n_random=1024)
    b, oy, ox = opix // (Ho * Wo), opix % (Ho * Wo) // Wo, opix % Wo
    patch = (b[:, None, None] * Hm + 2 * oy[:, None, None] + np.arange(2)[None, :, None]) * Wm + 2 * ox[:, None, None] + np.arange(2)[None, None, :]
    add("limit_slab64", "pixgemm", dict(B=B, aHs=Hm, aWs=Wm, aCs=Cin, amode=2, kh=2, kw=2, stride=2, Mrows=Ho * Wo, aW=Wo, K=4 * Cin, Kw=4 * Cin, N=64, oHs=Ho, oWs=Wo, oCs=64),
        wt, bias, opix, patch, dict(amode=2, kh=2, kw=2, stride=2, Mrows=1, aW=1, K=4 * Cin, N=64, wt=wt, bias=bias, out_shape=(1, 1, 64)))
    # conv3_kernel 64 -> 64: three images of 1.48 GB (4.4 GB together, each under the 2^31-byte image limit): the size_t image bases at image 1 and 2
    Hc = Wc = 3400
    B, Ho, Wo = 3, Hc - 2, Wc - 2
    assert B * Hc * Wc * 128 > 1 << 32 and Ho * Wo * 128 < (1 << 31) - 1
    wt, bias = weights(rng, 64, 576)
    opix = ck.sample(rng, B * Ho * Wo, [Ho * Wo, 2 * Ho * Wo, (1 << 32) // 128, (1 << 31) // 64], n_random=1024)
    b, oy, ox = opix // (Ho * Wo), opix % (Ho * Wo) // Wo, opix % Wo
    patch = (b[:, None, None] * Hc + oy[:, None, None] + np.arange(3)[None, :, None]) * Wc + ox[:, None, None] + np.arange(3)[None, None, :]
    add("limit_conv3_images", "conv3", dict(B=B, aHs=Hc, aWs=Wc, aCs=64, amode=2, kh=3, kw=3, Mrows=Ho * Wo, aW=Wo, K=576, Kw=576, N=64, oHs=Ho, oWs=Wo, oCs=64, act=1, alpha=0.2),
        wt, bias, opix, patch, dict(amode=2, kh=3, kw=3, Mrows=1, aW=1, K=576, N=64, wt=wt, bias=bias, act=1, alpha=0.2, out_shape=(1, 1, 64)))


# ---------------------------------------------------------------- the run
@pytest.fixture(scope="module")
def run(tmp_path_factory, pkg):
    t0 = time.time()
    d = str(tmp_path_factory.mktemp("cunet_check"))
    exe = kr.build_harness(os.path.join(d, "cunet_check"), "cunet_check.cpp")
    S = build_suite(d)
    t1 = time.time()
    p = subprocess.run([exe, LIB, d], capture_output=True, text=True, timeout=300)      # one child process; after a non-zero exit nothing is retried
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = {}
    for line in p.stdout.splitlines():
        if line.startswith("CASE "):
            f = line.split()
            res[f[1]] = {k: float(v) for k, v in (t.split("=") for t in f[2:])}
    assert set(res) == set(S.meta), set(S.meta) - set(res)
    print(f"cunet_check: {len(S.cases)} cases, build + inputs {t1 - t0:.1f} s, harness {time.time() - t1:.1f} s")
    S.cache = {}
    yield S, res
    print(f"cunet_check: the file took {time.time() - t0:.1f} s")


def _record(rec):
    if _OUT:
        with open(_OUT, "a") as f:
            f.write(json.dumps(rec) + "\n")
    print("KERNEL " + json.dumps(rec), flush=True)


# ---------------------------------------------------------------- evaluation
def judge(rec_name, got, exact, ideal, P=None, single_store=False, exact_derived=None):
    """The bounds of one output -> (record, violated bounds).  got: fp16 array; exact / ideal: float64, NaN where nothing is stored."""
    mask = ~np.isnan(exact)
    bad = []
    if not (got.view(np.uint16)[~mask] == 0xA5A5).all():
        bad.append("cells_outside_written")
    g64 = got.astype(np.float64)
    k, i = kr.error_metrics(g64[mask], exact[mask]), kr.error_metrics(ideal[mask], exact[mask])
    rec = {"case": rec_name, "kernel": k, "ideal_fp16": i}
    if not np.isfinite(g64[mask]).all():
        bad.append("non_finite")
    if not k["max_ulp"] <= i["max_ulp"] + REL_MAX_ALLOW:
        bad.append("max")
    if not k["rms_ulp"] <= REL_RMS_FACTOR * i["rms_ulp"]:
        bad.append("rms")
    if not k["frac_1ulp"] >= i["frac_1ulp"] - FRAC_MARGIN:
        bad.append("frac_1ulp")
    if not abs(k["mean_ulp"]) <= abs(i["mean_ulp"]) + MEAN_ALLOW + 4 * k["rms_ulp"] / np.sqrt(k["n"]):
        bad.append("mean_signed")
    if single_store and P is not None:
        q = dict(P, a=np.abs(np.nan_to_num(np.asarray(P["a"], np.float64))), wt=np.abs(P["wt"].astype(np.float64)), bias=np.abs(np.asarray(P["bias"], np.float64)), act=0, clip=None,
                 stats=False, pool=None)
        mag = kr.gemm_ref(q)["out"]
        ex = exact if exact_derived is None else exact_derived
        with np.errstate(invalid="ignore"):
            bound = 0.5 * kr.ulp16(np.maximum(np.abs(ex), np.abs(g64))) + (P["K"] + 1) * 2.0 ** -23 * mag
            excess = (np.abs(g64 - ex) - bound)[mask]
            rec["derived_bound_worst_margin"] = float((np.abs(g64 - ex) / bound)[mask].max())
        if not (excess <= 0).all():
            bad.append("derived_elementwise")
    rec["violations"] = bad
    return rec, bad


def resolve(S, P):
    """The parameter set with the maps and gates that an earlier case of the run wrote (the gate chain) read from their files."""
    Q = dict(P)
    for key, dt in (("a", np.float16), ("res", np.float16), ("a_scale", np.float32), ("res_scale", np.float32)):
        v = P.get(key)
        if isinstance(v, str):
            shp = (P.get("shapes") or {}).get(key)
            arr = np.fromfile(os.path.join(S.dir, v), dtype=dt)
            Q[key] = arr.reshape(shp) if shp else arr.reshape(np.asarray(Q["a" if key == "a_scale" else "res"]).shape[0], -1)
    return Q


def pool_check(rec, got_pool, stored, P, tiling, bad):
    """Partials against float64 column sums of the kernel's own stored outputs, per tile and in tile order: |err| <= (n - 1) 2^-24 sum |v|."""
    ref = kr.pool_sums(stored, P["Mrows"], P["aW"], tiling)
    mag, n = kr.pool_abs_counts(stored, P["Mrows"], P["aW"], tiling)
    got = got_pool.reshape(ref.shape).astype(np.float64)
    bound = (n - 1) * 2.0 ** -24 * mag
    with np.errstate(invalid="ignore", divide="ignore"):
        rec["pool_worst_margin"] = float(np.nan_to_num((np.abs(got - ref) / bound), nan=0.0, posinf=np.inf).max()) if got.size else 0.0
    rec["pool_partials"] = int(got.size)
    if not (np.abs(got - ref) <= bound).all():
        bad.append("pool")


def evaluate(S, res, name):
    """All records of one case: [(record, violations)]."""
    if name in S.cache:
        return S.cache[name]
    m = S.meta[name]
    out = []
    if "pair" in m:
        P1, P2 = m["pair"]
        exact_mid, exact = kr.two_launches(P1, P2)
        ideal_mid, ideal = kr.two_launches(P1, P2, True)
        oshape = (P2["a"].shape[0],) + tuple(P2["out_shape"])
        out.append(judge(name + ":first", S.read(name + ".mid", np.float16, exact_mid.shape), exact_mid, ideal_mid))
        out.append(judge(name, S.read(name + ".y", np.float16, oshape), exact, ideal))
        out.append(judge(name + ":fused", S.read(name + ".fy", np.float16, oshape), exact, ideal))
    elif "large" in m:
        L = m["large"]
        a = kr.gen_rows(L["patch"].reshape(-1), L["C"], L["seed"]).reshape(L["patch"].shape + (L["C"],))
        P = dict(L["P1"], a=a)
        exact, ideal = kr.gemm_ref(P)["out"], kr.gemm_ref(P, True)["out"]
        got = S.read(name + ".y", np.float16, (-1, L["oCs"])).reshape(exact.shape)
        out.append(judge(name, got, exact, ideal, P, True))
    elif "se" in m:
        se = m["se"]
        pool = np.fromfile(os.path.join(S.dir, se["pool"]), np.float32).reshape(se["shape"]) if isinstance(se["pool"], str) else np.asarray(se["pool"], np.float32)
        args = (pool, se["inv_count"], se["w1"], se["b1"], se["w2"], se["b2"])
        ref, f32, da = kr.se_ref(*args), kr.se_ref(*args, dtype=np.float32).astype(np.float64), kr.se_bound(*args)
        got = S.read(name + ".gates", np.float32, ref.shape).astype(np.float64)
        unit = 2.0 ** -24 * ref
        rec = {"case": name, "se": {"max_abs_err": float(np.abs(got - ref).max()), "kernel_err_units": float((np.abs(got - ref) / unit).max()),
                                    "numpy_f32_err_units": float((np.abs(f32 - ref) / unit).max()), "derived_da_quarter_units_min": float((0.25 * da / unit).min()),
                                    "allowed_units": SE_C, "bound_used_max": float((np.abs(got - ref) / (0.25 * da + SE_C * unit)).max())}}
        bad = [] if (np.abs(got - ref) <= 0.25 * da + SE_C * unit).all() and np.isfinite(got).all() else ["se_gate"]
        rec["violations"] = bad
        out.append((rec, bad))
    else:
        P = resolve(S, m["P"])
        tiling = {"conv3": ("tiles", 8, 64), "gemm": ("rows", 128)}
        Pg = P if P.get("a_scale") is None else dict(P, a=kr.f16(np.asarray(P["a"], np.float64) * np.asarray(P["a_scale"], np.float64)[:, None, None, :]), a_scale=None)
        exact = kr.gemm_ref(P)["out"]
        exact_d = kr.gemm_ref(Pg)["out"] if Pg is not P else None      # the derived bound's operands: a = fp16(x s)
        shape = exact.shape
        for ext, pext, tag, L in [(".y", ".pool", "", m["launcher"])] + ([(".gy", ".gpool", "@gemm", "gemm")] if m["also"] else []):
            ideal = kr.gemm_ref(dict(P, round_once=P.get("round_once") and L == "conv3h"), True)["out"]
            got = S.read(name + ext, np.float16, shape)
            rec, bad = judge(name + tag, got, exact, ideal, Pg, m["single_store"], exact_d)
            if m["pool"]:
                pool_check(rec, np.fromfile(os.path.join(S.dir, name + pext), np.float32), np.where(np.isnan(exact), 0.0, got.astype(np.float64)), P, tiling[L], bad)
            if P.get("poisoned") is not None:
                rec["poisoned_cells"] = P["poisoned"]
            out.append((rec, bad))
        if len(out) == 2:
            mask = ~np.isnan(exact)       # (ULP16 of the exact value with error_metrics' floor: the two kernels add in different orders)
            d = kr.error_metrics(S.read(name + ".y", np.float16, shape)[mask], S.read(name + ".gy", np.float16, shape).astype(np.float64)[mask])["max_ulp"]
            out[0][0]["against_gemm_kernel_ulp16"] = d
            if not (m["launcher"] == "conv3h" and P.get("res") is not None) and not d <= AGAINST_GEMM_MAX:      # (rounds once where gemm_kernel rounds twice: through the models only)
                out[0][1].append("against_gemm_kernel")
    S.cache[name] = out
    return out


def names(S, pred):
    return [n for n in S.meta if pred(n, S.meta[n])]


def test_every_case_ran_clean(run):
    S, res = run
    for n, m in S.meta.items():
        r = res[n]
        if m.get("refuse") or "predicate" in m:
            continue
        if m.get("rows"):
            assert r["err"] == 0, (n, "a workgroup of the kernel owns another number of rows than the cases around its edge assume")
            continue
        assert r["err"] == 0 and r["gerr"] == 0 and r["guards"] == 1, (n, r)
        assert r["det"] == 1, (n, "two runs differ")
        assert r["first"] == 1, (n, "the first image alone differs from the same image in the batch")
        assert r["untouched"] == 1, (n, "a fused launch wrote the map it replaces")


def test_refusals_and_predicate_audit(run):
    """launch_se refuses from the sizes alone (hipErrorInvalidValue, the gates untouched); every predicate refuses what its kernel could not address and still
    takes the engine's shapes."""
    S, res = run
    wrong = []
    for n in names(S, lambda n, m: m.get("refuse")):
        if not (res[n]["err"] == 1 and res[n]["untouched"] == 1):
            wrong.append((n, res[n]))
    for n in names(S, lambda n, m: "predicate" in m):
        if not ((res[n]["err"] == 0) == S.meta[n]["predicate"] and res[n]["untouched"] == 1):
            wrong.append((n, S.meta[n]["predicate"], res[n]))
    assert not wrong, wrong


FAMILIES = ["conv3_64x64", "conv3_64x128", "conv3_128x64", "conv3_128x256", "conv3_256x128", "stempair", "uppair", "head64", "head32", "head128", "slab", "pix", "gemm", "chain", "se_alone",
            "limit"]


@pytest.mark.parametrize("family", FAMILIES)
def test_kernels_against_float64(run, family):
    S, res = run
    failed = []
    cases = names(S, lambda n, m: "~" not in n and n.startswith(family))
    assert cases
    for n in cases:
        for rec, bad in evaluate(S, res, n):
            rec["harness"] = res[n]
            _record(rec)
            if bad:
                failed.append((rec["case"], bad, rec))
    assert not failed, failed


def test_fourth_channel_of_three_channel_heads(run):
    """Rows-mode heads with N = 3 store four halves per pixel: the fourth holds clip(res[..., 3]) - zero weights, zero bias - and exactly 0 without a skip map."""
    S, _ = run
    for n in names(S, lambda n, m: n.startswith("head") and "~" not in n and "_pix_" not in n):
        P = S.meta[n]["P"]
        ref = kr.gemm_ref(P, True)["out"][..., 3]
        mask = ~np.isnan(ref)
        got = S.read(n + ".y", np.float16, ref.shape + (4,))[..., 3].astype(np.float64)
        assert mask.any() and np.array_equal(got[mask], ref[mask]), n


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
        if n == "conv3_64x64_9x65~perm_row_swap@gemm":
            assert not bad, (n, "gemm_kernel reads p.wt, which the layout mutant leaves true", bad)
            continue
        assert bad, (n, "mutant passed every bound")
    assert "against_gemm_kernel" in caught["conv3_64x64_9x65~perm_row_swap"]      # the frag_conv3b copy disagrees with [N][K]: conv3_kernel parts from gemm_kernel
    deltas = sorted(float(n.split("=")[1].split("@")[0]) for n in caught if "bias_delta=" in n)
    assert deltas == [0.00048828125] * 2 + [0.00390625] * 2 + [0.03125] * 2 and smallest == 0.00048828125      # half an ULP16 of the typical output on one of 256 channels


def test_byte_identities(run):
    """STEM / UP against their two launches; conv3h_kernel<PIX, true> against the walk; a folded gate against launch_scale in place + the ungated launch."""
    S, res = run
    for n in names(S, lambda n, m: "pair" in m):
        a, b = np.fromfile(os.path.join(S.dir, n + ".y"), np.uint16), np.fromfile(os.path.join(S.dir, n + ".fy"), np.uint16)
        assert len(a) and np.array_equal(a, b), (n, int((a != b).sum()))
    tiles = names(S, lambda n, m: n.endswith("_tile"))
    assert len(tiles) == 20
    for n in tiles:
        a, b = np.fromfile(os.path.join(S.dir, n + ".y"), np.uint16), np.fromfile(os.path.join(S.dir, n[:-5] + ".y"), np.uint16)
        assert len(a) and np.array_equal(a, b), (n, int((a != b).sum()))
    folded = [c["name"] for c in S.cases if c.get("scale_ident")]
    assert len(folded) >= 20
    for n in folded:
        assert res[n]["ident"] == 1, (n, "folding the gate changed a bit")


def test_gates_of_the_two_producers_agree(run):
    """conv3_kernel<true, 0> and gemm_kernel pool the same map into different partials (4 pixel tiles, 5 row tiles): the gates launch_se makes of them agree within the
    sum of their derived bounds; and the partials' tile counts are conv3_tiles / ceil(Mrows / 128), which is what launch_se was told."""
    S, res = run
    for C in (64, 128):
        ga, gb = (S.read(f"chain{C}_se_{k}.gates", np.float32, (3, C)).astype(np.float64) for k in ("conv3", "gemm"))
        sa, sb = (S.meta[f"chain{C}_se_{k}"]["se"] for k in ("conv3", "gemm"))
        bound = 0.0
        for se in (sa, sb):
            pool = np.fromfile(os.path.join(S.dir, se["pool"]), np.float32).reshape(se["shape"])
            args = (pool, se["inv_count"], se["w1"], se["b1"], se["w2"], se["b2"])
            bound = bound + 0.25 * kr.se_bound(*args) + SE_C * 2.0 ** -24 * kr.se_ref(*args)
        # the two maps pooled are the two kernels' own outputs, at most AGAINST_GEMM_MAX ULP16 apart per element: a mean shift of at most that, through both layers
        y, gy = (S.read(f"chain{C}_prod" + e, np.float16, (3, 9, 65, C)).astype(np.float64) for e in (".y", ".gy"))
        dmean = np.abs(y - gy).mean(axis=(1, 2))
        bound = bound + 0.25 * (dmean @ np.abs(sa["w1"].astype(np.float64)).T) @ np.abs(sa["w2"].astype(np.float64)).T
        _record({"case": f"chain{C}_gates_agree", "max_diff": float(np.abs(ga - gb).max()), "bound_min": float(bound.min())})
        assert (np.abs(ga - gb) <= bound).all(), C


def test_recorded_fractions_cover_every_record(run):
    """tests/golden/cunet_kernel_frac.json holds the kernel's and the ideal model's fraction within 1 ULP16 of every unmutated record (the bound itself is the model's
    fraction computed here)."""
    S, res = run
    missing = []
    for n in names(S, lambda n, m: "~" not in n and not (m.get("refuse") or "predicate" in m or "se" in m or m.get("rows"))):
        for rec, _ in evaluate(S, res, n):
            if rec["case"] not in FRAC_RECORDED:
                missing.append(rec["case"])
    assert not missing, missing
