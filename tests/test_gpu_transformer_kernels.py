"""The four fused fp16 transformer kernels alone - swin_attn96_kernel, swin_attn192u_kernel, mlp96q_kernel (with and without the folded image head)
and mlp2_kernel<192,2,4> - against the float64 references of tests/kernel_ref.py, through the library as built (tools/kernel_check/transformer_check.cpp
calls w2x::launch_swin_attn / w2x::launch_mlp of libw2x.so, so the code objects and their build flags are the shipped ones).

Every case prints one KERNEL {json} line (errors in ULP16 of the exact reference; the same for the ideal fp16 kernel of kernel_ref.py) and is held to:
  * max    <= the ideal fp16 kernel's max + REL_MAX_ALLOW, rms <= 1.1 x its rms (parity_util's pattern at kernel scale);
  * the fraction within 1 ULP16 >= a floor just under the measured one (FRAC_MEASURED, profiles/kernel_check/);
  * |mean signed error| <= |the ideal kernel's| + MEAN_ALLOW (a systematic bias: a wrong GELU, a biased epilogue);
  * statistics outputs against float64 statistics of the kernel's own stored y (STATS_*);
  * guard bands around every output unchanged, two runs bit-identical, the first half of the rows / images alone bit-identical,
    one NaN confined to its row (MLP) or window (attention; swin_attn96_kernel: and the left-over queries of the window it shares a wave with),
    refused parameters refused without a launch.
Mutants (one value handed to the kernel changed, the reference keeping the true one) must fail those bounds.  The three run-splitting cases put a
pass just past the launchers' 4 GB cut and check sampled rows around it."""
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
# W2X_KERNEL_CHECK_OUT=<file>: the KERNEL records are appended there as JSON lines as well (how profiles/kernel_check/kernel_check.jsonl was taken)
_OUT = os.environ.get("W2X_KERNEL_CHECK_OUT")

# Bounds (profiles/kernel_check/: every case, the mutants).  The maxima of kernel and ideal kernel are taken over different elements; where the two
# round on opposite sides of the exact value they part by up to 1.55 ULP16 on y (mlp96_M385: 8.72 against 7.17, attn192_6x12_B2_shift: 5.27 against
# 4.26) and 2.4 ULP16 on the head's outputs, which round twice (y, then the head).  The smallest change of one bias entry that `max` alone sees:
# 0.03125 in log2 units at C = 96 (12.5 against 4.6 ULP16), 0.125 at C = 192 (7.3 against 4.7).
REL_MAX_ALLOW = 2.0      # ULP16 over the ideal fp16 kernel's max (y)
HEAD_MAX_ALLOW = 3.0     # the same for the folded image head's outputs
REL_RMS_FACTOR = 1.10    # on its rms (measured <= 1.02)
MEAN_ALLOW = 0.03        # ULP16 over the ideal kernel's |mean signed error|, plus 4 standard errors of the mean
FRAC_FLOOR_MARGIN = 0.005
# measured fraction within 1 ULP16 per case (the inputs are seeded, the kernels deterministic); the floor is FRAC_FLOOR_MARGIN below
FRAC_MEASURED = {
    "attn96_6x6_B1": 0.8898, "attn96_6x12_B2_shift": 0.8506, "attn96_12x6_B3_shift": 0.8503, "attn96_18x18_B3_random": 0.9051,
    "attn96_18x18_B2_shift": 0.8811, "attn96_18x18_B2_shift_table": 0.8811, "attn96_18x18_B1_shift_half": 0.882, "attn96_12x12_B2_offset": 1.0,
    "attn96_12x12_B2_wide": 1.0, "attn96_12x12_B2_spike": 0.8073, "attn96_engine_T64_48x48": 0.8942, "attn96_engine_T256_240x240": 0.9022,
    "attn192_6x6_B1": 0.9064, "attn192_6x12_B2_shift": 0.8566, "attn192_12x6_B3_shift": 0.8527, "attn192_18x18_B3_random": 0.903,
    "attn192_18x18_B2_shift": 0.8798, "attn192_18x18_B2_shift_table": 0.8798, "attn192_18x18_B1_shift_half": 0.8822, "attn192_12x12_B2_offset": 1.0,
    "attn192_12x12_B2_wide": 1.0, "attn192_12x12_B2_spike": 0.8373, "attn192_engine_T64_24x24": 0.8836, "attn192_engine_T64_12x12": 0.8694,
    "attn192_engine_T256_120x120": 0.9002, "attn192_engine_T256_60x60": 0.8966, "mlp96_M1": 0.8125, "mlp96_M31": 0.7954, "mlp96_M32": 0.8001,
    "mlp96_M33": 0.7907, "mlp96_M383": 0.7875, "mlp96_M384": 0.7942, "mlp96_M385": 0.7986, "mlp96_M3001": 0.7924, "mlp96_M3001_offset": 1.0,
    "mlp96_M3001_wide": 0.9999, "mlp96_M1500_half": 0.7934, "mlp96_engine_T256": 0.7917, "mlp96_head_B2_clip": 0.862, "mlp96_head_B2_noclip": 0.7118,
    "mlp96_head_engine_T256": 0.8639, "mlp192_M1": 0.7708, "mlp192_M31": 0.8253, "mlp192_M32": 0.8066, "mlp192_M33": 0.8164, "mlp192_M127": 0.812,
    "mlp192_M128": 0.8192, "mlp192_M129": 0.8194, "mlp192_M3001": 0.8151, "mlp192_M3001_offset": 1.0, "mlp192_M3001_wide": 1.0,
    "mlp192_M1500_half": 0.8146, "mlp192_engine_T256": 0.815, "split_attn192": 0.9234, "split_mlp192": 0.8398,
    "split_mlp96_head": 0.8711,
}
# |rstd / rstd64 - 1| / (1 + mean^2 / var), single-pass fp32 variance (sum_sq8): measured <= 3.6e-7; eps_out 1e-5 -> 1e-4 moves it by 3.8e-5 - 5.9e-5
STATS_RSTD_REL = 2.0e-6
STATS_MEAN_REL = 2.0e-7  # |mean - mean64| / sqrt(mean^2 + var): measured <= 4.3e-8
EPS = 1e-5


# ---------------------------------------------------------------- inputs
def f16a(a):
    return np.asarray(a, dtype=np.float64).astype(np.float16)


def rows_data(rng, shape, kind):
    if kind == "normal":
        return f16a(rng.normal(0, 1, shape))
    if kind == "offset":        # |mean| / std ~ 30 per row: the single-pass variance of the statistics
        m = rng.choice([-30.0, 30.0], shape[:-1] + (1,))
        return f16a(m + rng.normal(0, 1, shape))
    if kind == "wide":          # |x| up to 64
        return f16a(np.clip(rng.normal(0, 16, shape), -64, 64))
    raise ValueError(kind)


def attn_weights(rng, C):
    return {"wqkv": f16a(rng.normal(0, C ** -0.5, (3 * C, C))), "bqkv": rng.normal(0, 0.2, 3 * C).astype(np.float32),
            "wproj": f16a(rng.normal(0, C ** -0.5, (C, C))), "bproj": rng.normal(0, 0.2, C).astype(np.float32)}


def mlp_weights(rng, C):
    w1 = rng.normal(0, C ** -0.5, (2 * C, C))
    w1[:16] *= 6.0           # hidden units whose pre-activations pass the GELU clamp (|h| > 6.5) in both signs
    return {"w1": f16a(w1), "b1": rng.normal(0, 0.2, 2 * C).astype(np.float32), "w2": f16a(rng.normal(0, (2 * C) ** -0.5, (C, 2 * C))),
            "b2": rng.normal(0, 0.2, C).astype(np.float32), "tiw": f16a(rng.normal(0, C ** -0.5, (64, C))), "tib": rng.normal(0.5, 0.2, 64).astype(np.float32)}


class Suite:
    def __init__(self, d):
        self.dir, self.cases, self.meta = d, [], {}

    def put(self, name, arr):
        np.ascontiguousarray(arr).tofile(os.path.join(self.dir, name))
        return name

    def add(self, meta, **spec):
        self.cases.append(spec)
        self.meta[spec["name"]] = meta

    def read(self, name, dtype, shape):
        return np.fromfile(os.path.join(self.dir, name), dtype=dtype).reshape(shape)


def attn_case(S, rng, name, C, B, H, W, w, wname, data="normal", shift=0, nmask=None, stats=0, table=False, spike=False, x=None, mutate="", bias=None, maskid=None):
    nwin = H * W // 36
    if bias is None:
        if nmask is None:       # the real Swin mask classes (shift) or none, on a random rel-pos bias
            masks, maskid = kr.swin_shift_masks(H, W) if shift else (np.zeros((1, 36, 36)), np.zeros(nwin, np.int32))
            bias = f16a(rng.normal(0, 1, (len(masks), 6, 36, 36)) + masks[:, None])
        else:                   # random tables, random classes
            bias = f16a(rng.normal(0, 1, (nmask, 6, 36, 36)))
            maskid = rng.integers(0, nmask, nwin).astype(np.int32)
            maskid[-1] = nmask - 1
        if spike:               # one key of each query 25 (36 in log2 units) above the rest, in every window of the last class
            b = bias.astype(np.float64)
            b[-1, :, np.arange(36), rng.integers(0, 36, 36)] = 25.0
            bias = f16a(b)
    if x is None:
        x = rows_data(rng, (B, H, W, C), data)
    tab = kr.window_table(H, W, shift, shift)
    spec = dict(kind="attn", name=name, C=C, B=B, H=H, W=W, nmask=len(bias), stats=stats, w=wname, ry=-1 if table else shift, rx=-1 if table else shift,
                scale=(C // 6) ** -0.5, eps=EPS, eps_out=EPS, x=S.put(name + ".x", x), bias=S.put(name + ".bias", bias), maskid=S.put(name + ".maskid", maskid), mutate=mutate)
    if table:
        spec["table"] = S.put(name + ".table", tab)
    S.add(dict(x=x, w=w, bias=bias, maskid=maskid, table=tab, stats=stats, C=C), **spec)


def mlp_case(S, rng, name, C, M, w, wname, data="normal", stats=0, x=None, head=None, mutate=""):
    if x is None:
        x = rows_data(rng, (M, C), data)
    spec = dict(kind="mlp", name=name, C=C, M=M, stats=stats, w=wname, eps=EPS, eps_out=EPS, x=S.put(name + ".x", x), mutate=mutate)
    if head:
        spec.update(head=1, B=head["B"], ti_Hs=4 * head["Mrows"] // head["aW"], ti_Ws=4 * head["aW"], ti_Mrows=head["Mrows"], ti_aW=head["aW"],
                    ti_clip=1 if head.get("clip") else 0, ti_lo=(head.get("clip") or (0, 0))[0], ti_hi=(head.get("clip") or (0, 0))[1])
    S.add(dict(x=x, w=w, stats=stats, C=C, head=head), **spec)


# ---------------------------------------------------------------- run-splitting cases (inputs from the shared formula)
ATTN_MAX = 0xFFFFFF00                    # k_swinattn*.hip kMaxBufBytes: runs of whole images
MLP2_MAX = 0xFFF00000                    # launch_mlp2_c: runs of whole 128-row workgroups
MLP96_MAX = 0xFFF00000                   # k_mlp96q.hip kMaxBufBytes: runs of whole 32-row tiles, one workgroup per CU


def sample_rows(rng, cuts, total, n_random=4096):
    """First and last row of each run, +-8 rows around each cut, n_random random rows."""
    s = {0, total - 1}
    for c in cuts:
        s.update(range(max(0, c - 8), min(total, c + 8)))
    s.update(rng.integers(0, total, n_random).tolist())
    return np.array(sorted(s), dtype=np.int64)


def large_cases(S, rng, w96, w192, a192, ncu):
    seed = 20261015
    # C = 192 attention: the smallest B with two runs; windows sampled (every pixel of a sampled window comes back)
    H = W = 96
    nwin = 256
    img = nwin * 36 * 192 * 2
    per_run = ATTN_MAX // img
    B = per_run + 1
    masks, maskid = kr.swin_shift_masks(H, W)
    bias = f16a(rng.normal(0, 1, (len(masks), 6, 36, 36)) + masks[:, None])
    wins = set()
    for b in (0, 1, *range(per_run - 8, B)):
        wins.update((b, wl) for wl in (0, 1, nwin - 2, nwin - 1, *rng.integers(0, nwin, 4).tolist()))
    wins.update(zip(rng.integers(0, B, 120).tolist(), rng.integers(0, nwin, 120).tolist()))
    wins = sorted(wins)
    tab = kr.window_table(H, W, 3, 3)
    pix = np.array([b * H * W + tab[wl * 36 + t] for b, wl in wins for t in range(36)], dtype=np.int64)
    name = "split_attn192"
    S.add(dict(large=True, wins=wins, pix=pix, w=a192, bias=bias, maskid=maskid, C=192, seed=seed, stats=1, runs=[0, per_run], B=B),
          kind="attn", name=name, C=192, B=B, H=H, W=W, nmask=len(bias), stats=1, w="a192", ry=3, rx=3, scale=32 ** -0.5, eps=EPS, eps_out=EPS,
          gen=1, seed=seed, bias=S.put(name + ".bias", bias), maskid=S.put(name + ".maskid", maskid), rows=S.put(name + ".rows", pix), nrows=len(pix))
    # C = 192 MLP: just past one run
    max_rows = (MLP2_MAX // 384) // 128 * 128
    M = max_rows + 1000
    rows = sample_rows(rng, [max_rows], M)
    name = "split_mlp192"
    S.add(dict(large=True, rows=rows, w=w192, C=192, seed=seed + 1, stats=1, runs=[0, max_rows]),
          kind="mlp", name=name, C=192, M=M, stats=1, w="m192", eps=EPS, eps_out=EPS, gen=1, seed=seed + 1, rows=S.put(name + ".rows", rows), nrows=len(rows))
    # C = 96 MLP with the image head: 240 x 240 token maps (the engine's at T = 256), the cut inside an image
    max_rows = min(MLP96_MAX // (32 * 192), 0xFFFFFFFF // (32 * 192) - ncu * 12) * 32     # launch_mlp96q: room for the prefetch of 12 tiles per workgroup
    Mrows, aW = 240 * 240, 240
    B = max_rows // Mrows + 1
    M = B * Mrows
    rows = sample_rows(rng, [max_rows], M)
    b, r = rows // Mrows, rows % Mrows
    oy, ox = r // aW, r % aW
    hp = ((b[:, None] * (4 * Mrows // aW) + 4 * oy[:, None] + np.repeat(np.arange(4), 4)[None]) * (4 * aW) + 4 * ox[:, None] + np.tile(np.arange(4), 4)[None]).reshape(-1)
    name = "split_mlp96_head"
    head = dict(B=B, Mrows=Mrows, aW=aW, clip=(0.0, 1.0))
    S.add(dict(large=True, rows=rows, hpix=hp.astype(np.int64), w=w96, C=96, seed=seed + 2, stats=0, head=head, runs=[0, max_rows]),
          kind="mlp", name=name, C=96, M=M, stats=0, w="m96", eps=EPS, eps_out=EPS, gen=1, seed=seed + 2, rows=S.put(name + ".rows", rows), nrows=len(rows),
          hrows=S.put(name + ".hrows", hp.astype(np.int64)), nhrows=len(hp), head=1, B=B, ti_Hs=4 * Mrows // aW, ti_Ws=4 * aW, ti_Mrows=Mrows, ti_aW=aW,
          ti_clip=1, ti_lo=0.0, ti_hi=1.0)


# ---------------------------------------------------------------- the run
def build_suite(d, ncu):
    S = Suite(d)
    rng = np.random.default_rng(1015)
    W = {}
    for C in (96, 192):
        aw, mw = attn_weights(rng, C), mlp_weights(rng, C)
        W[f"a{C}"], W[f"m{C}"] = aw, mw
        S.put(f"a{C}.wqkv", aw["wqkv"]); S.put(f"a{C}.bqkv", aw["bqkv"]); S.put(f"a{C}.wproj", aw["wproj"]); S.put(f"a{C}.bproj", aw["bproj"])
        for k in ("w1", "b1", "w2", "b2", "tiw", "tib"):
            S.put(f"m{C}.{k}", mw[k])
    for C in (96, 192):
        w, wn = W[f"a{C}"], f"a{C}"
        a = lambda name, **k: attn_case(S, rng, f"attn{C}_{name}", C, w=w, wname=wn, **k)
        a("6x6_B1", B=1, H=6, W=6)
        a("6x12_B2_shift", B=2, H=6, W=12, shift=3)
        a("12x6_B3_shift", B=3, H=12, W=6, shift=3, stats=1)
        a("18x18_B3_random", B=3, H=18, W=18, nmask=5, stats=1)
        a("18x18_B2_shift", B=2, H=18, W=18, shift=3)
        m = S.meta[f"attn{C}_18x18_B2_shift"]
        a("18x18_B2_shift_table", B=2, H=18, W=18, shift=3, table=True, x=m["x"], bias=m["bias"], maskid=m["maskid"])
        a("18x18_B1_shift_half", B=1, H=18, W=18, shift=3, x=m["x"][:1], bias=m["bias"], maskid=m["maskid"])
        a("12x12_B2_offset", B=2, H=12, W=12, data="offset", stats=1)
        a("12x12_B2_wide", B=2, H=12, W=12, data="wide", shift=3)
        a("12x12_B2_spike", B=2, H=12, W=12, nmask=2, spike=True)
        r = S.meta[f"attn{C}_18x18_B3_random"]
        xn = r["x"].copy()
        xn[1, 7, 8, 5] = np.nan
        a("18x18_B3_random_nan", B=3, H=18, W=18, x=xn, bias=r["bias"], maskid=r["maskid"])
        # the token maps of swin_unet/art scale 4 at T = 64 and 256 (describe_plan: nwin 64 / 1600 at C = 96, 16, 4 / 400, 100 at C = 192)
        for T, hw in ((64, 48), (256, 240)) if C == 96 else ((64, 24), (64, 12), (256, 120), (256, 60)):
            a(f"engine_T{T}_{hw}x{hw}", B=1, H=hw, W=hw, shift=3, stats=int(hw % 5 == 0))
        # mutants
        for mut in ("bias_lane_swap", "maskid", "eps_out", "bias_delta=0.5", "bias_delta=0.125", "bias_delta=0.03125"):
            a(f"18x18_B3_random~{mut}", B=3, H=18, W=18, x=r["x"], bias=r["bias"], maskid=r["maskid"], stats=1, mutate=mut)
        a("18x18_B2_shift_table~table_swap", B=2, H=18, W=18, shift=3, table=True, x=m["x"], bias=m["bias"], maskid=m["maskid"], mutate="table_swap")
    for C in (96, 192):
        w, wn = W[f"m{C}"], f"m{C}"
        wg = 384 if C == 96 else 128         # rows per workgroup (mlp96q: 12 waves x 32; mlp2<192,2,4>: 4 waves x 32)
        mm = lambda name, **k: mlp_case(S, rng, f"mlp{C}_{name}", C, w=w, wname=wn, **k)
        for M in (1, 31, 32, 33, wg - 1, wg, wg + 1):
            mm(f"M{M}", M=M, stats=M % 2)
        mm("M3001", M=3001, stats=1)
        mm("M3001_offset", M=3001, data="offset", stats=1)
        mm("M3001_wide", M=3001, data="wide")
        x0 = S.meta[f"mlp{C}_M3001"]["x"]
        mm("M1500_half", M=1500, x=x0[:1500], stats=1)
        xn = x0.copy()
        xn[1234, 7] = np.nan
        mm("M3001_nan", M=3001, x=xn)
        mm("engine_T256", M=230400 if C == 96 else 57600, stats=0)
        for mut in ("w2_swap", "eps_out"):
            mm(f"M3001~{mut}", M=3001, x=x0, stats=1, mutate=mut)
        if C == 96:
            mm("head_B2_clip", M=384, head=dict(B=2, Mrows=192, aW=48, clip=(0.0, 1.0)))     # the image boundary (row 192) inside a workgroup
            mm("head_B2_noclip", M=384, head=dict(B=2, Mrows=192, aW=48))
            mm("head_engine_T256", M=57600, head=dict(B=1, Mrows=57600, aW=240, clip=(0.0, 1.0)))
    for what in ("attn_C128", "attn_hd32_at_C96", "attn_no_frag", "attn_image_beyond_4GB", "attn_no_windows", "mlp_C128", "mlp_C64", "mlp_no_frag",
                 "mlp96_head_ragged_image", "mlp96_head_with_stats"):
        S.add(dict(refuse=True), kind="refuse", name=f"refuse_{what}", what=what)
    large_cases(S, rng, W["m96"], W["m192"], W["a192"], ncu)
    with open(os.path.join(d, "cases.json"), "w") as f:
        json.dump(S.cases, f)
    return S


@pytest.fixture(scope="module")
def run(tmp_path_factory, pkg):
    t0 = time.time()
    d = str(tmp_path_factory.mktemp("kernel_check"))
    exe = kr.build_harness(os.path.join(d, "transformer_check"))
    import torch
    S = build_suite(d, torch.cuda.get_device_properties(0).multi_processor_count)
    t1 = time.time()
    p = subprocess.run([exe, LIB, d], capture_output=True, text=True, timeout=240)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = {}
    for line in p.stdout.splitlines():
        if line.startswith("CASE "):
            f = line.split()
            res[f[1]] = {k: float(v) for k, v in (t.split("=") for t in f[2:])}
    assert set(res) == set(S.meta), set(S.meta) - set(res)
    print(f"kernel_check: build + inputs {t1 - t0:.1f} s, harness {time.time() - t1:.1f} s")
    yield S, res
    print(f"kernel_check: the file took {time.time() - t0:.1f} s")


def _record(rec):
    if _OUT:
        with open(_OUT, "a") as f:
            f.write(json.dumps(rec) + "\n")
    print("KERNEL " + json.dumps(rec), flush=True)


# ---------------------------------------------------------------- evaluation
def references(S, name):
    m = S.meta[name]
    C = m["C"]
    if "wqkv" in m["w"]:
        w = m["w"]
        args = (w["wqkv"], w["bqkv"].astype(np.float64), w["wproj"], w["bproj"].astype(np.float64))
        if m.get("large"):
            X = kr.gen_rows(m["pix"], C, m["seed"]).astype(np.float64).reshape(-1, 36, C)
            bw = np.asarray(m["bias"], np.float64)[m["maskid"][[wl for _, wl in m["wins"]]]]
            sc = (C // 6) ** -0.5
            return [kr.attention_windows(X, *args, bw, sc, EPS, f) .reshape(-1, C) for f in (False, True)]
        return [kr.attention(m["x"].astype(np.float64), *args, m["bias"], m["maskid"], m["table"], (C // 6) ** -0.5, EPS, f) for f in (False, True)]
    w = m["w"]
    x = kr.gen_rows(m["rows"], C, m["seed"]) if m.get("large") else m["x"]
    out = []
    for f in (False, True):
        y = kr.mlp(x.astype(np.float64), w["w1"], w["b1"].astype(np.float64), w["w2"], w["b2"].astype(np.float64), EPS, f)
        if m.get("head"):
            h = m["head"]
            hy = np.asarray(y, np.float64) @ w["tiw"].astype(np.float64).T + w["tib"]
            hy = kr.f16(hy) if f else hy
            if h.get("clip"):
                hy = np.clip(hy, *h["clip"])
            if m.get("large"):
                y = hy.reshape(-1, 4)       # the 16 sub-pixels of each sampled row, in the order of hpix
            else:
                y = kr.image_head(y, w["tiw"], w["tib"].astype(np.float64), h["B"], h["Mrows"], h["aW"], h.get("clip"), f)
        out.append(y)
    return out


def kernel_output(S, name):
    m = S.meta[name]
    C = m["C"]
    if m.get("head"):
        h = m["head"]
        if m.get("large"):
            return S.read(name + ".head", np.float16, (-1, 4))
        return S.read(name + ".head", np.float16, (h["B"], 4 * h["Mrows"] // h["aW"], 4 * h["aW"], 4))
    if m.get("large"):
        return S.read(name + ".y", np.float16, (-1, C))
    return S.read(name + ".y", np.float16, m["x"].shape)


def evaluate(S, res, name):
    """The bounds of one case -> (record, list of violated bounds)."""
    m = S.meta[name]
    exact, ideal = references(S, name)
    got = kernel_output(S, name)
    k, i = kr.error_metrics(got, exact), kr.error_metrics(ideal, exact)
    rec = {"case": name, "kernel": k, "ideal_fp16": i, "harness": res[name]}
    bad = []
    if not k["max_ulp"] <= i["max_ulp"] + (HEAD_MAX_ALLOW if m.get("head") else REL_MAX_ALLOW):
        bad.append("max")
    if not k["rms_ulp"] <= REL_RMS_FACTOR * i["rms_ulp"]:
        bad.append("rms")
    base = name.split("~")[0]
    if FRAC_MEASURED.get(base) is None or not k["frac_1ulp"] >= FRAC_MEASURED[base] - FRAC_FLOOR_MARGIN:
        bad.append("frac_1ulp")
    if not abs(k["mean_ulp"]) <= abs(i["mean_ulp"]) + MEAN_ALLOW + 4 * k["rms_ulp"] / np.sqrt(k["n"]):
        bad.append("mean_signed")
    if m["stats"]:
        st = S.read(name + ".stats", np.float32, (-1, 2)).astype(np.float64)
        y = np.asarray(got, np.float64).reshape(-1, m["C"])
        ref = kr.row_stats(y, EPS)
        var = 1.0 / ref[:, 1] ** 2 - EPS
        rs = float((np.abs(st[:, 1] / ref[:, 1] - 1) / (1 + ref[:, 0] ** 2 / var)).max())
        ms = float((np.abs(st[:, 0] - ref[:, 0]) / np.sqrt(ref[:, 0] ** 2 + var)).max())
        rec["stats"] = {"rstd_rel": rs, "mean_rel": ms}
        if not rs <= STATS_RSTD_REL:
            bad.append("stats_rstd")
        if not ms <= STATS_MEAN_REL:
            bad.append("stats_mean")
    rec["violations"] = bad
    return rec, bad


def names(S, pred):
    return [n for n in S.meta if pred(n, S.meta[n])]


def test_every_case_ran_clean(run):
    S, res = run
    for n in S.meta:
        r = res[n]
        if S.meta[n].get("refuse"):
            continue
        assert r["err"] == 0 and r["guards"] == 1, (n, r)
        if not S.meta[n].get("large"):
            assert r["det"] == 1, (n, "two runs differ")
        if S.meta[n].get("head"):
            assert r["y_untouched"] == 1, (n, "y written with the head on")


def test_refused_parameters(run):
    S, res = run
    for n in names(S, lambda n, m: m.get("refuse")):
        assert res[n]["err"] == 1 and res[n]["y_untouched"] == 1, (n, res[n])    # hipErrorInvalidValue, nothing launched


@pytest.mark.parametrize("kind", ["attn96", "attn192", "mlp96", "mlp192", "split"])
def test_kernels_against_float64(run, kind):
    S, res = run
    failed = []
    cases = names(S, lambda n, m: "~" not in n and not n.endswith("_nan") and not m.get("refuse") and (n.startswith("split") if kind == "split" else n.startswith(kind + "_")))
    assert cases
    for n in cases:
        rec, bad = evaluate(S, res, n)
        _record(rec)
        if bad:
            failed.append((n, bad, rec))
    assert not failed, failed


def test_mutants_fail_their_bounds(run):
    S, res = run
    caught, smallest = {}, None
    for n in names(S, lambda n, m: "~" in n):
        rec, bad = evaluate(S, res, n)
        rec["mutant"] = True
        _record(rec)
        caught[n] = bad
        if n.split("~")[1].startswith("bias_delta=") and bad:
            d = float(n.split("=")[1])
            smallest = d if smallest is None else min(smallest, d)
    _record({"mutants": caught, "smallest_failing_bias_delta_log2": smallest})
    for n, bad in caught.items():
        if "bias_delta=" in n:
            continue        # (the perturbation scan: recorded, the largest must fail)
        assert bad, (n, "mutant passed every bound")
    assert smallest is not None and smallest <= 0.5


def test_bit_identities(run):
    S, _ = run
    for C in (96, 192):
        a = f"attn{C}_18x18_B2_shift"
        y = kernel_output(S, a)
        assert np.array_equal(kernel_output(S, a + "_table").view(np.uint16), y.view(np.uint16)), "table path differs from the closed form"
        assert np.array_equal(kernel_output(S, f"attn{C}_18x18_B1_shift_half").view(np.uint16), y[:1].view(np.uint16)), "first image alone differs"
        full = kernel_output(S, f"mlp{C}_M3001")
        assert np.array_equal(kernel_output(S, f"mlp{C}_M1500_half").view(np.uint16), full[:1500].view(np.uint16)), "first half of the rows alone differs"
        st, sh = S.read(f"mlp{C}_M3001.stats", np.float32, (-1, 2)), S.read(f"mlp{C}_M1500_half.stats", np.float32, (-1, 2))
        assert np.array_equal(st[:1500].view(np.uint32), sh.view(np.uint32))


def test_nan_stays_in_its_row_or_window(run):
    """One NaN in one channel: the MLP row (the attention window) that holds it goes non-finite, nothing else changes a bit - for the binaries built
    with -fno-honor-nans too (W2X_POISON and the stale-read tests rely on it).  swin_attn96_kernel's left-over queries (tokens 32..35) of the two
    windows of a workgroup share one score tile, the other window's q columns zeroed: 0 x NaN reaches them there, and only there."""
    S, _ = run
    for C in (96, 192):
        clean, dirty = kernel_output(S, f"mlp{C}_M3001"), kernel_output(S, f"mlp{C}_M3001_nan")
        assert not np.isfinite(dirty[1234].astype(np.float32)).all()
        others = np.ones(len(clean), bool)
        others[1234] = False
        assert np.array_equal(clean[others].view(np.uint16), dirty[others].view(np.uint16)), C
    for C in (96, 192):
        clean, dirty = kernel_output(S, f"attn{C}_18x18_B3_random"), kernel_output(S, f"attn{C}_18x18_B3_random_nan")
        assert not np.isfinite(dirty[1, 7, 8].astype(np.float32)).all()
        tab = kr.window_table(18, 18, 0, 0).reshape(9, 36)
        a, b = clean.reshape(3, 324, C), dirty.reshape(3, 324, C)
        changed = set()
        for img in range(3):
            for w in range(9):
                for t in range(36):
                    if not np.array_equal(a[img, tab[w, t]].view(np.uint16), b[img, tab[w, t]].view(np.uint16)):
                        changed.add((img, w, t))
        win = [w for w in range(9) if 7 * 18 + 8 in tab[w]][0]
        allowed = {(1, win, t) for t in range(36)}
        if C == 96:
            allowed |= {(1, win ^ 1, t) for t in range(32, 36)}
        _record({"case": f"attn{C}_nan_isolation", "nan_window": [1, win], "changed_rows_outside_it": sorted(c for c in changed if c[:2] != (1, win))})
        assert changed <= allowed, (C, sorted(changed - allowed))


def test_gelu_clamp_region_is_exercised(run):
    S, _ = run
    for C in (96, 192):
        m = S.meta[f"mlp{C}_M3001"]
        w = m["w"]
        h = kr.f16(kr.layer_norm(m["x"].astype(np.float64), EPS)) @ w["w1"].astype(np.float64).T + w["b1"]
        assert h.max() > 6.5 and h.min() < -6.5
