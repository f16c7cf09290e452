// Drives the convolution and projection kernels of swin_unet's path in a built libw2x.so - w2x::launch_gemm (gemm_kernel), launch_stem, launch_conv48,
// launch_conv48_stem and launch_pixgemm (pixgemm_kernel, merge_kernel, toimage_kernel), found by their mangled names, so the code objects checked are the
// shipped ones - on cases that tests/test_gpu_conv_kernels.py writes:
//
//     conv_check <path of libw2x.so> <case dir>      runs <case dir>/cases.json, writes <case dir>/<name>.y (.gy: the same parameters on launch_gemm,
//                                                    .stats / .gstats, .fy: the fused stem pair, .mid: the stem's map), one CASE line per case
//
// Safety rules of this harness (no launch is made to see what happens):
//   * a specialised kernel is launched only after its own *_supported() returned true for exactly the parameters it is handed;
//   * every launch - general or specialised, mutated or not - is first walked by accesses_ok(), which restates gemm_kernel's addressing in 64-bit
//     arithmetic and requires every element read or written to lie inside the view of its map AND inside the buffer allocated for it (buffers are
//     sized as plan.cpp sizes tensors: B x Hs x Ws x Cs elements; outputs between guard bands);
//   * the first HIP error ends the process (HIPCHECK), so nothing is launched after it;
//   * "refuse" / "predicate" cases call a predicate, or launch_gemm - which checks before it launches - and report that the output stayed untouched.
// Weight copies come from fragorder.h itself: frag_major, and the 448-column padding of conv48's matrix as engine.cpp does it.
// A mutation ("mutate") changes one value handed to the kernel - the reference keeps the true one - to show that the test's bounds see it.
#include "check_common.h"

namespace {

typedef hipError_t (*Launch1)(const GemmParams&, hipStream_t);
typedef hipError_t (*Launch2)(const GemmParams&, const GemmParams&, hipStream_t);
typedef bool (*Pred1)(const GemmParams&);
typedef bool (*Pred2)(const GemmParams&, const GemmParams&);
typedef hipError_t (*LaunchMlp)(const MlpParams&, hipStream_t);
Launch1 launch_gemm_fn, launch_stem_fn, launch_conv48_fn, launch_pixgemm_fn;
Launch2 launch_conv48_stem_fn;
Pred1 stem_ok_fn, conv48_ok_fn, pixgemm_ok_fn;
Pred2 conv48_stem_ok_fn;
LaunchMlp launch_mlp_fn;

constexpr int kErrUnsupported = -2, kErrBounds = -3;     // reported instead of launching

// ---- GemmParams from the numbers of a case (keys prefixed with `pre`); pointers are set by the caller
GemmParams numbers(const Case& c, const std::string& pre) {
    auto I = [&](const char* k, long d = 0) { return (int)c.i(pre + k, d); };
    GemmParams p;
    p.a.Hs = I("aHs"); p.a.Ws = I("aWs"); p.a.Cs = I("aCs"); p.a.y0 = I("ay0"); p.a.x0 = I("ax0");
    p.amode = I("amode"); p.kh = I("kh", 1); p.kw = I("kw", 1); p.stride = I("stride", 1);
    p.B = I("B"); p.Mrows = I("Mrows"); p.aW = I("aW");
    p.K = I("K"); p.N = I("N"); p.Kw = I("Kw");
    p.ln = I("ln"); p.act = I("act"); p.alpha = (float)c.num(pre + "alpha", 0);
    p.has_clip = I("has_clip"); p.clip_lo = (float)c.num(pre + "clip_lo", 0); p.clip_hi = (float)c.num(pre + "clip_hi", 0);
    p.res.Hs = I("rHs"); p.res.Ws = I("rWs"); p.res.Cs = I("rCs"); p.res.y0 = I("ry0"); p.res.x0 = I("rx0");
    p.res2.Hs = I("r2Hs"); p.res2.Ws = I("r2Ws"); p.res2.Cs = I("r2Cs"); p.res2.y0 = I("r2y0"); p.res2.x0 = I("r2x0");
    p.out.Hs = I("oHs"); p.out.Ws = I("oWs"); p.out.Cs = I("oCs");
    p.omode = I("omode"); p.r = I("r", 1); p.Cout = I("Cout", p.out.Cs); p.ln_eps = (float)c.num(pre + "ln_eps", 1e-5);
    return p;
}

// elements allocated behind each pointer of a parameter set
struct Extents { size_t a = 0, out = 0, res = 0, res2 = 0, stats_in = 0, stats_out = 0, wt = 0, bias = 0, csum = 0, table = 0; };

Extents extents_of(const GemmParams& p) {      // as plan.cpp sizes tensors: whole stored maps of the pass
    Extents e;
    e.a = (size_t)p.B * p.a.Hs * p.a.Ws * p.a.Cs; e.out = (size_t)p.B * p.out.Hs * p.out.Ws * p.out.Cs;
    e.res = (size_t)p.B * p.res.Hs * p.res.Ws * p.res.Cs; e.res2 = (size_t)p.B * p.res2.Hs * p.res2.Ws * p.res2.Cs;
    e.stats_in = (size_t)p.B * p.a.Hs * p.a.Ws * 2; e.stats_out = (size_t)p.B * p.out.Hs * p.out.Ws * 2;
    e.wt = (size_t)p.N * p.Kw; e.bias = (size_t)p.N; e.csum = (size_t)p.N; e.table = (size_t)p.Mrows;
    return e;
}

// gemm_kernel's addressing (k_gemm.hip: the per-row bookkeeping, load_regs, epilogue phase 2), in 64-bit arithmetic: every element of every map a launch
// of `p` reads or writes must lie inside the map's view and inside `e`.  The specialised kernels touch the same elements (k_stem.hip clamps its idle lanes
// onto the row's last pixel, k_conv48.hip fetches only halo pixels inside Ho + 2 x Wo + 2, k_pixgemm.hip reads rows and skip pixels of existing rows only).
// Passes of many rows without a table are walked at the corners of every image only: all offsets are monotone in the row's y and x.
bool accesses_ok(const GemmParams& p, const Extents& e, const std::vector<int>& table, std::string& why) {
    auto fail = [&](const std::string& w) { why = w; return false; };
    if (p.B <= 0 || p.Mrows <= 0 || p.aW <= 0 || p.K <= 0 || p.N <= 0 || p.Kw < p.K || p.Kw % 8) return fail("sizes");
    if (p.a.Cs != 4 && p.a.Cs % 8) return fail("a.Cs");
    const int AP = p.a.Cs == 4 ? 4 : 8, OP = p.out.Cs == 4 ? 4 : 8;
    const int r = p.omode == 2 ? p.r : 1, ncol = p.omode == 2 ? p.out.Cs : p.N;
    if (r < 1 || ncol % OP || ncol > p.out.Cs || (p.omode == 2 && p.N != r * r * p.out.Cs)) return fail("output width");
    if (e.wt < (size_t)p.N * p.Kw || e.bias < (size_t)p.N || (p.ln && e.csum < (size_t)p.N)) return fail("weights");
    if ((p.amode == 1 || p.omode == 1) && table.size() < (size_t)p.Mrows) return fail("table");
    const int Kr = (p.K + AP - 1) / AP * AP;         // the last piece of a row is read whole
    if (p.amode == 2 ? (p.K != p.kh * p.kw * p.a.Cs || (p.kw * p.a.Cs) % AP) : Kr > p.a.Cs) return fail("K against the view");
    if (p.res.p && (ncol > p.res.Cs)) return fail("res width");
    if (p.res2.p && (ncol > p.res2.Cs)) return fail("res2 width");
    const bool corners = (long)p.B * p.Mrows > (1l << 22) && p.amode != 1 && p.omode != 1;
    std::vector<int> rows;
    if (corners) { for (int ml : {0, p.aW - 1, p.Mrows - p.aW, p.Mrows - 1}) if (ml >= 0 && ml < p.Mrows) rows.push_back(ml); }
    else { rows.resize(p.Mrows); for (int i = 0; i < p.Mrows; ++i) rows[i] = i; }
    const int ah = p.amode == 2 ? p.kh : 1, aw = p.amode == 2 ? p.kw : 1;
    for (long b = 0; b < p.B; ++b) {
        for (int ml : rows) {
            const int src = p.amode == 1 ? table[ml] : ml;
            if (src < 0) return fail("table entry");
            const long y = (long)(src / p.aW) * p.stride + p.a.y0, x = (long)(src % p.aW) * p.stride + p.a.x0;
            if (y < 0 || x < 0 || y + ah > p.a.Hs || x + aw > p.a.Ws) return fail("a row outside its view");
            const long pixoff = (b * p.a.Hs + y) * p.a.Ws + x;
            const long last = p.amode == 2 ? (pixoff + (long)(ah - 1) * p.a.Ws) * p.a.Cs + (long)aw * p.a.Cs : pixoff * p.a.Cs + Kr;
            if ((size_t)last > e.a) return fail("a row outside its buffer");
            if (p.ln && (size_t)(2 * pixoff + 2) > e.stats_in) return fail("stats_in");
            const int dst = p.omode == 1 ? table[ml] : ml;
            const long oy = p.omode == 1 ? dst / p.out.Ws : ml / p.aW, ox = p.omode == 1 ? dst % p.out.Ws : ml % p.aW;
            for (int sg = 0; sg < r * r; ++sg) {
                const long Y = oy * r + sg / r, X = ox * r + sg % r;
                if (Y < 0 || X < 0 || Y >= p.out.Hs || X >= p.out.Ws) return fail("output pixel outside its view");
                const long opix = (b * p.out.Hs + Y) * p.out.Ws + X;
                if ((size_t)(opix * p.out.Cs + ncol) > e.out) return fail("output pixel outside its buffer");
                if (p.stats_out && (size_t)(2 * opix + 2) > e.stats_out) return fail("stats_out");
                const TView* rv[2] = {&p.res, &p.res2};
                const size_t re[2] = {e.res, e.res2};
                for (int k = 0; k < 2; ++k) {
                    if (!rv[k]->p) continue;
                    const long ry = Y + rv[k]->y0, rx = X + rv[k]->x0;
                    if (ry < 0 || rx < 0 || ry >= rv[k]->Hs || rx >= rv[k]->Ws) return fail("skip pixel outside its view");
                    if ((size_t)(((b * rv[k]->Hs + ry) * rv[k]->Ws + rx) * rv[k]->Cs + ncol) > re[k]) return fail("skip pixel outside its buffer");
                }
            }
        }
        if (corners && b == 0 && p.B > 2) b = p.B - 2;      // first and last image
    }
    return true;
}

// a map of a case: from its file, or (gen = 1: the maps of 4 GB) the shared formula with the pixel index as the row
void* upload_map(const Case& c, const std::string& key, size_t pixels, int C, uint64_t seed_off) {
    Case cc = c;
    cc.s["x"] = c.str(key);
    cc.n["seed"] = (double)(c.i("seed") + (long)seed_off);
    return upload_rows(cc, pixels, C);
}

std::vector<uint16_t> transpose_taps(const std::vector<uint16_t>& w, int N, int Kw, int kh, int kw, int Cs) {   // W[n][ky][kx][c] -> W[n][kx][ky][c] (kh == kw)
    std::vector<uint16_t> o = w;
    for (int n = 0; n < N; ++n)
        for (int ky = 0; ky < kh; ++ky)
            for (int kx = 0; kx < kw; ++kx)
                for (int ch = 0; ch < Cs; ++ch) o[(size_t)n * Kw + (ky * kw + kx) * Cs + ch] = w[(size_t)n * Kw + (kx * kw + ky) * Cs + ch];
    return o;
}

struct Result {
    int err = 0, gerr = 0;                   // the launcher under test; the same parameters on launch_gemm ("also_gemm")
    bool det = true, guards = true, first = true, untouched = true;
    double ms = 0;
};

void report(const Case& c, const Result& o) {
    printf("CASE %s err=%d gerr=%d det=%d guards=%d first=%d untouched=%d ms=%.3f\n", c.str("name").c_str(), o.err, o.gerr, (int)o.det, (int)o.guards, (int)o.first, (int)o.untouched, o.ms);
    fflush(stdout);
}

// everything a parameter set points to, owned for the length of a case
struct Operands {
    std::vector<std::unique_ptr<Dev<uint16_t>>> h;
    std::vector<std::unique_ptr<Dev<float>>> f;
    std::vector<std::unique_ptr<Dev<int>>> i;
    std::vector<void*> raw;
    std::vector<int> table;
    ~Operands() { for (void* p : raw) (void)hipFree(p); }
    const void* half(const std::vector<uint16_t>& v) { h.emplace_back(new Dev<uint16_t>(v)); return h.back()->p; }
    const float* flt(const std::vector<float>& v) { f.emplace_back(new Dev<float>(v)); return (const float*)f.back()->p; }
    const int* ints(const std::vector<int>& v) { i.emplace_back(new Dev<int>(v)); return (const int*)i.back()->p; }
};

// loads the operands of `p` (numbers already set) and applies the case's mutation to what the kernel is handed
void load_operands(const Case& c, const std::string& pre, GemmParams& p, Operands& ops, const std::string& launcher) {
    const std::string mut = pre.empty() ? c.str("mutate") : "";
    std::vector<uint16_t> wt = load<uint16_t>(c.str(pre + "wt"), (size_t)p.N * p.Kw);
    std::vector<float> bias = load<float>(c.str(pre + "bias"), p.N);
    if (mut == "wt_transpose_taps") wt = transpose_taps(wt, p.N, p.Kw, p.kh, p.kw, p.a.Cs);
    if (mut == "subpixel_swap")      // the weight blocks of sub-pixels 1 and 2 trade places (the bias stays)
        for (int n = 0; n < p.out.Cs; ++n)
            for (int k = 0; k < p.Kw; ++k) std::swap(wt[(size_t)(p.out.Cs + n) * p.Kw + k], wt[(size_t)(2 * p.out.Cs + n) * p.Kw + k]);
    if (mut.rfind("bias_delta=", 0) == 0) bias[5] += (float)atof(mut.c_str() + 11);
    if (mut == "ax0+1") p.a.x0 += 1;
    if (mut == "res_origin+1") p.res.x0 += 1;
    if (mut == "alpha") p.alpha *= 1.25f;
    if (mut == "clip_hi") p.clip_hi *= 0.75f;
    if (mut == "ln_eps") p.ln_eps = 1e-4f;
    p.wt = ops.half(wt); p.bias = ops.flt(bias);
    if (launcher == "pixgemm") p.wt_frag = ops.half(frag_major(wt.data(), p.N, p.Kw));
    if (launcher == "conv48" || launcher == "pair") {      // engine.cpp: K = 432 padded to 448 zero columns, then fragment-major
        const int Kp = 448;
        std::vector<uint16_t> padded((size_t)p.N * Kp, 0);
        for (int n = 0; n < p.N; ++n) memcpy(&padded[(size_t)n * Kp], &wt[(size_t)n * p.Kw], (size_t)p.K * 2);
        p.wt_frag = ops.half(frag_major(padded.data(), p.N, Kp));
    }
    if (p.ln) {
        std::vector<float> csum = load<float>(c.str(pre + "csum"), p.N);
        if (mut == "csum") csum[5] *= 1.05f;
        p.csum = ops.flt(csum);
        p.stats_in = ops.flt(load<float>(c.str(pre + "stats_in"), (size_t)p.B * p.a.Hs * p.a.Ws * 2));
    }
    if (p.amode == 1 || p.omode == 1) {
        ops.table = load<int>(c.str(pre + "win_table"), p.Mrows);
        if (mut == "table_swap") std::swap(ops.table[0], ops.table[1]);
        p.win_table = ops.ints(ops.table);
    }
    if (!c.str(pre + "a").empty() || c.i("gen")) { void* a = upload_map(c, pre + "a", (size_t)p.B * p.a.Hs * p.a.Ws, p.a.Cs, 0); ops.raw.push_back(a); p.a.p = a; }
    if (p.res.Cs) { void* m = upload_map(c, pre + "res", (size_t)p.B * p.res.Hs * p.res.Ws, p.res.Cs, 1); ops.raw.push_back(m); p.res.p = m; }
    if (p.res2.Cs) { void* m = upload_map(c, pre + "res2", (size_t)p.B * p.res2.Hs * p.res2.Ws, p.res2.Cs, 2); ops.raw.push_back(m); p.res2.p = m; }
}

bool supported(const std::string& launcher, const GemmParams& p) {
    return launcher == "stem" ? stem_ok_fn(p) : launcher == "conv48" ? conv48_ok_fn(p) : launcher == "pixgemm" ? pixgemm_ok_fn(p) : launcher == "gemm";
}
Launch1 launcher_fn(const std::string& launcher) {
    return launcher == "stem" ? launch_stem_fn : launcher == "conv48" ? launch_conv48_fn : launcher == "pixgemm" ? launch_pixgemm_fn : launch_gemm_fn;
}

// the pixels of an output to send back: all, or those of <name>.rows
void save_out(const Case& c, const std::string& ext, const Guarded& y, const Guarded* st, const std::string& st_ext, int Cs) {
    std::vector<long> idx;
    if (c.i("nrows")) idx = load<long>(c.str("rows"), (size_t)c.i("nrows"));
    const std::vector<long>* ip = c.i("nrows") ? &idx : nullptr;
    save(c.str("name") + ext, y.rows<uint16_t>(ip, Cs));
    if (st) save(c.str("name") + st_ext, st->rows<float>(ip, 2));
}

// One parameter set on its launcher ("launcher": gemm, stem, conv48, pixgemm), optionally on launch_gemm as well ("also_gemm"): twice (bit-identical or not),
// then the first image alone (bit-identical to the batch's or not), the guard bands.
void run_gemm_case(const Case& c) {
    const std::string launcher = c.str("launcher", "gemm");
    GemmParams p = numbers(c, "");
    Operands ops;
    load_operands(c, "", p, ops, launcher);
    const Extents e = extents_of(p);
    Result o;
    std::string why;
    for (int side = 0; side < (c.i("also_gemm") ? 2 : 1); ++side) {
        const std::string L = side ? "gemm" : launcher;
        int& err = side ? o.gerr : o.err;
        Guarded y(e.out * 2);
        std::unique_ptr<Guarded> st(c.i("stats") ? new Guarded(e.stats_out * 4) : nullptr);
        GemmParams q = p;
        q.out.p = y.p(); q.stats_out = st ? (float*)st->p() : nullptr;
        if (!supported(L, q)) { err = kErrUnsupported; continue; }
        if (!accesses_ok(q, e, ops.table, why)) { fprintf(stderr, "%s: not launched: %s\n", c.str("name").c_str(), why.c_str()); err = kErrBounds; continue; }
        std::vector<const Guarded*> outs = {&y};
        if (st) outs.push_back(st.get());
        const Outcome r = run_twice([&] { return launcher_fn(L)(q, 0); }, outs);
        err = r.err; o.det = o.det && r.det; o.guards = o.guards && r.guards;
        if (!side) o.ms = r.ms;
        if (r.err) continue;
        save_out(c, side ? ".gy" : ".y", y, st.get(), side ? ".gstats" : ".stats", p.out.Cs);
        if (p.B > 1 && !c.i("gen")) {                   // the first image alone: the same maps, B = 1, fresh outputs
            const size_t yb = e.out / p.B * 2, sb = e.stats_out / p.B * 4;
            Guarded y1(yb);
            std::unique_ptr<Guarded> st1(st ? new Guarded(sb) : nullptr);
            GemmParams q1 = q;
            q1.B = 1; q1.out.p = y1.p(); q1.stats_out = st1 ? (float*)st1->p() : nullptr;
            if (supported(L, q1) && accesses_ok(q1, extents_of(q1), ops.table, why)) {
                HIPCHECK(launcher_fn(L)(q1, 0));
                HIPCHECK(hipDeviceSynchronize());
                std::vector<unsigned char> full = y.rows<unsigned char>(nullptr, 1), one = y1.rows<unsigned char>(nullptr, 1);
                full.resize(yb);
                o.first = o.first && full == one && y1.guards_intact();
                if (st) { full = st->rows<unsigned char>(nullptr, 1); one = st1->rows<unsigned char>(nullptr, 1); full.resize(sb); o.first = o.first && full == one; }
            } else o.first = false;
        }
    }
    report(c, o);
}

// stem -> conv48: the two launches (.mid, .y), then conv48_kernel<true> on the same parameters (.fy); the fused launch must not touch the map between them
void run_pair(const Case& c) {
    GemmParams ps = numbers(c, "s_"), p = numbers(c, "");
    Operands ops;
    load_operands(c, "s_", ps, ops, "stem");
    load_operands(c, "", p, ops, "pair");
    const Extents es = extents_of(ps), e = extents_of(p);
    Result o;
    std::string why;
    Guarded mid(es.out * 2), y(e.out * 2), mid2(es.out * 2), fy(e.out * 2);
    ps.out.p = mid.p(); p.a.p = mid.p(); p.out.p = y.p();
    GemmParams ps2 = ps, p2 = p;
    ps2.out.p = mid2.p(); p2.a.p = mid2.p(); p2.out.p = fy.p();
    if (es.out != e.a) throw std::runtime_error("pair: the stem's output is not the convolution's input map");
    if (!stem_ok_fn(ps) || !conv48_ok_fn(p) || !conv48_stem_ok_fn(p2, ps2)) { o.err = kErrUnsupported; report(c, o); return; }
    if (!accesses_ok(ps, es, ops.table, why) || !accesses_ok(p, e, ops.table, why)) { fprintf(stderr, "%s: not launched: %s\n", c.str("name").c_str(), why.c_str()); o.err = kErrBounds; report(c, o); return; }
    Outcome r = run_twice([&] { hipError_t s = launch_stem_fn(ps, 0); return s != hipSuccess ? s : launch_conv48_fn(p, 0); }, {&mid, &y});
    o.err = r.err; o.det = r.det; o.guards = r.guards; o.ms = r.ms;
    if (!r.err) {
        r = run_twice([&] { return launch_conv48_stem_fn(p2, ps2, 0); }, {&fy});
        o.gerr = r.err; o.det = o.det && r.det; o.guards = o.guards && r.guards && mid2.guards_intact();
        o.untouched = mid2.untouched();
    }
    if (!o.err && !o.gerr) {
        save(c.str("name") + ".mid", mid.rows<uint16_t>(nullptr, 48));
        save(c.str("name") + ".y", y.rows<uint16_t>(nullptr, 96));
        save(c.str("name") + ".fy", fy.rows<uint16_t>(nullptr, 96));
    }
    report(c, o);
}

// The image head two ways on the rows of a C = 96 MLP (the weights and the case of tests/test_gpu_transformer_kernels.py: M = 384, B = 2, Mrows = 192,
// aW = 48): launch_mlp without the head, then toimage_kernel on its y (.y); launch_mlp with the head folded in (.fy).
void run_tihead(const Case& c) {
    const int C = 96, B = (int)c.i("B"), Mrows = (int)c.i("Mrows"), aW = (int)c.i("aW");
    const long M = (long)B * Mrows;
    const std::string w = c.str("w");
    const std::vector<uint16_t> w1 = load<uint16_t>(w + ".w1", (size_t)2 * C * C), w2 = load<uint16_t>(w + ".w2", (size_t)2 * C * C), tiw = load<uint16_t>(w + ".tiw", (size_t)64 * C);
    Dev<uint16_t> d1(w1), d2(w2), df1(frag32_major(w1.data(), 2 * C, C)), df2(frag32_w2(w2.data(), C)), dtw(tiw), dtf(frag_major(tiw.data(), 64, C));
    Dev<float> db1(load<float>(w + ".b1", 2 * C)), db2(load<float>(w + ".b2", C)), dtb(load<float>(w + ".tib", 64));
    void* x = upload_rows(c, (size_t)M, C);
    const int Hs = 4 * Mrows / aW, Ws = 4 * aW;
    Guarded y((size_t)M * C * 2), ydead((size_t)M * C * 2), img((size_t)B * Hs * Ws * 4 * 2), fimg((size_t)B * Hs * Ws * 4 * 2);
    MlpParams m;
    m.x = x; m.y = y.p(); m.M = M; m.C = C; m.w1 = d1.p; m.b1 = (const float*)db1.p; m.w2 = d2.p; m.b2 = (const float*)db2.p;
    m.w1_frag = df1.p; m.w2_frag = df2.p; m.frag32 = true;
    GemmParams g;
    g.a.p = y.p(); g.a.Hs = Mrows / aW; g.a.Ws = aW; g.a.Cs = C; g.B = B; g.Mrows = Mrows; g.aW = aW; g.K = C; g.N = 64; g.Kw = C;
    g.wt = dtw.p; g.wt_frag = dtf.p; g.bias = (const float*)dtb.p; g.has_clip = (int)c.i("has_clip"); g.clip_lo = (float)c.num("clip_lo", 0); g.clip_hi = (float)c.num("clip_hi", 1);
    g.out.p = img.p(); g.out.Hs = Hs; g.out.Ws = Ws; g.out.Cs = 4; g.omode = 2; g.r = 4; g.Cout = 4;
    MlpParams mh = m;
    mh.y = ydead.p(); mh.ti_w = dtf.p; mh.ti_b = (const float*)dtb.p; mh.ti_out = fimg.p(); mh.ti_Hs = Hs; mh.ti_Ws = Ws; mh.ti_Mrows = Mrows; mh.ti_aW = aW;
    mh.ti_clip = g.has_clip; mh.ti_lo = g.clip_lo; mh.ti_hi = g.clip_hi;
    Result o;
    std::string why;
    Extents e = extents_of(g);
    if (!pixgemm_ok_fn(g)) o.err = kErrUnsupported;
    else if (!accesses_ok(g, e, {}, why)) o.err = kErrBounds;
    else {
        Outcome r = run_twice([&] { hipError_t s = launch_mlp_fn(m, 0); return s != hipSuccess ? s : launch_pixgemm_fn(g, 0); }, {&y, &img});
        o.err = r.err; o.det = r.det; o.guards = r.guards; o.ms = r.ms;
        if (!r.err) {
            r = run_twice([&] { return launch_mlp_fn(mh, 0); }, {&fimg});
            o.gerr = r.err; o.det = o.det && r.det; o.guards = o.guards && r.guards; o.untouched = ydead.untouched();
        }
        if (!o.err && !o.gerr) { save(c.str("name") + ".y", img.rows<uint16_t>(nullptr, 4)); save(c.str("name") + ".fy", fimg.rows<uint16_t>(nullptr, 4)); }
    }
    HIPCHECK(hipFree(x));
    report(c, o);
}

// "predicate": the numbers of a case with stand-in pointers through a predicate alone (ok = what it answered; nothing is launched, nothing allocated).
// "refuse": the same through launch_gemm, which must answer hipErrorInvalidValue from the sizes alone - the output stays untouched.
void run_no_launch(const Case& c, bool through_gemm) {
    GemmParams p = numbers(c, "");
    Dev<uint16_t> dummy(std::vector<uint16_t>(4096, 0));
    Guarded y(4096);
    p.a.p = dummy.p; p.wt = dummy.p; p.bias = (const float*)dummy.p; p.out.p = y.p();
    if (c.i("frag", 1)) p.wt_frag = dummy.p;
    if (p.res.Cs) p.res.p = dummy.p;
    if (p.res2.Cs) p.res2.p = dummy.p;
    if (c.i("stats")) p.stats_out = (float*)dummy.p;
    if (p.ln) { p.csum = (const float*)dummy.p; p.stats_in = (const float*)dummy.p; }
    Result o;
    if (through_gemm) {
        o.err = (int)launch_gemm_fn(p, 0);
        HIPCHECK(hipDeviceSynchronize());
    } else {
        const std::string pred = c.str("pred");
        bool ok;
        if (pred == "conv48_stem") {
            GemmParams ps = numbers(c, "s_");
            ps.a.p = dummy.p; ps.wt = dummy.p; ps.bias = (const float*)dummy.p; ps.out.p = p.a.p;
            ok = conv48_stem_ok_fn(p, ps);
        } else ok = supported(pred, p);
        o.err = ok ? 0 : 1;
    }
    o.untouched = y.untouched();
    report(c, o);
}

void* sym(void* lib, const char* name) {
    void* f = dlsym(lib, name);
    if (!f) throw std::runtime_error(std::string("the library does not export ") + name);
    return f;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        if (argc != 3) { fprintf(stderr, "usage: conv_check <libw2x.so> <case dir>\n"); return 2; }
        dir = argv[2];
        void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
        if (!lib) { fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
        launch_gemm_fn = (Launch1)sym(lib, "_ZN3w2x11launch_gemmERKNS_10GemmParamsEP12ihipStream_t");
        launch_stem_fn = (Launch1)sym(lib, "_ZN3w2x11launch_stemERKNS_10GemmParamsEP12ihipStream_t");
        launch_conv48_fn = (Launch1)sym(lib, "_ZN3w2x13launch_conv48ERKNS_10GemmParamsEP12ihipStream_t");
        launch_pixgemm_fn = (Launch1)sym(lib, "_ZN3w2x14launch_pixgemmERKNS_10GemmParamsEP12ihipStream_t");
        launch_conv48_stem_fn = (Launch2)sym(lib, "_ZN3w2x18launch_conv48_stemERKNS_10GemmParamsES2_P12ihipStream_t");
        stem_ok_fn = (Pred1)sym(lib, "_ZN3w2x14stem_supportedERKNS_10GemmParamsE");
        conv48_ok_fn = (Pred1)sym(lib, "_ZN3w2x16conv48_supportedERKNS_10GemmParamsE");
        pixgemm_ok_fn = (Pred1)sym(lib, "_ZN3w2x17pixgemm_supportedERKNS_10GemmParamsE");
        conv48_stem_ok_fn = (Pred2)sym(lib, "_ZN3w2x21conv48_stem_supportedERKNS_10GemmParamsES2_");
        launch_mlp_fn = (LaunchMlp)sym(lib, "_ZN3w2x10launch_mlpERKNS_9MlpParamsEP12ihipStream_t");
        std::ifstream f(dir + "/cases.json");
        const std::string t((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        for (const Case& c : parse_cases(t)) {
            printf("RUN %s\n", c.str("name").c_str());   // names the case if it never reports
            fflush(stdout);
            const std::string kind = c.str("kind");
            if (kind == "gemm") run_gemm_case(c);
            else if (kind == "pair") run_pair(c);
            else if (kind == "tihead") run_tihead(c);
            else if (kind == "predicate") run_no_launch(c, false);
            else if (kind == "refuse") run_no_launch(c, true);
            else throw std::runtime_error("unknown case kind " + kind);
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "conv_check: %s\n", e.what());
        return 1;
    }
    return 0;
}
