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

typedef hipError_t (*LaunchMlp)(const MlpParams&, hipStream_t);
Launch1 launch_gemm_fn, launch_stem_fn, launch_conv48_fn, launch_pixgemm_fn;
Launch2 launch_conv48_stem_fn;
Pred1 stem_ok_fn, conv48_ok_fn, pixgemm_ok_fn;
Pred2 conv48_stem_ok_fn;
LaunchMlp launch_mlp_fn;

// (GemmParams from a case, accesses_ok, the operands, the mutations and run_gemm_case: check_common.h, shared with cunet_check.cpp)
bool supported(const std::string& launcher, const GemmParams& p) {
    return launcher == "stem" ? stem_ok_fn(p) : launcher == "conv48" ? conv48_ok_fn(p) : launcher == "pixgemm" ? pixgemm_ok_fn(p) : launcher == "gemm";
}
Launch1 launcher_fn(const std::string& launcher) {
    return launcher == "stem" ? launch_stem_fn : launcher == "conv48" ? launch_conv48_fn : launcher == "pixgemm" ? launch_pixgemm_fn : launch_gemm_fn;
}
const GemmBackend kBackend = {supported, launcher_fn, nullptr, nullptr};

// stem -> conv48: the two launches (.mid, .y), then conv48_kernel<true> on the same parameters (.fy); the fused launch must not touch the map between them
void run_pair(const Case& c) {
    GemmParams ps = numbers(c, "s_"), p = numbers(c, "");
    Operands ops;
    load_operands(c, "s_", ps, ops, "stem", "none");
    load_operands(c, "", p, ops, "pair", "none");
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
    run_no_launch(c, through_gemm ? launch_gemm_fn : nullptr, [](const Case& c, const GemmParams& p, const StandIns& s) {
        if (c.str("pred") != "conv48_stem") return supported(c.str("pred"), p);
        GemmParams ps = numbers(c, "s_");
        ps.a.p = s.dummy.p; ps.wt = s.dummy.p; ps.bias = (const float*)s.dummy.p; ps.out.p = p.a.p;
        return conv48_stem_ok_fn(p, ps);
    });
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
            if (kind == "gemm") run_gemm_case(c, kBackend);
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
