// Drives cunet's convolution, gate and head kernels in a built libw2x.so - w2x::launch_conv3 (conv3_kernel<false, 0> / <true, 0>), launch_conv3_stem (<false, 1>),
// launch_conv3_up (<false, 2>), launch_conv3h (conv3h_walk_kernel, conv3h_kernel), launch_pixgemm (merge_slab_kernel, pixgemm_kernel at K = 64 / 128), launch_gemm
// (its a_scale / res_scale / pool_out branches), launch_stem, launch_se, launch_scale, conv3_tiles and the *_supported predicates, found by their mangled names, so the
// code objects checked are the shipped ones - on cases that tests/test_gpu_cunet_kernels.py writes:
//
//     cunet_check <path of libw2x.so> <case dir>     runs <case dir>/cases.json in order, writes <case dir>/<name>.y (.gy: the same parameters on launch_gemm, .pool /
//                                                    .gpool: pooling partials, .mid / .fy: the first launch's map and the fused launch of a pair, .gates: launch_se),
//                                                    one CASE line per case
//
// A later case may name a file an earlier one wrote (the gate chain: a producer's .y and .pool, launch_se's .gates).
// Safety rules of this harness (no launch is made to see what happens): those of conv_check.cpp - a specialised kernel is launched only after its own predicate took
// exactly the parameters it is handed, every launch is first walked by accesses_ok() (check_common.h) against the buffers allocated for it, the first HIP error ends the
// process, "predicate" / "se_refuse" cases launch nothing that passes a check.  The fused launches read what their two launches read: the stem's input and the
// projection's rows and skip pixels are walked for the first launch's parameters, whose extents conv3_stem_supported / conv3_up_supported tie to the convolution's.
// Weight copies come from fragorder.h itself: frag_conv3b for wt_perm, frag_major for wt_frag.
// A case's "switch" (no_conv3h_walk for the <PIX, true> cases) is set through w2x::set_switch in this process for the length of the case: launch_conv3h reads switches()
// on every launch (k_conv3h.hip), so the "_tile" cases do run conv3h_kernel and not the walk again.
// "rows" cases ask pixgemm_rows_per_workgroup what the test assumed when it chose rows around a workgroup's edge (err = 0: as assumed).
#include "check_common.h"

namespace {

typedef hipError_t (*LaunchSe)(const SeParams&, hipStream_t);
typedef int (*Tiles)(const GemmParams&);
typedef bool (*SetSwitch)(const char*, long);
Launch1 launch_gemm_fn, launch_stem_fn, launch_conv3_fn, launch_conv3h_fn, launch_pixgemm_fn;
Launch2 launch_conv3_stem_fn, launch_conv3_up_fn;
Pred1 stem_ok_fn, conv3_ok_fn, conv3h_ok_fn, pixgemm_ok_fn;
Pred2 conv3_stem_ok_fn, conv3_up_ok_fn;
LaunchSe launch_se_fn;
LaunchScale launch_scale_fn;
Tiles conv3_tiles_fn, pixgemm_rows_fn;
SetSwitch set_switch_fn;

bool supported(const std::string& L, const GemmParams& p) {
    return L == "stem" ? stem_ok_fn(p) : L == "conv3" ? conv3_ok_fn(p) : L == "conv3h" ? conv3h_ok_fn(p) : L == "pixgemm" ? pixgemm_ok_fn(p) : L == "gemm";
}
Launch1 launcher_fn(const std::string& L) {
    return L == "stem" ? launch_stem_fn : L == "conv3" ? launch_conv3_fn : L == "conv3h" ? launch_conv3h_fn : L == "pixgemm" ? launch_pixgemm_fn : launch_gemm_fn;
}
int pool_tiles(const std::string& L, const GemmParams& p) {      // pooling partials per image: conv3_kernel one per pixel tile, gemm_kernel one per kGemmBM rows
    return L == "conv3" ? conv3_tiles_fn(p) : L == "gemm" ? (p.Mrows + kGemmBM - 1) / kGemmBM : 0;
}
GemmBackend backend() { return GemmBackend{supported, launcher_fn, pool_tiles, launch_scale_fn}; }

// a debug switch for the length of a case ("switch": its name in switches.h)
struct SwitchOn {
    std::string name;
    explicit SwitchOn(const Case& c) : name(c.str("switch")) { if (!name.empty() && !set_switch_fn(name.c_str(), 1)) throw std::runtime_error("unknown switch " + name); }
    ~SwitchOn() { if (!name.empty()) set_switch_fn(name.c_str(), 0); }
};

// first launch ("s_" keys: launch_stem, or launch_pixgemm with its gate and skip map) -> launch_conv3: the two launches (.mid, .y), then the fused launch on the same
// parameters (.fy), which must not touch the map between them.  "fuse": stem | up.  "s_mutate" / "mutate" change what BOTH ways are handed.
void run_pair(const Case& c) {
    const bool up = c.str("fuse") == "up";
    GemmParams ps = numbers(c, "s_"), p = numbers(c, "");
    Operands ops;
    load_operands(c, "s_", ps, ops, up ? "pixgemm" : "stem", "s_mutate");
    load_operands(c, "", p, ops, "conv3", "mutate");
    const Extents es = extents_of(ps), e = extents_of(p);
    Result o;
    std::string why;
    Guarded mid(es.out * 2), y(e.out * 2), mid2(es.out * 2), fy(e.out * 2);
    ps.out.p = mid.p(); p.a.p = mid.p(); p.out.p = y.p();
    GemmParams ps2 = ps, p2 = p;
    ps2.out.p = mid2.p(); p2.a.p = mid2.p(); p2.out.p = fy.p();
    if (es.out != e.a) throw std::runtime_error("pair: the first launch's output is not the convolution's input map");
    const Launch1 first = up ? launch_pixgemm_fn : launch_stem_fn;
    const bool ok = (up ? pixgemm_ok_fn(ps) : stem_ok_fn(ps)) && conv3_ok_fn(p) && (up ? conv3_up_ok_fn(p2, ps2) : conv3_stem_ok_fn(p2, ps2));
    if (!ok) { o.err = kErrUnsupported; report(c, o); return; }
    if (!accesses_ok(ps, es, ops.table, why) || !accesses_ok(p, e, ops.table, why)) { fprintf(stderr, "%s: not launched: %s\n", c.str("name").c_str(), why.c_str()); o.err = kErrBounds; report(c, o); return; }
    Outcome r = run_twice([&] { hipError_t s = first(ps, 0); return s != hipSuccess ? s : launch_conv3_fn(p, 0); }, {&mid, &y});
    o.err = r.err; o.det = r.det; o.guards = r.guards; o.ms = r.ms;
    if (!r.err) {
        r = run_twice([&] { return up ? launch_conv3_up_fn(p2, ps2, 0) : launch_conv3_stem_fn(p2, ps2, 0); }, {&fy});
        o.gerr = r.err; o.det = o.det && r.det; o.guards = o.guards && r.guards && mid2.guards_intact();
        o.untouched = mid2.untouched();
    }
    if (!o.err && !o.gerr && p.B > 1) {                  // the first image alone through the fused launch
        Guarded f1(e.out / p.B * 2), m1(es.out / p.B * 2);
        GemmParams pa = p2, pb = ps2;
        pa.B = pb.B = 1; pa.out.p = f1.p(); pa.a.p = m1.p(); pb.out.p = m1.p();
        if (up ? conv3_up_ok_fn(pa, pb) : conv3_stem_ok_fn(pa, pb)) {
            HIPCHECK(up ? launch_conv3_up_fn(pa, pb, 0) : launch_conv3_stem_fn(pa, pb, 0));
            HIPCHECK(hipDeviceSynchronize());
            std::vector<unsigned char> full = fy.rows<unsigned char>(nullptr, 1), one = f1.rows<unsigned char>(nullptr, 1);
            full.resize(one.size());
            o.first = full == one && f1.guards_intact();
        } else o.first = false;
    }
    if (!o.err && !o.gerr) {
        save(c.str("name") + ".mid", mid.rows<uint16_t>(nullptr, 1));
        save(c.str("name") + ".y", y.rows<uint16_t>(nullptr, 1));
        save(c.str("name") + ".fy", fy.rows<uint16_t>(nullptr, 1));
    }
    report(c, o);
}

SeParams se_numbers(const Case& c) {
    SeParams p;
    p.B = (int)c.i("B"); p.C = (int)c.i("C"); p.Cs = (int)c.i("Cs"); p.Cmid = (int)c.i("Cmid"); p.inv_count = (float)c.num("inv_count", 0);
    p.nblocks = (int)c.i("nblocks"); p.Mrows = (int)c.i("Mrows");
    return p;
}

// launch_se on the partials of <pool> ([B][nblocks][Cs] fp32: a file of the test's, or one an earlier case wrote) -> .gates [B][Cs]
void run_se(const Case& c) {
    SeParams p = se_numbers(c);
    if (p.B <= 0 || p.C <= 0 || p.C > 256 || p.Cs < p.C || p.Cs % 8 || p.Cmid <= 0 || p.Cmid > 256 || p.nblocks <= 0) throw std::runtime_error("se: sizes (a refusal is an se_refuse case)");
    Dev<float> pool(load<float>(c.str("pool"), (size_t)p.B * p.nblocks * p.Cs)), w1(load<float>(c.str("w1"), (size_t)p.Cmid * p.C)), b1(load<float>(c.str("b1"), p.Cmid)),
        w2(load<float>(c.str("w2"), (size_t)p.C * p.Cmid)), b2(load<float>(c.str("b2"), p.C));
    Guarded gates((size_t)p.B * p.Cs * 4);
    p.pool = (const float*)pool.p; p.scale = (float*)gates.p(); p.w1 = (const float*)w1.p; p.b1 = (const float*)b1.p; p.w2 = (const float*)w2.p; p.b2 = (const float*)b2.p;
    Result o;
    const Outcome r = run_twice([&] { return launch_se_fn(p, 0); }, {&gates});
    o.err = r.err; o.det = r.det; o.guards = r.guards; o.ms = r.ms;
    if (!r.err) save(c.str("name") + ".gates", gates.rows<float>(nullptr, 1));
    report(c, o);
}

// launch_se must answer hipErrorInvalidValue from the sizes alone: stand-in pointers, the gates untouched
void run_se_refuse(const Case& c) {
    SeParams p = se_numbers(c);
    Dev<float> dummy(std::vector<float>(4096, 0.f));
    Guarded gates(4096);
    p.pool = p.w1 = p.b1 = p.w2 = p.b2 = (const float*)dummy.p; p.scale = (float*)gates.p();
    if (p.B > 0 && p.C > 0 && p.C <= 256 && p.Cmid > 0 && p.nblocks > 0 && p.Cs >= p.C) throw std::runtime_error("se_refuse: these sizes would launch");
    Result o;
    o.err = (int)launch_se_fn(p, 0);
    HIPCHECK(hipDeviceSynchronize());
    o.untouched = gates.untouched();
    report(c, o);
}

void run_predicate(const Case& c) {
    run_no_launch(c, nullptr, [](const Case& c, GemmParams p, const StandIns& s) {
        const std::string pred = c.str("pred");
        if (c.i("gated")) p.a_scale = (const float*)s.dummy.p;
        if (c.i("pooled")) p.pool_out = (float*)s.dummy.p;
        if (pred != "conv3_stem" && pred != "conv3_up") return supported(pred, p);
        GemmParams ps = numbers(c, "s_");
        s.point(c, ps, false);
        ps.out.p = p.a.p;
        if (c.i("s_gated")) ps.a_scale = (const float*)s.dummy.p;
        return pred == "conv3_up" ? conv3_up_ok_fn(p, ps) : conv3_stem_ok_fn(p, ps);
    });
}

// pixgemm_rows_per_workgroup of the case's numbers against "expect" (nothing is launched)
void run_rows(const Case& c) {
    const GemmParams p = numbers(c, "");
    Result o;
    const int got = pixgemm_rows_fn(p);
    o.err = got == (int)c.i("expect") ? 0 : 1;
    if (o.err) fprintf(stderr, "%s: a workgroup owns %d rows, the test assumed %ld\n", c.str("name").c_str(), got, c.i("expect"));
    report(c, o);
}

}  // namespace

int main(int argc, char** argv) {
    try {
        if (argc != 3) { fprintf(stderr, "usage: cunet_check <libw2x.so> <case dir>\n"); return 2; }
        dir = argv[2];
        void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
        if (!lib) { fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
        launch_gemm_fn = (Launch1)sym(lib, "_ZN3w2x11launch_gemmERKNS_10GemmParamsEP12ihipStream_t");
        launch_stem_fn = (Launch1)sym(lib, "_ZN3w2x11launch_stemERKNS_10GemmParamsEP12ihipStream_t");
        launch_conv3_fn = (Launch1)sym(lib, "_ZN3w2x12launch_conv3ERKNS_10GemmParamsEP12ihipStream_t");
        launch_conv3h_fn = (Launch1)sym(lib, "_ZN3w2x13launch_conv3hERKNS_10GemmParamsEP12ihipStream_t");
        launch_pixgemm_fn = (Launch1)sym(lib, "_ZN3w2x14launch_pixgemmERKNS_10GemmParamsEP12ihipStream_t");
        launch_conv3_stem_fn = (Launch2)sym(lib, "_ZN3w2x17launch_conv3_stemERKNS_10GemmParamsES2_P12ihipStream_t");
        launch_conv3_up_fn = (Launch2)sym(lib, "_ZN3w2x15launch_conv3_upERKNS_10GemmParamsES2_P12ihipStream_t");
        stem_ok_fn = (Pred1)sym(lib, "_ZN3w2x14stem_supportedERKNS_10GemmParamsE");
        conv3_ok_fn = (Pred1)sym(lib, "_ZN3w2x15conv3_supportedERKNS_10GemmParamsE");
        conv3h_ok_fn = (Pred1)sym(lib, "_ZN3w2x16conv3h_supportedERKNS_10GemmParamsE");
        pixgemm_ok_fn = (Pred1)sym(lib, "_ZN3w2x17pixgemm_supportedERKNS_10GemmParamsE");
        conv3_stem_ok_fn = (Pred2)sym(lib, "_ZN3w2x20conv3_stem_supportedERKNS_10GemmParamsES2_");
        conv3_up_ok_fn = (Pred2)sym(lib, "_ZN3w2x18conv3_up_supportedERKNS_10GemmParamsES2_");
        launch_se_fn = (LaunchSe)sym(lib, "_ZN3w2x9launch_seERKNS_8SeParamsEP12ihipStream_t");
        launch_scale_fn = (LaunchScale)sym(lib, "_ZN3w2x12launch_scaleEPvPKfiiibP12ihipStream_t");
        conv3_tiles_fn = (Tiles)sym(lib, "_ZN3w2x11conv3_tilesERKNS_10GemmParamsE");
        pixgemm_rows_fn = (Tiles)sym(lib, "_ZN3w2x26pixgemm_rows_per_workgroupERKNS_10GemmParamsE");
        set_switch_fn = (SetSwitch)sym(lib, "_ZN3w2x10set_switchEPKcl");
        std::ifstream f(dir + "/cases.json");
        const std::string t((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const GemmBackend be = backend();
        for (const Case& c : parse_cases(t)) {
            printf("RUN %s\n", c.str("name").c_str());   // names the case if it never reports
            fflush(stdout);
            const std::string kind = c.str("kind");
            SwitchOn sw(c);
            if (kind == "gemm") run_gemm_case(c, be);
            else if (kind == "pair") run_pair(c);
            else if (kind == "se") run_se(c);
            else if (kind == "se_refuse") run_se_refuse(c);
            else if (kind == "predicate") run_predicate(c);
            else if (kind == "rows") run_rows(c);
            else throw std::runtime_error("unknown case kind " + kind);
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "cunet_check: %s\n", e.what());
        return 1;
    }
    return 0;
}
