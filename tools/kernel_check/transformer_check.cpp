// Drives the fused transformer kernels of a built libw2x.so - w2x::launch_swin_attn / w2x::launch_mlp, the dispatchers of k_dispatch.hip, so
// the code objects checked are the shipped ones with their shipped build flags - on cases that tests/test_gpu_transformer_kernels.py writes:
//
//     transformer_check <path of libw2x.so> <case dir>      runs <case dir>/cases.json, writes <case dir>/<name>.y / .stats / .head, one CASE line per case
//     transformer_check --gen-only <case dir>               writes <case dir>/gen.bin: the large-input formula at the rows of <case dir>/gen.rows (no HIP call)
//     transformer_check --pack-bias <dir> <nmask * heads>   writes <dir>/bias32.bin = swin_bias32 of <dir>/bias.bin (no HIP call)
//
// Weights are laid out exactly as engine.cpp does it (fragorder.h frag_major / frag_w2 / frag32_major / frag32_w2, swin_bias32 from the logical
// [nmask * heads][36][36] fp16 table).  Every output lies between guard bands filled with a sentinel; every case runs twice (bit-identical or not).
// Inputs of 4 GB and more (the launchers' run splitting) are not read from files: both sides compute them with gen_x16() of check_common.h
// (tests/kernel_ref.py gen_rows), and only the rows listed in <name>.rows / .hrows come back.
// A mutation ("mutate") changes one value handed to the kernel - the reference keeps the true one - to show that the test's bounds see it.
#include "check_common.h"

namespace {

typedef hipError_t (*LaunchAttn)(const SwinAttnParams&, hipStream_t);
typedef hipError_t (*LaunchMlp)(const MlpParams&, hipStream_t);
LaunchAttn launch_attn_fn = nullptr;
LaunchMlp launch_mlp_fn = nullptr;

void report(const Case& c, const Outcome& o) {
    printf("CASE %s err=%d det=%d guards=%d y_untouched=%d ms=%.3f\n", c.str("name").c_str(), o.err, (int)o.det, (int)o.guards, (int)o.y_untouched, o.ms);
    fflush(stdout);
}

void run_attn(const Case& c) {
    const int C = (int)c.i("C"), B = (int)c.i("B"), H = (int)c.i("H"), W = (int)c.i("W"), nmask = (int)c.i("nmask", 1);
    const int heads = 6, hd = C / heads, nwin = H * W / 36;
    const std::string mut = c.str("mutate"), w = c.str("w");
    const size_t pix = (size_t)B * H * W;
    const std::vector<uint16_t> wqkv = load<uint16_t>(w + ".wqkv", (size_t)3 * C * C), wproj = load<uint16_t>(w + ".wproj", (size_t)C * C);
    const std::vector<float> bqkv = load<float>(w + ".bqkv", 3 * C), bproj = load<float>(w + ".bproj", C);
    const std::vector<uint16_t> bias16 = load<uint16_t>(c.str("bias"), (size_t)nmask * heads * 36 * 36);
    std::vector<int> maskid = load<int>(c.str("maskid"), nwin);
    std::vector<int> table;
    if (c.i("ry") < 0) table = load<int>(c.str("table"), (size_t)H * W);
    std::vector<float> bias32 = swin_bias32(bias16.data(), nmask * heads, 36);
    // mutations: what the kernel is handed, not what the reference sees
    const int mc = nmask - 1;                              // the last mask class
    const size_t unit = (size_t)mc * heads * 3 * 576;      // its head 0
    if (mut == "bias_lane_swap") std::swap(bias32[unit + 5 * 4], bias32[unit + 21 * 4]);           // (query 5, key 0) <-> (query 5, key 4)
    if (mut.rfind("bias_delta=", 0) == 0) bias32[unit + 5 * 4] += (float)atof(mut.c_str() + 11);   // (query 5, key 0) of class mc, head 0 (log2 units)
    if (mut == "maskid") maskid[nwin - 1] = (maskid[nwin - 1] + 1) % nmask;
    if (mut == "table_swap") std::swap(table[0], table[1]);

    Dev<uint16_t> fq(frag_major(wqkv.data(), 3 * C, C)), fp(frag_major(wproj.data(), C, C)), dq(wqkv), dp(wproj);
    Dev<float> dbq(bqkv), dbp(bproj), db32(bias32);
    Dev<int> dm(maskid), dt(table.empty() ? std::vector<int>(1, 0) : table);
    void* x = upload_rows(c, pix, C);
    Guarded y(pix * C * 2);
    std::unique_ptr<Guarded> st(c.i("stats") ? new Guarded(pix * 2 * 4) : nullptr);
    SwinAttnParams p;
    p.x = x; p.y = y.p(); p.table = table.empty() ? nullptr : (const int*)dt.p; p.H = H; p.W = W; p.ry = (int)c.i("ry"); p.rx = (int)c.i("rx");
    p.B = B; p.nwin = nwin; p.C = C; p.hd = hd;
    p.wqkv = dq.p; p.bqkv = (const float*)dbq.p; p.scale = (float)c.num("scale", 1.0 / std::sqrt((double)hd));
    p.bias32 = (const float*)db32.p; p.maskid = (const int*)dm.p; p.wproj = dp.p; p.bproj = (const float*)dbp.p;
    p.eps = (float)c.num("eps", 1e-5); p.stats_out = st ? (float*)st->p() : nullptr; p.eps_out = (float)c.num("eps_out", 1e-5);
    if (mut == "eps_out") p.eps_out = 1e-4f;
    p.wqkv_frag = fq.p; p.wproj_frag = fp.p;
    std::vector<const Guarded*> outs = {&y};
    if (st) outs.push_back(st.get());
    Outcome o = run_twice([&] { return launch_attn_fn(p, 0); }, outs);
    if (!o.err) {
        std::vector<long> idx;
        if (c.i("gen")) { const std::vector<long> r = load<long>(c.str("rows"), (size_t)c.i("nrows")); idx = r; }
        const std::vector<long>* ip = c.i("gen") ? &idx : nullptr;
        save(c.str("name") + ".y", y.rows<uint16_t>(ip, C));
        if (st) save(c.str("name") + ".stats", st->rows<float>(ip, 2));
    }
    HIPCHECK(hipFree(x));
    report(c, o);
}

void run_mlp(const Case& c) {
    const int C = (int)c.i("C");
    const long M = c.i("M");
    const std::string mut = c.str("mutate"), w = c.str("w");
    const bool head = c.i("head") != 0;
    const std::vector<uint16_t> w1 = load<uint16_t>(w + ".w1", (size_t)2 * C * C), w2 = load<uint16_t>(w + ".w2", (size_t)2 * C * C);
    const std::vector<float> b1 = load<float>(w + ".b1", 2 * C), b2 = load<float>(w + ".b2", C);
    const bool f32 = mlp_frag32(C);
    std::vector<uint16_t> f1 = f32 ? frag32_major(w1.data(), 2 * C, C) : frag_major(w1.data(), 2 * C, C);
    std::vector<uint16_t> f2 = f32 ? frag32_w2(w2.data(), C) : frag_w2(w2.data(), C);
    if (mut == "w2_swap") std::swap(f2[0], f2[1]);     // chunk 0, n-tile 0, lane 0: two hidden units of output channel 0 trade weights
    Dev<uint16_t> d1(w1), d2(w2), df1(f1), df2(f2);
    Dev<float> db1(b1), db2(b2);
    void* x = upload_rows(c, (size_t)M, C);
    Guarded y((size_t)M * C * 2);
    std::unique_ptr<Guarded> st(c.i("stats") ? new Guarded((size_t)M * 2 * 4) : nullptr);
    MlpParams p;
    p.x = x; p.y = y.p(); p.M = M; p.C = C;
    p.w1 = d1.p; p.b1 = (const float*)db1.p; p.w2 = d2.p; p.b2 = (const float*)db2.p;
    p.eps = (float)c.num("eps", 1e-5); p.stats_out = st ? (float*)st->p() : nullptr; p.eps_out = (float)c.num("eps_out", 1e-5);
    if (mut == "eps_out") p.eps_out = 1e-4f;
    p.w1_frag = df1.p; p.w2_frag = df2.p; p.frag32 = f32;
    std::unique_ptr<Dev<uint16_t>> tw;
    std::unique_ptr<Dev<float>> tb;
    std::unique_ptr<Guarded> hout;
    const int Hs = (int)c.i("ti_Hs"), Ws = (int)c.i("ti_Ws"), B = (int)c.i("B", 1);
    if (head) {
        const std::vector<uint16_t> tiw = load<uint16_t>(w + ".tiw", (size_t)64 * C);
        tw.reset(new Dev<uint16_t>(frag_major(tiw.data(), 64, C)));
        tb.reset(new Dev<float>(load<float>(w + ".tib", 64)));
        hout.reset(new Guarded((size_t)B * Hs * Ws * 4 * 2));
        p.ti_w = tw->p; p.ti_b = (const float*)tb->p; p.ti_out = hout->p(); p.ti_Hs = Hs; p.ti_Ws = Ws;
        p.ti_Mrows = (int)c.i("ti_Mrows"); p.ti_aW = (int)c.i("ti_aW");
        p.ti_clip = (int)c.i("ti_clip"); p.ti_lo = (float)c.num("ti_lo", 0); p.ti_hi = (float)c.num("ti_hi", 1);
    }
    std::vector<const Guarded*> outs = {&y};
    if (st) outs.push_back(st.get());
    if (hout) outs.push_back(hout.get());
    Outcome o = run_twice([&] { return launch_mlp_fn(p, 0); }, outs);
    if (!o.err) {
        std::vector<long> idx, hidx;
        if (c.i("gen")) { idx = load<long>(c.str("rows"), (size_t)c.i("nrows")); if (head) hidx = load<long>(c.str("hrows"), (size_t)c.i("nhrows")); }
        const bool gen = c.i("gen") != 0;
        if (head) {
            save(c.str("name") + ".head", hout->rows<uint16_t>(gen ? &hidx : nullptr, 4));
            if (!gen) o.y_untouched = y.untouched();
            else { const std::vector<uint16_t> s = y.rows<uint16_t>(&idx, C); for (uint16_t v : s) o.y_untouched = o.y_untouched && v == 0xA5A5; }
        } else save(c.str("name") + ".y", y.rows<uint16_t>(gen ? &idx : nullptr, C));
        if (st) save(c.str("name") + ".stats", st->rows<float>(gen ? &idx : nullptr, 2));
    }
    HIPCHECK(hipFree(x));
    report(c, o);
}

// parameters the dispatchers refuse: they must return hipErrorInvalidValue from the sizes alone, and write nothing
void run_refuse(const Case& c) {
    const std::string what = c.str("what");
    std::vector<uint16_t> w((size_t)3 * 192 * 192, 0);
    std::vector<float> b(3 * 192, 0.f);
    Dev<uint16_t> dw(w), dx(w);
    Dev<float> db(b), dbias(std::vector<float>((size_t)6 * 3 * 576, 0.f));
    Dev<int> dm(std::vector<int>(64, 0));
    Guarded y(64 * 192 * 2);
    Outcome o;
    if (what.rfind("attn", 0) == 0) {
        SwinAttnParams p;
        p.x = dx.p; p.y = y.p(); p.H = 6; p.W = 6; p.ry = 0; p.rx = 0; p.B = 1; p.nwin = 1; p.C = 96; p.hd = 16;
        p.wqkv = dw.p; p.bqkv = (const float*)db.p; p.bias32 = (const float*)dbias.p; p.maskid = (const int*)dm.p; p.wproj = dw.p; p.bproj = (const float*)db.p;
        p.wqkv_frag = dw.p; p.wproj_frag = dw.p;
        if (what == "attn_C128") { p.C = 128; p.hd = 32; }
        if (what == "attn_hd32_at_C96") p.hd = 32;
        if (what == "attn_no_frag") p.wqkv_frag = nullptr;
        if (what == "attn_image_beyond_4GB") { p.C = 192; p.hd = 32; p.H = p.W = 3348; p.nwin = 558 * 558; }   // 311 364 windows x 36 x 384 B = 4.304e9 B per image
        if (what == "attn_no_windows") p.nwin = 0;
        o.err = (int)launch_attn_fn(p, 0);
    } else {
        MlpParams p;
        p.x = dx.p; p.y = y.p(); p.M = 64; p.C = 96;
        p.w1 = dw.p; p.b1 = (const float*)db.p; p.w2 = dw.p; p.b2 = (const float*)db.p; p.w1_frag = dw.p; p.w2_frag = dw.p; p.frag32 = true;
        if (what == "mlp_C128") p.C = 128;
        if (what == "mlp_C64") p.C = 64;
        if (what == "mlp_no_frag") p.w2_frag = nullptr;
        if (what == "mlp96_head_ragged_image" || what == "mlp96_head_with_stats") {   // the folded head needs whole 32-row tiles per image and no statistics
            p.ti_w = dw.p; p.ti_b = (const float*)db.p; p.ti_out = dx.p; p.ti_Hs = 8; p.ti_Ws = 128; p.ti_Mrows = 64; p.ti_aW = 32;
            if (what == "mlp96_head_ragged_image") p.ti_Mrows = 48;
            else p.stats_out = (float*)dx.p;
        }
        o.err = (int)launch_mlp_fn(p, 0);
    }
    HIPCHECK(hipDeviceSynchronize());
    o.y_untouched = y.untouched();
    report(c, o);
}

}  // namespace

int main(int argc, char** argv) {
    try {
        if (argc == 3 && !strcmp(argv[1], "--gen-only")) {
            dir = argv[2];
            std::ifstream f(dir + "/gen.json");
            const std::string t((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            const Case c = parse_cases("[" + t + "]")[0];
            const int C = (int)c.i("C");
            const std::vector<long> rows = load<long>("gen.rows", (size_t)c.i("nrows"));
            std::vector<uint16_t> out(rows.size() * C);
            for (size_t k = 0; k < rows.size(); ++k)
                for (int ch = 0; ch < C; ++ch) out[k * C + ch] = gen_x16((uint64_t)rows[k], ch, C, (uint64_t)c.i("seed"));
            save("gen.bin", out);
            printf("gen-only: %zu rows of %d\n", rows.size(), C);
            return 0;
        }
        if (argc == 4 && !strcmp(argv[1], "--pack-bias")) {   // the packing alone (no HIP call): <dir>/bias.bin fp16 [nmh][36][36] -> <dir>/bias32.bin
            dir = argv[2];
            const int nmh = atoi(argv[3]);
            save("bias32.bin", swin_bias32(load<uint16_t>("bias.bin", (size_t)nmh * 36 * 36).data(), nmh, 36));
            return 0;
        }
        if (argc != 3) { fprintf(stderr, "usage: transformer_check <libw2x.so> <case dir> | --gen-only <case dir>\n"); return 2; }
        dir = argv[2];
        void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
        if (!lib) { fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
        launch_attn_fn = (LaunchAttn)dlsym(lib, "_ZN3w2x16launch_swin_attnERKNS_14SwinAttnParamsEP12ihipStream_t");
        launch_mlp_fn = (LaunchMlp)dlsym(lib, "_ZN3w2x10launch_mlpERKNS_9MlpParamsEP12ihipStream_t");
        if (!launch_attn_fn || !launch_mlp_fn) { fprintf(stderr, "the library does not export w2x::launch_swin_attn / w2x::launch_mlp\n"); return 2; }
        std::ifstream f(dir + "/cases.json");
        const std::string t((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        for (const Case& c : parse_cases(t)) {
            printf("RUN %s\n", c.str("name").c_str());   // names the case if it never reports
            fflush(stdout);
            const std::string kind = c.str("kind");
            if (kind == "attn") run_attn(c);
            else if (kind == "mlp") run_mlp(c);
            else if (kind == "refuse") run_refuse(c);
            else throw std::runtime_error("unknown case kind " + kind);
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "transformer_check: %s\n", e.what());
        return 1;
    }
    return 0;
}
