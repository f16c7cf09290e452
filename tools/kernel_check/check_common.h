// What the kernel harnesses of this directory share (transformer_check.cpp, conv_check.cpp, cunet_check.cpp): the large-input formula, the flat JSON reader of
// cases.json, file helpers, guarded device buffers and the run-twice driver; for the two GemmParams harnesses also the parameters of a case, the address walk
// accesses_ok(), the operands with their mutations, and the one-launch case runner.  Host code only; each harness is one translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "common.h"
#include "fragorder.h"
#include "kernels.h"

using namespace w2x;

namespace {

// ---- the large-input formula (tests/kernel_ref.py gen_rows): fp16 k / 256 - 2, k in [0, 1024).  Channels 0..2 hold the row index in three
// 10-bit digits (every row of a 4 GB pass distinct), the others a splitmix64 hash of (row, channel, seed).
uint16_t gen_x16(uint64_t row, int c, int C, uint64_t seed) {
    uint64_t k;
    if (c < 3) k = (row >> (10 * c)) & 1023u;
    else {
        uint64_t z = (row * (uint64_t)C + (uint64_t)c) + seed * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        k = z >> 54;
    }
    return f32_to_f16((float)k / 256.f - 2.f);
}

// ---- a flat JSON reader: a list of objects whose values are numbers or strings (what the test writes)
struct Case {
    std::map<std::string, std::string> s;
    std::map<std::string, double> n;
    double num(const std::string& k, double d) const { auto it = n.find(k); return it == n.end() ? d : it->second; }
    long i(const std::string& k, long d = 0) const { return (long)num(k, (double)d); }
    std::string str(const std::string& k, const std::string& d = "") const { auto it = s.find(k); return it == s.end() ? d : it->second; }
};

std::vector<Case> parse_cases(const std::string& text) {
    std::vector<Case> out;
    size_t p = 0;
    auto ws = [&] { while (p < text.size() && isspace((unsigned char)text[p])) ++p; };
    auto expect = [&](char c) { ws(); if (p >= text.size() || text[p] != c) throw std::runtime_error(std::string("cases.json: expected ") + c); ++p; };
    auto string = [&] {
        expect('"');
        std::string r;
        while (p < text.size() && text[p] != '"') { if (text[p] == '\\') ++p; r += text[p++]; }
        ++p;
        return r;
    };
    expect('[');
    ws();
    if (text[p] == ']') return out;
    for (;;) {
        Case c;
        expect('{');
        ws();
        if (text[p] != '}')
            for (;;) {
                const std::string k = string();
                expect(':');
                ws();
                if (text[p] == '"') c.s[k] = string();
                else { char* e = nullptr; c.n[k] = strtod(text.c_str() + p, &e); p = e - text.c_str(); }
                ws();
                if (text[p] == ',') { ++p; continue; }
                break;
            }
        expect('}');
        out.push_back(c);
        ws();
        if (text[p] == ',') { ++p; continue; }
        expect(']');
        return out;
    }
}

std::string dir;

template <class T> std::vector<T> load(const std::string& name, size_t count) {
    std::ifstream f(dir + "/" + name, std::ios::binary);
    std::vector<T> v(count);
    if (!f.read((char*)v.data(), (std::streamsize)(count * sizeof(T)))) throw std::runtime_error("cannot read " + name + " (" + std::to_string(count) + " elements)");
    return v;
}
template <class T> void save(const std::string& name, const std::vector<T>& v) {
    std::ofstream f(dir + "/" + name, std::ios::binary);
    f.write((const char*)v.data(), (std::streamsize)(v.size() * sizeof(T)));
    if (!f) throw std::runtime_error("cannot write " + name);
}

#define HIPCHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); fflush(stdout); exit(3); } } while (0)

constexpr size_t kGuard = 4096;
constexpr unsigned char kSentinel = 0xA5;

// device buffer of `bytes` between two guard bands of the sentinel (the payload is filled with it too)
struct Guarded {
    unsigned char* base = nullptr; size_t bytes = 0;
    explicit Guarded(size_t b) : bytes(b) {
        HIPCHECK(hipMalloc(&base, b + 2 * kGuard));
        HIPCHECK(hipMemset(base, kSentinel, b + 2 * kGuard));
    }
    ~Guarded() { if (base) (void)hipFree(base); }
    Guarded(const Guarded&) = delete;
    void* p() const { return base + kGuard; }
    bool guards_intact() const {
        std::vector<unsigned char> g(kGuard);
        for (int side = 0; side < 2; ++side) {
            HIPCHECK(hipMemcpy(g.data(), base + (side ? kGuard + bytes : 0), kGuard, hipMemcpyDeviceToHost));
            for (unsigned char c : g) if (c != kSentinel) return false;
        }
        return true;
    }
    bool untouched() const {   // the payload too
        std::vector<unsigned char> g(bytes);
        HIPCHECK(hipMemcpy(g.data(), p(), bytes, hipMemcpyDeviceToHost));
        for (unsigned char c : g) if (c != kSentinel) return false;
        return guards_intact();
    }
    template <class T> std::vector<T> rows(const std::vector<long>* idx, size_t row_elems) const {   // all rows, or the listed ones
        std::vector<T> out;
        if (!idx) { out.resize(bytes / sizeof(T)); HIPCHECK(hipMemcpy(out.data(), p(), bytes, hipMemcpyDeviceToHost)); return out; }
        out.resize(idx->size() * row_elems);
        for (size_t k = 0; k < idx->size(); ++k)
            HIPCHECK(hipMemcpy(&out[k * row_elems], (const T*)p() + (size_t)(*idx)[k] * row_elems, row_elems * sizeof(T), hipMemcpyDeviceToHost));
        return out;
    }
};

// plain device copy with the engine's 256 bytes of slack behind it
template <class T> struct Dev {
    void* p = nullptr;
    explicit Dev(const std::vector<T>& v) {
        HIPCHECK(hipMalloc(&p, v.size() * sizeof(T) + 256));
        HIPCHECK(hipMemset(p, 0, v.size() * sizeof(T) + 256));
        HIPCHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    }
    ~Dev() { if (p) (void)hipFree(p); }
    Dev(const Dev&) = delete;
};

// the rows of a case: from <x> (small cases) or the formula (gen = 1), uploaded into a buffer of exactly rows * C halves
void* upload_rows(const Case& c, size_t rows, int C) {
    void* d = nullptr;
    const size_t n = rows * (size_t)C;
    HIPCHECK(hipMalloc(&d, n * 2));
    if (!c.i("gen")) {
        const std::vector<uint16_t> x = load<uint16_t>(c.str("x"), n);
        HIPCHECK(hipMemcpy(d, x.data(), n * 2, hipMemcpyHostToDevice));
        return d;
    }
    const uint64_t seed = (uint64_t)c.i("seed");
    const size_t chunk = (size_t)1 << 20;   // rows per host chunk
    std::vector<uint16_t> h(chunk * C);
    for (size_t r0 = 0; r0 < rows; r0 += chunk) {
        const size_t nr = std::min(chunk, rows - r0);
#pragma omp parallel for schedule(static)
        for (long r = 0; r < (long)nr; ++r)
            for (int ch = 0; ch < C; ++ch) h[(size_t)r * C + ch] = gen_x16(r0 + r, ch, C, seed);
        HIPCHECK(hipMemcpy((uint16_t*)d + r0 * C, h.data(), nr * C * 2, hipMemcpyHostToDevice));
    }
    return d;
}

struct Outcome { int err = 0; bool det = true, guards = true, y_untouched = true; double ms = 0; };

// runs `launch` twice; the outputs of the second run must equal the first's bit for bit
template <class F> Outcome run_twice(F launch, const std::vector<const Guarded*>& outs) {
    Outcome o;
    std::vector<std::vector<unsigned char>> first;
    for (int it = 0; it < 2; ++it) {
        const auto t0 = std::chrono::steady_clock::now();
        o.err = (int)launch();
        HIPCHECK(hipDeviceSynchronize());
        if (it == 0) o.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (o.err) return o;
        for (size_t k = 0; k < outs.size(); ++k) {
            std::vector<unsigned char> b;
            if (outs[k]->bytes <= ((size_t)1 << 31)) {   // (the 4 GB outputs of the run-splitting cases are not compared)
                b.resize(outs[k]->bytes);
                HIPCHECK(hipMemcpy(b.data(), outs[k]->p(), b.size(), hipMemcpyDeviceToHost));
            }
            if (it == 0) first.push_back(std::move(b));
            else if (b != first[k]) o.det = false;
        }
    }
    for (const Guarded* g : outs) o.guards = o.guards && g->guards_intact();
    return o;
}

// ================================================================ GemmParams cases (conv_check.cpp, cunet_check.cpp)
typedef hipError_t (*Launch1)(const GemmParams&, hipStream_t);
typedef hipError_t (*Launch2)(const GemmParams&, const GemmParams&, hipStream_t);
typedef bool (*Pred1)(const GemmParams&);
typedef bool (*Pred2)(const GemmParams&, const GemmParams&);
typedef hipError_t (*LaunchScale)(void*, const float*, int, int, int, bool, hipStream_t);

constexpr int kErrUnsupported = -2, kErrBounds = -3;     // reported instead of launching

inline void* sym(void* lib, const char* name) {
    void* f = dlsym(lib, name);
    if (!f) throw std::runtime_error(std::string("the library does not export ") + name);
    return f;
}

// ---- GemmParams from the numbers of a case (keys prefixed with `pre`); pointers are set by the caller
inline GemmParams numbers(const Case& c, const std::string& pre) {
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
    p.out.Hs = I("oHs"); p.out.Ws = I("oWs"); p.out.Cs = I("oCs"); p.out.y0 = I("oy0"); p.out.x0 = I("ox0");
    p.omode = I("omode"); p.r = I("r", 1); p.Cout = I("Cout", p.out.Cs); p.ln_eps = (float)c.num(pre + "ln_eps", 1e-5);
    return p;
}

// elements allocated behind each pointer of a parameter set
struct Extents { size_t a = 0, out = 0, res = 0, res2 = 0, stats_in = 0, stats_out = 0, wt = 0, bias = 0, csum = 0, table = 0; };

inline Extents extents_of(const GemmParams& p) {      // as plan.cpp sizes tensors: whole stored maps of the pass
    Extents e;
    e.a = (size_t)p.B * p.a.Hs * p.a.Ws * p.a.Cs; e.out = (size_t)p.B * p.out.Hs * p.out.Ws * p.out.Cs;
    e.res = (size_t)p.B * p.res.Hs * p.res.Ws * p.res.Cs; e.res2 = (size_t)p.B * p.res2.Hs * p.res2.Ws * p.res2.Cs;
    e.stats_in = (size_t)p.B * p.a.Hs * p.a.Ws * 2; e.stats_out = (size_t)p.B * p.out.Hs * p.out.Ws * 2;
    e.wt = (size_t)p.N * p.Kw; e.bias = (size_t)p.N; e.csum = (size_t)p.N; e.table = (size_t)p.Mrows;
    return e;
}

// gemm_kernel's addressing (k_gemm.hip: the per-row bookkeeping, load_regs, epilogue phase 2), in 64-bit arithmetic: every element of every map a launch
// of `p` reads or writes must lie inside the map's view and inside `e`.  The specialised kernels touch the same elements (k_stem.hip clamps its idle lanes
// onto the row's last pixel, k_conv48.hip / k_conv3.hip / k_conv3h.hip fetch only halo pixels inside Ho + 2 x Wo + 2, k_pixgemm.hip reads rows, 2 x 2 patches and
// skip pixels of existing rows only).  A head of fewer than 4 channels (out.Cs == 4, rows mode) stores all 4 halves of a pixel.
// Passes of many rows without a table are walked at the corners of every image only: all offsets are monotone in the row's y and x.
inline bool accesses_ok(const GemmParams& p, const Extents& e, const std::vector<int>& table, std::string& why) {
    auto fail = [&](const std::string& w) { why = w; return false; };
    if (p.B <= 0 || p.Mrows <= 0 || p.aW <= 0 || p.K <= 0 || p.N <= 0 || p.Kw < p.K || p.Kw % 8) return fail("sizes");
    if (p.a.Cs != 4 && p.a.Cs % 8) return fail("a.Cs");
    const int AP = p.a.Cs == 4 ? 4 : 8, OP = p.out.Cs == 4 ? 4 : 8;
    const int r = p.omode == 2 ? p.r : 1, ncol = p.omode == 2 ? p.out.Cs : (p.out.Cs == 4 && p.N < 4) ? 4 : p.N;
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
inline void* upload_map(const Case& c, const std::string& key, size_t pixels, int C, uint64_t seed_off) {
    Case cc = c;
    cc.s["x"] = c.str(key);
    cc.n["seed"] = (double)(c.i("seed") + (long)seed_off);
    return upload_rows(cc, pixels, C);
}

inline std::vector<uint16_t> transpose_taps(const std::vector<uint16_t>& w, int N, int Kw, int kh, int kw, int Cs) {   // W[n][ky][kx][c] -> W[n][kx][ky][c] (kh == kw)
    std::vector<uint16_t> o = w;
    for (int n = 0; n < N; ++n)
        for (int ky = 0; ky < kh; ++ky)
            for (int kx = 0; kx < kw; ++kx)
                for (int ch = 0; ch < Cs; ++ch) o[(size_t)n * Kw + (ky * kw + kx) * Cs + ch] = w[(size_t)n * Kw + (kx * kw + ky) * Cs + ch];
    return o;
}

struct Result {
    int err = 0, gerr = 0;                   // the launcher under test; the same parameters on launch_gemm ("also_gemm")
    bool det = true, guards = true, first = true, untouched = true, ident = true;
    double ms = 0;
};

inline void report(const Case& c, const Result& o) {
    printf("CASE %s err=%d gerr=%d det=%d guards=%d first=%d untouched=%d ident=%d ms=%.3f\n", c.str("name").c_str(), o.err, o.gerr, (int)o.det, (int)o.guards, (int)o.first, (int)o.untouched,
           (int)o.ident, o.ms);
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

// [B][C] gate rows of a case, mutated: every row taken from the next image / shifted by one channel
inline std::vector<float> load_gates(const Case& c, const std::string& key, int B, int C, const std::string& mut) {
    std::vector<float> g = load<float>(c.str(key), (size_t)B * C), o = g;
    if (mut == "gate_next_image") for (int b = 0; b < B; ++b) for (int ch = 0; ch < C; ++ch) o[(size_t)b * C + ch] = g[(size_t)((b + 1) % B) * C + ch];
    if (mut == "gate_shift_channel") for (int b = 0; b < B; ++b) for (int ch = 0; ch < C; ++ch) o[(size_t)b * C + ch] = g[(size_t)b * C + (ch + 1) % C];
    return o;
}

// loads the operands of `p` (numbers already set) and applies the case's mutation to what the kernel is handed.  `launcher` decides which weight copies exist:
// pixgemm: wt_frag = frag_major; conv48 / pair: the 448-column padding of engine.cpp, then frag_major; conv3: wt_perm = frag_conv3b (mutant perm_row_swap: of that copy alone).
inline void load_operands(const Case& c, const std::string& pre, GemmParams& p, Operands& ops, const std::string& launcher, const std::string& mut_key = "mutate") {
    const std::string mut = c.str(mut_key);
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
    if (launcher == "conv3") {
        std::vector<uint16_t> perm = frag_conv3b(wt.data(), p.N, p.Kw);
        if (mut == "perm_row_swap")      // the LAYOUT alone: lanes 1 and 4 (A rows 1 and 4) of k-group 0 trade places in every fragment of n-tile 0 of block 0 - p.wt stays true, so
            for (int ks = 0; ks < p.Kw / 32; ++ks)      // gemm_kernel on the same parameters is right and conv3_kernel is not
                for (int e = 0; e < 8; ++e) std::swap(perm[(((size_t)ks * 4 + 0) * 64 + 1) * 8 + e], perm[(((size_t)ks * 4 + 0) * 64 + 4) * 8 + e]);
        p.wt_perm = ops.half(perm);
    }
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
    if (!c.str(pre + "a_scale").empty()) p.a_scale = ops.flt(load_gates(c, pre + "a_scale", p.B, p.a.Cs, mut));
    if (!c.str(pre + "res_scale").empty()) p.res_scale = ops.flt(load_gates(c, pre + "res_scale", p.B, p.res.Cs, mut));
    if (!c.str(pre + "a").empty() || c.i("gen")) { void* a = upload_map(c, pre + "a", (size_t)p.B * p.a.Hs * p.a.Ws, p.a.Cs, 0); ops.raw.push_back(a); p.a.p = a; }
    if (p.res.Cs) { void* m = upload_map(c, pre + "res", (size_t)p.B * p.res.Hs * p.res.Ws, p.res.Cs, 1); ops.raw.push_back(m); p.res.p = m; }
    if (p.res2.Cs) { void* m = upload_map(c, pre + "res2", (size_t)p.B * p.res2.Hs * p.res2.Ws, p.res2.Cs, 2); ops.raw.push_back(m); p.res2.p = m; }
}

// the pixels of an output to send back: all, or those of <name>.rows
inline void save_out(const Case& c, const std::string& ext, const Guarded& y, const Guarded* st, const std::string& st_ext, int Cs) {
    std::vector<long> idx;
    if (c.i("nrows")) idx = load<long>(c.str("rows"), (size_t)c.i("nrows"));
    const std::vector<long>* ip = c.i("nrows") ? &idx : nullptr;
    save(c.str("name") + ext, y.rows<uint16_t>(ip, Cs));
    if (st) save(c.str("name") + st_ext, st->rows<float>(ip, 2));
}

// what a harness supplies to run_gemm_case: its launchers and predicates by name ("gemm": launch_gemm, no predicate), the pooling partials a launcher writes per image
// (0: it cannot pool), and launch_scale (null: no "scale_ident" cases)
struct GemmBackend {
    bool (*supported)(const std::string& launcher, const GemmParams& p) = nullptr;
    Launch1 (*fn)(const std::string& launcher) = nullptr;
    int (*pool_tiles)(const std::string& launcher, const GemmParams& p) = nullptr;
    LaunchScale scale = nullptr;
};

// One parameter set on its launcher, optionally on launch_gemm as well ("also_gemm"): twice (bit-identical or not), then the first image alone (bit-identical to the
// batch's or not), the guard bands.  "pool": the launch also writes pooling partials (.pool / .gpool: [B][tiles][out.Cs] fp32).  "scale_ident": the launch with its gates
// (a_scale / res_scale) must equal, byte for byte, launch_scale in place on a copy of the gated map followed by the same launch without the gate.
inline void run_gemm_case(const Case& c, const GemmBackend& be) {
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
        const int tiles = c.i("pool") && be.pool_tiles ? be.pool_tiles(L, q) : 0;
        std::unique_ptr<Guarded> pool(tiles > 0 ? new Guarded((size_t)p.B * tiles * p.out.Cs * 4) : nullptr);
        if (c.i("pool") && !pool) { err = kErrUnsupported; continue; }
        q.pool_out = pool ? (float*)pool->p() : nullptr;
        if (!be.supported(L, q)) { err = kErrUnsupported; continue; }
        if (!accesses_ok(q, e, ops.table, why)) { fprintf(stderr, "%s: not launched: %s\n", c.str("name").c_str(), why.c_str()); err = kErrBounds; continue; }
        std::vector<const Guarded*> outs = {&y};
        if (st) outs.push_back(st.get());
        if (pool) outs.push_back(pool.get());
        const Outcome r = run_twice([&] { return be.fn(L)(q, 0); }, outs);
        err = r.err; o.det = o.det && r.det; o.guards = o.guards && r.guards;
        if (!side) o.ms = r.ms;
        if (r.err) continue;
        save_out(c, side ? ".gy" : ".y", y, st.get(), side ? ".gstats" : ".stats", p.out.Cs);
        if (pool) save(c.str("name") + (side ? ".gpool" : ".pool"), pool->rows<float>(nullptr, 1));
        if (p.B > 1 && !c.i("gen")) {                   // the first image alone: the same maps, B = 1, fresh outputs
            const size_t yb = e.out / p.B * 2, sb = e.stats_out / p.B * 4, pb = pool ? pool->bytes / p.B : 0;
            Guarded y1(yb);
            std::unique_ptr<Guarded> st1(st ? new Guarded(sb) : nullptr), pool1(pool ? new Guarded(pb) : nullptr);
            GemmParams q1 = q;
            q1.B = 1; q1.out.p = y1.p(); q1.stats_out = st1 ? (float*)st1->p() : nullptr; q1.pool_out = pool1 ? (float*)pool1->p() : nullptr;
            if (be.supported(L, q1) && accesses_ok(q1, extents_of(q1), ops.table, why)) {
                HIPCHECK(be.fn(L)(q1, 0));
                HIPCHECK(hipDeviceSynchronize());
                std::vector<unsigned char> full = y.rows<unsigned char>(nullptr, 1), one = y1.rows<unsigned char>(nullptr, 1);
                full.resize(yb);
                o.first = o.first && full == one && y1.guards_intact();
                if (st) { full = st->rows<unsigned char>(nullptr, 1); one = st1->rows<unsigned char>(nullptr, 1); full.resize(sb); o.first = o.first && full == one; }
                if (pool) { full = pool->rows<unsigned char>(nullptr, 1); one = pool1->rows<unsigned char>(nullptr, 1); full.resize(pb); o.first = o.first && full == one && pool1->guards_intact(); }
            } else o.first = false;
        }
        if (c.i("scale_ident")) {                       // launch_scale in place on copies of the gated maps, then the launch without its gates
            if (!be.scale) throw std::runtime_error("scale_ident: this harness has no launch_scale");
            GemmParams q2 = q;
            Guarded y2(e.out * 2);
            q2.out.p = y2.p(); q2.pool_out = nullptr; q2.stats_out = nullptr;
            std::vector<void*> copies;
            auto scaled_copy = [&](const TView& v, const float* gate) {
                const size_t bytes = (size_t)p.B * v.Hs * v.Ws * v.Cs * 2;
                void* d = nullptr;
                HIPCHECK(hipMalloc(&d, bytes + 256));
                HIPCHECK(hipMemcpy(d, v.p, bytes, hipMemcpyDeviceToDevice));
                HIPCHECK(be.scale(d, gate, p.B, v.Hs * v.Ws, v.Cs, false, 0));
                copies.push_back(d);
                return d;
            };
            if (q.a_scale) { q2.a.p = scaled_copy(q.a, q.a_scale); q2.a_scale = nullptr; }
            if (q.res_scale) { q2.res.p = scaled_copy(q.res, q.res_scale); q2.res_scale = nullptr; }
            if (be.supported(L, q2)) {
                HIPCHECK(be.fn(L)(q2, 0));
                HIPCHECK(hipDeviceSynchronize());
                o.ident = o.ident && y.rows<unsigned char>(nullptr, 1) == y2.rows<unsigned char>(nullptr, 1) && y2.guards_intact();
            } else o.ident = false;
            for (void* d : copies) HIPCHECK(hipFree(d));
        }
    }
    report(c, o);
}

// "predicate" / "refuse" cases: the numbers of a case with stand-in pointers (nothing is launched by a predicate, nothing allocated behind the stand-ins)
struct StandIns {
    Dev<uint16_t> dummy;
    Guarded y;
    StandIns() : dummy(std::vector<uint16_t>(4096, 0)), y(4096) {}
    void point(const Case& c, GemmParams& p, bool is_output_owner = true) const {
        p.a.p = dummy.p; p.wt = dummy.p; p.bias = (const float*)dummy.p;
        if (is_output_owner) p.out.p = y.p();
        if (c.i("frag", 1)) { p.wt_frag = dummy.p; p.wt_perm = dummy.p; }
        if (p.res.Cs) p.res.p = dummy.p;
        if (p.res2.Cs) p.res2.p = dummy.p;
        if (c.i("stats")) p.stats_out = (float*)dummy.p;
        if (p.ln) { p.csum = (const float*)dummy.p; p.stats_in = (const float*)dummy.p; }
    }
};

// "predicate": pred(case, p, stand-ins) alone (ok = what it answered).  "refuse" (gemm != null): the same numbers through launch_gemm, which must answer
// hipErrorInvalidValue from the sizes alone.  Either way the stand-in output stays untouched.
template <class PredF> void run_no_launch(const Case& c, Launch1 gemm, PredF pred) {
    GemmParams p = numbers(c, "");
    StandIns s;
    s.point(c, p);
    Result o;
    if (gemm) {
        o.err = (int)gemm(p, 0);
        HIPCHECK(hipDeviceSynchronize());
    } else o.err = pred(c, p, s) ? 0 : 1;
    o.untouched = s.y.untouched();
    report(c, o);
}

}  // namespace
