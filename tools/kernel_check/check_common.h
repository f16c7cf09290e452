// What the kernel harnesses of this directory share (transformer_check.cpp, conv_check.cpp): the large-input formula, the flat JSON reader of
// cases.json, file helpers, guarded device buffers and the run-twice driver.  Host code only; each harness is one translation unit.
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

}  // namespace
