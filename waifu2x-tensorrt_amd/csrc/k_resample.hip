// Antialiased resize of a composed frame to any size between the input frame and the network's output (renderResized): the separable
// convolution resampler of PIL / torch interpolate(antialias=True) on the fp32 RGB canvas that compose_canvas_kernel writes, quantised like
// compose (sat(rint(x * 255)), 16-bit frames 65535) and stored as BGR.
//
// One launch, both passes.  A workgroup owns an output tile of kResampleRows x kResampleCols pixels.  Pass 1 filters the input rows the
// tile's output rows reach, horizontally, from the canvas (read through L1 / L2: neighbouring output columns share most of their taps) into
// LDS: [3][rows_max][kResampleCols] fp32.  Pass 2 filters those rows vertically out of LDS, a thread per four output pixels of a row, and
// stores the four pixels' 12 bytes as three dwords (compose's fast-path store) where the row allows.  The tap tables come from the host
// (tiles.h resize_taps): per output column its first input column and kx weights, per output row its first input row and ky weights;
// weights past the taps an output has are 0, and the loops stop at the canvas edge, so no read leaves the canvas.
// resample_yuv_kernel, further down, is the same resize with a YUV 4:2:0 output (renderYuvResized); the other YUV layouts: k_resample_yuv.hip.
// LDS: at a factor of 4 with bicubic taps (ky = 17) rows_max <= 15 * 4 + 1 + 17 = 78 rows, 3 * 78 * 256 B = 58.5 KiB: two workgroups per CU.
#include "kernels.h"

#include <type_traits>

namespace w2x {
namespace {

typedef float float4v __attribute__((ext_vector_type(4)));

constexpr int kTR = kResampleRows, kTC = kResampleCols, kThreads = 256;
static_assert(kTC == 64 && kTR * (kTC / 4) == kThreads, "pass 2 maps one thread to four pixels of the tile");

__device__ __forceinline__ unsigned q8(float v) { return (unsigned)min(max(__float2int_rn(v * 255.f), 0), 255); }
__device__ __forceinline__ unsigned q16(float v) { return (unsigned)min(max(__float2int_rn(v * 65535.f), 0), 65535); }

__global__ __launch_bounds__(kThreads) void resample_kernel(const ResampleParams p) {
    extern __shared__ float h[];                                          // [3][rows_max][kTC]
    const int ox0 = blockIdx.x * kTC, oy0 = blockIdx.y * kTR;
    const int tw = min(kTC, p.outW - ox0), th = min(kTR, p.outH - oy0);
    const int r0 = p.fy[oy0];
    const int nr = min(p.inH, p.fy[oy0 + th - 1] + p.ky) - r0;           // <= rows_max (resample_rows_max)
    const size_t plane = (size_t)p.inW * p.inH;
    const int rm = p.rows_max;
    // pass 1: input rows [r0, r0 + nr) filtered horizontally onto the tile's output columns
    for (int i = threadIdx.x; i < nr * kTC; i += kThreads) {
        const int r = i / kTC, c = i % kTC;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        if (c < tw) {
            const int X = ox0 + c, f = p.fx[X];
            const int n = min(p.kx, p.inW - f);
            const float* w = p.wx + (size_t)X * p.kx;
            const float* s = p.canvas + (size_t)(r0 + r) * p.inW + f;
            for (int k = 0; k < n; ++k) {
                const float wk = w[k];
                a0 += wk * s[k]; a1 += wk * s[plane + k]; a2 += wk * s[2 * plane + k];
            }
        }
        h[(0 * rm + r) * kTC + c] = a0; h[(1 * rm + r) * kTC + c] = a1; h[(2 * rm + r) * kTC + c] = a2;
    }
    __syncthreads();
    // pass 2: four output pixels of one row per thread
    const int ty = threadIdx.x / (kTC / 4), cg = threadIdx.x % (kTC / 4);
    if (ty >= th) return;
    const int Y = oy0 + ty, X = ox0 + 4 * cg;
    const int np = min(4, p.outW - X);
    if (np <= 0) return;
    const int f = p.fy[Y];
    const int n = min(p.ky, p.inH - f);
    const float* w = p.wy + (size_t)Y * p.ky;
    float4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0;
    for (int k = 0; k < n; ++k) {
        const float wk = w[k];
        const int r = f - r0 + k;
        a0 += wk * *(const float4v*)&h[(0 * rm + r) * kTC + 4 * cg];
        a1 += wk * *(const float4v*)&h[(1 * rm + r) * kTC + 4 * cg];
        a2 += wk * *(const float4v*)&h[(2 * rm + r) * kTC + 4 * cg];
    }
    uint8_t* d = p.dst + (size_t)Y * p.dst_step;
    if (!p.deep) {
        d += (size_t)X * 3;
        unsigned px[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) px[q] = q8(a2[q]) | q8(a1[q]) << 8 | q8(a0[q]) << 16;   // b | g << 8 | r << 16
        if (np == 4 && (((size_t)d) & 3) == 0) {
            unsigned* dw = (unsigned*)d;
            dw[0] = px[0] | px[1] << 24;
            dw[1] = px[1] >> 8 | px[2] << 16;
            dw[2] = px[2] >> 16 | px[3] << 8;
        } else {
            for (int q = 0; q < np; ++q) { d[3 * q] = (uint8_t)px[q]; d[3 * q + 1] = (uint8_t)(px[q] >> 8); d[3 * q + 2] = (uint8_t)(px[q] >> 16); }
        }
    } else {
        uint16_t* d16 = (uint16_t*)d + (size_t)X * 3;
        unsigned v[12];
#pragma unroll
        for (int q = 0; q < 4; ++q) { v[3 * q] = q16(a2[q]); v[3 * q + 1] = q16(a1[q]); v[3 * q + 2] = q16(a0[q]); }
        if (np == 4 && (((size_t)d16) & 3) == 0) {
            unsigned* dw = (unsigned*)d16;
#pragma unroll
            for (int j = 0; j < 6; ++j) dw[j] = v[2 * j] | v[2 * j + 1] << 16;
        } else {
            for (int j = 0; j < 3 * np; ++j) d16[j] = (uint16_t)v[j];
        }
    }
}

// ---- the same resize with a YUV 4:2:0 output (renderYuvResized): compose_yuv_kernel's encoding of the resized canvas
//
// The tile, the tap tables and pass 1 are resample_kernel's, over one more column: chroma site j filters the luma columns 2j - 1, 2j, 2j + 1, and tile
// origins are multiples of 16 rows and 64 columns, so every site and both of its rows lie in one tile and the only value from outside is output column
// ox0 - 1 (clamped at 0), the halo, kept at column kTC of the LDS rows.  Pass 2: a thread per chroma site = 2 x 2 luma pixels, 32 sites of one chroma
// row per half wave.  It filters columns 2j, 2j + 1 of its two rows vertically out of LDS (a float2 per plane and tap), clamps them to [0, 1], codes Y,
// averages the two rows, takes column 2j - 1 from the lane on its left (lanes 0 and 32, the row's first sites, from the halo, which lanes 0 .. 3 of the
// wave filter for its four luma rows) and codes Cb / Cr with the expressions of compose_yuv_kernel.  Four neighbouring lanes then pass their codes to
// the first of them, which stores 8 luma samples per row and 4 + 4 chroma samples in one store each (8 or 16 bytes of Y, 4 or 8 of U and V); a run cut
// by the right edge (or a caller's unaligned rows) stores sample by sample.
// LDS: [3][rows_max][kYP] fp32.  kYP = 66: even, so the float2 reads of pass 2 are 8-byte aligned; a half wave reads 64 consecutive dwords of one row
// (ds_read_b64 banks: address / 4 mod 64 within 32 lanes), conflict free whatever the pitch, and the halo reads of lanes 0 .. 3 hit rows 66 dwords apart
// (banks 2 apart).  Pass 1 writes 65 consecutive dwords per row, rows 66 apart: at most two lanes of 32 on one bank, which a 4-byte store hides.
// At a factor of 4 with bicubic taps rows_max <= 78: 3 * 78 * 66 * 4 B = 60.3 KiB, two workgroups per CU.
constexpr int kYP = kTC + 2;
typedef float float2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned yuv_code(float off, float scale, float v, int maxcode) { return (unsigned)min(max(__float2int_rn(off + scale * v), 0), maxcode); }
__device__ __forceinline__ float sat01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__global__ __launch_bounds__(kThreads) void resample_yuv_kernel(const ResampleYuvParams p) {
    extern __shared__ float h[];                                          // [3][rows_max][kYP]: columns 0 .. kTC - 1 the tile's, kTC the halo
    const int ox0 = blockIdx.x * kTC, oy0 = blockIdx.y * kTR;
    const int tw = min(kTC, p.outW - ox0), th = min(kTR, p.outH - oy0);
    const int r0 = p.fy[oy0];
    const int nr = min(p.inH, p.fy[oy0 + th - 1] + p.ky) - r0;           // <= rows_max (resample_rows_max)
    const size_t plane = (size_t)p.inW * p.inH;
    const int rm = p.rows_max;
    // pass 1: input rows [r0, r0 + nr) filtered horizontally onto the tile's output columns and onto column ox0 - 1
    for (int i = threadIdx.x; i < nr * (kTC + 1); i += kThreads) {
        const int r = i / (kTC + 1), c = i % (kTC + 1);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        if (c < tw || c == kTC) {
            const int X = c == kTC ? max(ox0 - 1, 0) : ox0 + c, f = p.fx[X];
            const int n = min(p.kx, p.inW - f);
            const float* w = p.wx + (size_t)X * p.kx;
            const float* s = p.canvas + (size_t)(r0 + r) * p.inW + f;
            for (int k = 0; k < n; ++k) {
                const float wk = w[k];
                a0 += wk * s[k]; a1 += wk * s[plane + k]; a2 += wk * s[2 * plane + k];
            }
        }
        h[(0 * rm + r) * kYP + c] = a0; h[(1 * rm + r) * kYP + c] = a1; h[(2 * rm + r) * kYP + c] = a2;
    }
    __syncthreads();
    // pass 2: a chroma site per thread.  No lane leaves before the cross-lane moves below: lanes outside the frame carry zeros.
    const YuvCoefs& k = p.k;
    const int lane = threadIdx.x % 64, ci = threadIdx.x / 32, cj = threadIdx.x % 32;
    const int Ya = oy0 + 2 * ci, X0 = ox0 + 2 * cj;
    const bool active = Ya < p.outH && X0 < p.outW;
    const bool has_b = Ya + 1 < p.outH, has_r = X0 + 1 < p.outW;          // odd sizes: row 2i + 1 / column 2j + 1 clamp to the frame
    // output row Y filtered vertically at LDS columns col .. col + N - 1, per plane
    auto vertical = [&](int Y, int col, auto* acc) {
        const int f = p.fy[Y];
        const int n = min(p.ky, p.inH - f);
        const float* w = p.wy + (size_t)Y * p.ky;
        const float* s = h + (f - r0) * kYP + col;
        for (int t = 0; t < n; ++t) {
            const float wk = w[t];
#pragma unroll
            for (int e = 0; e < 3; ++e) acc[e] += wk * *(const std::remove_reference_t<decltype(acc[0])>*)&s[(e * rm + t) * kYP];
        }
    };
    float2v a[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}}, b[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};   // rows 2i, 2i + 1: columns 2j, 2j + 1 of R, G, B
    if (active) {
        vertical(Ya, 2 * cj, a);
        if (has_b) vertical(Ya + 1, 2 * cj, b);
    }
    float halo[3] = {0.f, 0.f, 0.f};                                      // lanes 0 .. 3: column ox0 - 1 of the wave's four luma rows
    if (lane < 4 && oy0 + 4 * (int)(threadIdx.x / 64) + lane < p.outH) vertical(oy0 + 4 * (int)(threadIdx.x / 64) + lane, kTC, halo);
    float vl[3], vr[3], left[3];                                          // the site's columns 2j, 2j + 1 and 2j - 1, the two rows averaged
    unsigned ya[2], yb[2];
    {
        float oa[2][3], ob[2][3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            oa[0][e] = sat01(a[e][0]); oa[1][e] = sat01(a[e][1]);
            ob[0][e] = has_b ? sat01(b[e][0]) : oa[0][e]; ob[1][e] = has_b ? sat01(b[e][1]) : oa[1][e];
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            ya[q] = yuv_code(k.y_off, k.y_scale, k.kr * oa[q][0] + k.kg * oa[q][1] + k.kb * oa[q][2], k.maxcode);
            yb[q] = yuv_code(k.y_off, k.y_scale, k.kr * ob[q][0] + k.kg * ob[q][1] + k.kb * ob[q][2], k.maxcode);
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            vl[e] = 0.5f * (oa[0][e] + ob[0][e]);
            vr[e] = has_r ? 0.5f * (oa[1][e] + ob[1][e]) : vl[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const float hc = sat01(halo[e]);
        const float ha = __shfl(hc, 2 * (lane / 32)), hb = __shfl(hc, 2 * (lane / 32) + 1);
        const float from_left = __shfl_up(vr[e], 1);
        left[e] = cj ? from_left : 0.5f * (ha + (has_b ? hb : ha));
    }
    unsigned uv;                                                          // U | V << 16
    {
        float f[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) f[e] = 0.25f * left[e] + 0.5f * vl[e] + 0.25f * vr[e];
        const float Y = k.kr * f[0] + k.kg * f[1] + k.kb * f[2];
        uv = yuv_code(k.c_off, k.c_scale, (f[2] - Y) * k.cb_div, k.maxcode) | yuv_code(k.c_off, k.c_scale, (f[0] - Y) * k.cr_div, k.maxcode) << 16;
    }
    // stores: the run of four sites the lane belongs to goes out through its first lane where the run is whole and its rows are aligned
    const bool wide = p.dst.bits > 8;
    const int sh = wide ? 1 : 0;                                           // log2 bytes per sample
    const int Xr = ox0 + 2 * (cj & ~3), ic = Ya >> 1;
    uint8_t* const rowa = p.dst.p[0] + (size_t)Ya * p.dst.step[0];
    uint8_t* const rowb = rowa + p.dst.step[0];
    uint8_t* const rowu = p.dst.p[1] + (size_t)ic * p.dst.step[1];
    uint8_t* const rowv = p.dst.p[2] + (size_t)ic * p.dst.step[2];
    const size_t ymask = wide ? 15 : 7, cmask = wide ? 7 : 3;
    const bool packed = Xr + 8 <= p.outW &&
                        ((((size_t)rowa + ((size_t)Xr << sh)) | p.dst.step[0]) & ymask) == 0 &&
                        ((((size_t)rowu + ((size_t)(Xr >> 1) << sh)) | ((size_t)rowv + ((size_t)(Xr >> 1) << sh))) & cmask) == 0;
    const unsigned wa = ya[0] | ya[1] << (wide ? 16 : 8), wb = yb[0] | yb[1] << (wide ? 16 : 8);
    unsigned qa[4] = {wa, 0, 0, 0}, qb[4] = {wb, 0, 0, 0}, qc[4] = {uv, 0, 0, 0};
#pragma unroll
    for (int q = 1; q < 4; ++q) { qa[q] = __shfl_down(wa, q); qb[q] = __shfl_down(wb, q); qc[q] = __shfl_down(uv, q); }
    if (!active) return;
    if (packed) {
        if (cj & 3) return;
        if (!wide) {
            *(uint2*)(rowa + Xr) = make_uint2(qa[0] | qa[1] << 16, qa[2] | qa[3] << 16);
            if (has_b) *(uint2*)(rowb + Xr) = make_uint2(qb[0] | qb[1] << 16, qb[2] | qb[3] << 16);
            *(unsigned*)(rowu + (Xr >> 1)) = (qc[0] & 0xff) | (qc[1] & 0xff) << 8 | (qc[2] & 0xff) << 16 | (qc[3] & 0xff) << 24;
            *(unsigned*)(rowv + (Xr >> 1)) = (qc[0] >> 16) | (qc[1] >> 16) << 8 | (qc[2] >> 16) << 16 | (qc[3] >> 16) << 24;
        } else {
            *(uint4*)(rowa + 2 * (size_t)Xr) = make_uint4(qa[0], qa[1], qa[2], qa[3]);
            if (has_b) *(uint4*)(rowb + 2 * (size_t)Xr) = make_uint4(qb[0], qb[1], qb[2], qb[3]);
            *(uint2*)(rowu + Xr) = make_uint2((qc[0] & 0xffff) | qc[1] << 16, (qc[2] & 0xffff) | qc[3] << 16);
            *(uint2*)(rowv + Xr) = make_uint2(qc[0] >> 16 | (qc[1] & 0xffff0000u), qc[2] >> 16 | (qc[3] & 0xffff0000u));
        }
        return;
    }
    const int nc = has_r ? 2 : 1, j = X0 >> 1;
    if (!wide) {
        for (int q = 0; q < nc; ++q) { rowa[X0 + q] = (uint8_t)ya[q]; if (has_b) rowb[X0 + q] = (uint8_t)yb[q]; }
        rowu[j] = (uint8_t)uv; rowv[j] = (uint8_t)(uv >> 16);
    } else {
        for (int q = 0; q < nc; ++q) { ((uint16_t*)rowa)[X0 + q] = (uint16_t)ya[q]; if (has_b) ((uint16_t*)rowb)[X0 + q] = (uint16_t)yb[q]; }
        ((uint16_t*)rowu)[j] = (uint16_t)uv; ((uint16_t*)rowv)[j] = (uint16_t)(uv >> 16);
    }
}

}  // namespace

int resample_rows_max(const int* fy, int outH, int inH, int ky) {
    int m = 0;
    for (int y0 = 0; y0 < outH; y0 += kTR) {
        const int y1 = (y0 + kTR < outH ? y0 + kTR : outH) - 1;
        const int e = fy[y1] + ky < inH ? fy[y1] + ky : inH;
        if (e - fy[y0] > m) m = e - fy[y0];
    }
    return m;
}

hipError_t launch_resample(const ResampleParams& p, hipStream_t s) {
    if (p.outW <= 0 || p.outH <= 0) return hipSuccess;
    constexpr int kMaxRows = 104;                                        // factor 4, bicubic: 78 (a factor of 4 is the largest the engine asks for)
    const int lds = 3 * p.rows_max * kTC * (int)sizeof(float);
    if (p.rows_max <= 0 || p.rows_max > kMaxRows) return hipErrorInvalidValue;
    static unsigned lds_done = 0;
    hipError_t e = ensure_dynamic_lds((const void*)resample_kernel, 3 * kMaxRows * kTC * (int)sizeof(float), lds_done);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((p.outW + kTC - 1) / kTC), (unsigned)((p.outH + kTR - 1) / kTR));
    hipLaunchKernelGGL(resample_kernel, grid, dim3(kThreads), lds, s, p);
    return hipGetLastError();
}

hipError_t launch_resample_yuv(const ResampleYuvParams& p, hipStream_t s) {
    if (p.outW <= 0 || p.outH <= 0) return hipSuccess;
    constexpr int kMaxRows = 104;                                        // as launch_resample
    const int lds = 3 * p.rows_max * kYP * (int)sizeof(float);
    if (p.rows_max <= 0 || p.rows_max > kMaxRows || p.dst.rows != p.outH || p.dst.cols != p.outW || (p.dst.bits != 8 && p.dst.bits != 10)) return hipErrorInvalidValue;
    if (p.dst.layout != kYuvI420) return launch_resample_yuv_layout(p, s);   // I422, I444, NV12: k_resample_yuv.hip
    static unsigned lds_done = 0;
    hipError_t e = ensure_dynamic_lds((const void*)resample_yuv_kernel, 3 * kMaxRows * kYP * (int)sizeof(float), lds_done);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((p.outW + kTC - 1) / kTC), (unsigned)((p.outH + kTR - 1) / kTR));
    hipLaunchKernelGGL(resample_yuv_kernel, grid, dim3(kThreads), lds, s, p);
    return hipGetLastError();
}

}  // namespace w2x
