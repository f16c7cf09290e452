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
// LDS: at a factor of 4 with bicubic taps (ky = 17) rows_max <= 15 * 4 + 1 + 17 = 78 rows, 3 * 78 * 256 B = 58.5 KiB: two workgroups per CU.
#include "kernels.h"

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

}  // namespace w2x
