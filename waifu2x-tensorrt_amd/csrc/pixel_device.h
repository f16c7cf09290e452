// Device pieces shared by the frame formats: planar and gray frames (k_planar.hip), RGBA frames (k_rgba.hip, k_planar_rgba.hip) and every resize kernel, the BGR
// and YUV ones included (k_resample.hip, k_resample_yuv.hip).  The gather and compose pieces are the corresponding pieces of a BGR kernel (gather_kernel,
// compose_kernel of k_prepost.hip) with the format-specific load or store left to the caller: a format supplies a loader and a store and reuses the bodies.  The
// resize has no BGR original any more: its two passes and its launch sequence are stated here once, and a kernel adds its store.  The byte-for-byte
// contracts of DESIGN 9d - 9j rest on the arithmetic and its order: the same slots and clamps, compose_pixel_sums' weights in the order L, T, R, B, one resize
// tile, tap tables and tap order (a += wk * s[k]) and one quantisation, sat(rint(x * maxcode)).  k_prepost.hip does not include this header: the gather and
// compose kernels of the BGR and YUV paths keep their listings.
#pragma once
#include "kernels.h"
#include "prepost_device.h"
#include <type_traits>

namespace w2x {
namespace {

// ---- launch shapes
// gather: a flat grid-stride loop of workgroups of kGatherThreads, which the loop takes as a constant: in a device function blockDim.x is not folded to the
// launch's one workgroup size as it is in a kernel's own body, and costs a dependent load before the first index (0.5 us on a launch of 10 us)
constexpr int kGatherThreads = 256;
inline unsigned grid_for(long total) { long g = (total + kGatherThreads - 1) / kGatherThreads; return (unsigned)(g > 8192 ? 8192 : (g < 1 ? 1 : g)); }
// compose, four pixels per thread: compose_kernel's kComposeRows / kComposeThreads (kernels.h)
// resample: the output tile of every resize kernel (kernels.h) and its workgroup.  Byte equality between the formats rests on the same tile, the same tap order
// and the same quantisation.
constexpr int kRsRows = kResampleRows, kRsCols = kResampleCols, kRsThreads = 256;
static_assert(kRsCols == 64 && kRsRows * (kRsCols / 4) == kRsThreads, "pass 2 maps one thread to four pixels of the tile");
constexpr int kRsMaxRows = 104;                                          // factor 4, bicubic: 78 (a factor of 4 is the largest the engine asks for)

// The launch of a resize kernel over the tiles of an outW x outH frame: `row_dwords` of LDS per input row (all planes, a halo included), rows_max of them in this
// launch and kRsMaxRows at most, which is what the kernel is opted in to where that passes 64 KiB (one plane never does: 26 KiB, no call).  `done` is the
// kernel's own per-device mask (ensure_dynamic_lds).
template <typename... KA, typename... A>
hipError_t launch_resample_tiles(void (*kernel)(KA...), int row_dwords, int rows_max, unsigned& done, int outW, int outH, hipStream_t s, const A&... args) {
    if (rows_max <= 0 || rows_max > kRsMaxRows) return hipErrorInvalidValue;
    const int row = row_dwords * (int)sizeof(float);
    if (kRsMaxRows * row > 64 * 1024)
        if (hipError_t e = ensure_dynamic_lds((const void*)kernel, kRsMaxRows * row, done); e != hipSuccess) return e;
    const dim3 grid((unsigned)((outW + kRsCols - 1) / kRsCols), (unsigned)((outH + kRsRows - 1) / kRsRows));
    hipLaunchKernelGGL(kernel, grid, dim3(kRsThreads), (size_t)rows_max * row, s, args...);
    return hipGetLastError();
}

// launch(std::integral_constant<int, M>()) for the dithered mode of d (Ordered or BlueNoise; dither_args_ok(d)): the launchers' switch from the run-time mode
// to the kernel instantiation.  The table's bytes are not staged in LDS, so no resize launch counts them in its dynamic LDS.
template <typename Launch> hipError_t for_dither(const DitherArgs& d, Launch launch) {
    if (d.mode == kDitherOrdered) return launch(std::integral_constant<int, kDitherOrdered>());
    if (d.mode == kDitherBlueNoise && d.table) return launch(std::integral_constant<int, kDitherBlueNoise>());
    return hipErrorInvalidValue;                                         // no kernel for it: an error, never the undithered kernel
}

// launch(std::integral_constant<int, M>(), extra...) for the dither mode of d and the light mode of l: extra... is what the kernel takes behind its
// parameters - nothing, d, l, or d and l - and names the instantiation (kernel<.., M, std::decay_t<decltype(extra)>...>).  This is the one place where the two
// engine-wide settings pick a resize kernel, for every frame format.  Invalid arguments: an error, never another kernel.
// for_light: the same for a kernel that is never dithered (float samples).
template <typename Launch> hipError_t for_light(const LightArgs& l, Launch launch) {
    if (!light_args_ok(l)) return hipErrorInvalidValue;
    return l.mode != kLightGamma ? launch(std::integral_constant<int, kDitherNone>(), l) : launch(std::integral_constant<int, kDitherNone>());
}
template <typename Launch> hipError_t for_modes(const DitherArgs& d, const LightArgs& l, Launch launch) {
    if (!dither_args_ok(d) || !light_args_ok(l)) return hipErrorInvalidValue;
    if (d.mode == kDitherNone) return for_light(l, launch);
    const bool lin = l.mode != kLightGamma;
    return for_dither(d, [&](auto m) { return lin ? launch(m, d, l) : launch(m, d); });
}

// launch(std::integral_constant<int, E>()) for the edge mode of a gather launch: the switch from the run-time mode to the kernel instantiation
template <typename Launch> hipError_t for_edge(int edge, Launch launch) {
    if (edge == kEdgeReplicate) return launch(std::integral_constant<int, kEdgeReplicate>());
    if (edge == kEdgeWrap) return launch(std::integral_constant<int, kEdgeWrap>());
    if (edge == kEdgeMirror) return launch(std::integral_constant<int, kEdgeMirror>());
    return hipErrorInvalidValue;                                         // no kernel for it: an error, never the replicating kernel
}
// for_modes with the edge mode of a resize launch: Wrap and Mirror end the pack with one EdgeArgs, which names the edged instantiation; Replicate adds nothing
template <typename Launch> hipError_t for_light(const LightArgs& l, const EdgeArgs& e, Launch launch) {
    if (!edge_mode_ok(e.mode)) return hipErrorInvalidValue;
    if (e.mode == kEdgeReplicate) return for_light(l, launch);
    return for_light(l, [&](auto m, const auto&... extra) { return launch(m, extra..., e); });
}
template <typename Launch> hipError_t for_modes(const DitherArgs& d, const LightArgs& l, const EdgeArgs& e, Launch launch) {
    if (!edge_mode_ok(e.mode)) return hipErrorInvalidValue;
    if (e.mode == kEdgeReplicate) return for_modes(d, l, launch);
    return for_modes(d, l, [&](auto m, const auto&... extra) { return launch(m, extra..., e); });
}

// ---- the sample types: what a plane holds per pixel.  `maxcode` is 2^bits - 1 and `inv` fl32(1 / maxcode), both made on the host (launch_*).
struct U8 { typedef uint8_t T; };
struct U16 { typedef uint16_t T; };
struct F32 { typedef float T; };

template <typename S> __device__ __forceinline__ float load_sample(const uint8_t* row, int x, unsigned maxcode, float inv);
template <> __device__ __forceinline__ float load_sample<U8>(const uint8_t* row, int x, unsigned, float inv) { return (float)row[x] * inv; }
template <> __device__ __forceinline__ float load_sample<U16>(const uint8_t* row, int x, unsigned maxcode, float inv) {
    return (float)min((unsigned)((const uint16_t*)row)[x], maxcode) * inv;
}
template <> __device__ __forceinline__ float load_sample<F32>(const uint8_t* row, int x, unsigned, float) {
    const float v = ((const float*)row)[x];
    return !(v >= 0.f) ? 0.f : fminf(v, 1.f);                      // (NaN fails the comparison: 0)
}

// sat(rint(x * maxcode)): quantize_bgr's expression per sample (compose) and the one quantisation of every resize kernel, with the code range a launch
// argument - at 255 and 65535 the same product and the same rounding, which byte equality with the BGR kernels rests on.  Float: the sum clamped, never rounded.
__device__ __forceinline__ unsigned quant(float v, float scale, int maxcode) { return (unsigned)min(max(__float2int_rn(v * scale), 0), maxcode); }
__device__ __forceinline__ float sat01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
// the clamp of the YUV resize kernels: sat01(v), or V = encode(sat01(v)) in a kernel whose launch carries a curve
template <bool kLin> __device__ __forceinline__ float sat01_out(const LightArgs& c, float v) {
    if constexpr (kLin) return light_encode(c, sat01(v));
    else return sat01(v);
}

// Four consecutive samples of one plane's row, starting at column X (a multiple of 4): np == 4 and an aligned address leave as ONE store - a dword, 8 or 16
// bytes -, the 1 - 3 samples of a ragged right end (or a caller's unaligned rows) one by one.  From the engine's buffers (hipMalloc, rows padded to 16 bytes:
// planar_step) a full group is always aligned.
template <typename S> __device__ __forceinline__ void store4(uint8_t* row, int X, int np, const float v[4], float scale, int maxcode);
template <> __device__ __forceinline__ void store4<U8>(uint8_t* row, int X, int np, const float v[4], float scale, int maxcode) {
    uint8_t* d = row + X;
    unsigned q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = quant(v[k], scale, maxcode);
    if (np == 4 && (((size_t)d) & 3) == 0) *(unsigned*)d = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
    else for (int k = 0; k < np; ++k) d[k] = (uint8_t)q[k];
}
template <> __device__ __forceinline__ void store4<U16>(uint8_t* row, int X, int np, const float v[4], float scale, int maxcode) {
    uint16_t* d = (uint16_t*)row + X;
    unsigned q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = quant(v[k], scale, maxcode);
    if (np == 4 && (((size_t)d) & 7) == 0) *(uint2*)d = make_uint2(q[0] | q[1] << 16, q[2] | q[3] << 16);
    else for (int k = 0; k < np; ++k) d[k] = (uint16_t)q[k];
}
template <> __device__ __forceinline__ void store4<F32>(uint8_t* row, int X, int np, const float v[4], float, int) {
    float* d = (float*)row + X;
    if (np == 4 && (((size_t)d) & 15) == 0) *(float4v*)d = (float4v){sat01(v[0]), sat01(v[1]), sat01(v[2]), sat01(v[3])};
    else for (int k = 0; k < np; ++k) d[k] = sat01(v[k]);
}
// M: store4<S, M> is the store of plane index c, row Y of a kernel templated on the dither mode.  kDitherNone and float samples: the store above,
// untouched.  A dithered mode quantises sample k with the threshold of (X + k, Y) of plane c (quant_code, prepost_device.h) and packs the same stores.
template <typename S, int M>
__device__ __forceinline__ void store4(uint8_t* row, int X, int np, const float v[4], float scale, int maxcode, const DitherArgs& dz, int c, int Y) {
    if constexpr (M == kDitherNone || std::is_same<S, F32>::value) store4<S>(row, X, np, v, scale, maxcode);
    else {
        typename S::T* d = (typename S::T*)row + X;
        unsigned q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = quant_code<M>(v[k] * scale, maxcode, dz, c, X + k, Y);
        if constexpr (std::is_same<S, U8>::value) {
            if (np == 4 && (((size_t)d) & 3) == 0) *(unsigned*)d = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
            else for (int k = 0; k < np; ++k) d[k] = (uint8_t)q[k];
        } else {
            if (np == 4 && (((size_t)d) & 7) == 0) *(uint2*)d = make_uint2(q[0] | q[1] << 16, q[2] | q[3] << 16);
            else for (int k = 0; k < np; ++k) d[k] = (uint16_t)q[k];
        }
    }
}

// ---- gather_kernel's loop: tile pixel i of B tiles of T x T, the slot lookup, the zero pixel of a pad slot, the TTA source map and the edge rule E (edge_src;
// kEdgeReplicate: the replicate clamp) onto a frame of rows x cols.  load(slot, fy, fx) makes the tile pixel P of frame pixel (fy, fx).
template <typename P, int E = kEdgeReplicate, typename Load>
__device__ __forceinline__ void gather_loop(const TileSlot* slots, int B, int T, int rows, int cols, void* out, Load load) {
    const long total = (long)B * T * T;
    for (long i = (long)blockIdx.x * kGatherThreads + threadIdx.x; i < total; i += (long)gridDim.x * kGatherThreads) {
        int b = (int)(i / ((long)T * T));
        int rem = (int)(i - (long)b * T * T);
        int y = rem / T, x = rem - y * T;
        TileSlot sl = slots[b];
        P v = make_px<P>(0.f, 0.f, 0.f);
        if (sl.valid) {
            int sy, sx;
            aug_src(sl.aug, T - 1, y, x, sy, sx);
            int fy = edge_src<E>(sl.y + sy, rows);
            int fx = edge_src<E>(sl.x + sx, cols);
            v = load(sl, fy, fx);
        }
        *((P*)out + i) = v;
    }
}

// ---- compose_kernel's four-pixel fast path: the sums of pixels X .. X + 3 (X a multiple of 4) of row Y where the four share their covering tile columns
// a0 .. a1, lie inside each of them and no TTA is involved (the caller's test), the tiles [To][To][4] fp16.  A tile contributes its four pixels as two 16-byte
// loads; the per-pixel arithmetic and its order are compose_pixel_sums', so the sums are the ones the per-pixel path gives.  NC = 3 keeps the three channels
// (acc[0..2] = r, g, b), NC = 1 the green channel alone (acc[0]).
template <int NC, typename CP>
__device__ __forceinline__ void compose_quad_sums(const CP& p, int X, int Y, int a0, int a1, float (&acc)[NC][4]) {
    static_assert(NC == 1 || NC == 3, "green alone, or r, g, b");
    const int To = p.To, n = To - 1;
    float s[NC][4] = {};
    int j0 = Y - To + 1; j0 = j0 <= 0 ? 0 : (j0 + p.stride_y - 1) / p.stride_y;
    const int j1 = min(p.ny - 1, Y / p.stride_y);
    for (int ti = a0; ti <= a1; ++ti) {
        const int ox = ti * p.stride_x, lx = X - ox;
        const int rw = ox + To > p.outW ? p.outW - ox : To;
        for (int tj = j0; tj <= j1; ++tj) {
            const int oy = tj * p.stride_y, ly = Y - oy;
            const int rh = oy + To > p.outH ? p.outH - oy : To;
            const long tile = (long)ti * p.ny + tj - p.first_tile;
            const half4* tp = (const half4*)p.tiles + tile * (long)To * To + (long)ly * To + lx;
            half4 h[4];                                            // (NC == 1: only the green halves are converted, or loaded at all)
            if ((((size_t)tp) & 15) == 0) { const half8 u0 = *(const half8*)tp, u1 = *(const half8*)(tp + 2);
                h[0] = (half4){u0[0], u0[1], u0[2], u0[3]}; h[1] = (half4){u0[4], u0[5], u0[6], u0[7]}; h[2] = (half4){u1[0], u1[1], u1[2], u1[3]}; h[3] = (half4){u1[4], u1[5], u1[6], u1[7]}; }
            else if constexpr (NC == 1) { h[0][1] = tp[0][1]; h[1][1] = tp[1][1]; h[2][1] = tp[2][1]; h[3][1] = tp[3][1]; }
            else { h[0] = tp[0]; h[1] = tp[1]; h[2] = tp[2]; h[3] = tp[3]; }
            const bool wl = ox > 0, wt = oy > 0 && ly < p.ovy, wr = ox + rw < p.outW, wb = oy + rh < p.outH && n - ly < p.ovy;
            const float fy_t = wt ? p.ramp_y[ly] : 1.f, fy_b = wb ? p.ramp_y[n - ly] : 1.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float v[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) v[c] = (float)h[k][NC == 1 ? 1 : c];
                if (p.ovx || p.ovy) {
                    const int lk = lx + k;
                    if (wl && lk < p.ovx) { const float w = p.ramp_x[lk];
#pragma unroll
                        for (int c = 0; c < NC; ++c) v[c] *= w; }
                    if (wt) {
#pragma unroll
                        for (int c = 0; c < NC; ++c) v[c] *= fy_t; }
                    if (wr && n - lk < p.ovx) { const float w = p.ramp_x[n - lk];
#pragma unroll
                        for (int c = 0; c < NC; ++c) v[c] *= w; }
                    if (wb) {
#pragma unroll
                        for (int c = 0; c < NC; ++c) v[c] *= fy_b; }
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) s[c][k] += v[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[c][k] = s[c][k];
}

// ---- the two passes of every resize kernel over NP planes of the fp32 canvas (plane stride inW * inH).  A workgroup of kRsThreads owns an output tile of
// kRsRows x kRsCols pixels; h is its LDS.  The plain layout is [NP][rows_max][kRsCols] fp32.  Banks: a row is 64 dwords, one per bank; pass 1 stores dword c of
// a row from lane c, pass 2 reads 16 bytes per lane of one row, each plane by an instruction of its own - the planes lie a multiple of the bank count apart and
// add instructions, no conflicts.
// Pass 1: the input rows [r0, r0 + nr) the tile needs, filtered horizontally onto its output columns; returns r0.  The caller's barrier follows.  The value of
// plane q, input row r, tile column c goes to h[slot(q, r, c)].  kHalo: a 65th column, c == kRsCols, holds output column ox0 - 1 (clamped at 0), which the
// 4:2:0 and 4:2:2 kernels' chroma sites reach; where it lies is the slot's business (k_resample_yuv.hip).  The loop runs nr * 65 items then, nr * 64 without.
// kAbove: the rows start with those of output row oy0 - 1 (clamped at 0), the row halo of top-left sited chroma (resample_rows_max(.., 1) rows).
// kEdge: the tables are resize_taps_edge's - every output has its full support, fx / fy may be negative and f + k may pass the canvas - and every
// input index goes through the rule of mode `edge`: column index(f + k, inW), LDS row r holds canvas row index(r0 + r, inH), nr is not cut at inH (on a tiny
// canvas the same input row may fill several LDS rows).  false: the code below is the code it always was.
template <int NP, bool kHalo, bool kAbove = false, bool kEdge = false, typename RP, typename Slot>
__device__ __forceinline__ int resample_pass1_to(const RP& p, float* h, Slot slot, int edge = kEdgeReplicate) {
    constexpr int kCols = kRsCols + (kHalo ? 1 : 0);
    const int ox0 = blockIdx.x * kRsCols, oy0 = blockIdx.y * kRsRows;
    const int tw = min(kRsCols, p.outW - ox0), th = min(kRsRows, p.outH - oy0);
    const int r0 = p.fy[kAbove ? max(oy0 - 1, 0) : oy0];
    const int nr = (kEdge ? p.fy[oy0 + th - 1] + p.ky : min(p.inH, p.fy[oy0 + th - 1] + p.ky)) - r0;   // <= rows_max (resample_rows_max / _edge)
    const size_t plane = (size_t)p.inW * p.inH;
    for (int i = threadIdx.x; i < nr * kCols; i += kRsThreads) {
        const int r = i / kCols, c = i % kCols;
        float a[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) a[q] = 0.f;
        if (c < tw || (kHalo && c == kRsCols)) {
            const int X = kHalo && c == kRsCols ? max(ox0 - 1, 0) : ox0 + c, f = p.fx[X];
            const float* w = p.wx + (size_t)X * p.kx;
            if constexpr (kEdge) {
                const float* s = p.canvas + (size_t)edge_index_dev(edge, r0 + r, p.inH) * p.inW;
                for (int k = 0; k < p.kx; ++k) {
                    const float wk = w[k];
                    const int x = edge_index_dev(edge, f + k, p.inW);
#pragma unroll
                    for (int q = 0; q < NP; ++q) a[q] += wk * s[q * plane + x];
                }
            } else {
                const int n = min(p.kx, p.inW - f);
                const float* s = p.canvas + (size_t)(r0 + r) * p.inW + f;
                for (int k = 0; k < n; ++k) {
                    const float wk = w[k];
#pragma unroll
                    for (int q = 0; q < NP; ++q) a[q] += wk * s[q * plane + k];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NP; ++q) h[slot(q, r, c)] = a[q];
    }
    return r0;
}
// the plain layout, no halo
template <int NP, bool kEdge = false, typename RP>
__device__ __forceinline__ int resample_pass1(const RP& p, float* h, int edge = kEdgeReplicate) {
    const int rm = p.rows_max;
    return resample_pass1_to<NP, false, false, kEdge>(p, h, [rm](int q, int r, int c) { return (q * rm + r) * kRsCols + c; }, edge);
}
// Pass 2: the rows of LDS filtered vertically, four output pixels (X .. X + 3 of row Y, np of them inside the frame) per thread: a[q] their sums of plane q.
// false: the thread has no pixel to store.  kEdge: every output row has its ky taps in LDS (pass 1 loaded the rows past the canvas through the rule), so none
// is cut at inH; the arithmetic and its order are the same.
template <int NP, bool kEdge = false, typename RP>
__device__ __forceinline__ bool resample_pass2(const RP& p, const float* h, int r0, float4v (&a)[NP], int& X, int& Y, int& np) {
    const int ox0 = blockIdx.x * kRsCols, oy0 = blockIdx.y * kRsRows;
    const int th = min(kRsRows, p.outH - oy0);
    const int ty = threadIdx.x / (kRsCols / 4), cg = threadIdx.x % (kRsCols / 4);
    if (ty >= th) return false;
    Y = oy0 + ty; X = ox0 + 4 * cg;
    np = min(4, p.outW - X);
    if (np <= 0) return false;
    const int rm = p.rows_max;
    const int f = p.fy[Y];
    const int n = kEdge ? p.ky : min(p.ky, p.inH - f);
    const float* w = p.wy + (size_t)Y * p.ky;
#pragma unroll
    for (int q = 0; q < NP; ++q) a[q] = (float4v){0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < n; ++k) {
        const float wk = w[k];
        const int r = f - r0 + k;
#pragma unroll
        for (int q = 0; q < NP; ++q) a[q] += wk * *(const float4v*)&h[(q * rm + r) * kRsCols + 4 * cg];
    }
    return true;
}

}  // namespace
}  // namespace w2x
