// Planar RGB frames (renderPlanar): three planes R, G, B in, three planes out, at 8, 10, 12, 16 bits or float32, the two sides independent.  The
// result is defined by the BGR path - at 8 / 8 and 16 / 16 bits the planes of render() of the interleaved frame, byte for byte - and the three kernels here are
// the BGR kernels of k_prepost.hip / k_resample.hip reading and writing planes at a sample type S; those files stay as they are.
//   gather_planar  : gather_kernel's indexing (slots, replicate padding, the TTA source map); the tile pixel is make_px(r, g, b), a sample
//                    min(code, maxcode) * fl32(1 / maxcode) (8 / 16 bits: gather_kernel's fl32(1/255) / fl32(1/65535)); float: min(max(x, 0), 1), NaN -> 0.
//   compose_planar : compose_kernel's launch shape and four-pixel fast path - at every output depth: the fast path only changes how the sums are fetched -,
//                    elsewhere compose_pixel_sums (prepost_device.h, the code compose_kernel inlines); integer sat(rint(x * maxcode)), float min(max(x, 0), 1);
//                    four samples leave as one store per plane: a dword (8 bits), 8 bytes (10 / 12 / 16), 16 bytes (float).
//   resample_planar: resample_kernel over compose_canvas_kernel's canvas - the same 16 x 64 output tile, tap tables and tap order (a += wk * s[k]) - with the
//                    three accumulators stored like compose_planar's.
#include "kernels.h"
#include "prepost_device.h"

namespace w2x {
namespace {

// the sample types: what a plane holds per pixel.  `maxcode` is 2^bits - 1 and `inv` fl32(1 / maxcode), both made on the host (launch_*).
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

template <typename P, typename S>
__global__ __launch_bounds__(256) void gather_planar_kernel(const GatherPlanarParams p, unsigned maxcode, float inv) {
    const int T = p.T;
    const long total = (long)p.B * T * T;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int b = (int)(i / ((long)T * T));
        int rem = (int)(i - (long)b * T * T);
        int y = rem / T, x = rem - y * T;
        TileSlot sl = p.slots[b];
        P v = make_px<P>(0.f, 0.f, 0.f);
        if (sl.valid) {
            int sy, sx;
            aug_src(sl.aug, T - 1, y, x, sy, sx);
            int fy = min(max(sl.y + sy, 0), p.src.rows - 1);
            int fx = min(max(sl.x + sx, 0), p.src.cols - 1);
            v = make_px<P>(load_sample<S>(p.src.p[0] + (size_t)fy * p.src.step[0], fx, maxcode, inv),
                           load_sample<S>(p.src.p[1] + (size_t)fy * p.src.step[1], fx, maxcode, inv),
                           load_sample<S>(p.src.p[2] + (size_t)fy * p.src.step[2], fx, maxcode, inv));
        }
        *((P*)p.out + i) = v;
    }
}

// sat(rint(x * maxcode)): quantize_bgr's expression per sample (compose) and k_resample.hip's q8 / q16 (resample) with the code range a launch argument - at
// 255 and 65535 the same product and the same rounding, which byte equality with the BGR kernels rests on.  Float: the sum clamped, never rounded to a code.
__device__ __forceinline__ unsigned quant(float v, float scale, int maxcode) { return (unsigned)min(max(__float2int_rn(v * scale), 0), maxcode); }
__device__ __forceinline__ float sat01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

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

// (second copies of k_prepost.hip's kComposeRows / kComposeThreads: a shared header would have changed that file's translation unit.  The values only shape
//  the launch; the bytes do not depend on them.)
constexpr int kPlanarRows = 4, kPlanarThreads = 64;

// compose_kernel with three planes behind it.  A thread owns four consecutive pixels of a row and walks kPlanarRows rows; what depends on the column only is
// computed once per thread.  Where the four share their covering tiles, lie inside each of them and no TTA is involved, a tile contributes its four pixels as two
// 16-byte loads (the tiles are [To][To][4] fp16); the per-pixel arithmetic and its order are compose_pixel_sums', so the sums are the ones the per-pixel path
// gives - at every output depth, since the fast path is about how the sums are fetched and not about what is stored.  The whole canvas: planar frames take no
// strips or shards.
template <typename P, typename S>
__global__ __launch_bounds__(kPlanarThreads) void compose_planar_kernel(const ComposePlanarParams q, float scale, int maxcode) {
    constexpr bool kHalf = sizeof(P) == 8;
    const ComposeParams& p = q.c;
    const int gw = (p.outW + 3) >> 2;
    const int xg = blockIdx.x * kPlanarThreads + threadIdx.x;
    if (xg >= gw) return;
    const P* tiles = (const P*)p.tiles;
    const int To = p.To, n = To - 1;
    const int X = 4 * xg;
    const int np = min(4, p.outW - X);
    int a0 = X - To + 1; a0 = a0 <= 0 ? 0 : (a0 + p.stride_x - 1) / p.stride_x;
    int b0 = X + 3 - To + 1; b0 = b0 <= 0 ? 0 : (b0 + p.stride_x - 1) / p.stride_x;
    const int a1 = min(p.nx - 1, X / p.stride_x), b1 = min(p.nx - 1, (X + 3) / p.stride_x);
    const bool fast = kHalf && np == 4 && !p.tta && a0 == b0 && a1 == b1;
    const int Y0 = blockIdx.y * kPlanarRows, Y1 = min(p.outH, Y0 + kPlanarRows);
    for (int Y = Y0; Y < Y1; ++Y) {
        float acc[3][4] = {};                                      // [plane][pixel]
        if (fast) {
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
                    half4 h[4];
                    if ((((size_t)tp) & 15) == 0) { const half8 u0 = *(const half8*)tp, u1 = *(const half8*)(tp + 2);
                        h[0] = (half4){u0[0], u0[1], u0[2], u0[3]}; h[1] = (half4){u0[4], u0[5], u0[6], u0[7]}; h[2] = (half4){u1[0], u1[1], u1[2], u1[3]}; h[3] = (half4){u1[4], u1[5], u1[6], u1[7]}; }
                    else { h[0] = tp[0]; h[1] = tp[1]; h[2] = tp[2]; h[3] = tp[3]; }
                    const bool wl = ox > 0, wt = oy > 0 && ly < p.ovy, wr = ox + rw < p.outW, wb = oy + rh < p.outH && n - ly < p.ovy;
                    const float fy_t = wt ? p.ramp_y[ly] : 1.f, fy_b = wb ? p.ramp_y[n - ly] : 1.f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float v0 = (float)h[k][0], v1 = (float)h[k][1], v2 = (float)h[k][2];
                        if (p.ovx || p.ovy) {
                            const int lk = lx + k;
                            if (wl && lk < p.ovx) { float w = p.ramp_x[lk]; v0 *= w; v1 *= w; v2 *= w; }
                            if (wt) { v0 *= fy_t; v1 *= fy_t; v2 *= fy_t; }
                            if (wr && n - lk < p.ovx) { float w = p.ramp_x[n - lk]; v0 *= w; v1 *= w; v2 *= w; }
                            if (wb) { v0 *= fy_b; v1 *= fy_b; v2 *= fy_b; }
                        }
                        acc[0][k] += v0; acc[1][k] += v1; acc[2][k] += v2;
                    }
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < np) compose_pixel_sums<P>(p, tiles, X + k, Y, acc[0][k], acc[1][k], acc[2][k]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) store4<S>(q.dst.p[c] + (size_t)Y * q.dst.step[c], X, np, acc[c], scale, maxcode);
    }
}

// resample_kernel (k_resample.hip) with three planes behind it: the same output tile per workgroup, the same tap tables, pass 1 horizontally from the canvas
// into LDS, pass 2 vertically out of LDS with a thread per four pixels of a row, the three planes accumulated with resample_kernel's expressions in its tap order.
// LDS: [3][rows_max][64] fp32, resample_kernel's (58.5 KiB at a factor of 4 with bicubic taps), and its bank pattern: pass 1 stores dword c of a row from
// lane c, pass 2 reads 16 bytes per lane of one row.
// (kRs*: second copies of k_resample.hip's kTR / kTC / kThreads - a shared device header would have changed that file's translation unit.  They must stay in
//  step with it: byte equality with resample_kernel rests on the same tile, the same tap order and the same quantisation.)
constexpr int kRsRows = kResampleRows, kRsCols = kResampleCols, kRsThreads = 256;
static_assert(kRsCols == 64 && kRsRows * (kRsCols / 4) == kRsThreads, "pass 2 maps one thread to four pixels of the tile");

template <typename S>
__global__ __launch_bounds__(kRsThreads) void resample_planar_kernel(const ResamplePlanarParams p, float scale, int maxcode) {
    extern __shared__ float h[];                                          // [3][rows_max][kRsCols]
    const int ox0 = blockIdx.x * kRsCols, oy0 = blockIdx.y * kRsRows;
    const int tw = min(kRsCols, p.outW - ox0), th = min(kRsRows, p.outH - oy0);
    const int r0 = p.fy[oy0];
    const int nr = min(p.inH, p.fy[oy0 + th - 1] + p.ky) - r0;           // <= rows_max (resample_rows_max)
    const size_t plane = (size_t)p.inW * p.inH;
    const int rm = p.rows_max;
    // pass 1: input rows [r0, r0 + nr) filtered horizontally onto the tile's output columns
    for (int i = threadIdx.x; i < nr * kRsCols; i += kRsThreads) {
        const int r = i / kRsCols, c = i % kRsCols;
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
        h[(0 * rm + r) * kRsCols + c] = a0; h[(1 * rm + r) * kRsCols + c] = a1; h[(2 * rm + r) * kRsCols + c] = a2;
    }
    __syncthreads();
    // pass 2: four output pixels of one row per thread
    const int ty = threadIdx.x / (kRsCols / 4), cg = threadIdx.x % (kRsCols / 4);
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
        a0 += wk * *(const float4v*)&h[(0 * rm + r) * kRsCols + 4 * cg];
        a1 += wk * *(const float4v*)&h[(1 * rm + r) * kRsCols + 4 * cg];
        a2 += wk * *(const float4v*)&h[(2 * rm + r) * kRsCols + 4 * cg];
    }
    const float v0[4] = {a0[0], a0[1], a0[2], a0[3]}, v1[4] = {a1[0], a1[1], a1[2], a1[3]}, v2[4] = {a2[0], a2[1], a2[2], a2[3]};
    store4<S>(p.dst.p[0] + (size_t)Y * p.dst.step[0], X, np, v0, scale, maxcode);
    store4<S>(p.dst.p[1] + (size_t)Y * p.dst.step[1], X, np, v1, scale, maxcode);
    store4<S>(p.dst.p[2] + (size_t)Y * p.dst.step[2], X, np, v2, scale, maxcode);
}

inline unsigned grid_for(long total) { long g = (total + 255) / 256; return (unsigned)(g > 8192 ? 8192 : (g < 1 ? 1 : g)); }

// three planes of rows x cols samples of `bits`, every step holding a row, u16 / f32 samples aligned to their size
inline bool planes_ok(const PlanarPlanes& f, int rows, int cols) {
    if (!planar_bits_ok(f.bits) || f.rows != rows || f.cols != cols || rows <= 0 || cols <= 0) return false;
    const size_t bps = planar_sample_bytes(f.bits);
    for (int k = 0; k < 3; ++k) if (!f.p[k] || f.step[k] < (size_t)cols * bps || ((((size_t)f.p[k]) | f.step[k]) & (bps - 1)) != 0) return false;
    return true;
}
inline int max_code(int bits) { return bits == 32 ? 0 : (1 << bits) - 1; }

}  // namespace

hipError_t launch_gather_planar(const GatherPlanarParams& p, hipStream_t s) {
    if (!planes_ok(p.src, p.src.rows, p.src.cols)) return hipErrorInvalidValue;
    const dim3 grid(grid_for((long)p.B * p.T * p.T));
    const int bits = p.src.bits;
    const unsigned maxcode = (unsigned)max_code(bits);
    const float inv = bits == 32 ? 0.f : (float)(1.0 / (double)maxcode);
#define W2X_GATHER_PLANAR(S) \
    do { if (p.fp32) hipLaunchKernelGGL((gather_planar_kernel<float4v, S>), grid, dim3(256), 0, s, p, maxcode, inv); \
         else hipLaunchKernelGGL((gather_planar_kernel<half4, S>), grid, dim3(256), 0, s, p, maxcode, inv); } while (0)
    if (bits == 8) W2X_GATHER_PLANAR(U8); else if (bits == 32) W2X_GATHER_PLANAR(F32); else W2X_GATHER_PLANAR(U16);
#undef W2X_GATHER_PLANAR
    return hipGetLastError();
}
hipError_t launch_compose_planar(const ComposePlanarParams& p, hipStream_t s) {
    if (p.c.outW <= 0 || p.c.outH <= 0) return hipSuccess;
    if (!planes_ok(p.dst, p.c.outH, p.c.outW)) return hipErrorInvalidValue;
    const int gw = (p.c.outW + 3) / 4;
    const dim3 grid((unsigned)((gw + kPlanarThreads - 1) / kPlanarThreads), (unsigned)((p.c.outH + kPlanarRows - 1) / kPlanarRows));
    const int bits = p.dst.bits, maxcode = max_code(bits);
    const float scale = (float)maxcode;
#define W2X_COMPOSE_PLANAR(S) \
    do { if (p.c.fp32) hipLaunchKernelGGL((compose_planar_kernel<float4v, S>), grid, dim3(kPlanarThreads), 0, s, p, scale, maxcode); \
         else hipLaunchKernelGGL((compose_planar_kernel<half4, S>), grid, dim3(kPlanarThreads), 0, s, p, scale, maxcode); } while (0)
    if (bits == 8) W2X_COMPOSE_PLANAR(U8); else if (bits == 32) W2X_COMPOSE_PLANAR(F32); else W2X_COMPOSE_PLANAR(U16);
#undef W2X_COMPOSE_PLANAR
    return hipGetLastError();
}
template <typename S>
static hipError_t resample_planar(const ResamplePlanarParams& p, int lds, int lds_max, const dim3& grid, float scale, int maxcode, hipStream_t s) {
    static unsigned lds_done = 0;
    if (hipError_t e = ensure_dynamic_lds((const void*)resample_planar_kernel<S>, lds_max, lds_done); e != hipSuccess) return e;
    hipLaunchKernelGGL(resample_planar_kernel<S>, grid, dim3(kRsThreads), lds, s, p, scale, maxcode);
    return hipGetLastError();
}
hipError_t launch_resample_planar(const ResamplePlanarParams& p, hipStream_t s) {
    if (p.outW <= 0 || p.outH <= 0) return hipSuccess;
    constexpr int kMaxRows = 104;                                        // as launch_resample: factor 4, bicubic is 78
    if (p.rows_max <= 0 || p.rows_max > kMaxRows || !p.canvas || !planes_ok(p.dst, p.outH, p.outW)) return hipErrorInvalidValue;
    const int lds = 3 * p.rows_max * kRsCols * (int)sizeof(float), lds_max = 3 * kMaxRows * kRsCols * (int)sizeof(float);
    const dim3 grid((unsigned)((p.outW + kRsCols - 1) / kRsCols), (unsigned)((p.outH + kRsRows - 1) / kRsRows));
    const int bits = p.dst.bits, maxcode = max_code(bits);
    const float scale = (float)maxcode;
    if (bits == 8) return resample_planar<U8>(p, lds, lds_max, grid, scale, maxcode, s);
    if (bits == 32) return resample_planar<F32>(p, lds, lds_max, grid, scale, maxcode, s);
    return resample_planar<U16>(p, lds, lds_max, grid, scale, maxcode, s);
}

}  // namespace w2x
