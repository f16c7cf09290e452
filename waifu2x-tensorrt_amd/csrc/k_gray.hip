// Gray frames (renderGray): one sample per pixel in, one sample per pixel out.  The result is defined by the BGR path - renderGray(g) is the green
// channel of render() of the frame B = G = R = g, byte for byte - and the four kernels here are the BGR kernels of k_prepost.hip / k_resample.hip with the two
// channels nobody looks at left out; those files stay as they are.
//   gather_gray        : gather_kernel's indexing (slots, replicate padding, the TTA source map) on a one-sample frame: the tile pixel is (a, a, a, 0),
//                        a = u8 * fl32(1/255) (16-bit: u16 * fl32(1/65535)) - the pixel gather_kernel makes of B = G = R.
//   compose_gray       : compose_kernel's launch shape and four-pixel fast path on the green channel of the tiles; elsewhere compose_pixel_sums' green sum
//                        (prepost_device.h, the code compose_kernel inlines); sat(rint(x * 255)) (16-bit: 65535); four samples leave as one dword (8 bytes).
//   compose_canvas_gray: compose_canvas_kernel's mapping, the green sums unquantised as ONE fp32 plane (resized frames).
//   resample_gray      : resample_kernel over that plane - the same 16 x 64 output tile, tap tables, tap order (a += wk * s[k]) and quantisation.
#include "kernels.h"
#include "prepost_device.h"

namespace w2x {
namespace {

template <typename P>
__global__ __launch_bounds__(256) void gather_gray_kernel(const GatherGrayParams p) {
    const int T = p.T;
    const long total = (long)p.B * T * T;
    const float inv255 = (float)(1.0 / 255.0), inv65535 = (float)(1.0 / 65535.0);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int b = (int)(i / ((long)T * T));
        int rem = (int)(i - (long)b * T * T);
        int y = rem / T, x = rem - y * T;
        TileSlot sl = p.slots[b];
        P v = make_px<P>(0.f, 0.f, 0.f);
        if (sl.valid) {
            int sy, sx;
            aug_src(sl.aug, T - 1, y, x, sy, sx);
            int fy = min(max(sl.y + sy, 0), p.rows - 1);
            int fx = min(max(sl.x + sx, 0), p.cols - 1);
            const uint8_t* row = p.frame + (size_t)fy * p.step;
            const float a = p.deep ? (float)((const uint16_t*)row)[fx] * inv65535 : (float)row[fx] * inv255;
            v = make_px<P>(a, a, a);
        }
        *((P*)p.out + i) = v;
    }
}

// sat(rint(x * 255)) / sat(rint(x * 65535)): quantize_bgr's expression per sample (compose) and k_resample.hip's q8 / q16 (resample) - second copies of the
// latter, since a shared device header would have changed that file's translation unit; byte equality with the BGR kernels rests on them.
__device__ __forceinline__ unsigned q8(float v) { return (unsigned)min(max(__float2int_rn(v * 255.f), 0), 255); }
__device__ __forceinline__ unsigned q16(float v) { return (unsigned)min(max(__float2int_rn(v * 65535.f), 0), 65535); }

// (second copies of k_prepost.hip's kComposeRows / kComposeThreads: a shared header would have changed that file's translation unit.  The values only shape
//  the launch; the bytes do not depend on them.)
constexpr int kGrayRows = 4, kGrayThreads = 64;

// compose_kernel on the green channel.  A thread owns four consecutive pixels of a row and walks kGrayRows rows; what depends on the column only is computed
// once per thread.  Where the four share their covering tiles, lie inside each of them, no TTA is involved and the frame is 8-bit, a tile contributes its four
// pixels as two 16-byte loads (the tiles are [To][To][4]: the same bytes compose_kernel reads, of which the green halves are used); the per-pixel arithmetic
// and its order are compose_pixel_sums', so the sample is the one the per-pixel path gives.  The whole canvas: gray frames take no strips or shards.
// Stores: a full group leaves as one dword (16-bit: 8 bytes), the 1 - 3 samples the right edge leaves one by one.  The address test in front of the wide
// store only states the launcher's contract (any dst / dst_step that holds the rows): the engine's own buffers come from hipMalloc with rows padded to 16
// bytes (gray_step) and X is a multiple of 4, so from the engine a full group is always aligned and that test never fails.
template <typename P>
__global__ __launch_bounds__(kGrayThreads) void compose_gray_kernel(const ComposeParams p) {
    constexpr bool kHalf = sizeof(P) == 8;
    const int gw = (p.outW + 3) >> 2;
    const int xg = blockIdx.x * kGrayThreads + threadIdx.x;
    if (xg >= gw) return;
    const P* tiles = (const P*)p.tiles;
    const int To = p.To, n = To - 1;
    const int X = 4 * xg;
    const int np = min(4, p.outW - X);
    int a0 = X - To + 1; a0 = a0 <= 0 ? 0 : (a0 + p.stride_x - 1) / p.stride_x;
    int b0 = X + 3 - To + 1; b0 = b0 <= 0 ? 0 : (b0 + p.stride_x - 1) / p.stride_x;
    const int a1 = min(p.nx - 1, X / p.stride_x), b1 = min(p.nx - 1, (X + 3) / p.stride_x);
    const bool fast = kHalf && np == 4 && !p.tta && !p.deep && a0 == b0 && a1 == b1;
    const int Y0 = blockIdx.y * kGrayRows, Y1 = min(p.outH, Y0 + kGrayRows);
    for (int Y = Y0; Y < Y1; ++Y) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
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
                    _Float16 h[4];
                    if ((((size_t)tp) & 15) == 0) { const half8 u0 = *(const half8*)tp, u1 = *(const half8*)(tp + 2); h[0] = u0[1]; h[1] = u0[5]; h[2] = u1[1]; h[3] = u1[5]; }
                    else { h[0] = tp[0][1]; h[1] = tp[1][1]; h[2] = tp[2][1]; h[3] = tp[3][1]; }
                    const bool wl = ox > 0, wt = oy > 0 && ly < p.ovy, wr = ox + rw < p.outW, wb = oy + rh < p.outH && n - ly < p.ovy;
                    const float fy_t = wt ? p.ramp_y[ly] : 1.f, fy_b = wb ? p.ramp_y[n - ly] : 1.f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float v1 = (float)h[k];
                        if (p.ovx || p.ovy) {
                            const int lk = lx + k;
                            if (wl && lk < p.ovx) { float w = p.ramp_x[lk]; v1 *= w; }
                            if (wt) { v1 *= fy_t; }
                            if (wr && n - lk < p.ovx) { float w = p.ramp_x[n - lk]; v1 *= w; }
                            if (wb) { v1 *= fy_b; }
                        }
                        acc[k] += v1;
                    }
                }
            }
        } else {
            for (int k = 0; k < np; ++k) {
                float r, b;
                compose_pixel_sums<P>(p, tiles, X + k, Y, r, acc[k], b);
            }
        }
        uint8_t* row = p.dst + (size_t)Y * p.dst_step;
        if (!p.deep) {
            uint8_t* d = row + X;
            unsigned q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = q8(acc[k]);
            if (np == 4 && (((size_t)d) & 3) == 0) *(unsigned*)d = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
            else for (int k = 0; k < np; ++k) d[k] = (uint8_t)q[k];
        } else {
            uint16_t* d = (uint16_t*)row + X;
            unsigned q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = q16(acc[k]);
            if (np == 4 && (((size_t)d) & 7) == 0) *(uint2*)d = make_uint2(q[0] | q[1] << 16, q[2] | q[3] << 16);
            else for (int k = 0; k < np; ++k) d[k] = (uint16_t)q[k];
        }
    }
}

// compose_canvas_kernel's mapping (a thread per pixel along a row, a workgroup row per canvas row) writing the green sums alone: the plane compose_canvas_kernel
// puts at canvas[1] for the frame B = G = R
template <typename P>
__global__ __launch_bounds__(256) void compose_canvas_gray_kernel(const ComposeParams p, float* canvas) {
    const int X = blockIdx.x * 256 + threadIdx.x;
    if (X >= p.outW) return;
    for (int Y = blockIdx.y; Y < p.outH; Y += gridDim.y) {
        float r, g, b;
        compose_pixel_sums<P>(p, (const P*)p.tiles, X, Y, r, g, b);
        canvas[(size_t)Y * p.outW + X] = g;
    }
}

// resample_kernel (k_resample.hip) over one plane: the same output tile per workgroup, the same tap tables, pass 1 horizontally from the canvas into LDS, pass 2
// vertically out of LDS with a thread per four pixels of a row, the plane accumulated with resample_kernel's expressions in its tap order.
// LDS: [rows_max][64] fp32; at a factor of 4 with bicubic taps rows_max <= 78: 19.5 KiB.  Banks: a row is 64 dwords, one per bank; pass 1 stores dword c of a row
// from lane c, pass 2 reads 16 bytes per lane of rows that are whole multiples of the bank count apart - resample_rgba_kernel's pattern with one plane.
// (kRs*: second copies of k_resample.hip's kTR / kTC / kThreads, like q8 / q16 above - a shared device header would have changed that file's translation unit.
//  They must stay in step with it: byte equality with resample_kernel rests on the same tile, the same tap order and the same quantisation.)
constexpr int kRsRows = kResampleRows, kRsCols = kResampleCols, kRsThreads = 256;
static_assert(kRsCols == 64 && kRsRows * (kRsCols / 4) == kRsThreads, "pass 2 maps one thread to four pixels of the tile");

__global__ __launch_bounds__(kRsThreads) void resample_gray_kernel(const ResampleGrayParams p) {
    extern __shared__ float h[];                                          // [rows_max][kRsCols]
    const int ox0 = blockIdx.x * kRsCols, oy0 = blockIdx.y * kRsRows;
    const int tw = min(kRsCols, p.outW - ox0), th = min(kRsRows, p.outH - oy0);
    const int r0 = p.fy[oy0];
    const int nr = min(p.inH, p.fy[oy0 + th - 1] + p.ky) - r0;           // <= rows_max (resample_rows_max)
    // pass 1: input rows [r0, r0 + nr) filtered horizontally onto the tile's output columns
    for (int i = threadIdx.x; i < nr * kRsCols; i += kRsThreads) {
        const int r = i / kRsCols, c = i % kRsCols;
        float a1 = 0.f;
        if (c < tw) {
            const int X = ox0 + c, f = p.fx[X];
            const int n = min(p.kx, p.inW - f);
            const float* w = p.wx + (size_t)X * p.kx;
            const float* s = p.canvas + (size_t)(r0 + r) * p.inW + f;
            for (int k = 0; k < n; ++k) {
                const float wk = w[k];
                a1 += wk * s[k];
            }
        }
        h[r * kRsCols + c] = a1;
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
    float4v a1 = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < n; ++k) {
        const float wk = w[k];
        const int r = f - r0 + k;
        a1 += wk * *(const float4v*)&h[r * kRsCols + 4 * cg];
    }
    uint8_t* row = p.dst + (size_t)Y * p.dst_step;
    if (!p.deep) {
        uint8_t* d = row + X;
        unsigned q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = q8(a1[k]);
        if (np == 4 && (((size_t)d) & 3) == 0) *(unsigned*)d = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
        else for (int k = 0; k < np; ++k) d[k] = (uint8_t)q[k];
    } else {
        uint16_t* d = (uint16_t*)row + X;
        unsigned q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = q16(a1[k]);
        if (np == 4 && (((size_t)d) & 7) == 0) *(uint2*)d = make_uint2(q[0] | q[1] << 16, q[2] | q[3] << 16);
        else for (int k = 0; k < np; ++k) d[k] = (uint16_t)q[k];
    }
}

inline unsigned grid_for(long total) { long g = (total + 255) / 256; return (unsigned)(g > 8192 ? 8192 : (g < 1 ? 1 : g)); }

// a frame of one sample per pixel whose rows hold `cols` samples of `deep ? 2 : 1` bytes, 16-bit samples 2-byte aligned
inline bool plane_ok(const void* base, size_t step, int cols, int deep) {
    const size_t bps = deep ? 2 : 1;
    return base && step >= (size_t)cols * bps && (!deep || ((((size_t)base) | step) & 1) == 0);
}

}  // namespace

hipError_t launch_gather_gray(const GatherGrayParams& p, hipStream_t s) {
    if (p.rows <= 0 || p.cols <= 0 || !plane_ok(p.frame, p.step, p.cols, p.deep)) return hipErrorInvalidValue;
    const dim3 grid(grid_for((long)p.B * p.T * p.T));
    if (p.fp32) hipLaunchKernelGGL(gather_gray_kernel<float4v>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(gather_gray_kernel<half4>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_compose_gray(const ComposeParams& p, hipStream_t s) {
    if (p.outW <= 0 || p.outH <= 0) return hipSuccess;
    if (!plane_ok(p.dst, p.dst_step, p.outW, p.deep)) return hipErrorInvalidValue;
    const int gw = (p.outW + 3) / 4;
    const dim3 grid((unsigned)((gw + kGrayThreads - 1) / kGrayThreads), (unsigned)((p.outH + kGrayRows - 1) / kGrayRows));
    if (p.fp32) hipLaunchKernelGGL(compose_gray_kernel<float4v>, grid, dim3(kGrayThreads), 0, s, p);
    else hipLaunchKernelGGL(compose_gray_kernel<half4>, grid, dim3(kGrayThreads), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_compose_canvas_gray(const ComposeParams& p, float* canvas, hipStream_t s) {
    if (p.outW <= 0 || p.outH <= 0) return hipSuccess;
    if (!canvas) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.outW + 255) / 256), (unsigned)(p.outH < 65535 ? p.outH : 65535));
    if (p.fp32) hipLaunchKernelGGL(compose_canvas_gray_kernel<float4v>, grid, dim3(256), 0, s, p, canvas);
    else hipLaunchKernelGGL(compose_canvas_gray_kernel<half4>, grid, dim3(256), 0, s, p, canvas);
    return hipGetLastError();
}
hipError_t launch_resample_gray(const ResampleGrayParams& p, hipStream_t s) {
    if (p.outW <= 0 || p.outH <= 0) return hipSuccess;
    constexpr int kMaxRows = 104;                                        // as launch_resample: factor 4, bicubic is 78 (26 KiB here: no opt-in to large LDS needed)
    if (p.rows_max <= 0 || p.rows_max > kMaxRows || !p.canvas || !plane_ok(p.dst, p.dst_step, p.outW, p.deep)) return hipErrorInvalidValue;
    const int lds = p.rows_max * kRsCols * (int)sizeof(float);
    const dim3 grid((unsigned)((p.outW + kRsCols - 1) / kRsCols), (unsigned)((p.outH + kRsRows - 1) / kRsRows));
    hipLaunchKernelGGL(resample_gray_kernel, grid, dim3(kRsThreads), lds, s, p);
    return hipGetLastError();
}

}  // namespace w2x
