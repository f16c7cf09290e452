// RGBA frames (renderRgba): the three kernels that stand beside gather / compose of k_prepost.hip, which stay as they are.
//   alpha_bleed : uploaded u8 BGRA frame -> u8 BGR frame + u8 alpha plane, the colours of the visible pixels (alpha > 0) spread `radius` pixels outward
//                 under the transparent ones, all iterations in one launch; max(A) and max(255 - A) of the frame reduced into two device words.
//   gather_rgba : gather_kernel with a slot that says which plane it reads: the BGR frame (the bytes of gather_kernel) or the alpha plane as a gray pixel.
//   compose_rgba: per output pixel compose_pixel_sums (prepost_device.h, the code compose_kernel inlines) over the colour tiles and over the alpha
//                 tiles, quantised alike, stored as one BGRA dword.
#include "kernels.h"
#include "prepost_device.h"

namespace w2x {
namespace {

// The bleed (integer, exact; tiles.h alpha_bleed is the host statement): known_0 = A > 0; in iteration it = 1..R every pixel unknown in state it - 1 with
// n > 0 known neighbours among its eight (inside the frame) becomes their mean, (sum + (n >> 1)) / n per channel, and known; Jacobi - every read is of
// state it - 1.  A pixel after R iterations depends on the radius-R neighbourhood at iteration 0 only, so a workgroup that holds its tile plus a halo of
// R pixels computes its tile exactly: iteration it is evaluated on the tile grown by R - it pixels, which reads state it - 1 on the tile grown by
// R - it + 1, all of it written the iteration before.
// Workgroup = 256 threads on a tile of 64 x 32 output pixels.  LDS: two buffers (state it - 1, state it) of (64 + 2R) x (32 + 2R) packed dwords
// B | G << 8 | R << 16 | flag << 24 (flag 0 unknown, 1 known, 2 outside the frame: never known, never filled).  R = 16: 2 x 96 x 64 x 4 B = 48 KiB, three
// workgroups (12 waves) in a CU's 160 KiB; R = 8: 2 x 80 x 48 x 4 B = 30 KiB, five; a 1920 x 1080 frame is 30 x 34 = 1020 workgroups over 256 CUs.  Rows of
// the tile are 64 dwords wide plus the halo: the eight neighbour reads of a wave walk consecutive dwords (no bank conflict).  A wider tile would lower
// the halo's share (at R = 16 the LDS region is 3x the tile) but leave fewer workgroups per CU to hide the frame read behind; the iterations stop at the
// first one that changes nothing in the workgroup's region (an opaque tile runs one).
// Output: a thread takes four consecutive pixels: 12 BGR bytes as three dwords and 4 alpha bytes as one where the row address allows, bytes otherwise.
// radius 0: no LDS, the planes are split straight from the frame.
constexpr unsigned kKnown = 1u << 24, kOutside = 2u << 24;

__global__ __launch_bounds__(256) void alpha_bleed_kernel(const AlphaBleedParams p) {
    extern __shared__ unsigned bleed_lds[];
    __shared__ unsigned wg_max[2];
    const int R = p.radius, tid = threadIdx.x;
    const int LW = kBleedTileW + 2 * R, LH = kBleedTileH + 2 * R;
    const int x0 = blockIdx.x * kBleedTileW, y0 = blockIdx.y * kBleedTileH;
    unsigned* cur = bleed_lds;
    unsigned* nxt = bleed_lds + LW * LH;
    if (tid < 2) wg_max[tid] = 0u;
    if (R > 0) {
        for (int i = tid; i < LW * LH; i += 256) {
            const int ly = i / LW, lx = i - ly * LW;
            const int fy = y0 - R + ly, fx = x0 - R + lx;
            unsigned v = kOutside;
            if (fy >= 0 && fy < p.rows && fx >= 0 && fx < p.cols) {
                const unsigned px = ((const unsigned*)(p.bgra + (size_t)fy * p.step))[fx];
                v = (px & 0xFFFFFFu) | ((px >> 24) ? kKnown : 0u);
            }
            cur[i] = v;
        }
        __syncthreads();
        for (int it = 1; it <= R; ++it) {
            const int w = LW - 2 * it, h = LH - 2 * it;
            int changed = 0;
            for (int i = tid; i < w * h; i += 256) {
                const int ry = i / w;
                const int idx = (it + ry) * LW + it + (i - ry * w);
                unsigned v = cur[idx];
                if ((v >> 24) == 0u) {
                    unsigned n = 0, sb = 0, sg = 0, sr = 0;
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            if (dy == 0 && dx == 0) continue;
                            const unsigned q = cur[idx + dy * LW + dx];
                            if ((q >> 24) == 1u) { ++n; sb += q & 255u; sg += (q >> 8) & 255u; sr += (q >> 16) & 255u; }
                        }
                    if (n) {
                        const unsigned half = n >> 1;
                        v = (sb + half) / n | ((sg + half) / n) << 8 | ((sr + half) / n) << 16 | kKnown;
                        changed = 1;
                    }
                }
                nxt[idx] = v;
            }
            unsigned* t = cur; cur = nxt; nxt = t;
            if (!__syncthreads_or(changed)) break;      // (also the barrier between state it and state it + 1)
        }
    } else __syncthreads();
    unsigned amax = 0u, imax = 0u;                      // max(A), max(255 - A) over this thread's pixels
    constexpr int kGroups = kBleedTileW / 4;
    for (int g = tid; g < kGroups * kBleedTileH; g += 256) {
        const int gy = g / kGroups, gx = (g - gy * kGroups) * 4;
        const int y = y0 + gy, x = x0 + gx;
        if (y >= p.rows || x >= p.cols) continue;
        const int np = min(4, p.cols - x);
        const unsigned* srow = (const unsigned*)(p.bgra + (size_t)y * p.step) + x;
        unsigned c[4] = {0u, 0u, 0u, 0u}, a[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < np) {
                const unsigned px = srow[k];
                a[k] = px >> 24;
                c[k] = (R > 0 ? cur[(gy + R) * LW + gx + R + k] : px) & 0xFFFFFFu;
                amax = max(amax, a[k]); imax = max(imax, 255u - a[k]);
            }
        uint8_t* d = p.bgr + (size_t)y * p.bgr_step + (size_t)x * 3;
        if (np == 4 && (((size_t)d) & 3) == 0) {
            unsigned* dw = (unsigned*)d;
            dw[0] = c[0] | c[1] << 24;
            dw[1] = c[1] >> 8 | c[2] << 16;
            dw[2] = c[2] >> 16 | c[3] << 8;
        } else {
            for (int k = 0; k < np; ++k) { d[3 * k] = (uint8_t)c[k]; d[3 * k + 1] = (uint8_t)(c[k] >> 8); d[3 * k + 2] = (uint8_t)(c[k] >> 16); }
        }
        uint8_t* da = p.alpha + (size_t)y * p.alpha_step + x;
        if (np == 4 && (((size_t)da) & 3) == 0) *(unsigned*)da = a[0] | a[1] << 8 | a[2] << 16 | a[3] << 24;
        else for (int k = 0; k < np; ++k) da[k] = (uint8_t)a[k];
    }
    // the frame's alpha range: per workgroup in LDS, then one vector atomic per word and workgroup
    atomicMax(&wg_max[0], amax);
    atomicMax(&wg_max[1], imax);
    __syncthreads();
    if (tid < 2) atomicMax(p.minmax + tid, wg_max[tid]);
}

// gather_kernel's indexing (replicate padding, the TTA source map) on the plane the slot names
template <typename P>
__global__ __launch_bounds__(256) void gather_rgba_kernel(const GatherRgbaParams p) {
    const int T = p.T;
    const long total = (long)p.B * T * T;
    const float inv255 = (float)(1.0 / 255.0);
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
            if (sl.valid == kSlotAlpha) {
                const float a = (float)p.alpha[(size_t)fy * p.alpha_step + fx] * inv255;
                v = make_px<P>(a, a, a);
            } else {
                const uint8_t* px = p.bgr + (size_t)fy * p.bgr_step + (size_t)fx * 3;
                v = make_px<P>((float)px[2] * inv255, (float)px[1] * inv255, (float)px[0] * inv255);
            }
        }
        *((P*)p.out + i) = v;
    }
}

// A thread per pixel along a row (a wave stores 256 contiguous bytes), a workgroup row per output row.
template <typename P>
__global__ __launch_bounds__(256) void compose_rgba_kernel(const ComposeRgbaParams p) {
    const ComposeParams& c = p.c;
    const int X = blockIdx.x * 256 + threadIdx.x;
    if (X >= c.outW) return;
    for (int Y = blockIdx.y; Y < c.outH; Y += gridDim.y) {
        float r, g, b;
        compose_pixel_sums<P>(c, (const P*)c.tiles, X, Y, r, g, b);
        const unsigned bgr = quantize_bgr(r, g, b);
        unsigned A = p.alpha_value;
        if (p.alpha_tiles) {
            compose_pixel_sums<P>(c, (const P*)p.alpha_tiles, X, Y, r, g, b);
            A = (quantize_bgr(0.f, g, 0.f) >> 8) & 255u;
        }
        ((unsigned*)(c.dst + (size_t)Y * c.dst_step))[X] = bgr | A << 24;
    }
}

inline unsigned grid_for(long total) { long g = (total + 255) / 256; return (unsigned)(g > 8192 ? 8192 : (g < 1 ? 1 : g)); }

}  // namespace

hipError_t launch_alpha_bleed(const AlphaBleedParams& p, hipStream_t s) {
    if (p.rows <= 0 || p.cols <= 0 || p.radius < 0 || p.radius > kBleedMaxRadius) return hipErrorInvalidValue;
    const int R = p.radius;
    const size_t lds = R > 0 ? (size_t)2 * (kBleedTileW + 2 * R) * (kBleedTileH + 2 * R) * sizeof(unsigned) : 0;
    const dim3 grid((unsigned)((p.cols + kBleedTileW - 1) / kBleedTileW), (unsigned)((p.rows + kBleedTileH - 1) / kBleedTileH));
    hipLaunchKernelGGL(alpha_bleed_kernel, grid, dim3(256), lds, s, p);
    return hipGetLastError();
}
hipError_t launch_gather_rgba(const GatherRgbaParams& p, hipStream_t s) {
    const dim3 grid(grid_for((long)p.B * p.T * p.T));
    if (p.fp32) hipLaunchKernelGGL(gather_rgba_kernel<float4v>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(gather_rgba_kernel<half4>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_compose_rgba(const ComposeRgbaParams& p, hipStream_t s) {
    if (p.c.outW <= 0 || p.c.outH <= 0) return hipSuccess;
    const dim3 grid((unsigned)((p.c.outW + 255) / 256), (unsigned)(p.c.outH < 65535 ? p.c.outH : 65535));
    if (p.c.fp32) hipLaunchKernelGGL(compose_rgba_kernel<float4v>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(compose_rgba_kernel<half4>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace w2x
