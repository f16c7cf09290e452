// RGBA frames (renderRgba): the three kernels that stand beside gather / compose of k_prepost.hip, which stay as they are.
//   alpha_bleed : uploaded u8 BGRA frame -> u8 BGR frame + u8 alpha plane, the colours of the visible pixels (alpha > 0) spread `radius` pixels outward
//                 under the transparent ones, all iterations in one launch; max(A) and max(255 - A) of the frame reduced into two device words.
//   gather_rgba : gather_kernel (gather_loop, pixel_device.h) with a slot that says which plane it reads: the BGR frame (the bytes of gather_kernel) or
//                 the alpha plane as a gray pixel.
//   compose_rgba: per output pixel compose_pixel_sums (prepost_device.h, the code compose_kernel inlines) over the colour tiles and over the alpha
//                 tiles, quantised alike, stored as one BGRA dword.
// Resized RGBA frames (renderRgbaResized), further down: compose_canvas_rgba (the same sums left unquantised as four fp32 planes) and
// resample_rgba (k_resample.hip's resize over the four planes - the shared passes of pixel_device.h -, stored as BGRA dwords).
#include "kernels.h"
#include "pixel_device.h"

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

// kWrap (EdgeMode::Wrap): the halo outside the frame holds the frame's periodic continuation (edge_src<kEdgeWrap>) instead of the outside flag, so a
// pixel's eight neighbours always exist and colour spreads across the joint; the iterations are the same.  false: the kernel it always was.
template <bool kWrap = false>
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
            int fy = y0 - R + ly, fx = x0 - R + lx;
            if constexpr (kWrap) { fy = edge_src<kEdgeWrap>(fy, p.rows); fx = edge_src<kEdgeWrap>(fx, p.cols); }
            unsigned v = kOutside;
            if (kWrap || (fy >= 0 && fy < p.rows && fx >= 0 && fx < p.cols)) {
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

// gather_kernel's indexing (gather_loop: replicate padding, the TTA source map) on the plane the slot names
template <typename P, int E = kEdgeReplicate>
__global__ __launch_bounds__(kGatherThreads) void gather_rgba_kernel(const GatherRgbaParams p) {
    const float inv255 = (float)(1.0 / 255.0);
    gather_loop<P, E>(p.slots, p.B, p.T, p.rows, p.cols, p.out, [&](const TileSlot& sl, int fy, int fx) {
        if (sl.valid == kSlotAlpha) {
            const float a = (float)p.alpha[(size_t)fy * p.alpha_step + fx] * inv255;
            return make_px<P>(a, a, a);
        }
        const uint8_t* px = p.bgr + (size_t)fy * p.bgr_step + (size_t)fx * 3;
        return make_px<P>((float)px[2] * inv255, (float)px[1] * inv255, (float)px[0] * inv255);
    });
}

// A thread per pixel along a row (a wave stores 256 contiguous bytes), a workgroup row per output row.
// M: kDitherNone - no further argument - is the kernel above; a dithered mode takes its DitherArgs behind p (dither_of).  The colour channels alone
// are dithered; alpha keeps sat(rint(x * 255)) - an opaque cut-out stays 255 everywhere.
template <typename P, int M = kDitherNone, typename... D>
__global__ __launch_bounds__(256) void compose_rgba_kernel(const ComposeRgbaParams p, const D... dzs) {
    static_assert(dither_pack_ok<M, D...>, "kDitherNone: no argument; else one DitherArgs");
    const DitherArgs& dz = dither_of(dzs...);
    const ComposeParams& c = p.c;
    const int X = blockIdx.x * 256 + threadIdx.x;
    if (X >= c.outW) return;
    for (int Y = blockIdx.y; Y < c.outH; Y += gridDim.y) {
        float r, g, b;
        compose_pixel_sums<P>(c, (const P*)c.tiles, X, Y, r, g, b);
        const unsigned bgr = quantize_bgr_at<M>(r, g, b, dz, X, Y);
        unsigned A = p.alpha_value;
        if (p.alpha_tiles) {
            compose_pixel_sums<P>(c, (const P*)p.alpha_tiles, X, Y, r, g, b);
            A = (quantize_bgr(0.f, g, 0.f) >> 8) & 255u;
        }
        ((unsigned*)(c.dst + (size_t)Y * c.dst_step))[X] = bgr | A << 24;
    }
}

// ---- resized RGBA frames (renderRgbaResized)
//
// compose_canvas_kernel's thread and grid mapping (a thread per pixel along a row, a workgroup row per canvas row) over both tile sets: the unquantised sums
// of the colour tiles as planes R, G, B and the green sum of the alpha tiles as plane A.
// L: empty - the kernel above -, or one LightArgs: the colour planes hold decode(sat01(sum)); plane A, coverage, is never decoded
template <typename P, typename... L>
__global__ __launch_bounds__(256) void compose_canvas_rgba_kernel(const ComposeCanvasRgbaParams p, const L... ls) {
    static_assert(dither_pack_ok<kDitherNone, L...>, "no argument, or one LightArgs");
    constexpr bool kLin = light_on<L...>;
    const LightArgs& lz = light_of(ls...);
    const ComposeParams& c = p.c;
    const int X = blockIdx.x * 256 + threadIdx.x;
    if (X >= c.outW) return;
    const size_t plane = (size_t)c.outW * c.outH;
    for (int Y = blockIdx.y; Y < c.outH; Y += gridDim.y) {
        float r, g, b;
        compose_pixel_sums<P>(c, (const P*)c.tiles, X, Y, r, g, b);
        const size_t i = (size_t)Y * c.outW + X;
        p.canvas[i] = light_canvas<kLin>(lz, r); p.canvas[plane + i] = light_canvas<kLin>(lz, g); p.canvas[2 * plane + i] = light_canvas<kLin>(lz, b);
        if (p.alpha_tiles) {
            compose_pixel_sums<P>(c, (const P*)p.alpha_tiles, X, Y, r, g, b);
            p.canvas[3 * plane + i] = g;
        }
    }
}

// resample_kernel (k_resample.hip) over four planes: resample_pass1 / resample_pass2 (pixel_device.h) at NP = 4 - NP = 3 when the alpha plane is uniform and not
// filtered -, so a plane's value is the one resample_kernel gives for the same canvas plane, and the quantisation is its sat(rint(x * 255)).
// LDS: [NP][rows_max][64] fp32.  At a factor of 4 with bicubic taps rows_max <= 78: 4 * 78 * 256 B = 78 KiB, two workgroups per CU in its 160 KiB (NP = 3:
// resample_kernel's 58.5 KiB).  Banks: a row is 64 dwords, one per bank.  Pass 1 stores dword c of a row from lane c: a wave covers one whole row, every bank
// once.  Pass 2 reads 16 bytes per lane (ds_read_b128, served in four groups of 16 lanes that are not contiguous: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}
// and the same in the upper half wave).  Lanes 0-15 of a half wave are the 16 column groups of one output row, lanes 16-31 those of the next, so a group
// holds column groups 0-3 and 12-15 of one output row - dwords 0-15 and 48-63 of its LDS row - and column groups 4-11 of the other - dwords 16-47 of that
// row's LDS row (or the complement).  The two LDS rows may differ (each output row's taps start where they start), but a row is exactly 64 dwords, so the
// bank is the dword's column: the group touches every bank once.
// Stores: the thread's four BGRA dwords as one 16-byte store where the address is 16-byte aligned (dst is packed: the pitch outW * 4 is a multiple of 16
// only when outW % 4 == 0, so this is decided per row from the address), dword by dword otherwise and for the 1 - 3 pixels the right edge leaves.
// M: as above - colour dithered at (X + q, Y), alpha rounded to nearest.
template <bool kAlpha, int M = kDitherNone, typename... D>
__global__ __launch_bounds__(kRsThreads) void resample_rgba_kernel(const ResampleRgbaParams p, const D... dzs) {
    static_assert(dither_pack_ok<M, D...>, "kDitherNone: no DitherArgs, else one; then one LightArgs or none");
    const DitherArgs& dz = dither_of(dzs...);
    constexpr int NP = kAlpha ? 4 : 3;
    constexpr bool kEdge = edge_on<D...>;                                 // 
    extern __shared__ float rs_lds[];
    const int r0 = resample_pass1<NP, kEdge>(p, rs_lds, edge_of(dzs...).mode);
    __syncthreads();
    float4v a[NP];
    int X, Y, np;
    if (!resample_pass2<NP, kEdge>(p, rs_lds, r0, a, X, Y, np)) return;
    if constexpr (light_on<D...>) {                                       // (the colour is encoded, alpha - a[3] - is not)
        const LightArgs& lz = light_of(dzs...);
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) a[c][q] = light_out<true>(lz, a[c][q]);
    }
    unsigned px[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                                         // b | g << 8 | r << 16 | a << 24
        if constexpr (M == kDitherNone)
            px[q] = quant(a[2][q], 255.f, 255) | quant(a[1][q], 255.f, 255) << 8 | quant(a[0][q], 255.f, 255) << 16 | (kAlpha ? quant(a[NP - 1][q], 255.f, 255) : p.alpha_value) << 24;
        else
            px[q] = quantize_bgr_at<M>(a[0][q], a[1][q], a[2][q], dz, X + q, Y) | (kAlpha ? quant(a[NP - 1][q], 255.f, 255) : p.alpha_value) << 24;
    }
    unsigned* d = (unsigned*)(p.dst + (size_t)Y * p.dst_step) + X;
    if (np == 4 && (((size_t)d) & 15) == 0) *(uint4*)d = make_uint4(px[0], px[1], px[2], px[3]);
    else for (int q = 0; q < np; ++q) d[q] = px[q];
}

}  // namespace

hipError_t launch_alpha_bleed(const AlphaBleedParams& p, hipStream_t s, bool wrap) {
    if (p.rows <= 0 || p.cols <= 0 || p.radius < 0 || p.radius > kBleedMaxRadius) return hipErrorInvalidValue;
    const int R = p.radius;
    const size_t lds = R > 0 ? (size_t)2 * (kBleedTileW + 2 * R) * (kBleedTileH + 2 * R) * sizeof(unsigned) : 0;
    const dim3 grid((unsigned)((p.cols + kBleedTileW - 1) / kBleedTileW), (unsigned)((p.rows + kBleedTileH - 1) / kBleedTileH));
    if (wrap) hipLaunchKernelGGL(alpha_bleed_kernel<true>, grid, dim3(256), lds, s, p);
    else hipLaunchKernelGGL(alpha_bleed_kernel<false>, grid, dim3(256), lds, s, p);
    return hipGetLastError();
}
hipError_t launch_gather_rgba(const GatherRgbaParams& p, hipStream_t s, int edge) {
    const dim3 grid(grid_for((long)p.B * p.T * p.T));
    return for_edge(edge, [&](auto e) {
        constexpr int E = decltype(e)::value;
        if (p.fp32) hipLaunchKernelGGL((gather_rgba_kernel<float4v, E>), grid, dim3(kGatherThreads), 0, s, p);
        else hipLaunchKernelGGL((gather_rgba_kernel<half4, E>), grid, dim3(kGatherThreads), 0, s, p);
        return hipGetLastError();
    });
}
hipError_t launch_compose_rgba(const ComposeRgbaParams& p, hipStream_t s, const DitherArgs& d) {
    if (p.c.outW <= 0 || p.c.outH <= 0) return hipSuccess;
    if (!dither_args_ok(d)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.c.outW + 255) / 256), (unsigned)(p.c.outH < 65535 ? p.c.outH : 65535));
    if (d.mode != kDitherNone) return for_dither(d, [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (p.c.fp32) hipLaunchKernelGGL((compose_rgba_kernel<float4v, M, DitherArgs>), grid, dim3(256), 0, s, p, d);
        else hipLaunchKernelGGL((compose_rgba_kernel<half4, M, DitherArgs>), grid, dim3(256), 0, s, p, d);
        return hipGetLastError();
    });
    if (p.c.fp32) hipLaunchKernelGGL(compose_rgba_kernel<float4v>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(compose_rgba_kernel<half4>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_compose_canvas_rgba(const ComposeCanvasRgbaParams& p, hipStream_t s, const LightArgs& l) {
    if (p.c.outW <= 0 || p.c.outH <= 0) return hipSuccess;
    if (!p.canvas || !light_args_ok(l)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.c.outW + 255) / 256), (unsigned)(p.c.outH < 65535 ? p.c.outH : 65535));
    if (l.mode != kLightGamma) {
        if (p.c.fp32) hipLaunchKernelGGL((compose_canvas_rgba_kernel<float4v, LightArgs>), grid, dim3(256), 0, s, p, l);
        else hipLaunchKernelGGL((compose_canvas_rgba_kernel<half4, LightArgs>), grid, dim3(256), 0, s, p, l);
        return hipGetLastError();
    }
    if (p.c.fp32) hipLaunchKernelGGL(compose_canvas_rgba_kernel<float4v>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(compose_canvas_rgba_kernel<half4>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_resample_rgba(const ResampleRgbaParams& p, hipStream_t s, const DitherArgs& d, const LightArgs& l, const EdgeArgs& e) {
    if (p.outW <= 0 || p.outH <= 0) return hipSuccess;
    if ((p.dst_step & 3) || p.dst_step < (size_t)p.outW * 4 || (((size_t)p.dst) & 3)) return hipErrorInvalidValue;
    return for_modes(d, l, e, [&](auto m, const auto&... extra) {
        constexpr int M = decltype(m)::value;
        static unsigned lds_done[2] = {0, 0};                            // (a pair per instantiation of this lambda's body)
        if (p.uniform) return launch_resample_tiles(resample_rgba_kernel<false, M, std::decay_t<decltype(extra)>...>, 3 * kRsCols, p.rows_max, lds_done[0], p.outW, p.outH, s, p, extra...);
        return launch_resample_tiles(resample_rgba_kernel<true, M, std::decay_t<decltype(extra)>...>, 4 * kRsCols, p.rows_max, lds_done[1], p.outW, p.outH, s, p, extra...);
    });
}

}  // namespace w2x
