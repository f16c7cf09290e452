// Frames of planes: NP planes of one sample type S in, NP planes out.  NP = 3 is a planar RGB frame (renderPlanar: R, G, B at 8, 10, 12, 16
// bits or float32, the two sides independent), NP = 1 a gray frame (renderGray: 8 or 16 bits), which is the planar frame R = G = B = g with the two planes
// nobody looks at left out.  The result is defined by the BGR path - at 8 / 8 and 16 / 16 bits the planes of render() of the interleaved frame, gray: its green
// channel, byte for byte - and the kernels here are the BGR kernels of k_prepost.hip / k_resample.hip reading and writing planes; those files stay as they
// are, and the bodies copied from them are written once in pixel_device.h.
//   gather_planes      : gather_kernel's indexing (gather_loop); the tile pixel is make_px(r, g, b) - NP = 1: (a, a, a, 0) -, a sample
//                        min(code, maxcode) * fl32(1 / maxcode) (8 / 16 bits: gather_kernel's fl32(1/255) / fl32(1/65535)); float: min(max(x, 0), 1), NaN -> 0.
//   compose_planes     : compose_kernel's launch shape and four-pixel fast path (compose_quad_sums) - at every output depth: the fast path only changes how the
//                        sums are fetched -, elsewhere compose_pixel_sums (prepost_device.h, the code compose_kernel inlines); NP = 1 keeps the green sum;
//                        integer sat(rint(x * maxcode)), float min(max(x, 0), 1); four samples leave as one store per plane (store4).
//   compose_canvas_gray: compose_canvas_kernel's mapping, the green sums unquantised as ONE fp32 plane (resized gray frames; planar frames use
//                        compose_canvas_kernel's own canvas).
//   resample_planes    : resample_kernel over that canvas (resample_pass1 / resample_pass2), the NP accumulators stored like compose_planes'.
#include "kernels.h"
#include "pixel_device.h"

namespace w2x {
namespace {

template <typename P, typename S, int NP, int E = kEdgeReplicate>
__global__ __launch_bounds__(kGatherThreads) void gather_planes_kernel(const GatherPlanarParams p, unsigned maxcode, float inv) {
    gather_loop<P, E>(p.slots, p.B, p.T, p.src.rows, p.src.cols, p.out, [&](const TileSlot&, int fy, int fx) {
        float a[NP];
#pragma unroll
        for (int c = 0; c < NP; ++c) a[c] = load_sample<S>(p.src.p[c] + (size_t)fy * p.src.step[c], fx, maxcode, inv);
        return make_px<P>(a[0], a[NP / 2], a[NP - 1]);             // NP = 3: (r, g, b); NP = 1: (a, a, a)
    });
}

// compose_kernel with NP planes behind it.  A thread owns four consecutive pixels of a row and walks kComposeRows rows; what depends on the column only is computed
// once per thread.  Where the four share their covering tiles, lie inside each of them and no TTA is involved, the sums come from compose_quad_sums - at every
// output depth, since the fast path is about how the sums are fetched and not about what is stored.  The whole canvas: these frames take no strips or shards.
// M: kDitherNone - no further argument - is the kernel above; a dithered mode takes its DitherArgs behind maxcode (dither_of).  A gray frame's one
// plane has plane index 1.
template <typename P, typename S, int NP, int M = kDitherNone, typename... D>
__global__ __launch_bounds__(kComposeThreads) void compose_planes_kernel(const ComposePlanarParams q, float scale, int maxcode, const D... dzs) {
    static_assert(dither_pack_ok<M, D...>, "kDitherNone: no argument; else one DitherArgs");
    const DitherArgs& dz = dither_of(dzs...);
    constexpr bool kHalf = sizeof(P) == 8;
    const ComposeParams& p = q.c;
    const int gw = (p.outW + 3) >> 2;
    const int xg = blockIdx.x * kComposeThreads + threadIdx.x;
    if (xg >= gw) return;
    const P* tiles = (const P*)p.tiles;
    const int To = p.To;
    const int X = 4 * xg;
    const int np = min(4, p.outW - X);
    int a0 = X - To + 1; a0 = a0 <= 0 ? 0 : (a0 + p.stride_x - 1) / p.stride_x;
    int b0 = X + 3 - To + 1; b0 = b0 <= 0 ? 0 : (b0 + p.stride_x - 1) / p.stride_x;
    const int a1 = min(p.nx - 1, X / p.stride_x), b1 = min(p.nx - 1, (X + 3) / p.stride_x);
    const bool fast = kHalf && np == 4 && !p.tta && a0 == b0 && a1 == b1;
    const int Y0 = blockIdx.y * kComposeRows, Y1 = min(p.outH, Y0 + kComposeRows);
    for (int Y = Y0; Y < Y1; ++Y) {
        float acc[NP][4] = {};                                     // [plane][pixel]
        if (fast) compose_quad_sums<NP>(p, X, Y, a0, a1, acc);
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < np) {
                float r, b;
                if constexpr (NP == 3) compose_pixel_sums<P>(p, tiles, X + k, Y, acc[0][k], acc[1][k], acc[2][k]);
                else compose_pixel_sums<P>(p, tiles, X + k, Y, r, acc[0][k], b);
            }
        }
#pragma unroll
        for (int c = 0; c < NP; ++c) store4<S, M>(q.dst.p[c] + (size_t)Y * q.dst.step[c], X, np, acc[c], scale, maxcode, dz, NP == 1 ? 1 : c, Y);
    }
}

// compose_canvas_kernel's mapping (a thread per pixel along a row, a workgroup row per canvas row) writing the green sums alone: the plane compose_canvas_kernel
// puts at canvas[1] for the frame B = G = R
// L: empty - the kernel above -, or one LightArgs: the plane holds decode(sat01(g))
template <typename P, typename... L>
__global__ __launch_bounds__(256) void compose_canvas_gray_kernel(const ComposeParams p, float* canvas, const L... ls) {
    static_assert(dither_pack_ok<kDitherNone, L...>, "no argument, or one LightArgs");
    const int X = blockIdx.x * 256 + threadIdx.x;
    if (X >= p.outW) return;
    for (int Y = blockIdx.y; Y < p.outH; Y += gridDim.y) {
        float r, g, b;
        compose_pixel_sums<P>(p, (const P*)p.tiles, X, Y, r, g, b);
        canvas[(size_t)Y * p.outW + X] = light_canvas<light_on<L...>>(light_of(ls...), g);
    }
}

// resample_kernel (k_resample.hip) with NP planes behind it.  LDS: [NP][rows_max][64] fp32 - NP = 3: resample_kernel's (58.5 KiB at a factor of 4 with bicubic
// taps), NP = 1: 19.5 KiB.
template <typename S, int NP, int M = kDitherNone, typename... D>
__global__ __launch_bounds__(kRsThreads) void resample_planes_kernel(const ResamplePlanarParams p, float scale, int maxcode, const D... dzs) {
    static_assert(dither_pack_ok<M, D...>, "kDitherNone: no DitherArgs, else one; then one LightArgs or none");
    const DitherArgs& dz = dither_of(dzs...);
    constexpr bool kLin = light_on<D...>;                                 // 
    const LightArgs& lz = light_of(dzs...);
    constexpr bool kEdge = edge_on<D...>;                                 // 
    extern __shared__ float h[];
    const int r0 = resample_pass1<NP, kEdge>(p, h, edge_of(dzs...).mode);
    __syncthreads();
    float4v a[NP];
    int X, Y, np;
    if (!resample_pass2<NP, kEdge>(p, h, r0, a, X, Y, np)) return;
#pragma unroll
    for (int c = 0; c < NP; ++c) {
        const float v[4] = {light_out<kLin>(lz, a[c][0]), light_out<kLin>(lz, a[c][1]), light_out<kLin>(lz, a[c][2]), light_out<kLin>(lz, a[c][3])};
        store4<S, M>(p.dst.p[c] + (size_t)Y * p.dst.step[c], X, np, v, scale, maxcode, dz, NP == 1 ? 1 : c, Y);
    }
}

// one or three planes of rows x cols samples of `bits` (one plane: 8 or 16 as gray frames have them, never float), every step holding a row, u16 / f32 samples
// aligned to their size
inline bool planes_ok(const PlanarPlanes& f, int rows, int cols) {
    if (!planar_bits_ok(f.bits) || (f.n != 3 && (f.n != 1 || f.bits == 32)) || f.rows != rows || f.cols != cols || rows <= 0 || cols <= 0) return false;
    const size_t bps = planar_sample_bytes(f.bits);
    for (int k = 0; k < f.n; ++k) if (!f.p[k] || f.step[k] < (size_t)cols * bps || ((((size_t)f.p[k]) | f.step[k]) & (bps - 1)) != 0) return false;
    return true;
}
inline int max_code(int bits) { return bits == 32 ? 0 : (1 << bits) - 1; }

// launch(Planes<S, NP>()) for the sample type and plane count of f (planes_ok(f)): NP = 1 exists at U8 and U16
template <typename S, int NP> struct Planes { typedef S Sample; static constexpr int kPlanes = NP; };
template <typename Launch> hipError_t for_planes(const PlanarPlanes& f, Launch launch) {
    if (f.n == 1) return f.bits == 8 ? launch(Planes<U8, 1>()) : launch(Planes<U16, 1>());
    return f.bits == 8 ? launch(Planes<U8, 3>()) : f.bits == 32 ? launch(Planes<F32, 3>()) : launch(Planes<U16, 3>());
}

}  // namespace

hipError_t launch_gather_planar(const GatherPlanarParams& p, hipStream_t s, int edge) {
    if (!planes_ok(p.src, p.src.rows, p.src.cols)) return hipErrorInvalidValue;
    const dim3 grid(grid_for((long)p.B * p.T * p.T));
    const unsigned maxcode = (unsigned)max_code(p.src.bits);
    const float inv = p.src.bits == 32 ? 0.f : (float)(1.0 / (double)maxcode);
    return for_planes(p.src, [&](auto k) {
        typedef typename decltype(k)::Sample S;
        constexpr int NP = decltype(k)::kPlanes;
        return for_edge(edge, [&](auto e) {
            constexpr int E = decltype(e)::value;
            if (p.fp32) hipLaunchKernelGGL((gather_planes_kernel<float4v, S, NP, E>), grid, dim3(kGatherThreads), 0, s, p, maxcode, inv);
            else hipLaunchKernelGGL((gather_planes_kernel<half4, S, NP, E>), grid, dim3(kGatherThreads), 0, s, p, maxcode, inv);
            return hipGetLastError();
        });
    });
}
hipError_t launch_compose_planar(const ComposePlanarParams& p, hipStream_t s, const DitherArgs& d) {
    if (p.c.outW <= 0 || p.c.outH <= 0) return hipSuccess;
    if (!planes_ok(p.dst, p.c.outH, p.c.outW) || !dither_args_ok(d)) return hipErrorInvalidValue;
    const int gw = (p.c.outW + 3) / 4;
    const dim3 grid((unsigned)((gw + kComposeThreads - 1) / kComposeThreads), (unsigned)((p.c.outH + kComposeRows - 1) / kComposeRows));
    const int maxcode = max_code(p.dst.bits);
    const float scale = (float)maxcode;
    return for_planes(p.dst, [&](auto k) {
        typedef typename decltype(k)::Sample S;
        constexpr int NP = decltype(k)::kPlanes;
        if constexpr (!std::is_same<S, F32>::value) {                 // (float samples are never dithered: their one kernel below)
            if (d.mode != kDitherNone) return for_dither(d, [&](auto m) {
                constexpr int M = decltype(m)::value;
                if (p.c.fp32) hipLaunchKernelGGL((compose_planes_kernel<float4v, S, NP, M, DitherArgs>), grid, dim3(kComposeThreads), 0, s, p, scale, maxcode, d);
                else hipLaunchKernelGGL((compose_planes_kernel<half4, S, NP, M, DitherArgs>), grid, dim3(kComposeThreads), 0, s, p, scale, maxcode, d);
                return hipGetLastError();
            });
        }
        if (p.c.fp32) hipLaunchKernelGGL((compose_planes_kernel<float4v, S, NP>), grid, dim3(kComposeThreads), 0, s, p, scale, maxcode);
        else hipLaunchKernelGGL((compose_planes_kernel<half4, S, NP>), grid, dim3(kComposeThreads), 0, s, p, scale, maxcode);
        return hipGetLastError();
    });
}
hipError_t launch_compose_canvas_gray(const ComposeParams& p, float* canvas, hipStream_t s, const LightArgs& l) {
    if (p.outW <= 0 || p.outH <= 0) return hipSuccess;
    if (!canvas || !light_args_ok(l)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.outW + 255) / 256), (unsigned)(p.outH < 65535 ? p.outH : 65535));
    if (l.mode != kLightGamma) {
        if (p.fp32) hipLaunchKernelGGL((compose_canvas_gray_kernel<float4v, LightArgs>), grid, dim3(256), 0, s, p, canvas, l);
        else hipLaunchKernelGGL((compose_canvas_gray_kernel<half4, LightArgs>), grid, dim3(256), 0, s, p, canvas, l);
        return hipGetLastError();
    }
    if (p.fp32) hipLaunchKernelGGL(compose_canvas_gray_kernel<float4v>, grid, dim3(256), 0, s, p, canvas);
    else hipLaunchKernelGGL(compose_canvas_gray_kernel<half4>, grid, dim3(256), 0, s, p, canvas);
    return hipGetLastError();
}
hipError_t launch_resample_planar(const ResamplePlanarParams& p, hipStream_t s, const DitherArgs& d, const LightArgs& l, const EdgeArgs& e) {
    if (p.outW <= 0 || p.outH <= 0) return hipSuccess;
    if (!p.canvas || !planes_ok(p.dst, p.outH, p.outW) || !dither_args_ok(d)) return hipErrorInvalidValue;
    const int maxcode = max_code(p.dst.bits);
    const float scale = (float)maxcode;
    return for_planes(p.dst, [&](auto k) {
        typedef typename decltype(k)::Sample S;
        constexpr int NP = decltype(k)::kPlanes;
        auto go = [&](auto m, const auto&... extra) {
            static unsigned lds_done = 0;                                // (one per instantiation of this lambda's body)
            return launch_resample_tiles(resample_planes_kernel<S, NP, decltype(m)::value, std::decay_t<decltype(extra)>...>, NP * kRsCols, p.rows_max, lds_done, p.outW, p.outH, s, p, scale, maxcode, extra...);
        };
        if constexpr (std::is_same<S, F32>::value) return for_light(l, e, go);   // (float samples are never dithered: no such kernels)
        else return for_modes(d, l, e, go);
    });
}

}  // namespace w2x
