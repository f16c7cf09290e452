// The hand-off between two stages of a chained render (renderChained*): stage k's canvas becomes stage k + 1's source frame without leaving HBM,
// as ONE pixel vector per pixel, [H][W][4] in the tile pixel type of the CONSUMING engine (half4: 8 bytes, float4v: 16 bytes; lane 3 zero).
//   compose_px : compose_planes_kernel's launch shape and four-pixel fast path (compose_quad_sums), elsewhere compose_pixel_sums; a pixel is
//                make_px<Q>(sat01(r), sat01(g), sat01(b)) - the clamp of a float planar destination (store4<F32>), then ONE rounding to the consumer's type,
//                float -> _Float16 to nearest even (make_px), float4v none - stored as one 8- or 16-byte vector.
//   gather_px  : gather_kernel's indexing (gather_loop: slots, pad slots, TTA source map, replicate clamp); the tile pixel is the frame's vector, one load and one
//                store, no conversion and no clamp - the producer has done both.
// The value chain is renderPlanar(dst.bits = 32) followed by renderPlanar(src.bits = 32): sat01 of the fp32 sums, stored as fp32; load_sample<F32> clamps again
// (the identity on [0, 1]) and make_px rounds to the tile type.  Same sums, same clamp, same one rounding: the tiles of the consuming stage are bit-equal.
#include "kernels.h"
#include "pixel_device.h"

namespace w2x {
namespace {

// P: the tile pixel of the producing engine's slab, Q: that of the consuming engine (the frame's vector)
template <typename P, typename Q>
__global__ __launch_bounds__(kComposeThreads) void compose_px_kernel(const ComposeParams p, Q* frame) {
    constexpr bool kHalf = sizeof(P) == 8;
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
        float acc[3][4] = {};                                      // [r, g, b][pixel]
        if (fast) compose_quad_sums<3>(p, X, Y, a0, a1, acc);
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < np) compose_pixel_sums<P>(p, tiles, X + k, Y, acc[0][k], acc[1][k], acc[2][k]);
        }
        Q* const d = frame + (size_t)Y * p.outW + X;
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < np) d[k] = make_px<Q>(sat01(acc[0][k]), sat01(acc[1][k]), sat01(acc[2][k]));
    }
}

template <typename P, int E = kEdgeReplicate>
__global__ __launch_bounds__(kGatherThreads) void gather_px_kernel(const GatherPxParams p) {
    const P* const frame = (const P*)p.frame;
    const int cols = p.cols;
    gather_loop<P, E>(p.slots, p.B, p.T, p.rows, p.cols, p.out, [&](const TileSlot&, int fy, int fx) { return frame[(size_t)fy * cols + fx]; });
}

}  // namespace

hipError_t launch_compose_px(const ComposePxParams& p, hipStream_t s) {
    if (p.c.outW <= 0 || p.c.outH <= 0) return hipSuccess;
    const size_t px = p.frame_fp32 ? 16 : 8;
    if (!p.frame || !p.c.tiles || (((size_t)p.frame) & (px - 1)) != 0) return hipErrorInvalidValue;
    const int gw = (p.c.outW + 3) / 4;
    const dim3 grid((unsigned)((gw + kComposeThreads - 1) / kComposeThreads), (unsigned)((p.c.outH + kComposeRows - 1) / kComposeRows));
    if (p.c.fp32) {
        if (p.frame_fp32) hipLaunchKernelGGL((compose_px_kernel<float4v, float4v>), grid, dim3(kComposeThreads), 0, s, p.c, (float4v*)p.frame);
        else hipLaunchKernelGGL((compose_px_kernel<float4v, half4>), grid, dim3(kComposeThreads), 0, s, p.c, (half4*)p.frame);
    } else {
        if (p.frame_fp32) hipLaunchKernelGGL((compose_px_kernel<half4, float4v>), grid, dim3(kComposeThreads), 0, s, p.c, (float4v*)p.frame);
        else hipLaunchKernelGGL((compose_px_kernel<half4, half4>), grid, dim3(kComposeThreads), 0, s, p.c, (half4*)p.frame);
    }
    return hipGetLastError();
}

hipError_t launch_gather_px(const GatherPxParams& p, hipStream_t s, int edge) {
    if (p.B <= 0) return hipSuccess;
    const size_t px = p.fp32 ? 16 : 8;
    if (!p.frame || !p.out || !p.slots || p.rows <= 0 || p.cols <= 0 || p.T <= 0 || (((size_t)p.frame) & (px - 1)) != 0) return hipErrorInvalidValue;
    const dim3 grid(grid_for((long)p.B * p.T * p.T));
    return for_edge(edge, [&](auto e) {
        constexpr int E = decltype(e)::value;
        if (p.fp32) hipLaunchKernelGGL((gather_px_kernel<float4v, E>), grid, dim3(kGatherThreads), 0, s, p);
        else hipLaunchKernelGGL((gather_px_kernel<half4, E>), grid, dim3(kGatherThreads), 0, s, p);
        return hipGetLastError();
    });
}

}  // namespace w2x
