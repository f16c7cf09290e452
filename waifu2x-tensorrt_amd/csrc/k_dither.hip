// Dithered output: the device's copy of the blue-noise table and the test hook that runs the store of the compose / resample kernels alone.
//   kBlueNoiseDevice     : the 64 x 64 ranks of dither_table.h as initialised device memory of this code object - every device that loads the library has
//                          them, nothing is allocated or uploaded, and dither_table_device() is an address lookup.
//   dither_planes_kernel : Img2Img::ditherPlanes.  n planes of fp32 values in, n planes of 8 .. 16-bit samples out through store4<S, M> (pixel_device.h): the
//                          quantisation, the packing and the ragged / unaligned paths of compose_planes_kernel and resample_planes_kernel, with no network and no
//                          tiles in front.  The values are taken as they are - not clamped - so that the saturation of the store is part of what is tested.
#include "kernels.h"
#include "pixel_device.h"

namespace w2x {

// (external linkage: the runtime registers it, and hipGetSymbolAddress finds it whether or not a kernel of this file names it)
__device__ uint16_t kBlueNoiseDevice[kDitherSide * kDitherSide] = {
#include "dither_table.h"
};

namespace {

constexpr int kDitherPlanesThreads = 64;

// a thread owns four consecutive samples of a row of every plane; blockIdx.y walks the rows
template <typename S, int M>
__global__ __launch_bounds__(kDitherPlanesThreads) void dither_planes_kernel(const PlanarPlanes src, const PlanarPlanes dst, float scale, int maxcode, const DitherArgs dz) {
    const int X = 4 * (blockIdx.x * kDitherPlanesThreads + threadIdx.x);
    if (X >= dst.cols) return;
    const int np = min(4, dst.cols - X);
    for (int Y = blockIdx.y; Y < dst.rows; Y += gridDim.y) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= dst.n) break;
            const float* s = (const float*)(src.p[c] + (size_t)Y * src.step[c]) + X;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < np; ++k) v[k] = s[k];
            store4<S, M>(dst.p[c] + (size_t)Y * dst.step[c], X, np, v, scale, maxcode, dz, dst.n == 1 ? 1 : c, Y);
        }
    }
}

inline bool dither_planes_ok(const PlanarPlanes& f, bool fp32) {
    if ((f.n != 1 && f.n != 3) || f.rows <= 0 || f.cols <= 0) return false;
    if (fp32 ? f.bits != 32 : (f.bits != 8 && f.bits != 10 && f.bits != 12 && f.bits != 16)) return false;
    const size_t bps = planar_sample_bytes(f.bits);
    for (int k = 0; k < f.n; ++k) if (!f.p[k] || f.step[k] < (size_t)f.cols * bps || ((((size_t)f.p[k]) | f.step[k]) & (bps - 1)) != 0) return false;
    return true;
}

}  // namespace

const uint16_t* dither_table_device(hipError_t* err) {
    void* p = nullptr;
    const hipError_t e = hipGetSymbolAddress(&p, HIP_SYMBOL(kBlueNoiseDevice));
    if (err) *err = e;
    return e == hipSuccess ? (const uint16_t*)p : nullptr;
}

hipError_t launch_dither_planes(const PlanarPlanes& src, const PlanarPlanes& dst, const DitherArgs& d, hipStream_t s) {
    if (!dither_planes_ok(src, true) || !dither_planes_ok(dst, false) || src.n != dst.n || src.rows != dst.rows || src.cols != dst.cols || !dither_args_ok(d))
        return hipErrorInvalidValue;
    const int groups = (dst.cols + 3) / 4;
    const dim3 grid((unsigned)((groups + kDitherPlanesThreads - 1) / kDitherPlanesThreads), (unsigned)(dst.rows < 65535 ? dst.rows : 65535));
    const int maxcode = (1 << dst.bits) - 1;
    const float scale = (float)maxcode;
    auto launch = [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (dst.bits == 8) hipLaunchKernelGGL((dither_planes_kernel<U8, M>), grid, dim3(kDitherPlanesThreads), 0, s, src, dst, scale, maxcode, d);
        else hipLaunchKernelGGL((dither_planes_kernel<U16, M>), grid, dim3(kDitherPlanesThreads), 0, s, src, dst, scale, maxcode, d);
        return hipGetLastError();
    };
    if (d.mode == kDitherNone) return launch(std::integral_constant<int, kDitherNone>());
    return for_dither(d, launch);
}

}  // namespace w2x
