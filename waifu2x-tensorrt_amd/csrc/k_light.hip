// Resize in linear light: the test hook's decode.  Img2Img::resizePlanes takes caller-supplied fp32 planes as the canvas; this kernel does to them
// what compose_canvas_kernel does to its sums - light_canvas<true>, the device function the canvas kernels call (prepost_device.h) - in place, a value per
// thread in a grid-stride loop.  The resize and the store behind it are the production kernels (resample_planes_kernel).
#include "kernels.h"
#include "prepost_device.h"

namespace w2x {
namespace {

constexpr int kLightThreads = 256;

__global__ __launch_bounds__(kLightThreads) void light_decode_planes_kernel(float* v, size_t n, const LightArgs lz) {
    for (size_t i = (size_t)blockIdx.x * kLightThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kLightThreads) v[i] = light_canvas<true>(lz, v[i]);
}

}  // namespace

hipError_t launch_light_decode_planes(float* v, size_t n, const LightArgs& l, hipStream_t s) {
    if (!light_args_ok(l) || (!v && n)) return hipErrorInvalidValue;
    if (l.mode == kLightGamma || n == 0) return hipSuccess;
    const size_t groups = (n + kLightThreads - 1) / kLightThreads;
    hipLaunchKernelGGL(light_decode_planes_kernel, dim3((unsigned)(groups < 4096 ? groups : 4096)), dim3(kLightThreads), 0, s, v, n, l);
    return hipGetLastError();
}

}  // namespace w2x
