// Antialiased resize of a composed frame to any size between the input frame and the network's output (renderResized): the separable
// convolution resampler of PIL / torch interpolate(antialias=True) on the fp32 RGB canvas that compose_canvas_kernel writes, quantised like
// compose (sat(rint(x * 255)), 16-bit frames 65535) and stored as BGR.
//
// One launch, both passes, and both are the shared ones of pixel_device.h (resample_pass1 / resample_pass2), which every frame format's resize
// kernel runs: this file adds the BGR store alone.  A workgroup owns an output tile of kResampleRows x kResampleCols pixels.  Pass 1 filters
// the input rows the tile's output rows reach, horizontally, from the canvas (read through L1 / L2: neighbouring output columns share most of
// their taps) into LDS: [3][rows_max][kResampleCols] fp32.  Pass 2 filters those rows vertically out of LDS, a thread per four output pixels
// of a row, and the four pixels' 12 bytes leave as three dwords (compose's fast-path store), 24 bytes at 16 bits as six, where the row
// allows.  The tap tables come from the host (tiles.h resize_taps): per output column its first input column and kx weights, per output row
// its first input row and ky weights; weights past the taps an output has are 0, and the loops stop at the canvas edge, so no read leaves the
// canvas.  The same resize with a YUV output (renderYuvResized), every layout: k_resample_yuv.hip.
// LDS: at a factor of 4 with bicubic taps (ky = 17) rows_max <= 15 * 4 + 1 + 17 = 78 rows, 3 * 78 * 256 B = 58.5 KiB: two workgroups per CU.
#include "pixel_device.h"

namespace w2x {
namespace {

// M: kDitherNone - no further argument - is the kernel above; a dithered mode takes its DitherArgs behind p (dither_of).  Pixel X + q of row Y:
// the channels r, g, b are the plane indices 0, 1, 2.
template <int M = kDitherNone, typename... D>
__global__ __launch_bounds__(kRsThreads) void resample_kernel(const ResampleParams p, const D... dzs) {
    static_assert(dither_pack_ok<M, D...>, "kDitherNone: no DitherArgs, else one; then one LightArgs or none");
    const DitherArgs& dz = dither_of(dzs...);
    constexpr bool kLin = light_on<D...>;                                 // (the resized values are linear light and are encoded before they are quantised)
    const LightArgs& lz = light_of(dzs...);
    constexpr bool kEdge = edge_on<D...>;                                 // (the input indices of the passes go through the edge rule)
    extern __shared__ float h[];                                          // [3][rows_max][kRsCols]
    const int r0 = resample_pass1<3, kEdge>(p, h, edge_of(dzs...).mode);
    __syncthreads();
    float4v a[3];                                                         // R, G, B of four pixels
    int X, Y, np;
    if (!resample_pass2<3, kEdge>(p, h, r0, a, X, Y, np)) return;
    if constexpr (kLin) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) a[c][q] = light_out<true>(lz, a[c][q]);
    }
    uint8_t* d = p.dst + (size_t)Y * p.dst_step;
    if (!p.deep) {
        d += (size_t)X * 3;
        unsigned px[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if constexpr (M == kDitherNone) px[q] = quant(a[2][q], 255.f, 255) | quant(a[1][q], 255.f, 255) << 8 | quant(a[0][q], 255.f, 255) << 16;   // b | g << 8 | r << 16
            else px[q] = quantize_bgr_at<M>(a[0][q], a[1][q], a[2][q], dz, X + q, Y);
        }
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
        for (int q = 0; q < 4; ++q) {
            if constexpr (M == kDitherNone) { v[3 * q] = quant(a[2][q], 65535.f, 65535); v[3 * q + 1] = quant(a[1][q], 65535.f, 65535); v[3 * q + 2] = quant(a[0][q], 65535.f, 65535); }
            else {
#pragma unroll
                for (int e = 0; e < 3; ++e) v[3 * q + e] = quant_code<M>(a[2 - e][q] * 65535.f, 65535, dz, 2 - e, X + q, Y);
            }
        }
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

int resample_rows_max(const int* fy, int outH, int inH, int ky, int rows_above) {
    int m = 0;
    for (int y0 = 0; y0 < outH; y0 += kRsRows) {
        const int y1 = (y0 + kRsRows < outH ? y0 + kRsRows : outH) - 1;
        const int e = fy[y1] + ky < inH ? fy[y1] + ky : inH;
        const int first = fy[y0 - rows_above > 0 ? y0 - rows_above : 0];
        if (e - first > m) m = e - first;
    }
    return m;
}

int resample_rows_max_edge(const int* fy, int outH, int ky) {
    int m = 0;
    for (int y0 = 0; y0 < outH; y0 += kRsRows) {
        const int y1 = (y0 + kRsRows < outH ? y0 + kRsRows : outH) - 1;
        if (fy[y1] + ky - fy[y0] > m) m = fy[y1] + ky - fy[y0];
    }
    return m;
}

hipError_t launch_resample(const ResampleParams& p, hipStream_t s, const DitherArgs& d, const LightArgs& l, const EdgeArgs& e) {
    if (p.outW <= 0 || p.outH <= 0) return hipSuccess;
    return for_modes(d, l, e, [&](auto m, const auto&... extra) {
        static unsigned lds_done = 0;                                    // (one per instantiation of this lambda's body)
        return launch_resample_tiles(resample_kernel<decltype(m)::value, std::decay_t<decltype(extra)>...>, 3 * kRsCols, p.rows_max, lds_done, p.outW, p.outH, s, p, extra...);
    });
}

}  // namespace w2x
