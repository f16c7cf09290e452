// Pre/post kernels of the tile pipeline (HBM-bound byte/fp32 work, bit-exact against the oracle):
//   gather  : frame u8 BGR -> network input tiles fp16 [B][T][T][4] (RGB, x*fl32(1/255)), replicate padding and the
//             TTA dihedral transform folded into the source index.   Replaces cv::cuda::cvtColor(BGR2RGB)
//             (img2img_render.cpp:227), padRoi (:68-105), applyAugmentation (:134-177), blobFromImages
//             (img2img_infer.cpp:5-21) and the D2D copy (:76-77).
//   compose : network output tiles fp16 -> frame u8 BGR.  Per output pixel, the covering tiles are visited in
//             ascending tile index, TTA de-augmentation + fp32 sum in aug order + *0.125f, ramp weights multiplied
//             in the order left, top, right, bottom, fp32 overlap-add, *255 -> rint -> saturate -> BGR.  Replaces
//             imagesFromBlob (img2img_infer.cpp:23-39), reverseAugmentation/TTA accumulate (:179-222,:305-318),
//             applyWeights (:107-121), the canvas add (:329-330) and the final convertTo/cvtColor (:342-343).
//   gather_yuv / compose_yuv: the same two steps on YUV 4:2:0 frames (renderYuv): colour conversion and chroma resampling
//             folded into the tile reads and the canvas writes.  Both are instantiated per layout (I420, I422, I444, NV12 / P010: DESIGN 9f);
//             compose_yuv444_kernel is the 4:4:4 output in compose_kernel's shape.
//   se/scale: cunet squeeze-excite gate and channel scaling.
#include "kernels.h"
#include "prepost_device.h"
#include <type_traits>

namespace w2x {
namespace {

// E: the edge rule of the two source-index lines (edge_src); kEdgeReplicate is the clamp
template <typename P, int E = kEdgeReplicate>
__global__ __launch_bounds__(256) void gather_kernel(const GatherParams p) {
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
            int fy = edge_src<E>(sl.y + sy, p.rows);
            int fx = edge_src<E>(sl.x + sx, p.cols);
            if (!p.deep) {
                const uint8_t* px = p.frame + (size_t)fy * p.step + (size_t)fx * 3;
                v = make_px<P>((float)px[2] * inv255, (float)px[1] * inv255, (float)px[0] * inv255);
            } else {   // 16-bit samples (extension, README.md:88 lists it as a TODO upstream): the same conversion with 65535
                const uint16_t* px = (const uint16_t*)(p.frame + (size_t)fy * p.step) + (size_t)fx * 3;
                v = make_px<P>((float)px[2] * inv65535, (float)px[1] * inv65535, (float)px[0] * inv65535);
            }
        }
        *((P*)p.out + i) = v;
    }
}

template <typename P, int M>
__device__ __forceinline__ unsigned compose_pixel(const ComposeParams& p, const P* tiles, int X, int Y, const DitherArgs& dz) {
    float a0, a1, a2;
    compose_pixel_sums<P>(p, tiles, X, Y, a0, a1, a2);
    return quantize_bgr_at<M>(a0, a1, a2, dz, X, Y);
}
// launch(std::integral_constant<int, M>()) for the dithered mode of d: the switch from the run-time mode to the kernel instantiation
template <typename Launch> hipError_t for_dither(const DitherArgs& d, Launch launch) {
    if (d.mode == kDitherOrdered) return launch(std::integral_constant<int, kDitherOrdered>());
    if (d.mode == kDitherBlueNoise && d.table) return launch(std::integral_constant<int, kDitherBlueNoise>());
    return hipErrorInvalidValue;                                    // no kernel for it: an error, never the undithered kernel
}

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

// A thread owns four consecutive pixels of a row.  Where the four have the same covering tiles, lie inside each of them and no TTA
// is involved (all but the columns next to a tile edge), a tile contributes its four pixels as two 16-byte loads and the 12
// output bytes leave as three dwords; the per-pixel arithmetic and its order are those of compose_pixel, so the bytes are the
// same.  Everything else takes the per-pixel path.  (The output is 100 MB of u8 per 4K frame: single-byte stores and 8-byte loads
// were the kernel's bound; four pixels per thread on the per-pixel path alone lose the loads' coalescing and measured slower.)
// Launch shape (round 3): blockIdx.x / threadIdx.x pick the four-pixel column group, blockIdx.y a band of kComposeRows rows that the
// thread walks (four: more rows per thread leave too few workgroups in flight, fewer repeat the column arithmetic).  Everything that depends on the column only (covering tile columns, whether the group takes the fast path, the ramp
// weights of its four pixels) is computed once per thread, what depends on the row is the same for a whole workgroup (scalar
// registers) - the flat grid-stride loop it replaces paid a 64-bit division and six 32-bit ones per four pixels, and the kernel ran at
// 3.1 TB/s with its integer unit busier than its memory pipe.
// (measured at config 3, profiles/r3_kernels/compose_geometry.txt: rows x threads 8 x 128 0.140 ms, 4 x 128 0.119, 16 x 128 0.177, 4 x 64 0.115-0.118, 2 x 64 0.117, 1 x 64 0.125)
// (kComposeRows / kComposeThreads: kernels.h, shared with the kernels of k_planar.hip that have this launch shape)
// M: kDitherNone - no further argument - is the kernel above; a dithered mode takes its DitherArgs behind p (dither_of).  (X, Y) are canvas
// coordinates, so a strip's or a shard's rect gets the thresholds the whole frame would.
template <typename P, int M = kDitherNone, typename... D>
__global__ __launch_bounds__(kComposeThreads) void compose_kernel(const ComposeParams p, const D... dzs) {
    static_assert(dither_pack_ok<M, D...>, "kDitherNone: no argument; else one DitherArgs");
    const DitherArgs& dz = dither_of(dzs...);
    constexpr bool kHalf = sizeof(P) == 8;                          // the four-pixel fast path reads fp16 tiles
    const int x1 = p.x1 > 0 ? p.x1 : p.outW, sw = x1 - p.x0;
    const int gw = (sw + 3) >> 2;                                   // pixel groups per row
    const int xg = blockIdx.x * kComposeThreads + threadIdx.x;
    if (xg >= gw) return;
    const P* tiles = (const P*)p.tiles;
    const int To = p.To, n = To - 1;
    const int X = p.x0 + 4 * xg;
    const int np = min(4, x1 - X);
    // tile columns covering the first and the last pixel of the group
    int a0 = X - To + 1; a0 = a0 <= 0 ? 0 : (a0 + p.stride_x - 1) / p.stride_x;
    int b0 = X + 3 - To + 1; b0 = b0 <= 0 ? 0 : (b0 + p.stride_x - 1) / p.stride_x;
    const int a1 = min(p.nx - 1, X / p.stride_x), b1 = min(p.nx - 1, (X + 3) / p.stride_x);
    const bool fast_col = kHalf && np == 4 && !p.tta && !p.deep && a0 == b0 && a1 == b1;
    const int Y0 = p.y0 + blockIdx.y * kComposeRows, Y1 = min(p.y1 > 0 ? p.y1 : p.outH, Y0 + kComposeRows);
    for (int Y = Y0; Y < Y1; ++Y) {
        uint8_t* d = p.dst + (size_t)Y * p.dst_step + (size_t)X * 3;
        unsigned px[4] = {0u, 0u, 0u, 0u};
        if (p.deep) {   // 16-bit output (extension): the same sums, rint(x * 65535) saturated, BGR
            uint16_t* d16 = (uint16_t*)(p.dst + (size_t)Y * p.dst_step) + (size_t)X * 3;
            for (int k = 0; k < np; ++k) {
                float r, g, b;
                compose_pixel_sums<P>(p, tiles, X + k, Y, r, g, b);
                if constexpr (M == kDitherNone) {
                    d16[3 * k] = (uint16_t)min(max(__float2int_rn(b * 65535.f), 0), 65535);
                    d16[3 * k + 1] = (uint16_t)min(max(__float2int_rn(g * 65535.f), 0), 65535);
                    d16[3 * k + 2] = (uint16_t)min(max(__float2int_rn(r * 65535.f), 0), 65535);
                } else {
                    d16[3 * k] = (uint16_t)quant_code<M>(b * 65535.f, 65535, dz, 2, X + k, Y);
                    d16[3 * k + 1] = (uint16_t)quant_code<M>(g * 65535.f, 65535, dz, 1, X + k, Y);
                    d16[3 * k + 2] = (uint16_t)quant_code<M>(r * 65535.f, 65535, dz, 0, X + k, Y);
                }
            }
            continue;
        }
        const bool fast = fast_col && (((size_t)d) & 3) == 0;
        if (fast) {
            int j0 = Y - To + 1; j0 = j0 <= 0 ? 0 : (j0 + p.stride_y - 1) / p.stride_y;
            const int j1 = min(p.ny - 1, Y / p.stride_y);
            float acc[4][3] = {};
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
                        acc[k][0] += v0; acc[k][1] += v1; acc[k][2] += v2;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) px[k] = quantize_bgr_at<M>(acc[k][0], acc[k][1], acc[k][2], dz, X + k, Y);
            unsigned* dw = (unsigned*)d;
            dw[0] = px[0] | px[1] << 24;
            dw[1] = px[1] >> 8 | px[2] << 16;
            dw[2] = px[2] >> 16 | px[3] << 8;
        } else {
            for (int k = 0; k < np; ++k) {
                const unsigned v = compose_pixel<P, M>(p, tiles, X + k, Y, dz);
                d[3 * k] = (uint8_t)v; d[3 * k + 1] = (uint8_t)(v >> 8); d[3 * k + 2] = (uint8_t)(v >> 16);
            }
        }
    }
}

// The canvas of a resized frame (renderResized): compose_pixel_sums for every pixel of the rect, unquantised, as three fp32 planes.  A thread
// per pixel along a row (the plane stores of a wave are 256 contiguous bytes each), a workgroup row per canvas row.
// L: empty - the kernel above -, or one LightArgs: the planes hold decode(sat01(sum)), linear light, for the resize to average.  This is where a
// decode costs one evaluation per canvas pixel and not one per tap.
template <typename P, typename... L>
__global__ __launch_bounds__(256) void compose_canvas_kernel(const ComposeParams p, float* canvas, const L... ls) {
    static_assert(dither_pack_ok<kDitherNone, L...>, "no argument, or one LightArgs");
    constexpr bool kLin = light_on<L...>;
    const LightArgs& lz = light_of(ls...);
    const int x1 = p.x1 > 0 ? p.x1 : p.outW, y1 = p.y1 > 0 ? p.y1 : p.outH;
    const int X = p.x0 + blockIdx.x * 256 + threadIdx.x;
    if (X >= x1) return;
    const size_t plane = (size_t)p.outW * p.outH;
    for (int Y = p.y0 + blockIdx.y; Y < y1; Y += gridDim.y) {
        float r, g, b;
        compose_pixel_sums<P>(p, (const P*)p.tiles, X, Y, r, g, b);
        const size_t i = (size_t)Y * p.outW + X;
        canvas[i] = light_canvas<kLin>(lz, r); canvas[plane + i] = light_canvas<kLin>(lz, g); canvas[2 * plane + i] = light_canvas<kLin>(lz, b);
    }
}

// YUV 4:2:0 frames (renderYuv).  One sample of plane `pl` (8-bit: uint8, 10-bit: uint16).
__device__ __forceinline__ float yuv_sample(const YuvPlanes& f, int pl, int y, int x) {
    const uint8_t* row = f.p[pl] + (size_t)y * f.step[pl];
    return f.bits > 8 ? (float)((const uint16_t*)row)[x] : (float)row[x];
}

// The same for a frame of layout L: Y of P010 (NV12 at 10 bits) carries its code in the high 10 bits; chroma component pl (1: U, 2: V) at (y, x) of
// the chroma grid comes from plane pl, or for NV12 from sample 2x + pl - 1 of plane 1.
template <int L>
__device__ __forceinline__ float yuv_luma(const YuvPlanes& f, int y, int x) {
    if constexpr (L != kYuvNV12) return yuv_sample(f, 0, y, x);
    const uint8_t* row = f.p[0] + (size_t)y * f.step[0];
    return f.bits > 8 ? (float)(((const uint16_t*)row)[x] >> 6) : (float)row[x];
}
template <int L>
__device__ __forceinline__ float yuv_chroma(const YuvPlanes& f, int pl, int y, int x) {
    if constexpr (L != kYuvNV12) return yuv_sample(f, pl, y, x);
    const uint8_t* row = f.p[1] + (size_t)y * f.step[1];
    const int i = 2 * x + pl - 1;
    return f.bits > 8 ? (float)(((const uint16_t*)row)[i] >> 6) : (float)row[i];
}

// gather_kernel on a YUV frame: the same tile layout, slots and source index (clamped, through aug_src); per tile pixel Y and the 2 x 2 chroma
// neighbours of its source position, chroma upsampled to the luma grid (columns: even x C[x/2], odd x the mean of C[(x-1)/2] and C[(x+1)/2]; rows:
// 2k takes 1/4 C[k-1] + 3/4 C[k], 2k+1 takes 3/4 C[k] + 1/4 C[k+1]; indices clamped), the matrix inverted in fp32, R, G, B clamped to [0, 1].
// (The upsampled codes are exact in fp32: integers below 2^10 times quarters.)  That is I420, and NV12 through yuv_luma / yuv_chroma; I422 keeps the
// column rule and takes chroma row fy itself; I444 takes the chroma of the pixel.
// S: the siting of the frame's chroma.  kYuvLeft is the above, its statements untouched.  The others take the same 2 x 2 neighbourhood by
// yuv_axis_taps, one 1-D rule per axis: kYuvCenter centred columns (1/4, 3/4 like the rows), kYuvTopLeft co-sited rows (the column rule's shape); the codes
// stay exact (integers below 2^10 times sixteenths).  I422 has the column rule only, so its kYuvTopLeft is kYuvLeft, as every siting of I444 is
// (launch_gather_yuv).
// The two chroma samples and weights of luma index n along one axis of cn samples: co-sited - even n C[n/2] alone, odd n the mean of C[(n-1)/2] and
// C[(n+1)/2]; centred - n = 2k 1/4 C[k-1] + 3/4 C[k], n = 2k+1 3/4 C[k] + 1/4 C[k+1]; indices clamped to the plane.
template <bool kCentred>
__device__ __forceinline__ void yuv_axis_taps(int n, int cn, int& i0, int& i1, float& w0, float& w1) {
    const int k = n >> 1;
    const bool odd = n & 1;
    if constexpr (kCentred) {
        i0 = odd ? k : max(k - 1, 0); i1 = odd ? min(k + 1, cn - 1) : k;
        w0 = odd ? 0.75f : 0.25f; w1 = odd ? 0.25f : 0.75f;
    } else {
        i0 = k; i1 = odd ? min(k + 1, cn - 1) : k;
        w0 = 0.5f; w1 = 0.5f;
    }
}
template <typename P, int L, int S = kYuvLeft>
__global__ __launch_bounds__(256) void gather_yuv_kernel(const GatherYuvParams p) {
    static_assert(S == kYuvLeft || L == kYuvI420 || L == kYuvNV12 || (L == kYuvI422 && S == kYuvCenter), "a siting the layout does not tell from kYuvLeft");
    const int T = p.T;
    const long total = (long)p.B * T * T;
    const int rows = p.src.rows, cols = p.src.cols, ch = (rows + 1) >> 1, cw = (cols + 1) >> 1;
    const YuvCoefs& k = p.k;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int b = (int)(i / ((long)T * T));
        int rem = (int)(i - (long)b * T * T);
        int y = rem / T, x = rem - y * T;
        TileSlot sl = p.slots[b];
        P v = make_px<P>(0.f, 0.f, 0.f);
        if (sl.valid) {
            int sy, sx;
            aug_src(sl.aug, T - 1, y, x, sy, sx);
            const int fy = min(max(sl.y + sy, 0), rows - 1), fx = min(max(sl.x + sx, 0), cols - 1);
            float u, w;
            if constexpr (S != kYuvLeft) {
                int c0, c1, r0 = fy, r1 = fy;
                float wc0, wc1, w0 = 0.5f, w1 = 0.5f;
                yuv_axis_taps<yuv_cols_centred(S)>(fx, cw, c0, c1, wc0, wc1);
                if constexpr (L != kYuvI422) yuv_axis_taps<yuv_rows_centred(S)>(fy, ch, r0, r1, w0, w1);
                u = w0 * (wc0 * yuv_chroma<L>(p.src, 1, r0, c0) + wc1 * yuv_chroma<L>(p.src, 1, r0, c1)) + w1 * (wc0 * yuv_chroma<L>(p.src, 1, r1, c0) + wc1 * yuv_chroma<L>(p.src, 1, r1, c1));
                w = w0 * (wc0 * yuv_chroma<L>(p.src, 2, r0, c0) + wc1 * yuv_chroma<L>(p.src, 2, r0, c1)) + w1 * (wc0 * yuv_chroma<L>(p.src, 2, r1, c0) + wc1 * yuv_chroma<L>(p.src, 2, r1, c1));
            } else if constexpr (L == kYuvI444) {
                u = yuv_chroma<L>(p.src, 1, fy, fx); w = yuv_chroma<L>(p.src, 2, fy, fx);
            } else if constexpr (L == kYuvI422) {
                const int cj = fx >> 1, c1 = (fx & 1) ? min(cj + 1, cw - 1) : cj;
                u = 0.5f * (yuv_chroma<L>(p.src, 1, fy, cj) + yuv_chroma<L>(p.src, 1, fy, c1));
                w = 0.5f * (yuv_chroma<L>(p.src, 2, fy, cj) + yuv_chroma<L>(p.src, 2, fy, c1));
            } else {
                const int ck = fy >> 1, cj = fx >> 1;
                const bool odd_y = fy & 1;
                const int r0 = odd_y ? ck : max(ck - 1, 0), r1 = odd_y ? min(ck + 1, ch - 1) : ck;
                const float w0 = odd_y ? 0.75f : 0.25f, w1 = odd_y ? 0.25f : 0.75f;
                const int c1 = (fx & 1) ? min(cj + 1, cw - 1) : cj;
                u = w0 * (0.5f * (yuv_chroma<L>(p.src, 1, r0, cj) + yuv_chroma<L>(p.src, 1, r0, c1))) + w1 * (0.5f * (yuv_chroma<L>(p.src, 1, r1, cj) + yuv_chroma<L>(p.src, 1, r1, c1)));
                w = w0 * (0.5f * (yuv_chroma<L>(p.src, 2, r0, cj) + yuv_chroma<L>(p.src, 2, r0, c1))) + w1 * (0.5f * (yuv_chroma<L>(p.src, 2, r1, cj) + yuv_chroma<L>(p.src, 2, r1, c1)));
            }
            const float Y = (yuv_luma<L>(p.src, fy, fx) - k.y_off) * k.y_mul, cb = (u - k.c_off) * k.c_mul, cr = (w - k.c_off) * k.c_mul;
            const float R = Y + k.r_cr * cr, G = Y + k.g_cb * cb + k.g_cr * cr, B = Y + k.b_cb * cb;
            v = make_px<P>(fminf(fmaxf(R, 0.f), 1.f), fminf(fmaxf(G, 0.f), 1.f), fminf(fmaxf(B, 0.f), 1.f));
        }
        *((P*)p.out + i) = v;
    }
}

__device__ __forceinline__ unsigned yuv_code(float off, float scale, float v, int maxcode) { return (unsigned)min(max(__float2int_rn(off + scale * v), 0), maxcode); }

// M: the code of sample (x, y) of plane c (Y, U, V = 0, 1, 2; chroma samples in their own plane's coordinates, NV12's as the I420 samples they are).
// kDitherNone is yuv_code; a dithered mode adds the sample's threshold to the same value - the expression as yuv_code writes it - and rounds down.
template <int M>
__device__ __forceinline__ unsigned yuv_code_at(float off, float scale, float v, int maxcode, const DitherArgs& dz, int c, int x, int y) {
    if constexpr (M == kDitherNone) return yuv_code(off, scale, v, maxcode);
    else return dither_code<M>(off + scale * v, dither_t<M>(dz, c, x, y), maxcode);
}

// compose_kernel for a YUV 4:2:0 output.  A thread owns kYuvSites consecutive chroma sites of one chroma row: the 2 x 8 luma pixels under them
// (rows 2i, 2i + 1, columns 8t .. 8t + 7).  Each pixel's sums come from compose_pixel_sums (the blend and TTA order of the u8 path), clamped to [0, 1];
// Y is coded per pixel.  Chroma site j filters the two rows (1/2, 1/2) and columns 2j - 1, 2j, 2j + 1 (1/4, 1/2, 1/4), coordinates clamped to the
// frame.  Column 8t - 1 belongs to the lane on the left: it arrives by a cross-lane move (ds_bpermute), and only lane 0 of the wave, whose left
// neighbour lies in another workgroup, computes it again.  A full run stores Y as 8 (10-bit: 16) bytes per row and U, V as 4 (8) bytes; the ragged
// right end stores sample by sample.  Workgroup = one wave along a chroma row; no canvas goes through HBM.
// L: kYuvI420 is the above.  kYuvNV12 is the same arithmetic with U and V stored interleaved in plane 1 (8 bytes per full run, 10-bit: 16)
// and, at 10 bits, every code shifted into the high bits (P010).  kYuvI422 has one luma row per chroma row: no vertical pair, a thread owns four
// sites (8 luma columns) of row i and filters the columns of that row alone.
// S: the siting of the chroma sites.  kYuvLeft is the above.  kYuvCenter: site j is the mean of columns 2j and 2j + 1 (of the two rows averaged, as
// above) - nothing from the lane on the left, no cross-lane move, no column recomputed by lane 0.  kYuvTopLeft (I420 / NV12; I422 has no row rule and takes
// kYuvLeft): site (i, j) filters rows 2i - 1, 2i, 2i + 1 (1/4, 1/2, 1/4) and then the columns as kYuvLeft does.  Row 2i - 1 is the second row of the chroma row
// above, so a workgroup walks a BAND of kYuvBand consecutive chroma rows (blockIdx.y picks the band) and carries that row's clamped R, G, B - 8 columns x 3
// floats per lane and lane 0's left column - in registers from one chroma row into the next; only the luma row above a band's first chroma row is computed a
// second time (row -1 clamps to row 0: nothing to compute).  Pixel sums: (2 kYuvBand + 1) / (2 kYuvBand) of kYuvLeft's.
// M: kDitherNone - no further argument - is the above; a dithered mode takes its DitherArgs behind p (dither_of): Y at (X0 + q, Y), the codes of
// chroma site (ci, j0 + s) at that position of planes 1 and 2.
template <typename P, int L, int S = kYuvLeft, int M = kDitherNone, typename... D>
__global__ __launch_bounds__(kYuvThreads) void compose_yuv_kernel(const ComposeYuvParams p, const D... dzs) {
    static_assert(dither_pack_ok<M, D...>, "kDitherNone: no argument; else one DitherArgs");
    const DitherArgs& dz = dither_of(dzs...);
    static_assert(kYuvSites == 4, "the packed stores below are written for four sites per thread");
    static_assert(L == kYuvI420 || L == kYuvI422 || L == kYuvNV12, "4:4:4 output is compose_yuv444_kernel");
    static_assert(S == kYuvLeft || S == kYuvCenter || (S == kYuvTopLeft && L != kYuvI422), "I422 has no row rule: its kYuvTopLeft is kYuvLeft");
    constexpr int kCols = 2 * kYuvSites;
    constexpr bool kPair = L != kYuvI422, kSemi = L == kYuvNV12;
    constexpr bool kBand = S == kYuvTopLeft, kLeftCol = S != kYuvCenter;   // rows 2i - 1 carried down a band; column 2j - 1 taken from the left
    const ComposeParams& c = p.c;
    const P* tiles = (const P*)c.tiles;
    const YuvCoefs& k = p.k;
    const int W = c.outW, H = c.outH, cw = (W + 1) >> 1, ch = kPair ? (H + 1) >> 1 : H;
    const int runs = (cw + kYuvSites - 1) / kYuvSites;
    const int t = blockIdx.x * kYuvThreads + threadIdx.x;
    const bool active = t < runs;
    const int j0 = t * kYuvSites, X0 = 2 * j0;
    const int ncols = active ? min(kCols, W - X0) : 0;         // luma columns of the run inside the frame (>= 1 for an active lane)
    const bool wide = p.dst.bits > 8;
    const int sh = kSemi && wide ? 6 : 0;                       // P010
    auto pixel = [&](int X, int Y, float* o) {
        float r, g, b;
        compose_pixel_sums<P>(c, tiles, X, Y, r, g, b);
        o[0] = fminf(fmaxf(r, 0.f), 1.f); o[1] = fminf(fmaxf(g, 0.f), 1.f); o[2] = fminf(fmaxf(b, 0.f), 1.f);
    };
    // the chroma rows of this workgroup: every gridDim.y-th, or (kBand) the kYuvBand consecutive rows of band blockIdx.y
    const int ci0 = kBand ? blockIdx.y * kYuvBand : blockIdx.y;
    float above[kBand ? kCols : 1][3] = {}, above_left[3] = {0.f, 0.f, 0.f};   // kBand: luma row 2 ci - 1 (clamped R, G, B), and its column X0 - 1 in lane 0
    for (int ci = ci0; ci < (kBand ? min(ch, ci0 + kYuvBand) : ch); ci += kBand ? 1 : gridDim.y) {
        const int Ya = kPair ? 2 * ci : ci, Yb = kPair ? min(2 * ci + 1, H - 1) : ci;
        float v[kCols][3];                                      // the run's columns, the two rows averaged (kBand: rows 2i - 1, 2i, 2i + 1 by 1/4, 1/2, 1/4)
        float left[3] = {0.f, 0.f, 0.f};
        if constexpr (kBand) {
            if (ci == ci0 && ci > 0) {                              // the band's first chroma row: the luma row above it comes from the tiles once more
#pragma unroll
                for (int q = 0; q < kCols; ++q) {
                    float o[3] = {0.f, 0.f, 0.f};
                    if (q < ncols) pixel(X0 + q, Ya - 1, o);
#pragma unroll
                    for (int e = 0; e < 3; ++e) above[q][e] = o[e];
                }
                if (threadIdx.x == 0 && active && X0 > 0) pixel(X0 - 1, Ya - 1, above_left);
            }
        }
        for (int r = 0; r < (kPair ? 2 : 1); ++r) {
            const int Y = r ? Yb : Ya;
            const bool store_y = r == 0 || Yb != Ya;
            unsigned yc[kCols];
#pragma unroll
            for (int q = 0; q < kCols; ++q) {
                float o[3] = {0.f, 0.f, 0.f};
                if (q < ncols) pixel(X0 + q, Y, o);
                yc[q] = yuv_code_at<M>(k.y_off, k.y_scale, k.kr * o[0] + k.kg * o[1] + k.kb * o[2], k.maxcode, dz, 0, X0 + q, Y) << sh;
                if constexpr (kBand) {
#pragma unroll
                    for (int e = 0; e < 3; ++e) {                   // row 2i: 1/4 of the row above (row -1 clamps to row 0) + 1/2; row 2i + 1: + 1/4, and carried down
                        if (r == 0) v[q][e] = 0.25f * (ci ? above[q][e] : o[e]) + 0.5f * o[e];
                        else { v[q][e] += 0.25f * o[e]; above[q][e] = o[e]; }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 3; ++e) v[q][e] = r ? 0.5f * (v[q][e] + o[e]) : o[e];
                }
            }
            if (kLeftCol && threadIdx.x == 0 && active && X0 > 0) {  // the wave's first lane: column X0 - 1 from the tiles
                float o[3];
                pixel(X0 - 1, Y, o);
                if constexpr (kBand) {
#pragma unroll
                    for (int e = 0; e < 3; ++e) {
                        if (r == 0) left[e] = 0.25f * (ci ? above_left[e] : o[e]) + 0.5f * o[e];
                        else { left[e] += 0.25f * o[e]; above_left[e] = o[e]; }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 3; ++e) left[e] = r ? 0.5f * (left[e] + o[e]) : o[e];
                }
            }
            if (!active || !store_y) continue;
            uint8_t* row = p.dst.p[0] + (size_t)Y * p.dst.step[0];
            if (!wide) {
                uint8_t* d = row + X0;
                if (ncols == kCols && (((size_t)d) & 7) == 0)
                    *(uint2*)d = make_uint2(yc[0] | yc[1] << 8 | yc[2] << 16 | yc[3] << 24, yc[4] | yc[5] << 8 | yc[6] << 16 | yc[7] << 24);
                else for (int q = 0; q < ncols; ++q) d[q] = (uint8_t)yc[q];
            } else {
                uint16_t* d = (uint16_t*)row + X0;
                if (ncols == kCols && (((size_t)d) & 15) == 0)
                    *(uint4*)d = make_uint4(yc[0] | yc[1] << 16, yc[2] | yc[3] << 16, yc[4] | yc[5] << 16, yc[6] | yc[7] << 16);
                else for (int q = 0; q < ncols; ++q) d[q] = (uint16_t)yc[q];
            }
        }
        // column X0 - 1: the left lane's last column (every lane takes part in the move; lane 0 keeps its own)
        if constexpr (kLeftCol) {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const float from_left = __shfl_up(v[kCols - 1][e], 1);
                if (threadIdx.x != 0) left[e] = from_left;
                if (X0 == 0) left[e] = v[0][e];                      // column -1 clamps to column 0
            }
        }
        if (!active) continue;
        const int nsites = min(kYuvSites, cw - j0);
        unsigned uc[kYuvSites], vc[kYuvSites];
#pragma unroll
        for (int s = 0; s < kYuvSites; ++s) {
            const int qc = 2 * s, qr = min(2 * s + 1, ncols - 1);   // column 2j + 1 clamped to the frame (odd W)
            float f[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) f[e] = kLeftCol ? 0.25f * (s ? v[qc - 1][e] : left[e]) + 0.5f * v[qc][e] + 0.25f * v[qr][e] : 0.5f * v[qc][e] + 0.5f * v[qr][e];
            const float Y = k.kr * f[0] + k.kg * f[1] + k.kb * f[2];
            uc[s] = yuv_code_at<M>(k.c_off, k.c_scale, (f[2] - Y) * k.cb_div, k.maxcode, dz, 1, j0 + s, ci);
            vc[s] = yuv_code_at<M>(k.c_off, k.c_scale, (f[0] - Y) * k.cr_div, k.maxcode, dz, 2, j0 + s, ci);
        }
        if constexpr (kSemi) {                                      // NV12 / P010: U, V, U, V, ... in plane 1
            uint8_t* row = p.dst.p[1] + (size_t)ci * p.dst.step[1];
            if (!wide) {
                uint8_t* d = row + 2 * j0;
                if (nsites == kYuvSites && (((size_t)d) & 7) == 0)
                    *(uint2*)d = make_uint2(uc[0] | vc[0] << 8 | uc[1] << 16 | vc[1] << 24, uc[2] | vc[2] << 8 | uc[3] << 16 | vc[3] << 24);
                else for (int s = 0; s < nsites; ++s) { d[2 * s] = (uint8_t)uc[s]; d[2 * s + 1] = (uint8_t)vc[s]; }
            } else {
                uint16_t* d = (uint16_t*)row + 2 * j0;
                if (nsites == kYuvSites && (((size_t)d) & 15) == 0)
                    *(uint4*)d = make_uint4((uc[0] | vc[0] << 16) << 6, (uc[1] | vc[1] << 16) << 6, (uc[2] | vc[2] << 16) << 6, (uc[3] | vc[3] << 16) << 6);
                else for (int s = 0; s < nsites; ++s) { d[2 * s] = (uint16_t)(uc[s] << 6); d[2 * s + 1] = (uint16_t)(vc[s] << 6); }
            }
            continue;
        }
        for (int pl = 1; pl < 3; ++pl) {
            const unsigned* cc = pl == 1 ? uc : vc;
            uint8_t* row = p.dst.p[pl] + (size_t)ci * p.dst.step[pl];
            if (!wide) {
                uint8_t* d = row + j0;
                if (nsites == kYuvSites && (((size_t)d) & 3) == 0) *(unsigned*)d = cc[0] | cc[1] << 8 | cc[2] << 16 | cc[3] << 24;
                else for (int s = 0; s < nsites; ++s) d[s] = (uint8_t)cc[s];
            } else {
                uint16_t* d = (uint16_t*)row + j0;
                if (nsites == kYuvSites && (((size_t)d) & 7) == 0) *(uint2*)d = make_uint2(cc[0] | cc[1] << 16, cc[2] | cc[3] << 16);
                else for (int s = 0; s < nsites; ++s) d[s] = (uint16_t)cc[s];
            }
        }
    }
}

// compose_kernel for a YUV 4:4:4 output: compose_kernel's launch shape and its four-pixel fast path - a thread owns four consecutive pixels
// of a row and walks a band of kComposeRows rows; where the four share their covering tiles and no TTA is involved, a tile contributes them as two
// 16-byte loads, elsewhere each pixel goes through compose_pixel_sums; the sums and their order are compose_pixel_sums' either way.  Each pixel's R, G, B
// are clamped to [0, 1] and coded on the spot: Y by compose_yuv_kernel's expression (the same bytes on the same canvas), Cb and Cr from the pixel's own
// colour - no filter, no neighbour.  A full group stores 4 bytes per plane (10-bit: 8); the ragged right end stores sample by sample.
template <typename P, int M = kDitherNone, typename... D>
__global__ __launch_bounds__(kComposeThreads) void compose_yuv444_kernel(const ComposeYuvParams p, const D... dzs) {
    static_assert(dither_pack_ok<M, D...>, "kDitherNone: no argument; else one DitherArgs");
    const DitherArgs& dz = dither_of(dzs...);
    constexpr bool kHalf = sizeof(P) == 8;
    const ComposeParams& c = p.c;
    const YuvCoefs& k = p.k;
    const int W = c.outW, H = c.outH;
    const int gw = (W + 3) >> 2;
    const int xg = blockIdx.x * kComposeThreads + threadIdx.x;
    if (xg >= gw) return;
    const P* tiles = (const P*)c.tiles;
    const int To = c.To, n = To - 1;
    const int X = 4 * xg;
    const int np = min(4, W - X);
    int a0 = X - To + 1; a0 = a0 <= 0 ? 0 : (a0 + c.stride_x - 1) / c.stride_x;
    int b0 = X + 3 - To + 1; b0 = b0 <= 0 ? 0 : (b0 + c.stride_x - 1) / c.stride_x;
    const int a1 = min(c.nx - 1, X / c.stride_x), b1 = min(c.nx - 1, (X + 3) / c.stride_x);
    const bool fast = kHalf && np == 4 && !c.tta && a0 == b0 && a1 == b1;
    const bool wide = p.dst.bits > 8;
    const int Y0 = blockIdx.y * kComposeRows, Y1 = min(H, Y0 + kComposeRows);
    for (int Y = Y0; Y < Y1; ++Y) {
        float acc[4][3] = {};
        if (fast) {
            int j0 = Y - To + 1; j0 = j0 <= 0 ? 0 : (j0 + c.stride_y - 1) / c.stride_y;
            const int j1 = min(c.ny - 1, Y / c.stride_y);
            for (int ti = a0; ti <= a1; ++ti) {
                const int ox = ti * c.stride_x, lx = X - ox;
                const int rw = ox + To > W ? W - ox : To;
                for (int tj = j0; tj <= j1; ++tj) {
                    const int oy = tj * c.stride_y, ly = Y - oy;
                    const int rh = oy + To > H ? H - oy : To;
                    const long tile = (long)ti * c.ny + tj - c.first_tile;
                    const half4* tp = (const half4*)c.tiles + tile * (long)To * To + (long)ly * To + lx;
                    half4 h[4];
                    if ((((size_t)tp) & 15) == 0) { const half8 u0 = *(const half8*)tp, u1 = *(const half8*)(tp + 2);
                        h[0] = (half4){u0[0], u0[1], u0[2], u0[3]}; h[1] = (half4){u0[4], u0[5], u0[6], u0[7]}; h[2] = (half4){u1[0], u1[1], u1[2], u1[3]}; h[3] = (half4){u1[4], u1[5], u1[6], u1[7]}; }
                    else { h[0] = tp[0]; h[1] = tp[1]; h[2] = tp[2]; h[3] = tp[3]; }
                    const bool wl = ox > 0, wt = oy > 0 && ly < c.ovy, wr = ox + rw < W, wb = oy + rh < H && n - ly < c.ovy;
                    const float fy_t = wt ? c.ramp_y[ly] : 1.f, fy_b = wb ? c.ramp_y[n - ly] : 1.f;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float v0 = (float)h[q][0], v1 = (float)h[q][1], v2 = (float)h[q][2];
                        if (c.ovx || c.ovy) {
                            const int lk = lx + q;
                            if (wl && lk < c.ovx) { float w = c.ramp_x[lk]; v0 *= w; v1 *= w; v2 *= w; }
                            if (wt) { v0 *= fy_t; v1 *= fy_t; v2 *= fy_t; }
                            if (wr && n - lk < c.ovx) { float w = c.ramp_x[n - lk]; v0 *= w; v1 *= w; v2 *= w; }
                            if (wb) { v0 *= fy_b; v1 *= fy_b; v2 *= fy_b; }
                        }
                        acc[q][0] += v0; acc[q][1] += v1; acc[q][2] += v2;
                    }
                }
            }
        } else {
            for (int q = 0; q < np; ++q) compose_pixel_sums<P>(c, tiles, X + q, Y, acc[q][0], acc[q][1], acc[q][2]);
        }
        unsigned yc[4], uc[4], vc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float o[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) o[e] = fminf(fmaxf(acc[q][e], 0.f), 1.f);
            const float Yn = k.kr * o[0] + k.kg * o[1] + k.kb * o[2];
            yc[q] = yuv_code_at<M>(k.y_off, k.y_scale, Yn, k.maxcode, dz, 0, X + q, Y);
            uc[q] = yuv_code_at<M>(k.c_off, k.c_scale, (o[2] - Yn) * k.cb_div, k.maxcode, dz, 1, X + q, Y);
            vc[q] = yuv_code_at<M>(k.c_off, k.c_scale, (o[0] - Yn) * k.cr_div, k.maxcode, dz, 2, X + q, Y);
        }
        for (int pl = 0; pl < 3; ++pl) {
            const unsigned* cc = pl == 0 ? yc : pl == 1 ? uc : vc;
            uint8_t* row = p.dst.p[pl] + (size_t)Y * p.dst.step[pl];
            if (!wide) {
                uint8_t* d = row + X;
                if (np == 4 && (((size_t)d) & 3) == 0) *(unsigned*)d = cc[0] | cc[1] << 8 | cc[2] << 16 | cc[3] << 24;
                else for (int q = 0; q < np; ++q) d[q] = (uint8_t)cc[q];
            } else {
                uint16_t* d = (uint16_t*)row + X;
                if (np == 4 && (((size_t)d) & 7) == 0) *(uint2*)d = make_uint2(cc[0] | cc[1] << 16, cc[2] | cc[3] << 16);
                else for (int q = 0; q < np; ++q) d[q] = (uint16_t)cc[q];
            }
        }
    }
}

__global__ void se_kernel(const SeParams p) {
    // one block per batch item; tiny (C <= 256)
    extern __shared__ float sm[];
    float* mean = sm;            // [C]
    float* mid = sm + p.C;       // [Cmid]
    float* part = mid + p.Cmid;  // [slices][C]
    const int b = blockIdx.x;
    // add the producing GEMM's per-workgroup partial sums: the workgroups are split into `slices` contiguous ranges (one per
    // thread group), each summed in block order, then the slices are added in slice order - a fixed tree, so deterministic
    const int slices = blockDim.x / p.C > 0 ? blockDim.x / p.C : 1;
    const int per = (p.nblocks + slices - 1) / slices;
    {
        const int c = threadIdx.x % p.C, sl = threadIdx.x / p.C;
        if (sl < slices) {
            float s = 0.f;
            const int t1 = min(p.nblocks, (sl + 1) * per);
            for (int t = sl * per; t < t1; ++t) s += p.pool[((size_t)b * p.nblocks + t) * p.Cs + c];
            part[sl * p.C + c] = s;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < p.C; c += blockDim.x) {
        float s = 0.f;
        for (int sl = 0; sl < slices; ++sl) s += part[sl * p.C + c];
        mean[c] = s * p.inv_count;
    }
    __syncthreads();
    for (int m = threadIdx.x; m < p.Cmid; m += blockDim.x) {
        float a = p.b1[m];
        for (int c = 0; c < p.C; ++c) a += p.w1[m * p.C + c] * mean[c];
        mid[m] = a > 0.f ? a : 0.f;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < p.Cs; c += blockDim.x) {
        float s = 0.f;
        if (c < p.C) {
            float a = p.b2[c];
            for (int m = 0; m < p.Cmid; ++m) a += p.w2[c * p.Cmid + m] * mid[m];
            s = 1.f / (1.f + __expf(-a));
        }
        p.scale[b * p.Cs + c] = s;
    }
}

__global__ __launch_bounds__(256) void scale_kernel(_Float16* x, const float* scale, int B, long HW, int Cs) {
    const int pc = Cs / 8;
    const long total = (long)B * HW * pc;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int cp = (int)(i % pc);
        long pix = i / pc;
        int b = (int)(pix / HW);
        *((half8*)x + i) = gate::gate8(*((half8*)x + i), scale + b * Cs + cp * 8);   // the arithmetic of the folded gates (kernels.h)
    }
}

__global__ __launch_bounds__(256) void scale32_kernel(float* x, const float* scale, int B, long HW, int Cs) {
    const int pc = Cs / 4;
    const long total = (long)B * HW * pc;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cp = (int)(i % pc);
        const int b = (int)(i / pc / HW);
        float4v v = *((float4v*)x + i);
        const float* sc = scale + b * Cs + cp * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= sc[e];
        *((float4v*)x + i) = v;
    }
}

template <typename P>
__global__ __launch_bounds__(256) void blob_to_nhwc_kernel(const float* nchw, P* out, int B, int T) {
    const long total = (long)B * T * T;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int b = (int)(i / ((long)T * T));
        long rem = i - (long)b * T * T;
        const float* s = nchw + (long)b * 3 * T * T + rem;
        out[i] = make_px<P>(s[0], s[(long)T * T], s[2L * T * T]);
    }
}

template <typename P>
__global__ __launch_bounds__(256) void nhwc_to_blob_kernel(const P* in, float* nchw, int B, int T) {
    const long total = (long)B * T * T;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int b = (int)(i / ((long)T * T));
        long rem = i - (long)b * T * T;
        const P v = in[i];
        float* d = nchw + (long)b * 3 * T * T + rem;
        d[0] = (float)v[0]; d[(long)T * T] = (float)v[1]; d[2L * T * T] = (float)v[2];
    }
}

inline unsigned grid_for(long total) { long g = (total + 255) / 256; return (unsigned)(g > 8192 ? 8192 : (g < 1 ? 1 : g)); }

}  // namespace

template <int E>
static hipError_t launch_gather_as(const GatherParams& p, dim3 grid, hipStream_t s) {
    if (p.fp32) hipLaunchKernelGGL((gather_kernel<float4v, E>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((gather_kernel<half4, E>), grid, dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_gather(const GatherParams& p, hipStream_t s, int edge) {
    const dim3 grid(grid_for((long)p.B * p.T * p.T));
    switch (edge) {
        case kEdgeReplicate: return launch_gather_as<kEdgeReplicate>(p, grid, s);
        case kEdgeWrap: return launch_gather_as<kEdgeWrap>(p, grid, s);
        case kEdgeMirror: return launch_gather_as<kEdgeMirror>(p, grid, s);
    }
    return hipErrorInvalidValue;                                    // no kernel for it: an error, never the replicating kernel
}
hipError_t launch_compose(const ComposeParams& p, hipStream_t s, const DitherArgs& d) {
    if (!dither_args_ok(d)) return hipErrorInvalidValue;
    const int gw = (((p.x1 > 0 ? p.x1 : p.outW) - p.x0) + 3) / 4;
    if (gw <= 0 || p.outH <= 0) return hipSuccess;
    const int nrows = (p.y1 > 0 ? p.y1 : p.outH) - p.y0;
    if (nrows <= 0) return hipSuccess;
    const dim3 grid((unsigned)((gw + kComposeThreads - 1) / kComposeThreads), (unsigned)((nrows + kComposeRows - 1) / kComposeRows));
    if (d.mode != kDitherNone) return for_dither(d, [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (p.fp32) hipLaunchKernelGGL((compose_kernel<float4v, M, DitherArgs>), grid, dim3(kComposeThreads), 0, s, p, d);
        else hipLaunchKernelGGL((compose_kernel<half4, M, DitherArgs>), grid, dim3(kComposeThreads), 0, s, p, d);
        return hipGetLastError();
    });
    if (p.fp32) hipLaunchKernelGGL(compose_kernel<float4v>, grid, dim3(kComposeThreads), 0, s, p);
    else hipLaunchKernelGGL(compose_kernel<half4>, grid, dim3(kComposeThreads), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_compose_canvas(const ComposeParams& p, float* canvas, hipStream_t s, const LightArgs& l) {
    const int w = (p.x1 > 0 ? p.x1 : p.outW) - p.x0, h = (p.y1 > 0 ? p.y1 : p.outH) - p.y0;
    if (w <= 0 || h <= 0) return hipSuccess;
    if (!light_args_ok(l)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((w + 255) / 256), (unsigned)(h < 65535 ? h : 65535));
    if (l.mode != kLightGamma) {
        if (p.fp32) hipLaunchKernelGGL((compose_canvas_kernel<float4v, LightArgs>), grid, dim3(256), 0, s, p, canvas, l);
        else hipLaunchKernelGGL((compose_canvas_kernel<half4, LightArgs>), grid, dim3(256), 0, s, p, canvas, l);
        return hipGetLastError();
    }
    if (p.fp32) hipLaunchKernelGGL(compose_canvas_kernel<float4v>, grid, dim3(256), 0, s, p, canvas);
    else hipLaunchKernelGGL(compose_canvas_kernel<half4>, grid, dim3(256), 0, s, p, canvas);
    return hipGetLastError();
}
template <int L, int S = kYuvLeft>
static void launch_gather_yuv_as(const GatherYuvParams& p, dim3 grid, hipStream_t s) {
    if (p.fp32) hipLaunchKernelGGL((gather_yuv_kernel<float4v, L, S>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((gather_yuv_kernel<half4, L, S>), grid, dim3(256), 0, s, p);
}
// The siting a layout tells apart: I444 none, I422 the column rule alone (kYuvTopLeft is kYuvLeft); -1: no such siting
static int yuv_effective_siting(int layout, int siting) {
    if (siting < kYuvLeft || siting > kYuvTopLeft) return -1;
    if (layout == kYuvI444 || (layout == kYuvI422 && siting == kYuvTopLeft)) return kYuvLeft;
    return siting;
}
hipError_t launch_gather_yuv(const GatherYuvParams& p, hipStream_t s) {
    const dim3 grid(grid_for((long)p.B * p.T * p.T));
    switch (yuv_effective_siting(p.src.layout, p.src.siting)) {
        case kYuvLeft:
            switch (p.src.layout) {
                case kYuvI420: launch_gather_yuv_as<kYuvI420>(p, grid, s); break;
                case kYuvI422: launch_gather_yuv_as<kYuvI422>(p, grid, s); break;
                case kYuvI444: launch_gather_yuv_as<kYuvI444>(p, grid, s); break;
                case kYuvNV12: launch_gather_yuv_as<kYuvNV12>(p, grid, s); break;
                default: return hipErrorInvalidValue;               // no kernel for it: an error, never another layout's kernel
            }
            break;
        case kYuvCenter:
            switch (p.src.layout) {
                case kYuvI420: launch_gather_yuv_as<kYuvI420, kYuvCenter>(p, grid, s); break;
                case kYuvI422: launch_gather_yuv_as<kYuvI422, kYuvCenter>(p, grid, s); break;
                case kYuvNV12: launch_gather_yuv_as<kYuvNV12, kYuvCenter>(p, grid, s); break;
                default: return hipErrorInvalidValue;
            }
            break;
        case kYuvTopLeft:
            switch (p.src.layout) {
                case kYuvI420: launch_gather_yuv_as<kYuvI420, kYuvTopLeft>(p, grid, s); break;
                case kYuvNV12: launch_gather_yuv_as<kYuvNV12, kYuvTopLeft>(p, grid, s); break;
                default: return hipErrorInvalidValue;
            }
            break;
        default: return hipErrorInvalidValue;                       // no kernel for it: an error, never another siting's kernel
    }
    return hipGetLastError();
}
// the kernels of mode M with their extra arguments dz: none, or the DitherArgs
template <int L, int S, int M, typename... D>
static void launch_compose_yuv_as(const ComposeYuvParams& p, dim3 grid, hipStream_t s, const D&... dz) {
    if (p.c.fp32) hipLaunchKernelGGL((compose_yuv_kernel<float4v, L, S, M, D...>), grid, dim3(kYuvThreads), 0, s, p, dz...);
    else hipLaunchKernelGGL((compose_yuv_kernel<half4, L, S, M, D...>), grid, dim3(kYuvThreads), 0, s, p, dz...);
}
template <int M, typename... D>
static hipError_t launch_compose_yuv_mode(const ComposeYuvParams& p, hipStream_t s, const D&... dz) {
    if (p.c.outW <= 0 || p.c.outH <= 0) return hipSuccess;
    const int siting = yuv_effective_siting(p.dst.layout, p.dst.siting);
    if (siting < 0) return hipErrorInvalidValue;
    if (p.dst.layout == kYuvI444) {
        const int gw = (p.c.outW + 3) / 4;
        const dim3 grid((unsigned)((gw + kComposeThreads - 1) / kComposeThreads), (unsigned)((p.c.outH + kComposeRows - 1) / kComposeRows));
        if (p.c.fp32) hipLaunchKernelGGL((compose_yuv444_kernel<float4v, M, D...>), grid, dim3(kComposeThreads), 0, s, p, dz...);
        else hipLaunchKernelGGL((compose_yuv444_kernel<half4, M, D...>), grid, dim3(kComposeThreads), 0, s, p, dz...);
        return hipGetLastError();
    }
    const int cw = (p.c.outW + 1) / 2, ch = yuv_chroma_rows(p.c.outH, p.dst.layout);
    const int runs = (cw + kYuvSites - 1) / kYuvSites;
    const dim3 grid((unsigned)((runs + kYuvThreads - 1) / kYuvThreads), (unsigned)(ch < 65535 ? ch : 65535));
    if (siting == kYuvTopLeft) {                                    // a workgroup per band of kYuvBand chroma rows (at most 65535 bands: 1.5 million luma rows)
        const int bands = (ch + kYuvBand - 1) / kYuvBand;
        if (bands > 65535) return hipErrorInvalidValue;
        const dim3 bgrid(grid.x, (unsigned)bands);
        switch (p.dst.layout) {
            case kYuvI420: launch_compose_yuv_as<kYuvI420, kYuvTopLeft, M>(p, bgrid, s, dz...); break;
            case kYuvNV12: launch_compose_yuv_as<kYuvNV12, kYuvTopLeft, M>(p, bgrid, s, dz...); break;
            default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    if (siting == kYuvCenter) {
        switch (p.dst.layout) {
            case kYuvI420: launch_compose_yuv_as<kYuvI420, kYuvCenter, M>(p, grid, s, dz...); break;
            case kYuvI422: launch_compose_yuv_as<kYuvI422, kYuvCenter, M>(p, grid, s, dz...); break;
            case kYuvNV12: launch_compose_yuv_as<kYuvNV12, kYuvCenter, M>(p, grid, s, dz...); break;
            default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    switch (p.dst.layout) {
        case kYuvI420: launch_compose_yuv_as<kYuvI420, kYuvLeft, M>(p, grid, s, dz...); break;
        case kYuvI422: launch_compose_yuv_as<kYuvI422, kYuvLeft, M>(p, grid, s, dz...); break;
        case kYuvNV12: launch_compose_yuv_as<kYuvNV12, kYuvLeft, M>(p, grid, s, dz...); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
hipError_t launch_compose_yuv(const ComposeYuvParams& p, hipStream_t s, const DitherArgs& d) {
    if (!dither_args_ok(d)) return hipErrorInvalidValue;
    if (d.mode == kDitherNone) return launch_compose_yuv_mode<kDitherNone>(p, s);
    return for_dither(d, [&](auto m) { return launch_compose_yuv_mode<decltype(m)::value>(p, s, d); });
}
// (nblocks must be the partials per image the producer wrote: conv3_tiles(p) behind launch_conv3, ceil(Mrows / kGemmBM) behind launch_gemm - se_kernel reads
// pool[b * nblocks + t], the producers write by global tile index)
hipError_t launch_se(const SeParams& p, hipStream_t s) {
    if (p.B <= 0 || p.C <= 0 || p.C > 256 || p.Cs < p.C || p.Cmid <= 0 || p.nblocks <= 0) return hipErrorInvalidValue;
    const int threads = 1024, slices = threads / p.C > 0 ? threads / p.C : 1;
    hipLaunchKernelGGL(se_kernel, dim3(p.B), dim3(threads), (p.C + p.Cmid + slices * p.C) * sizeof(float), s, p);
    return hipGetLastError();
}
hipError_t launch_scale(void* x, const float* scale, int B, int HW, int Cs, bool fp32, hipStream_t s) {
    if (fp32) hipLaunchKernelGGL(scale32_kernel, dim3(grid_for((long)B * HW * (Cs / 4))), dim3(256), 0, s, (float*)x, scale, B, (long)HW, Cs);
    else hipLaunchKernelGGL(scale_kernel, dim3(grid_for((long)B * HW * (Cs / 8))), dim3(256), 0, s, (_Float16*)x, scale, B, (long)HW, Cs);
    return hipGetLastError();
}
hipError_t launch_blob_to_nhwc(const float* nchw, void* out, int B, int T, bool fp32, hipStream_t s) {
    const dim3 grid(grid_for((long)B * T * T));
    if (fp32) hipLaunchKernelGGL(blob_to_nhwc_kernel<float4v>, grid, dim3(256), 0, s, nchw, (float4v*)out, B, T);
    else hipLaunchKernelGGL(blob_to_nhwc_kernel<half4>, grid, dim3(256), 0, s, nchw, (half4*)out, B, T);
    return hipGetLastError();
}
hipError_t launch_nhwc_to_blob(const void* in, float* nchw, int B, int T, bool fp32, hipStream_t s) {
    const dim3 grid(grid_for((long)B * T * T));
    if (fp32) hipLaunchKernelGGL(nhwc_to_blob_kernel<float4v>, grid, dim3(256), 0, s, (const float4v*)in, nchw, B, T);
    else hipLaunchKernelGGL(nhwc_to_blob_kernel<half4>, grid, dim3(256), 0, s, (const half4*)in, nchw, B, T);
    return hipGetLastError();
}

}  // namespace w2x
