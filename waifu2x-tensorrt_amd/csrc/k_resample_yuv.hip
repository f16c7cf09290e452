// Resized YUV output in every layout (renderYuvResized; dst.layout I420, I422, I444 or NV12): the resize of the fp32 RGB canvas that
// resample_kernel (k_resample.hip) does - the 16 x 64 tile, the tap tables, rows_max and the two passes of pixel_device.h - with the encoding of
// compose_yuv_kernel / compose_yuv444_kernel behind it.  The canvas is resized unclamped; R, G, B are clamped to [0, 1] after the resize and coded with the
// expressions below, one statement of each for all four kernels.  launch_resample_yuv, at the end, is the one entry.
//
//   resample_yuv444_kernel   the two shared passes (resample_pass1 / resample_pass2: a thread per four pixels of a row, float4 LDS reads, no halo); each pixel
//                            codes Y, Cb and Cr from its own clamped colour.  4 samples per plane and store.
//   resample_yuv422_kernel   the same shape, two chroma sites per thread: site j filters columns 2j - 1, 2j, 2j + 1 of its own row (1/4, 1/2, 1/4, indices clamped
//                            to the frame).  Column 2j - 1 of a thread's first site is the last column of the lane on its left; the first thread of a tile row
//                            takes it from the halo, output column ox0 - 1 (clamped at 0), which pass 1 filters as a 65th column.
//   resample_yuv_kernel      4:2:0, a thread per chroma site = 2 x 2 pixels (resample_yuv420): I420, U and V in planes 1 and 2.
//   resample_yuv_nv12_kernel the same body: U and V interleaved in plane 1, every code << 6 at 10 bits (P010).
#include "pixel_device.h"

#include <type_traits>

namespace w2x {
namespace {

// The encoding expressions, each rounding stated (no contraction left to the compiler), so that the byte equalities between the layouts - the Y plane of every
// layout is I420's, NV12 holds I420's samples - hold by the source and not by what a compiler makes of it.  They are the forms the first I420 kernel had as
// compiled for gfx950, whose output the later ones had to meet: it fused the last product of Y' = kr R + kg G + kb B on the odd rows of the frame (the second
// row of a chroma site) and rounded it on its own on the even rows; the chroma expressions were fused throughout.  A fused operation is
// stated by __fmaf_rn; an operation that must not fuse with its neighbour needs contraction switched off around it, as in luma_even_row - the one place where a
// product feeds a sum that is not meant to be an fma.  Everywhere else a product feeds an __fmaf_rn or a sum feeds a product, which nothing can contract.
__device__ __forceinline__ unsigned yuv_code(float off, float scale, float v, int maxcode) { return (unsigned)min(max(__float2int_rn(__fmaf_rn(scale, v, off)), 0), maxcode); }
// M: the code of sample (x, y) of plane c (Y, U, V = 0, 1, 2; chroma samples in their own plane's coordinates, NV12's as the I420 samples they are).
// kDitherNone is yuv_code; a dithered mode adds the sample's threshold to the same fused value and rounds down (dither_code, prepost_device.h).
template <int M>
__device__ __forceinline__ unsigned yuv_code_at(float off, float scale, float v, int maxcode, const DitherArgs& dz, int c, int x, int y) {
    if constexpr (M == kDitherNone) return yuv_code(off, scale, v, maxcode);
    else return dither_code<M>(__fmaf_rn(scale, v, off), dither_t<M>(dz, c, x, y), maxcode);
}
__device__ __forceinline__ float luma_fused(const YuvCoefs& k, float r, float g, float b) { return __fmaf_rn(k.kb, b, __fmaf_rn(k.kr, r, __fmul_rn(k.kg, g))); }
__device__ __forceinline__ float luma_even_row(const YuvCoefs& k, float r, float g, float b) {
#pragma clang fp contract(off)   // (__fadd_rn / __fmul_rn are `+` and `*` to the compiler, which fuses them where it may: only this keeps kb * b a product of its own)
    const float pb = k.kb * b;
    return pb + __fmaf_rn(k.kr, r, k.kg * g);
}
__device__ __forceinline__ float luma_of_row(const YuvCoefs& k, int Y, float r, float g, float b) { return (Y & 1) ? luma_fused(k, r, g, b) : luma_even_row(k, r, g, b); }
// a chroma site's colour from the columns 2j - 1, 2j, 2j + 1 (1/4, 1/2, 1/4)
__device__ __forceinline__ float site_filter(float left, float mid, float right) { return __fmaf_rn(0.25f, right, __fmaf_rn(0.25f, left, __fmul_rn(0.5f, mid))); }
// centred columns: the mean of columns 2j and 2j + 1
__device__ __forceinline__ float site_mean(float mid, float right) { return __fmul_rn(0.5f, __fadd_rn(mid, right)); }
// co-sited rows: rows 2i - 1, 2i, 2i + 1 by (1/4, 1/2, 1/4)
__device__ __forceinline__ float rows_cosited(float above, float mid, float below) { return __fmaf_rn(0.25f, below, __fmaf_rn(0.25f, above, __fmul_rn(0.5f, mid))); }
__device__ __forceinline__ float chroma_of(float c, float y, float div) { return __fmul_rn(__fsub_rn(c, y), div); }

// Four consecutive codes of one plane's row from column X (a multiple of 4): np == 4 and an aligned address leave as one store of 4 (10 bits: 8) bytes, a run
// cut by the right edge (or a caller's unaligned rows) sample by sample
__device__ __forceinline__ void store_codes4(uint8_t* row, int X, int np, const unsigned (&q)[4], bool wide) {
    if (!wide) {
        uint8_t* d = row + X;
        if (np == 4 && (((size_t)d) & 3) == 0) *(unsigned*)d = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
        else for (int k = 0; k < np; ++k) d[k] = (uint8_t)q[k];
    } else {
        uint16_t* d = (uint16_t*)row + X;
        if (np == 4 && (((size_t)d) & 7) == 0) *(uint2*)d = make_uint2(q[0] | q[1] << 16, q[2] | q[3] << 16);
        else for (int k = 0; k < np; ++k) d[k] = (uint16_t)q[k];
    }
}

// ---- 4:4:4.  LDS [3][rows_max][kRsCols] fp32: resample_kernel's, 58.5 KiB at a factor of 4 with bicubic taps, two workgroups per CU
template <int M = kDitherNone, typename... D>
__global__ __launch_bounds__(kRsThreads) void resample_yuv444_kernel(const ResampleYuvParams p, const D... dzs) {
    static_assert(dither_pack_ok<M, D...>, "kDitherNone: no DitherArgs, else one; then one LightArgs or none");
    const DitherArgs& dz = dither_of(dzs...);
    constexpr bool kLin = light_on<D...>;                                 // (R, G, B are encoded where they are clamped, ahead of the matrix)
    const LightArgs& lz = light_of(dzs...);
    extern __shared__ float h[];
    const int r0 = resample_pass1<3>(p, h);
    __syncthreads();
    float4v a[3];
    int X, Y, np;
    if (!resample_pass2<3>(p, h, r0, a, X, Y, np)) return;
    const YuvCoefs& k = p.k;
    unsigned yc[4], uc[4], vc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float o0 = sat01_out<kLin>(lz, a[0][q]), o1 = sat01_out<kLin>(lz, a[1][q]), o2 = sat01_out<kLin>(lz, a[2][q]);
        const float Yn = luma_of_row(k, Y, o0, o1, o2);
        yc[q] = yuv_code_at<M>(k.y_off, k.y_scale, Yn, k.maxcode, dz, 0, X + q, Y);
        uc[q] = yuv_code_at<M>(k.c_off, k.c_scale, chroma_of(o2, Yn, k.cb_div), k.maxcode, dz, 1, X + q, Y);
        vc[q] = yuv_code_at<M>(k.c_off, k.c_scale, chroma_of(o0, Yn, k.cr_div), k.maxcode, dz, 2, X + q, Y);
    }
    const bool wide = p.dst.bits > 8;
    store_codes4(p.dst.p[0] + (size_t)Y * p.dst.step[0], X, np, yc, wide);
    store_codes4(p.dst.p[1] + (size_t)Y * p.dst.step[1], X, np, uc, wide);
    store_codes4(p.dst.p[2] + (size_t)Y * p.dst.step[2], X, np, vc, wide);
}

// ---- 4:2:2.  LDS: [3][rows_max][kRsCols] fp32, resample_kernel's image at its pitch of 64 dwords, and behind it the halo column as [3][rows_max].
// Banks (ds_read_b128: address / 4 mod 64 within groups of 16 lanes that hold eight lanes of one output row and eight of the next): at a pitch of 64 the 16 lanes
// of a row read the row's 16 slots of 16 bytes whichever input row each output row starts at, so the reads are conflict free as resample_kernel's are.  A pitch
// of 68, which would keep the halo inside the row, shifts a row's slots by its row number: two output rows whose input rows lie d apart then share 8 - |d mod 16|
// slots in a group - a two-way conflict at every factor but one.  Hence the halo lies apart.  Pass 1 writes 65 values per input row from consecutive lanes
// (ds_write_b32: address / 4 mod 32 within 32 lanes): 32 lanes hold at most one row end, so their image addresses are 32 consecutive dwords less one gap and
// the one halo dword falls on a bank in use - two lanes on one bank at most, which a 4-byte store hides.  The halo is read by the first lane of each tile row
// (4 lanes of a wave, ds_read_b32), rows a few dwords apart.
// At a factor of 4 with bicubic taps rows_max <= 78: 3 * 78 * 65 * 4 B = 59.4 KiB, two workgroups per CU.
// S: kYuvLeft is the above (resample_yuv422_kernel).  kYuvCenter: site j is the mean of columns 2j and 2j + 1 - pass 1 filters no halo column and
// nothing crosses lanes before the stores.  (I422 has no row rule: kYuvTopLeft is kYuvLeft.)
template <int S, int M = kDitherNone, typename... D>
__global__ __launch_bounds__(kRsThreads) void resample_yuv422_kernel(const ResampleYuvParams p, const D... dzs) {
    static_assert(dither_pack_ok<M, D...>, "kDitherNone: no DitherArgs, else one; then one LightArgs or none");
    const DitherArgs& dz = dither_of(dzs...);
    constexpr bool kLin = light_on<D...>;                                 // (every pixel, the halo column's included, is encoded before the site filter reads it)
    const LightArgs& lz = light_of(dzs...);
    constexpr bool kLeftCol = S != kYuvCenter;
    extern __shared__ __attribute__((aligned(16))) float h422[];   // (the alignment stated: pass 2 reads 16 bytes per lane and plane, ds_read_b128)
    float* const h = h422;
    const int rm = p.rows_max;
    float* const halo = h + 3 * rm * kRsCols;
    const int ox0 = blockIdx.x * kRsCols, oy0 = blockIdx.y * kRsRows;
    const int r0 = resample_pass1_to<3, kLeftCol>(p, h, [rm](int q, int r, int c) { return c == kRsCols ? 3 * rm * kRsCols + q * rm + r : (q * rm + r) * kRsCols + c; });
    __syncthreads();
    // pass 2: four pixels = two chroma sites of one row per thread.  No lane leaves before the cross-lane moves below: lanes outside the frame carry zeros.
    const YuvCoefs& k = p.k;
    const int ty = threadIdx.x / (kRsCols / 4), cg = threadIdx.x % (kRsCols / 4);
    const int Y = oy0 + ty, X = ox0 + 4 * cg;
    const bool active = Y < p.outH && X < p.outW;
    const int np = active ? min(4, p.outW - X) : 0;
    float4v a[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    float hl[3] = {0.f, 0.f, 0.f};                                        // column ox0 - 1 of the row: the first lane of a tile row
    if (active) {
        const int f = p.fy[Y];
        const int n = min(p.ky, p.inH - f);
        const float* w = p.wy + (size_t)Y * p.ky;
        for (int t = 0; t < n; ++t) {
            const float wk = w[t];
            const int r = f - r0 + t;
#pragma unroll
            for (int e = 0; e < 3; ++e) a[e] += wk * *(const float4v*)&h[(e * rm + r) * kRsCols + 4 * cg];
        }
        if (kLeftCol && cg == 0)
            for (int t = 0; t < n; ++t) {
                const float wk = w[t];
#pragma unroll
                for (int e = 0; e < 3; ++e) hl[e] += wk * halo[e * rm + f - r0 + t];
            }
    }
    float o[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 3; ++e) o[q][e] = sat01_out<kLin>(lz, a[e][q]);
    unsigned yc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) yc[q] = yuv_code_at<M>(k.y_off, k.y_scale, luma_of_row(k, Y, o[q][0], o[q][1], o[q][2]), k.maxcode, dz, 0, X + q, Y);
    unsigned uc[2], vc[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        float f[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            float left = 0.f;
            if constexpr (kLeftCol) {
                if (s == 0) {
                    const float from_left = __shfl_up(o[3][e], 1);        // (the lane on the left is of the same row for every cg > 0)
                    left = cg ? from_left : sat01_out<kLin>(lz, hl[e]);
                } else left = o[1][e];
            }
            const float right = 2 * s + 1 < np ? o[2 * s + 1][e] : o[2 * s][e];   // column 2j + 1 clamped to the frame (odd widths)
            f[e] = kLeftCol ? site_filter(left, o[2 * s][e], right) : site_mean(o[2 * s][e], right);
        }
        const float Yn = luma_fused(k, f[0], f[1], f[2]);
        uc[s] = yuv_code_at<M>(k.c_off, k.c_scale, chroma_of(f[2], Yn, k.cb_div), k.maxcode, dz, 1, (X >> 1) + s, Y);   // (site (X / 2 + s, Y) of the chroma plane)
        vc[s] = yuv_code_at<M>(k.c_off, k.c_scale, chroma_of(f[0], Yn, k.cr_div), k.maxcode, dz, 2, (X >> 1) + s, Y);
    }
    // chroma stores: the two sites of an odd lane go out through the even lane on its left where the pair's eight pixels are whole and its rows are aligned
    const unsigned uu = uc[0] | uc[1] << 16, vv = vc[0] | vc[1] << 16;
    const unsigned nu = __shfl_down(uu, 1), nv = __shfl_down(vv, 1);
    if (!active) return;
    const bool wide = p.dst.bits > 8;
    const int sh = wide ? 1 : 0;                                           // log2 bytes per sample
    store_codes4(p.dst.p[0] + (size_t)Y * p.dst.step[0], X, np, yc, wide);
    uint8_t* const rowu = p.dst.p[1] + (size_t)Y * p.dst.step[1];
    uint8_t* const rowv = p.dst.p[2] + (size_t)Y * p.dst.step[2];
    const int Xr = ox0 + 4 * (cg & ~1);                                    // the pair's first pixel, a multiple of 8: its first site is Xr / 2
    const size_t cmask = wide ? 7 : 3;
    const bool packed = Xr + 8 <= p.outW && ((((size_t)rowu + ((size_t)(Xr >> 1) << sh)) | ((size_t)rowv + ((size_t)(Xr >> 1) << sh))) & cmask) == 0;
    if (packed) {
        if (cg & 1) return;
        if (!wide) {
            *(unsigned*)(rowu + (Xr >> 1)) = (uu & 0xff) | (uu >> 16) << 8 | (nu & 0xff) << 16 | (nu >> 16) << 24;
            *(unsigned*)(rowv + (Xr >> 1)) = (vv & 0xff) | (vv >> 16) << 8 | (nv & 0xff) << 16 | (nv >> 16) << 24;
        } else {
            *(uint2*)(rowu + Xr) = make_uint2(uu, nu);
            *(uint2*)(rowv + Xr) = make_uint2(vv, nv);
        }
        return;
    }
    const int ns = (np + 1) >> 1, j = X >> 1;
    if (!wide) {
        for (int s = 0; s < ns; ++s) { rowu[j + s] = (uint8_t)(s ? uc[1] : uc[0]); rowv[j + s] = (uint8_t)(s ? vc[1] : vc[0]); }
    } else {
        for (int s = 0; s < ns; ++s) { ((uint16_t*)rowu)[j + s] = (uint16_t)(s ? uc[1] : uc[0]); ((uint16_t*)rowv)[j + s] = (uint16_t)(s ? vc[1] : vc[0]); }
    }
}

// ---- 4:2:0: I420 and, with kNV12, NV12 / P010 - the samples are the same, only the stores differ: U and V of a site in planes 1 and 2, or side by side in
// plane 1 with, at 10 bits, every code in the high bits.
// The tile and pass 1 are resample_kernel's, over one more column: chroma site j filters the luma columns 2j - 1, 2j, 2j + 1, and tile origins are multiples of
// 16 rows and 64 columns, so every site and both of its rows lie in one tile and the only value from outside is output column ox0 - 1 (clamped at 0), the halo,
// kept at column kRsCols of the LDS rows.  Pass 2: a thread per chroma site = 2 x 2 luma pixels, 32 sites of one chroma row per half wave.  It filters columns
// 2j, 2j + 1 of its two rows vertically out of LDS (a float2 per plane and tap), clamps them to [0, 1], codes Y, averages the two rows, takes column 2j - 1 from
// the lane on its left (lanes 0 and 32, the row's first sites, from the halo, which lanes 0 .. 3 of the wave filter for its four luma rows) and codes Cb / Cr.
// Four neighbouring lanes then pass their codes to the first of them, which stores 8 luma samples per row and 4 + 4 chroma samples in one store each (8 or 16
// bytes of Y; 4 or 8 of U and of V, or 8 or 16 of UV); a run cut by the right edge (or a caller's unaligned rows) stores sample by sample.
// LDS: [3][rows_max][kYP] fp32.  kYP = 66: even, so the float2 reads of pass 2 are 8-byte aligned; a half wave reads 64 consecutive dwords of one row
// (ds_read_b64 banks: address / 4 mod 64 within 32 lanes), conflict free whatever the pitch, and the halo reads of lanes 0 .. 3 hit rows 66 dwords apart
// (banks 2 apart).  Pass 1 writes 65 consecutive dwords per row, rows 66 apart: at most two lanes of 32 on one bank, which a 4-byte store hides.
// At a factor of 4 with bicubic taps rows_max <= 78: 3 * 78 * 66 * 4 B = 60.3 KiB, two workgroups per CU.
constexpr int kYP = kRsCols + 2;
typedef float float2v __attribute__((ext_vector_type(2)));

// S: kYuvLeft is the above.  kYuvCenter: site j is the mean of columns 2j and 2j + 1 of the two rows averaged - no halo column in pass 1, no move
// from the lane on the left.  kYuvTopLeft: a site filters rows 2i - 1, 2i, 2i + 1 (1/4, 1/2, 1/4), then the columns as kYuvLeft.  Row 2i - 1 of a tile's
// first chroma row is output row oy0 - 1 of the tile above: a ROW halo, handled as the column halo is - pass 1 starts at the input rows that row reaches
// (resample_pass1_to's kAbove; rows_max is resample_rows_max(.., 1), one output row's stride of input rows more) and every thread filters row 2i - 1 at its two
// columns itself (row -1 clamps to row 0), lanes 0 .. 4 of a wave the halo column of its five luma rows.  That is 3 vertical filters per thread where kYuvLeft
// has 2; the horizontal pass, the kernel's larger part at 17 taps, grows by one output row's reach in 16.
// LDS at a factor of 4 with bicubic taps: rows_max <= 82 (16 * 4 + 1 + 17), 3 * 82 * 66 * 4 B = 63.4 KiB - two workgroups per CU still fit the CU's 160 KiB.
// kLin: every resized pixel - the two or three rows of a site, the halo column's and the row halo's included - is encoded where it is clamped, so the
// site filters, which are defined on encoded values, read V.
template <bool kNV12, int S = kYuvLeft, int M = kDitherNone, bool kLin = false>
__device__ __forceinline__ void resample_yuv420(const ResampleYuvParams& p, float* h, const DitherArgs& dz, const LightArgs& lz) {   // h: [3][rows_max][kYP], columns 0 .. 63 the tile's, 64 the halo
    constexpr bool kLeftCol = S != kYuvCenter, kAbove = S == kYuvTopLeft;
    const int ox0 = blockIdx.x * kRsCols, oy0 = blockIdx.y * kRsRows;
    const int rm = p.rows_max;
    const int r0 = resample_pass1_to<3, kLeftCol, kAbove>(p, h, [rm](int q, int r, int c) { return (q * rm + r) * kYP + c; });
    __syncthreads();
    // pass 2: a chroma site per thread.  No lane leaves before the cross-lane moves below: lanes outside the frame carry zeros.
    const YuvCoefs& k = p.k;
    const int lane = threadIdx.x % 64, ci = threadIdx.x / 32, cj = threadIdx.x % 32;
    const int Ya = oy0 + 2 * ci, X0 = ox0 + 2 * cj;
    const bool active = Ya < p.outH && X0 < p.outW;
    const bool has_b = Ya + 1 < p.outH, has_r = X0 + 1 < p.outW;          // odd sizes: row 2i + 1 / column 2j + 1 clamp to the frame
    // output row Y filtered vertically at LDS columns col .. col + N - 1, per plane
    auto vertical = [&](int Y, int col, auto* acc) {
        const int f = p.fy[Y];
        const int n = min(p.ky, p.inH - f);
        const float* w = p.wy + (size_t)Y * p.ky;
        const float* s = h + (f - r0) * kYP + col;
        for (int t = 0; t < n; ++t) {
            const float wk = w[t];
#pragma unroll
            for (int e = 0; e < 3; ++e) acc[e] += wk * *(const std::remove_reference_t<decltype(acc[0])>*)&s[(e * rm + t) * kYP];
        }
    };
    float2v a[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}}, b[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};   // rows 2i, 2i + 1: columns 2j, 2j + 1 of R, G, B
    float2v z[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};                  // kAbove: row 2i - 1
    if (active) {
        vertical(Ya, 2 * cj, a);
        if (has_b) vertical(Ya + 1, 2 * cj, b);
        if constexpr (kAbove) vertical(max(Ya - 1, 0), 2 * cj, z);
    }
    float halo[3] = {0.f, 0.f, 0.f};                                      // lanes 0 .. 3: column ox0 - 1 of the wave's four luma rows
    if constexpr (kAbove) {                                               // lanes 0 .. 4: of the row above them and the four
        const int Yh = oy0 + 4 * (int)(threadIdx.x / 64) - 1 + lane;
        if (lane < 5 && Yh < p.outH) vertical(max(Yh, 0), kRsCols, halo);
    } else if constexpr (kLeftCol) {
        if (lane < 4 && oy0 + 4 * (int)(threadIdx.x / 64) + lane < p.outH) vertical(oy0 + 4 * (int)(threadIdx.x / 64) + lane, kRsCols, halo);
    }
    float vl[3], vr[3], left[3];                                          // the site's columns 2j, 2j + 1 and 2j - 1, the two rows averaged
    unsigned ya[2], yb[2];
    {
        float oa[2][3], ob[2][3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            oa[0][e] = sat01_out<kLin>(lz, a[e][0]); oa[1][e] = sat01_out<kLin>(lz, a[e][1]);
            ob[0][e] = has_b ? sat01_out<kLin>(lz, b[e][0]) : oa[0][e]; ob[1][e] = has_b ? sat01_out<kLin>(lz, b[e][1]) : oa[1][e];
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            ya[q] = yuv_code_at<M>(k.y_off, k.y_scale, luma_even_row(k, oa[q][0], oa[q][1], oa[q][2]), k.maxcode, dz, 0, X0 + q, Ya);
            yb[q] = yuv_code_at<M>(k.y_off, k.y_scale, luma_fused(k, ob[q][0], ob[q][1], ob[q][2]), k.maxcode, dz, 0, X0 + q, Ya + 1);
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            if constexpr (kAbove) {
                vl[e] = rows_cosited(sat01_out<kLin>(lz, z[e][0]), oa[0][e], ob[0][e]);
                vr[e] = has_r ? rows_cosited(sat01_out<kLin>(lz, z[e][1]), oa[1][e], ob[1][e]) : vl[e];
            } else {
                vl[e] = __fmul_rn(0.5f, __fadd_rn(oa[0][e], ob[0][e]));
                vr[e] = has_r ? __fmul_rn(0.5f, __fadd_rn(oa[1][e], ob[1][e])) : vl[e];
            }
        }
    }
    if constexpr (kAbove) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {                                     // the halo column of rows 2i - 1, 2i, 2i + 1: lanes 2 hw, 2 hw + 1, 2 hw + 2 of the wave
            const float hc = sat01_out<kLin>(lz, halo[e]);
            const float hz = __shfl(hc, 2 * (lane / 32)), ha = __shfl(hc, 2 * (lane / 32) + 1), hb = __shfl(hc, 2 * (lane / 32) + 2);
            const float from_left = __shfl_up(vr[e], 1);
            left[e] = cj ? from_left : rows_cosited(hz, ha, has_b ? hb : ha);
        }
    } else if constexpr (kLeftCol) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const float hc = sat01_out<kLin>(lz, halo[e]);
            const float ha = __shfl(hc, 2 * (lane / 32)), hb = __shfl(hc, 2 * (lane / 32) + 1);
            const float from_left = __shfl_up(vr[e], 1);
            left[e] = cj ? from_left : __fmul_rn(0.5f, __fadd_rn(ha, has_b ? hb : ha));
        }
    }
    const bool wide = p.dst.bits > 8;
    const int sbits = wide ? 16 : 8, up = kNV12 && wide ? 6 : 0;          // bits per stored sample; P010: the code in the high ten bits
    unsigned uc, vc;
    {
        float f[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) f[e] = kLeftCol ? site_filter(left[e], vl[e], vr[e]) : site_mean(vl[e], vr[e]);
        const float Y = luma_fused(k, f[0], f[1], f[2]);
        if constexpr (M == kDitherNone) {
            uc = yuv_code(k.c_off, k.c_scale, chroma_of(f[2], Y, k.cb_div), k.maxcode) << up;
            vc = yuv_code(k.c_off, k.c_scale, chroma_of(f[0], Y, k.cr_div), k.maxcode) << up;
        } else {                                                           // site (j, i) of the chroma plane, NV12 too
            uc = yuv_code_at<M>(k.c_off, k.c_scale, chroma_of(f[2], Y, k.cb_div), k.maxcode, dz, 1, X0 >> 1, Ya >> 1) << up;
            vc = yuv_code_at<M>(k.c_off, k.c_scale, chroma_of(f[0], Y, k.cr_div), k.maxcode, dz, 2, X0 >> 1, Ya >> 1) << up;
        }
    }
    // stores: the run of four sites the lane belongs to goes out through its first lane where the run is whole and its rows are aligned
    const int sh = wide ? 1 : 0;                                           // log2 bytes per sample
    const int Xr = ox0 + 2 * (cj & ~3), ic = Ya >> 1, j = X0 >> 1;
    uint8_t* const rowa = p.dst.p[0] + (size_t)Ya * p.dst.step[0];
    uint8_t* const rowb = rowa + p.dst.step[0];
    uint8_t* const rowu = p.dst.p[1] + (size_t)ic * p.dst.step[1];        // NV12: U, V, U, V, ...: site j at samples 2j, 2j + 1
    uint8_t* const rowv = kNV12 ? rowu : p.dst.p[2] + (size_t)ic * p.dst.step[2];
    const size_t ymask = wide ? 15 : 7, cmask = wide ? 7 : 3;
    const bool chroma_aligned = kNV12 ? (((size_t)rowu + ((size_t)Xr << sh)) & ymask) == 0
                                      : ((((size_t)rowu + ((size_t)(Xr >> 1) << sh)) | ((size_t)rowv + ((size_t)(Xr >> 1) << sh))) & cmask) == 0;
    const bool packed = Xr + 8 <= p.outW && ((((size_t)rowa + ((size_t)Xr << sh)) | p.dst.step[0]) & ymask) == 0 && chroma_aligned;
    const unsigned wa = (ya[0] | ya[1] << sbits) << up, wb = (yb[0] | yb[1] << sbits) << up;
    const unsigned uv = uc | vc << (kNV12 ? sbits : 16);                   // NV12: as the pair lies in plane 1
    unsigned qa[4] = {wa, 0, 0, 0}, qb[4] = {wb, 0, 0, 0}, qc[4] = {uv, 0, 0, 0};
#pragma unroll
    for (int q = 1; q < 4; ++q) { qa[q] = __shfl_down(wa, q); qb[q] = __shfl_down(wb, q); qc[q] = __shfl_down(uv, q); }
    if (!active) return;
    if (packed) {
        if (cj & 3) return;
        if (!wide) {
            *(uint2*)(rowa + Xr) = make_uint2(qa[0] | qa[1] << 16, qa[2] | qa[3] << 16);
            if (has_b) *(uint2*)(rowb + Xr) = make_uint2(qb[0] | qb[1] << 16, qb[2] | qb[3] << 16);
            if constexpr (kNV12) *(uint2*)(rowu + Xr) = make_uint2(qc[0] | qc[1] << 16, qc[2] | qc[3] << 16);
            else {
                *(unsigned*)(rowu + (Xr >> 1)) = (qc[0] & 0xff) | (qc[1] & 0xff) << 8 | (qc[2] & 0xff) << 16 | (qc[3] & 0xff) << 24;
                *(unsigned*)(rowv + (Xr >> 1)) = (qc[0] >> 16) | (qc[1] >> 16) << 8 | (qc[2] >> 16) << 16 | (qc[3] >> 16) << 24;
            }
        } else {
            *(uint4*)(rowa + 2 * (size_t)Xr) = make_uint4(qa[0], qa[1], qa[2], qa[3]);
            if (has_b) *(uint4*)(rowb + 2 * (size_t)Xr) = make_uint4(qb[0], qb[1], qb[2], qb[3]);
            if constexpr (kNV12) *(uint4*)(rowu + 2 * (size_t)Xr) = make_uint4(qc[0], qc[1], qc[2], qc[3]);
            else {
                *(uint2*)(rowu + Xr) = make_uint2((qc[0] & 0xffff) | qc[1] << 16, (qc[2] & 0xffff) | qc[3] << 16);
                *(uint2*)(rowv + Xr) = make_uint2(qc[0] >> 16 | (qc[1] & 0xffff0000u), qc[2] >> 16 | (qc[3] & 0xffff0000u));
            }
        }
        return;
    }
    const int nc = has_r ? 2 : 1, ju = kNV12 ? X0 : j, jv = kNV12 ? X0 + 1 : j;   // the samples of U and V in their rows
    if (!wide) {
        for (int q = 0; q < nc; ++q) { rowa[X0 + q] = (uint8_t)(wa >> 8 * q); if (has_b) rowb[X0 + q] = (uint8_t)(wb >> 8 * q); }
        rowu[ju] = (uint8_t)uc; rowv[jv] = (uint8_t)vc;
    } else {
        for (int q = 0; q < nc; ++q) { ((uint16_t*)rowa)[X0 + q] = (uint16_t)(wa >> 16 * q); if (has_b) ((uint16_t*)rowb)[X0 + q] = (uint16_t)(wb >> 16 * q); }
        ((uint16_t*)rowu)[ju] = (uint16_t)uc; ((uint16_t*)rowv)[jv] = (uint16_t)vc;
    }
}

// M: kDitherNone - no further argument - is the kernel the undithered engine launches; a dithered mode takes its DitherArgs behind p (dither_of)
template <int M = kDitherNone, typename... D>
__global__ __launch_bounds__(kRsThreads) void resample_yuv_kernel(const ResampleYuvParams p, const D... dzs) {
    static_assert(dither_pack_ok<M, D...>, "kDitherNone: no DitherArgs, else one; then one LightArgs or none");
    extern __shared__ float h[];
    resample_yuv420<false, kYuvLeft, M, light_on<D...>>(p, h, dither_of(dzs...), light_of(dzs...));
}
template <int M = kDitherNone, typename... D>
__global__ __launch_bounds__(kRsThreads) void resample_yuv_nv12_kernel(const ResampleYuvParams p, const D... dzs) {
    static_assert(dither_pack_ok<M, D...>, "kDitherNone: no DitherArgs, else one; then one LightArgs or none");
    extern __shared__ float h[];
    resample_yuv420<true, kYuvLeft, M, light_on<D...>>(p, h, dither_of(dzs...), light_of(dzs...));
}
// the other sitings of the pair
template <bool kNV12, int S, int M = kDitherNone, typename... D>
__global__ __launch_bounds__(kRsThreads) void resample_yuv_sited_kernel(const ResampleYuvParams p, const D... dzs) {
    static_assert(dither_pack_ok<M, D...>, "kDitherNone: no DitherArgs, else one; then one LightArgs or none");
    extern __shared__ float h[];
    resample_yuv420<kNV12, S, M, light_on<D...>>(p, h, dither_of(dzs...), light_of(dzs...));
}

}  // namespace

// dst.layout picks the kernel.  The layouts beside I420 also ask for a canvas and for every plane of the layout, with a step that holds its row and 10-bit
// planes at even addresses.
hipError_t launch_resample_yuv(const ResampleYuvParams& params, int rows_max_above, hipStream_t s, const DitherArgs& d, const LightArgs& l) {
    if (!dither_args_ok(d) || !light_args_ok(l)) return hipErrorInvalidValue;
    ResampleYuvParams p = params;
    if (p.outW <= 0 || p.outH <= 0) return hipSuccess;
    if (p.dst.rows != p.outH || p.dst.cols != p.outW || (p.dst.bits != 8 && p.dst.bits != 10)) return hipErrorInvalidValue;
    const int layout = p.dst.layout;
    if (layout != kYuvI420) {
        if (layout != kYuvI422 && layout != kYuvI444 && layout != kYuvNV12) return hipErrorInvalidValue;
        if (!p.canvas) return hipErrorInvalidValue;
        const size_t bps = p.dst.bits > 8 ? 2 : 1;
        for (int i = 0; i < (layout == kYuvNV12 ? 2 : 3); ++i) {
            const size_t samples = (size_t)(i ? yuv_chroma_samples(p.outW, layout) : p.outW);
            if (!p.dst.p[i] || p.dst.step[i] < samples * bps || ((((size_t)p.dst.p[i]) | p.dst.step[i]) & (bps - 1)) != 0) return hipErrorInvalidValue;
        }
    }
    // the siting the layout tells apart: I444 none, I422 the column rule alone
    if (p.dst.siting < kYuvLeft || p.dst.siting > kYuvTopLeft) return hipErrorInvalidValue;
    const int siting = layout == kYuvI444 || (layout == kYuvI422 && p.dst.siting == kYuvTopLeft) ? kYuvLeft : p.dst.siting;
    // the kernels of mode M with their extra arguments dz (none, the DitherArgs, the LightArgs or both: for_modes); the LDS opt-in masks are per instantiation of this body
    auto go = [&](auto m, const auto&... dz) -> hipError_t {
        constexpr int M = decltype(m)::value;
        if (siting != kYuvLeft) {
            static unsigned done_c = 0, done_cn = 0, done_c422 = 0, done_t = 0, done_tn = 0;
            const bool tl = siting == kYuvTopLeft;
            switch (layout) {
                case kYuvI420: return tl ? launch_resample_tiles(resample_yuv_sited_kernel<false, kYuvTopLeft, M, std::decay_t<decltype(dz)>...>, 3 * kYP, p.rows_max, done_t, p.outW, p.outH, s, p, dz...)
                                         : launch_resample_tiles(resample_yuv_sited_kernel<false, kYuvCenter, M, std::decay_t<decltype(dz)>...>, 3 * kYP, p.rows_max, done_c, p.outW, p.outH, s, p, dz...);
                case kYuvNV12: return tl ? launch_resample_tiles(resample_yuv_sited_kernel<true, kYuvTopLeft, M, std::decay_t<decltype(dz)>...>, 3 * kYP, p.rows_max, done_tn, p.outW, p.outH, s, p, dz...)
                                         : launch_resample_tiles(resample_yuv_sited_kernel<true, kYuvCenter, M, std::decay_t<decltype(dz)>...>, 3 * kYP, p.rows_max, done_cn, p.outW, p.outH, s, p, dz...);
                case kYuvI422: return launch_resample_tiles(resample_yuv422_kernel<kYuvCenter, M, std::decay_t<decltype(dz)>...>, 3 * (kRsCols + 1), p.rows_max, done_c422, p.outW, p.outH, s, p, dz...);
                default: return hipErrorInvalidValue;
            }
        }
        static unsigned done420 = 0, done422 = 0, done444 = 0, done_nv12 = 0;
        switch (layout) {                                                  // LDS dwords per input row: three planes of the kernel's pitch
            case kYuvI420: return launch_resample_tiles(resample_yuv_kernel<M, std::decay_t<decltype(dz)>...>, 3 * kYP, p.rows_max, done420, p.outW, p.outH, s, p, dz...);
            case kYuvI422: return launch_resample_tiles(resample_yuv422_kernel<kYuvLeft, M, std::decay_t<decltype(dz)>...>, 3 * (kRsCols + 1), p.rows_max, done422, p.outW, p.outH, s, p, dz...);
            case kYuvI444: return launch_resample_tiles(resample_yuv444_kernel<M, std::decay_t<decltype(dz)>...>, 3 * kRsCols, p.rows_max, done444, p.outW, p.outH, s, p, dz...);
            default: return launch_resample_tiles(resample_yuv_nv12_kernel<M, std::decay_t<decltype(dz)>...>, 3 * kYP, p.rows_max, done_nv12, p.outW, p.outH, s, p, dz...);
        }
    };
    if (siting == kYuvTopLeft) {                                           // pass 1 starts at the output row above the tile: the LDS holds those input rows too
        if (rows_max_above < p.rows_max) return hipErrorInvalidValue;
        p.rows_max = rows_max_above;
    }
    return for_modes(d, l, go);
}

}  // namespace w2x
