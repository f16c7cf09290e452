// Device helpers shared by the tile pre/post kernels (k_prepost.hip) and the RGBA kernels (k_rgba.hip): the tile pixel types, the TTA source maps of
// gather and compose, and the per-pixel compose sums.  The arithmetic and its order are what makes frames byte-identical to the oracle: the code
// lives here once and both files inline it.
#pragma once
#include "kernels.h"
#include <tuple>
#include <type_traits>

namespace w2x {
namespace {

typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float4v __attribute__((ext_vector_type(4)));
// a tile pixel is four stored channels (r, g, b, 0) in the plan's precision: half4 (fp16 engines) or float4v (fp32 engines)
template <typename P> __device__ __forceinline__ P make_px(float r, float g, float b);
template <> __device__ __forceinline__ half4 make_px<half4>(float r, float g, float b) { return (half4){(_Float16)r, (_Float16)g, (_Float16)b, (_Float16)0.f}; }
template <> __device__ __forceinline__ float4v make_px<float4v>(float r, float g, float b) { return (float4v){r, g, b, 0.f}; }

// source coordinate inside the un-augmented tile for pixel (y,x) of the augmented tile (applyAugmentation)
__device__ __forceinline__ void aug_src(int k, int n, int y, int x, int& sy, int& sx) {
    switch (k) {
        default: sy = y; sx = x; break;
        case 1: sy = n - y; sx = x; break;          // flip code 0
        case 2: sy = y; sx = n - x; break;          // flip code 1
        case 3: sy = x; sx = n - y; break;          // rot90
        case 4: sy = n - y; sx = n - x; break;      // rot180
        case 5: sy = n - x; sx = y; break;          // rot270
        case 6: sy = n - x; sx = n - y; break;      // flip0 then rot90
        case 7: sy = x; sx = y; break;              // flip1 then rot90
    }
}
// The edge rule (edge.h states it): the source index of frame coordinate i in a dimension of n >= 1 samples, for any i.  E is a template parameter of
// every gather of the RGB family; its kEdgeReplicate instantiation is the clamp the kernels always had, instruction for instruction.  Wrap and Mirror fold as
// often as needed (one signed remainder): a tile border may be several times a small frame.
template <int E>
__device__ __forceinline__ int edge_src(int i, int n) {
    if constexpr (E != kEdgeReplicate) { if ((unsigned)i < (unsigned)n) return i; }   // (inside the frame, which is nearly every call: no division)
    if constexpr (E == kEdgeWrap) { const int r = i % n; return r < 0 ? r + n : r; }
    else if constexpr (E == kEdgeMirror) {
        if (n == 1) return 0;
        const int p = 2 * (n - 1);
        int r = i % p;
        if (r < 0) r += p;
        return r < n ? r : p - r;
    }
    else return min(max(i, 0), n - 1);
}
// the same with the mode as data (the edged resize kernels and the wrapped bleed: one instantiation for Wrap and Mirror)
__device__ __forceinline__ int edge_index_dev(int mode, int i, int n) { return mode == kEdgeWrap ? edge_src<kEdgeWrap>(i, n) : mode == kEdgeMirror ? edge_src<kEdgeMirror>(i, n) : edge_src<kEdgeReplicate>(i, n); }
// source coordinate inside the network output for pixel (y,x) of the de-augmented tile (reverseAugmentation)
__device__ __forceinline__ void deaug_src(int k, int n, int y, int x, int& sy, int& sx) {
    switch (k) {
        default: sy = y; sx = x; break;
        case 1: sy = n - y; sx = x; break;
        case 2: sy = y; sx = n - x; break;
        case 3: sy = n - x; sx = y; break;          // rot270
        case 4: sy = n - y; sx = n - x; break;
        case 5: sy = x; sx = n - y; break;          // rot90
        case 6: sy = n - x; sx = n - y; break;      // rot270 then flip0
        case 7: sy = x; sx = y; break;              // rot270 then flip1
    }
}

// One output pixel: the covering tiles in ascending tile index (img2img_render.cpp:329-330), ramp weights L, T, R, B in that order on
// the clipped rect (:110-120), fp32 sums, then rint(x * 255) saturated (:342), RGB -> BGR (:343).  Returns b | g << 8 | r << 16.
__device__ __forceinline__ unsigned quantize_bgr(float r, float g, float b) {
    const unsigned B = (unsigned)min(max(__float2int_rn(b * 255.f), 0), 255), G = (unsigned)min(max(__float2int_rn(g * 255.f), 0), 255),
                   R = (unsigned)min(max(__float2int_rn(r * 255.f), 0), 255);
    return B | G << 8 | R << 16;
}
// ---- dithered quantisation (dither.h states the rule).  M is a template parameter of every kernel that stores integer samples; its kDitherNone
// instantiation contains none of the code below and is the undithered kernel, instruction for instruction.
// The threshold t = (rank + 0.5) / N of the sample (x, y) of plane index c.  Ordered: the Bayer rank from the bits of u = x + dx, v = y + dy, no table -
// q_b = ((u_b ^ v_b) << 1) | v_b, rank = q_0 << 4 | q_1 << 2 | q_2.  BlueNoise: one 2-byte load from the 8 KiB table, which every workgroup of the launch reads
// and the vector L1 keeps (a thread's four samples start at any (x + dx) & 63 and wrap, so they are four loads, not one).  c is a compile-time constant or a
// loop counter of an unrolled loop wherever this is called: d.dx[c] / d.dy[c] are scalar registers.
// A kernel templated on M ends its parameter list with a pack: empty for kDitherNone - the argument list, and so the kernarg offsets, of the undithered kernel -
// and one DitherArgs for a dithered mode.  dither_of(dzs...) is that argument, or a default nobody reads.
// Resize in linear light: the pack of a kernel that encodes may end in one LightArgs behind that - (), (DitherArgs), (LightArgs) or (DitherArgs,
// LightArgs); light_on<D...> is the kernel's compile-time switch and light_of(dzs...) the curve, or a default nobody reads.
__device__ __forceinline__ DitherArgs dither_of() { return DitherArgs(); }
__device__ __forceinline__ const DitherArgs& dither_of(const DitherArgs& d) { return d; }
__device__ __forceinline__ DitherArgs dither_of(const LightArgs&) { return DitherArgs(); }
__device__ __forceinline__ const DitherArgs& dither_of(const DitherArgs& d, const LightArgs&) { return d; }
__device__ __forceinline__ LightArgs light_of() { return LightArgs(); }
__device__ __forceinline__ LightArgs light_of(const DitherArgs&) { return LightArgs(); }
__device__ __forceinline__ const LightArgs& light_of(const LightArgs& l) { return l; }
__device__ __forceinline__ const LightArgs& light_of(const DitherArgs&, const LightArgs& l) { return l; }
// Edge modes: the pack of a resize kernel may end in one EdgeArgs behind all that - the kernel whose pass 1 takes every input index through the
// rule; edge_on<D...> is the compile-time switch and edge_of(dzs...) the mode, or a default nobody reads.  A pack without it names the kernel it always named.
__device__ __forceinline__ DitherArgs dither_of(const EdgeArgs&) { return DitherArgs(); }
__device__ __forceinline__ const DitherArgs& dither_of(const DitherArgs& d, const EdgeArgs&) { return d; }
__device__ __forceinline__ DitherArgs dither_of(const LightArgs&, const EdgeArgs&) { return DitherArgs(); }
__device__ __forceinline__ const DitherArgs& dither_of(const DitherArgs& d, const LightArgs&, const EdgeArgs&) { return d; }
__device__ __forceinline__ LightArgs light_of(const EdgeArgs&) { return LightArgs(); }
__device__ __forceinline__ LightArgs light_of(const DitherArgs&, const EdgeArgs&) { return LightArgs(); }
__device__ __forceinline__ const LightArgs& light_of(const LightArgs& l, const EdgeArgs&) { return l; }
__device__ __forceinline__ const LightArgs& light_of(const DitherArgs&, const LightArgs& l, const EdgeArgs&) { return l; }
__device__ __forceinline__ EdgeArgs edge_of() { return EdgeArgs(); }
template <typename A, typename... R> __device__ __forceinline__ EdgeArgs edge_of(const A& a, const R&... r) {
    if constexpr (std::is_same<A, EdgeArgs>::value) return a;
    else return edge_of(r...);
}
template <typename... D> constexpr bool light_on = (std::is_same<D, LightArgs>::value || ...);
template <typename... D> constexpr bool edge_on = (std::is_same<D, EdgeArgs>::value || ...);
template <int M> constexpr int kLightAt = (M == kDitherNone ? 0 : 1);                  // where the LightArgs of a pack stands
template <int M, typename... D> constexpr bool dither_pack_ok =
    sizeof...(D) == (M == kDitherNone ? 0 : 1) + (light_on<D...> ? 1 : 0) + (edge_on<D...> ? 1 : 0) &&
    (M == kDitherNone || std::is_same<std::tuple_element_t<0, std::tuple<D..., void>>, DitherArgs>::value) &&
    (!light_on<D...> || std::is_same<std::tuple_element_t<kLightAt<M>, std::tuple<D..., void, void>>, LightArgs>::value) &&
    (!edge_on<D...> || std::is_same<std::tuple_element_t<sizeof...(D) == 0 ? 0 : sizeof...(D) - 1, std::tuple<D..., void>>, EdgeArgs>::value);
// The two curve functions on the device (light.h states them and their roundings; the power goes through the hardware's log2 / exp2, v_log_f32 / v_exp_f32,
// whose arguments here are never subnormal: the base of decode is at least 1 / (1 + a) > 0.9 a, the argument of encode's power at least t / k).  The curve is
// data: both branches are computed and one is selected.  e and l are in [0, 1] - the callers clamp.  Contraction is off: every product and sum below is the
// stated one.
__device__ __forceinline__ float light_decode(const LightArgs& c, float e) {
#pragma clang fp contract(off)
    const float lin = __fmul_rn(e, c.inv_k);
    const float base = __fmaf_rn(__fsub_rn(e, 1.f), c.inv_1a, 1.f);
    const float pw = __builtin_amdgcn_exp2f(__fmul_rn(c.g, __builtin_amdgcn_logf(base)));
    return e < c.t ? lin : pw;
}
__device__ __forceinline__ float light_encode(const LightArgs& c, float l) {
#pragma clang fp contract(off)
    const float lin = __fmul_rn(c.k, l);
    const float p = __builtin_amdgcn_exp2f(__fmul_rn(c.inv_g, __builtin_amdgcn_logf(l)));
    const float pw = __fmaf_rn(c.a, __fsub_rn(p, 1.f), p);
    return l < c.tl ? lin : pw;
}
__device__ __forceinline__ float light_sat01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
// the canvas value of a colour sum s: s itself, or decode(sat01(s)) where the launch carries a curve (kOn)
template <bool kOn>
__device__ __forceinline__ float light_canvas(const LightArgs& c, float s) {
    if constexpr (kOn) return light_decode(c, light_sat01(s));
    else return s;
}
// the resized value the store of an encoding kernel takes: encode(sat01(v)) (kOn; the stores clamp and quantise it as they do any value), else v untouched
template <bool kOn>
__device__ __forceinline__ float light_out(const LightArgs& c, float v) {
    if constexpr (kOn) return light_encode(c, light_sat01(v));
    else return v;
}
template <int M>
__device__ __forceinline__ float dither_t(const DitherArgs& d, int c, int x, int y) {
    static_assert(M == kDitherOrdered || M == kDitherBlueNoise, "None adds nothing");
    const unsigned u = (unsigned)(x + d.dx[c]), v = (unsigned)(y + d.dy[c]);
    if constexpr (M == kDitherOrdered) {
        const unsigned w = u ^ v;
        const unsigned rank = (w & 1u) << 5 | (v & 1u) << 4 | (w & 2u) << 2 | (v & 2u) << 1 | (w & 4u) >> 1 | (v & 4u) >> 2;
        return ((float)rank + 0.5f) * (1.f / 64.f);
    } else {
        const unsigned rank = d.table[(v & (kDitherSide - 1)) * kDitherSide + (u & (kDitherSide - 1))];
        return ((float)rank + 0.5f) * (1.f / 4096.f);
    }
}
// min(max(floor(fl32(V + t)), 0), maxcode): V the value the undithered kernel rounds to nearest, made by the caller with the contraction it has there.  The
// addition is one rounded fp32 add: contraction is off in this block, so the product or fma that made V is never fused with it.
template <int M>
__device__ __forceinline__ unsigned dither_code(float V, float t, int maxcode) {
#pragma clang fp contract(off)
    const float s = __fadd_rn(V, t);
    return (unsigned)min(max(__float2int_rd(s), 0), maxcode);
}
// sat(rint(V)) or the dithered code of sample (x, y) of plane c: the one quantisation of a kernel templated on M
template <int M>
__device__ __forceinline__ unsigned quant_code(float V, int maxcode, const DitherArgs& d, int c, int x, int y) {
    if constexpr (M == kDitherNone) return (unsigned)min(max(__float2int_rn(V), 0), maxcode);
    else return dither_code<M>(V, dither_t<M>(d, c, x, y), maxcode);
}
// quantize_bgr of pixel (x, y) of a BGR frame: b | g << 8 | r << 16, R, G, B = planes 0, 1, 2
template <int M>
__device__ __forceinline__ unsigned quantize_bgr_at(float r, float g, float b, const DitherArgs& d, int x, int y) {
    if constexpr (M == kDitherNone) return quantize_bgr(r, g, b);
    else return quant_code<M>(b * 255.f, 255, d, 2, x, y) | quant_code<M>(g * 255.f, 255, d, 1, x, y) << 8 | quant_code<M>(r * 255.f, 255, d, 0, x, y) << 16;
}

template <typename P>
__device__ __forceinline__ void compose_pixel_sums(const ComposeParams& p, const P* tiles, int X, int Y, float& r0, float& r1, float& r2) {
    const int To = p.To, n = To - 1;
    const int steps = p.tta ? 8 : 1;
    // candidate tile columns/rows: origin = idx*stride, extent To (clipped to the canvas)
    int i0 = X - To + 1; i0 = i0 <= 0 ? 0 : (i0 + p.stride_x - 1) / p.stride_x;
    int i1 = min(p.nx - 1, X / p.stride_x);
    int j0 = Y - To + 1; j0 = j0 <= 0 ? 0 : (j0 + p.stride_y - 1) / p.stride_y;
    int j1 = min(p.ny - 1, Y / p.stride_y);
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
    for (int ti = i0; ti <= i1; ++ti) {
        const int ox = ti * p.stride_x, lx = X - ox;
        const int rw = ox + To > p.outW ? p.outW - ox : To;
        for (int tj = j0; tj <= j1; ++tj) {
            const int oy = tj * p.stride_y, ly = Y - oy;
            const int rh = oy + To > p.outH ? p.outH - oy : To;
            const long tile = (long)ti * p.ny + tj - p.first_tile;
            const P* tp = tiles + tile * steps * (long)To * To;
            float v0, v1, v2;
            if (!p.tta) {
                const P h = tp[(long)ly * To + lx];
                v0 = (float)h[0]; v1 = (float)h[1]; v2 = (float)h[2];
            } else {
                float s0 = 0.f, s1 = 0.f, s2 = 0.f;
                P h;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    int sy, sx;
                    deaug_src(k, n, ly, lx, sy, sx);
                    h = tp[(long)k * To * To + (long)sy * To + sx];
                    s0 += (float)h[0]; s1 += (float)h[1]; s2 += (float)h[2];
                }
                if (p.tta_bug_compat) { v0 = (float)h[0]; v1 = (float)h[1]; v2 = (float)h[2]; }
                else { v0 = s0 * 0.125f; v1 = s1 * 0.125f; v2 = s2 * 0.125f; }
            }
            if (p.ovx || p.ovy) {
                if (ox > 0 && lx < p.ovx) { float w = p.ramp_x[lx]; v0 *= w; v1 *= w; v2 *= w; }
                if (oy > 0 && ly < p.ovy) { float w = p.ramp_y[ly]; v0 *= w; v1 *= w; v2 *= w; }
                if (ox + rw < p.outW && n - lx < p.ovx) { float w = p.ramp_x[n - lx]; v0 *= w; v1 *= w; v2 *= w; }
                if (oy + rh < p.outH && n - ly < p.ovy) { float w = p.ramp_y[n - ly]; v0 *= w; v1 *= w; v2 *= w; }
            }
            acc0 += v0; acc1 += v1; acc2 += v2;
        }
    }
    r0 = acc0; r1 = acc1; r2 = acc2;
}

}  // namespace
}  // namespace w2x
