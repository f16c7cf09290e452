// Planar RGBA frames (renderPlanarRgba): four planes R, G, B, A of one sample type S in - 8, 10, 12, 16 bits or float32 -, four planes out, the two
// sides independent.  The frame is renderRgba's two-tile-set frame (k_rgba.hip) on renderPlanar's samples (k_planar.hip); those files and k_prepost.hip /
// k_resample.hip stay as they are, the parameter structs here are this file's own, and the shared bodies are pixel_device.h's.
//   alpha_bleed_planes : the four uploaded planes -> three colour planes (codes clamped to 2^bits - 1, the visible colours spread `radius` pixels under the
//                        pixels of alpha == 0) and the alpha plane, in the single buffers the passes gather from; the alpha range reduced into two device words.
//   gather_planes_rgba : gather_loop with a slot that says which planes it reads (kSlotColour: make_px(r, g, b), kSlotAlpha: (a, a, a)), load_sample<S> per sample:
//                        gather_planes_kernel's arithmetic, down to how its listing rounds a product to a half (TilePx).
//   compose_planes_rgba: compose_planes_kernel's launch shape and fast path over the colour tiles at three planes and over the alpha tiles at one (the green
//                        sum), store4<S> per plane; a uniform alpha plane whose tiles were not run is its value through the same store.
//   resample_planes_rgba: resample_pass1 / resample_pass2 over compose_canvas_rgba_kernel's canvas at NP = 4 (uniform: 3), store4<S> per plane.
#include <type_traits>

#include "kernels.h"
#include "pixel_device.h"

namespace w2x {
namespace {

// The bleed (integer, exact; tiles.h alpha_bleed_planes is the host statement): alpha_bleed_kernel's scheme (k_rgba.hip) - a workgroup of 256 threads owns a tile
// of kBleedTileW x kBleedTileH = 64 x 32 output pixels and holds it plus a halo of R pixels in LDS; iteration it = 1 .. R is evaluated on the tile grown by
// R - it pixels and reads state it - 1 on the tile grown by R - it + 1; all iterations run in one launch and stop at the first one that changes nothing in the
// workgroup's region (an opaque tile runs one).
// State: ONE buffer of 8-byte states, x = c0 | c1 << 16, y = c2 | flag << 16, for 8- and 16-bit samples alike (three 16-bit codes need 48 bits; one layout keeps
// one body for both sample types, and separate 16-bit planes plus a flag plane would turn each neighbour into four LDS reads instead of one).  flag: 0 unknown,
// k >= 1 known since state k - 1 (1: alpha > 0), kOutsideFlag outside the frame (never known, never filled).  A known pixel never changes, so a single buffer
// serves the Jacobi iteration: a reader in iteration `it` counts only neighbours whose flag lies in [1, it] - known in state it - 1 -, and the pixels written in
// iteration `it` carry flag it + 1 (before: 0), so they are invisible to it whether the reader sees them before or after the write; colour and flag of a state
// leave in one 8-byte write.  A barrier (__syncthreads_or, also the early exit) separates the iterations.
// LDS: (64 + 2R) x (32 + 2R) x 8 B - R = 16: 96 x 64 x 8 = 48 KiB, three workgroups (12 waves) in a CU's 160 KiB; R = 8: 80 x 48 x 8 = 30 KiB, five; R = 1:
// 66 x 34 x 8 = 17.5 KiB, nine, where the 32 wave slots of a CU hold eight.  Never above 64 KiB: no opt-in (ensure_dynamic_lds) is needed.  These are the
// counts the allocation allows; the occupancy reached on the device has not been measured.
// Banks: a row is 64 + 2R states of two dwords.  The lanes of a wave walk consecutive states of a region row, and each of the eight neighbour reads is one
// 8-byte read per lane at a fixed offset from the lane's own state: the 32 lanes of a half wave read 64 consecutive dwords, every one of the 64 banks once; where
// a wave wraps to the next region row (the region is narrower than the LDS row by 2 it states) the two runs are 2 (64 + 2R) dwords apart and overlap in 4 it mod
// 64 banks (two-way).  The 8-byte write of a half wave covers the same 64 consecutive dwords, two per bank on the 32 banks a write is served from: the minimum
// for 64 dwords.
// Global traffic: the halo is read sample by sample (1, 2 bytes per lane, consecutive lanes consecutive samples).  Output: a thread takes four consecutive
// pixels, and per plane they leave as one store where the row address allows - a dword (8 bits), 8 bytes (10 - 16 bits), 16 bytes (float) -, one by one at a
// ragged right edge.  Radius 0 (and float): no LDS, the planes are copied with the codes clamped.
constexpr unsigned kOutsideFlag = 0xFFFFu;

template <typename T> __device__ __forceinline__ void put4(uint8_t* row, int X, int np, const T v[4]) {
    T* d = (T*)row + X;
    typedef T vec4 __attribute__((ext_vector_type(4)));
    if (np == 4 && (((size_t)d) & (4 * sizeof(T) - 1)) == 0) *(vec4*)d = (vec4){v[0], v[1], v[2], v[3]};
    else for (int k = 0; k < np; ++k) d[k] = v[k];
}
// the order key of an alpha sample (kernels.h AlphaBleedPlanesParams::minmax): the clamped code, or the bits of the clamped float
template <typename S> __device__ __forceinline__ unsigned alpha_key(typename S::T a, unsigned maxcode) { return min((unsigned)a, maxcode); }
template <> __device__ __forceinline__ unsigned alpha_key<F32>(float a, unsigned) { return a > 0.f ? __float_as_uint(fminf(a, 1.f)) : 0u; }   // (NaN, -0.0, < 0: 0)

// kWrap (EdgeMode::Wrap): the halo outside the frame holds the frame's periodic continuation (edge_src<kEdgeWrap>) instead of the outside flag, so a
// pixel's eight neighbours always exist and colour spreads across the joint; the iterations are the same.  false: the kernel it always was.
template <typename S, bool kWrap = false>
__global__ __launch_bounds__(256) void alpha_bleed_planes_kernel(const AlphaBleedPlanesParams p, unsigned maxcode) {
    typedef typename S::T T;
    constexpr bool kInt = !std::is_same<S, F32>::value;
    extern __shared__ uint2 bleedp_lds[];
    __shared__ unsigned wg_max[2];
    const int R = kInt ? p.radius : 0, tid = threadIdx.x;
    const int rows = p.src.rows, cols = p.src.cols;
    const int LW = kBleedTileW + 2 * R;
    const int x0 = blockIdx.x * kBleedTileW, y0 = blockIdx.y * kBleedTileH;
    uint2* st = bleedp_lds;
    if (tid < 2) wg_max[tid] = 0u;
    if constexpr (kInt) {
        if (R > 0) {
            const int LH = kBleedTileH + 2 * R;
            for (int i = tid; i < LW * LH; i += 256) {
                const int ly = i / LW, lx = i - ly * LW;
                int fy = y0 - R + ly, fx = x0 - R + lx;
                if constexpr (kWrap) { fy = edge_src<kEdgeWrap>(fy, rows); fx = edge_src<kEdgeWrap>(fx, cols); }
                uint2 v = make_uint2(0u, kOutsideFlag << 16);
                if (kWrap || (fy >= 0 && fy < rows && fx >= 0 && fx < cols)) {
                    unsigned c[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) c[k] = min((unsigned)((const T*)(p.src.p[k] + (size_t)fy * p.src.step[k]))[fx], maxcode);
                    v = make_uint2(c[0] | c[1] << 16, c[2] | (c[3] ? 1u << 16 : 0u));
                }
                st[i] = v;
            }
            __syncthreads();
            for (int it = 1; it <= R; ++it) {
                const int w = LW - 2 * it, h = LH - 2 * it;
                const unsigned last = (unsigned)it;             // flags 1 .. it: known in state it - 1
                int changed = 0;
                for (int i = tid; i < w * h; i += 256) {
                    const int ry = i / w;
                    const int idx = (it + ry) * LW + it + (i - ry * w);
                    if ((st[idx].y >> 16) != 0u) continue;
                    unsigned n = 0, s0 = 0, s1 = 0, s2 = 0;     // (eight 16-bit codes: below 2^19)
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            if (dy == 0 && dx == 0) continue;
                            const uint2 q = st[idx + dy * LW + dx];
                            if ((q.y >> 16) - 1u < last) { ++n; s0 += q.x & 0xFFFFu; s1 += q.x >> 16; s2 += q.y & 0xFFFFu; }
                        }
                    if (n) {
                        const unsigned half = n >> 1;
                        st[idx] = make_uint2((s0 + half) / n | ((s1 + half) / n) << 16, (s2 + half) / n | (last + 1u) << 16);
                        changed = 1;
                    }
                }
                if (!__syncthreads_or(changed)) break;          // (also the barrier between state it and state it + 1)
            }
        } else __syncthreads();
    } else __syncthreads();
    unsigned kmax = 0u, imax = 0u;                              // max(key), max(top - key) over this thread's pixels
    const unsigned top = kInt ? maxcode : 0x3F800000u;
    constexpr int kGroups = kBleedTileW / 4;
    for (int g = tid; g < kGroups * kBleedTileH; g += 256) {
        const int gy = g / kGroups, gx = (g - gy * kGroups) * 4;
        const int y = y0 + gy, x = x0 + gx;
        if (y >= rows || x >= cols) continue;
        const int np = min(4, cols - x);
        T c[3][4] = {}, a[4] = {};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < np) {
                a[k] = ((const T*)(p.src.p[3] + (size_t)y * p.src.step[3]))[x + k];
                const unsigned key = alpha_key<S>(a[k], maxcode);
                kmax = max(kmax, key); imax = max(imax, top - key);
                if (R > 0) {
                    const uint2 q = st[(gy + R) * LW + gx + R + k];
                    c[0][k] = (T)(q.x & 0xFFFFu); c[1][k] = (T)(q.x >> 16); c[2][k] = (T)(q.y & 0xFFFFu);
                } else {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const T v = ((const T*)(p.src.p[ch] + (size_t)y * p.src.step[ch]))[x + k];
                        if constexpr (kInt) c[ch][k] = (T)min((unsigned)v, maxcode); else c[ch][k] = v;
                    }
                }
            }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) put4<T>(p.colour[ch] + (size_t)y * p.colour_step, x, np, c[ch]);
        put4<T>(p.alpha + (size_t)y * p.alpha_step, x, np, a);
    }
    // the frame's alpha range: per workgroup in LDS, then one vector atomic per word and workgroup
    atomicMax(&wg_max[0], kmax);
    atomicMax(&wg_max[1], imax);
    __syncthreads();
    if (tid < 2) atomicMax(p.minmax + tid, wg_max[tid]);
}

// The tile pixel of three samples as gather_planes_kernel forms it.  fp32 engines: make_px of the three load_sample values.  fp16 engines: the byte-for-byte
// contract with renderPlanar() reaches down to how code * inv becomes a half, and gather_planes_kernel's listing (every instantiation, one plane or three) rounds
// the first two elements of the pixel twice - v_mul_f32 to fp32, then v_cvt_pk_f16_f32 - and the third once, the exact product in v_fma_mixlo_f16.  The two
// differ for two codes each at 12 bits (2047, 4094) and at 16 (65455, 65519), and a swin graph spreads one such input sample over its whole window.  Here the
// choice is not left to instruction selection: an empty asm keeps the fp32 product of R and G apart from its conversion, and B is the mixed FMA written out.
// (Float samples are converted once either way: the product is x * 1.)
template <typename P, typename S> struct TilePx;
template <typename S> struct TilePx<float4v, S> {
    static __device__ __forceinline__ float4v make(const uint8_t* r, const uint8_t* g, const uint8_t* b, int x, unsigned maxcode, float inv) {
        return make_px<float4v>(load_sample<S>(r, x, maxcode, inv), load_sample<S>(g, x, maxcode, inv), load_sample<S>(b, x, maxcode, inv));
    }
};
template <typename S> struct TilePx<half4, S> {
    static __device__ __forceinline__ half4 make(const uint8_t* r, const uint8_t* g, const uint8_t* b, int x, unsigned maxcode, float inv) {
        float fr = load_sample<S>(r, x, maxcode, inv), fg = load_sample<S>(g, x, maxcode, inv);
        asm volatile("" : "+v"(fr), "+v"(fg));                     // (the fp32 products exist as such)
        const float cb = load_sample<S>(b, x, maxcode, 1.f);       // the clamped code itself (float samples: the clamped value)
        const float mb = std::is_same<S, F32>::value ? 1.f : inv, zero = 0.f;
        unsigned hb = 0u;
        asm("v_fma_mixlo_f16 %0, %1, %2, %3" : "+v"(hb) : "v"(cb), "v"(mb), "v"(zero));
        return (half4){(_Float16)fr, (_Float16)fg, __builtin_bit_cast(_Float16, (unsigned short)hb), (_Float16)0.f};
    }
};

// gather_kernel's indexing (gather_loop) on the planes the slot names: the three colour planes, or the alpha plane three times - the frame (A, A, A)
template <typename P, typename S, int E = kEdgeReplicate>
__global__ __launch_bounds__(kGatherThreads) void gather_planes_rgba_kernel(const GatherPlanarRgbaParams p, unsigned maxcode, float inv) {
    gather_loop<P, E>(p.slots, p.B, p.T, p.rows, p.cols, p.out, [&](const TileSlot& sl, int fy, int fx) {
        if (sl.valid == kSlotAlpha) {
            const uint8_t* a = p.alpha + (size_t)fy * p.alpha_step;
            return TilePx<P, S>::make(a, a, a, fx, maxcode, inv);
        }
        const size_t row = (size_t)fy * p.colour_step;
        return TilePx<P, S>::make(p.colour[0] + row, p.colour[1] + row, p.colour[2] + row, fx, maxcode, inv);
    });
}

// the sums of NP planes for the four pixels X .. X + 3 of row Y as compose_planes_kernel forms them: the fast path where the four share their tiles, else per pixel
template <typename P, int NP>
__device__ __forceinline__ void quad_sums(const ComposeParams& p, int X, int Y, int np, bool fast, int a0, int a1, float (&acc)[NP][4]) {
    if (fast) { compose_quad_sums<NP>(p, X, Y, a0, a1, acc); return; }
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < np) {
        float r, b;
        if constexpr (NP == 3) compose_pixel_sums<P>(p, (const P*)p.tiles, X + k, Y, acc[0][k], acc[1][k], acc[2][k]);
        else compose_pixel_sums<P>(p, (const P*)p.tiles, X + k, Y, r, acc[0][k], b);
    }
}
// compose_planes_kernel (k_planar.hip) over both tile sets: per thread four consecutive pixels of a row and kComposeRows rows; the colour planes are its NP = 3
// sums over c.tiles, the alpha plane its NP = 1 sum over alpha_tiles.
// M: kDitherNone - no further argument - is the kernel above; a dithered mode takes its DitherArgs behind maxcode (dither_of).  The colour planes
// are dithered; the alpha plane, the uniform one included, keeps sat(rint(.)).
template <typename P, typename S, int M = kDitherNone, typename... D>
__global__ __launch_bounds__(kComposeThreads) void compose_planes_rgba_kernel(const ComposePlanarRgbaParams q, float scale, int maxcode, const D... dzs) {
    static_assert(dither_pack_ok<M, D...>, "kDitherNone: no argument; else one DitherArgs");
    const DitherArgs& dz = dither_of(dzs...);
    constexpr bool kHalf = sizeof(P) == 8;
    const ComposeParams& p = q.c;
    const int gw = (p.outW + 3) >> 2;
    const int xg = blockIdx.x * kComposeThreads + threadIdx.x;
    if (xg >= gw) return;
    ComposeParams pa = q.c;
    pa.tiles = q.alpha_tiles;
    const int To = p.To;
    const int X = 4 * xg;
    const int np = min(4, p.outW - X);
    int a0 = X - To + 1; a0 = a0 <= 0 ? 0 : (a0 + p.stride_x - 1) / p.stride_x;
    int b0 = X + 3 - To + 1; b0 = b0 <= 0 ? 0 : (b0 + p.stride_x - 1) / p.stride_x;
    const int a1 = min(p.nx - 1, X / p.stride_x), b1 = min(p.nx - 1, (X + 3) / p.stride_x);
    const bool fast = kHalf && np == 4 && !p.tta && a0 == b0 && a1 == b1;
    const int Y0 = blockIdx.y * kComposeRows, Y1 = min(p.outH, Y0 + kComposeRows);
    for (int Y = Y0; Y < Y1; ++Y) {
        float acc[3][4] = {};                                      // [plane][pixel]
        quad_sums<P, 3>(p, X, Y, np, fast, a0, a1, acc);
#pragma unroll
        for (int c = 0; c < 3; ++c) store4<S, M>(q.dst.p[c] + (size_t)Y * q.dst.step[c], X, np, acc[c], scale, maxcode, dz, c, Y);
        float al[1][4] = {{q.alpha_value, q.alpha_value, q.alpha_value, q.alpha_value}};
        if (q.alpha_tiles) quad_sums<P, 1>(pa, X, Y, np, fast, a0, a1, al);
        store4<S>(q.dst.p[3] + (size_t)Y * q.dst.step[3], X, np, al[0], scale, maxcode);
    }
}

// resample_planes_kernel (k_planar.hip) over the canvas of an RGBA frame: NP = 4, or NP = 3 and the alpha plane its one value.  LDS: [NP][rows_max][64] fp32, at
// a factor of 4 with bicubic taps 78 KiB (NP = 3: 58.5 KiB), resample_rgba_kernel's.
template <typename S, int NP, int M = kDitherNone, typename... D>
__global__ __launch_bounds__(kRsThreads) void resample_planes_rgba_kernel(const ResamplePlanarRgbaParams p, float scale, int maxcode, const D... dzs) {
    static_assert(dither_pack_ok<M, D...>, "kDitherNone: no DitherArgs, else one; then one LightArgs or none");
    const DitherArgs& dz = dither_of(dzs...);
    constexpr bool kEdge = edge_on<D...>;                                 // 
    extern __shared__ float rsp_lds[];
    const int r0 = resample_pass1<NP, kEdge>(p, rsp_lds, edge_of(dzs...).mode);
    __syncthreads();
    float4v a[NP];
    int X, Y, np;
    if (!resample_pass2<NP, kEdge>(p, rsp_lds, r0, a, X, Y, np)) return;
    if constexpr (light_on<D...>) {                                       // (the colour planes are encoded, plane 3 - alpha - is not)
        const LightArgs& lz = light_of(dzs...);
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) a[c][q] = light_out<true>(lz, a[c][q]);
    }
#pragma unroll
    for (int c = 0; c < NP; ++c) {
        const float v[4] = {a[c][0], a[c][1], a[c][2], a[c][3]};
        if (M != kDitherNone && c < 3) store4<S, M>(p.dst.p[c] + (size_t)Y * p.dst.step[c], X, np, v, scale, maxcode, dz, c, Y);   // (plane 3 is alpha)
        else store4<S>(p.dst.p[c] + (size_t)Y * p.dst.step[c], X, np, v, scale, maxcode);
    }
    if constexpr (NP == 3) {
        const float v[4] = {p.alpha_value, p.alpha_value, p.alpha_value, p.alpha_value};
        store4<S>(p.dst.p[3] + (size_t)Y * p.dst.step[3], X, np, v, scale, maxcode);
    }
}

// four planes of rows x cols samples of `bits`, every step holding a row, u16 / f32 samples aligned to their size
inline bool rgba_planes_ok(const RgbaPlanes& f, int rows, int cols) {
    if (!planar_bits_ok(f.bits) || f.rows != rows || f.cols != cols || rows <= 0 || cols <= 0) return false;
    const size_t bps = planar_sample_bytes(f.bits);
    for (int k = 0; k < 4; ++k) if (!f.p[k] || f.step[k] < (size_t)cols * bps || ((((size_t)f.p[k]) | f.step[k]) & (bps - 1)) != 0) return false;
    return true;
}
inline bool plane_ok(const uint8_t* p, size_t step, int cols, int bits) {
    const size_t bps = planar_sample_bytes(bits);
    return p && step >= (size_t)cols * bps && ((((size_t)p) | step) & (bps - 1)) == 0;
}
inline int max_code(int bits) { return bits == 32 ? 0 : (1 << bits) - 1; }
inline float inv_code(int bits) { return bits == 32 ? 0.f : (float)(1.0 / (double)max_code(bits)); }

// launch(S()) for the sample type of `bits`
template <typename Launch> hipError_t for_sample(int bits, Launch launch) { return bits == 8 ? launch(U8()) : bits == 32 ? launch(F32()) : launch(U16()); }

}  // namespace

hipError_t launch_alpha_bleed_planes(const AlphaBleedPlanesParams& p, hipStream_t s, bool wrap) {
    const int rows = p.src.rows, cols = p.src.cols, bits = p.src.bits, R = p.radius;
    if (!rgba_planes_ok(p.src, rows, cols) || R < 0 || R > kBleedMaxRadius || (bits == 32 && R > 0) || !p.minmax) return hipErrorInvalidValue;
    for (int k = 0; k < 3; ++k) if (!plane_ok(p.colour[k], p.colour_step, cols, bits)) return hipErrorInvalidValue;
    if (!plane_ok(p.alpha, p.alpha_step, cols, bits)) return hipErrorInvalidValue;
    const size_t lds = R > 0 ? (size_t)(kBleedTileW + 2 * R) * (kBleedTileH + 2 * R) * sizeof(uint2) : 0;   // 48 KiB at most
    const dim3 grid((unsigned)((cols + kBleedTileW - 1) / kBleedTileW), (unsigned)((rows + kBleedTileH - 1) / kBleedTileH));
    const unsigned maxcode = (unsigned)max_code(bits);
    return for_sample(bits, [&](auto k) {
        typedef decltype(k) S;
        if (wrap) hipLaunchKernelGGL((alpha_bleed_planes_kernel<S, true>), grid, dim3(256), lds, s, p, maxcode);
        else hipLaunchKernelGGL(alpha_bleed_planes_kernel<S>, grid, dim3(256), lds, s, p, maxcode);
        return hipGetLastError();
    });
}
hipError_t launch_gather_planar_rgba(const GatherPlanarRgbaParams& p, hipStream_t s, int edge) {
    if (!planar_bits_ok(p.bits) || p.rows <= 0 || p.cols <= 0 || !plane_ok(p.alpha, p.alpha_step, p.cols, p.bits)) return hipErrorInvalidValue;
    for (int k = 0; k < 3; ++k) if (!plane_ok(p.colour[k], p.colour_step, p.cols, p.bits)) return hipErrorInvalidValue;
    const dim3 grid(grid_for((long)p.B * p.T * p.T));
    const unsigned maxcode = (unsigned)max_code(p.bits);
    const float inv = inv_code(p.bits);
    return for_sample(p.bits, [&](auto k) {
        typedef decltype(k) S;
        return for_edge(edge, [&](auto e) {
            constexpr int E = decltype(e)::value;
            if (p.fp32) hipLaunchKernelGGL((gather_planes_rgba_kernel<float4v, S, E>), grid, dim3(kGatherThreads), 0, s, p, maxcode, inv);
            else hipLaunchKernelGGL((gather_planes_rgba_kernel<half4, S, E>), grid, dim3(kGatherThreads), 0, s, p, maxcode, inv);
            return hipGetLastError();
        });
    });
}
hipError_t launch_compose_planar_rgba(const ComposePlanarRgbaParams& p, hipStream_t s, const DitherArgs& d) {
    if (p.c.outW <= 0 || p.c.outH <= 0) return hipSuccess;
    if (!rgba_planes_ok(p.dst, p.c.outH, p.c.outW) || !dither_args_ok(d)) return hipErrorInvalidValue;
    const int gw = (p.c.outW + 3) / 4;
    const dim3 grid((unsigned)((gw + kComposeThreads - 1) / kComposeThreads), (unsigned)((p.c.outH + kComposeRows - 1) / kComposeRows));
    const int maxcode = max_code(p.dst.bits);
    const float scale = (float)maxcode;
    return for_sample(p.dst.bits, [&](auto k) {
        typedef decltype(k) S;
        if constexpr (!std::is_same<S, F32>::value) {                 // (float samples are never dithered)
            if (d.mode != kDitherNone) return for_dither(d, [&](auto m) {
                constexpr int M = decltype(m)::value;
                if (p.c.fp32) hipLaunchKernelGGL((compose_planes_rgba_kernel<float4v, S, M, DitherArgs>), grid, dim3(kComposeThreads), 0, s, p, scale, maxcode, d);
                else hipLaunchKernelGGL((compose_planes_rgba_kernel<half4, S, M, DitherArgs>), grid, dim3(kComposeThreads), 0, s, p, scale, maxcode, d);
                return hipGetLastError();
            });
        }
        if (p.c.fp32) hipLaunchKernelGGL((compose_planes_rgba_kernel<float4v, S>), grid, dim3(kComposeThreads), 0, s, p, scale, maxcode);
        else hipLaunchKernelGGL((compose_planes_rgba_kernel<half4, S>), grid, dim3(kComposeThreads), 0, s, p, scale, maxcode);
        return hipGetLastError();
    });
}
hipError_t launch_resample_planar_rgba(const ResamplePlanarRgbaParams& p, hipStream_t s, const DitherArgs& d, const LightArgs& l, const EdgeArgs& e) {
    if (p.outW <= 0 || p.outH <= 0) return hipSuccess;
    if (!p.canvas || !rgba_planes_ok(p.dst, p.outH, p.outW) || !dither_args_ok(d)) return hipErrorInvalidValue;
    const int maxcode = max_code(p.dst.bits);
    const float scale = (float)maxcode;
    return for_sample(p.dst.bits, [&](auto k) {
        typedef decltype(k) S;
        auto go = [&](auto m, const auto&... extra) {
            constexpr int M = decltype(m)::value;
            static unsigned lds_done[2] = {0, 0};                        // (a pair per instantiation of this lambda's body)
            if (p.uniform) return launch_resample_tiles(resample_planes_rgba_kernel<S, 3, M, std::decay_t<decltype(extra)>...>, 3 * kRsCols, p.rows_max, lds_done[0], p.outW, p.outH, s, p, scale, maxcode, extra...);
            return launch_resample_tiles(resample_planes_rgba_kernel<S, 4, M, std::decay_t<decltype(extra)>...>, 4 * kRsCols, p.rows_max, lds_done[1], p.outW, p.outH, s, p, scale, maxcode, extra...);
        };
        if constexpr (std::is_same<S, F32>::value) return for_light(l, e, go);   // (float samples are never dithered: no such kernels)
        else return for_modes(d, l, e, go);
    });
}

}  // namespace w2x
