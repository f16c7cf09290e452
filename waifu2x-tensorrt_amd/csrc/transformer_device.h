// Helpers shared by the fused transformer kernels (k_mlp2.hip, k_mlp96q.hip, k_swinattn96.hip, k_swinattn192u.hip) and the retired schedules kept beside
// the A/B builders (tools/ab/k_*.hip): the vector types, the LayerNorm row pieces, the GELU, the lane exchanges, the buffer-resource contract, and the two
// loops with which the launchers cut a pass that is longer than 32-bit byte offsets reach.  Everything here is inlined into its callers: each lives here
// once with the one comment that explains it, and a file keeps what only it uses (and the constants that differ on purpose: kMaxBufBytes, tile geometry,
// build switches).  Included by .hip files only.
#pragma once
#include "kernels.h"

#include <algorithm>

#ifndef W2X_GELU_DEG
#define W2X_GELU_DEG 4   // coefficients of q(u): 6 -> 3.1e-7, 5 -> 7.1e-7, 4 -> 8.7e-6 absolute error of GELU (tools/fit_gelu.py).  4: a third of
                         // the fp16 rounding of the smallest hidden values that matter, network parity unchanged (2.0 ULP16 on every full-width
                         // graph, same mean error), MLP kernels 5-7 % faster (round 2, profiles/r2_final/gelu_degree_ab.txt; now: tools/ab/lib_variants.sh "k_mlp2.hip:-DW2X_GELU_DEG=6")
#endif

namespace w2x {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef float float4v __attribute__((ext_vector_type(4)));
typedef float float16v __attribute__((ext_vector_type(16)));
typedef unsigned uint4v __attribute__((ext_vector_type(4)));
typedef int int2v __attribute__((ext_vector_type(2)));

// ---- rows through buffer resources
// The kernels fetch and store their rows through raw buffer resources over x / y: 32-bit byte offsets, bounds-checked by the hardware.  An offset at or
// beyond num_records reads zeros and its store is dropped, so rows that do not exist (a ragged last tile, a window past the end, a prefetch past the last
// tile) and the idle lanes of a row need neither a predicate nor masking of the data.  kNoRow is the offset of "no row"; saturating adds keep it there.
// Offsets are 32 bits: every launcher cuts a pass of more than its kMaxBufBytes into runs (for_mlp_runs / for_attn_runs below).
constexpr unsigned kNoRow = 0xFFFFFFFFu;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);   // raw buffer, 32-bit offsets, bounds-checked
}

// ---- LayerNorm pieces
// the sum and the sum of squares of 8 halves (v_dot2_f32_f16, fp32 accumulation): sum_sq8_acc adds them to s and q (the MLP kernels: a lane's pieces of one
// row), sum_sq8 starts from zero (the attention kernels: one piece per lane)
__device__ __forceinline__ void sum_sq8_acc(const half8 v, float& s, float& q) {
    const half2v one = {(_Float16)1.f, (_Float16)1.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const half2v h = {v[2 * k], v[2 * k + 1]};
        s = __builtin_amdgcn_fdot2(h, one, s, false);
        q = __builtin_amdgcn_fdot2(h, h, q, false);
    }
}
__device__ __forceinline__ void sum_sq8(const half8 v, float& s, float& q) { s = 0.f; q = 0.f; sum_sq8_acc(v, s, q); }
// (x * rstd + nm) on 8 halves with fp32 arithmetic: v_fma_mixlo / mixhi read the f16 halves directly and write f16 (one instruction
// per element; the compiler's own lowering converts both ways around a packed fp32 fma)
__device__ __forceinline__ half8 norm8(const half8 v, float rstd, float nm) {
    uint4v x = __builtin_bit_cast(uint4v, v), o;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        unsigned r;
        asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(x[d]), "v"(rstd), "v"(nm));
        asm("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(r) : "v"(x[d]), "v"(rstd), "v"(nm));
        o[d] = r;
    }
    return __builtin_bit_cast(half8, o);
}

// ---- GELU
// GELU(x) = max(x,0) - 0.5 u 2^-q(u), u = min(|x|, 6.5): tools/fit_gelu.py (|err| < 8.7e-6 with the four-coefficient q, W2X_GELU_DEG)
// Two values at a time: the polynomial, the products and the final fma are v_pk_*_f32 (one issue slot for both values);
// min / max / exp2 have no packed form.  Same operations per element as the scalar form, so the results are identical.
__device__ __forceinline__ float2v splat2(float c) { return (float2v){c, c}; }
#ifdef W2X_GELU_SCALAR   // A/B: the same polynomial on single-value instructions
__device__ __forceinline__ float gelu_fast1(float x) {
    const float u = fminf(fabsf(x), 6.5f);
    float q = fmaf(-2.992485764e-05f, u, 7.398797018e-04f);
    q = fmaf(q, u, -7.977479093e-03f);
    q = fmaf(q, u, 5.323820859e-02f);
    q = fmaf(q, u, 4.589156733e-01f);
    q = fmaf(q, u, 1.151147085e+00f);
    return fmaf(-0.5f * u, __builtin_amdgcn_exp2f(-(q * u)), fmaxf(x, 0.f));
}
__device__ __forceinline__ float2v gelu_fast2(float2v x) { return (float2v){gelu_fast1(x[0]), gelu_fast1(x[1])}; }
#else
__device__ __forceinline__ float2v gelu_fast2(float2v x) {
    const float2v u = {fminf(fabsf(x[0]), 6.5f), fminf(fabsf(x[1]), 6.5f)};
#if W2X_GELU_DEG == 5
    float2v q = __builtin_elementwise_fma(splat2(4.881020589e-04f), u, splat2(-7.198718011e-03f));
    q = __builtin_elementwise_fma(q, u, splat2(5.214663110e-02f));
    q = __builtin_elementwise_fma(q, u, splat2(4.595958449e-01f));
    q = __builtin_elementwise_fma(q, u, splat2(1.151000542e+00f));
#elif W2X_GELU_DEG == 4
    float2v q = __builtin_elementwise_fma(splat2(-4.161669730e-03f), u, splat2(4.573546095e-02f));
    q = __builtin_elementwise_fma(q, u, splat2(4.649304537e-01f));
    q = __builtin_elementwise_fma(q, u, splat2(1.149566979e+00f));
#else
    float2v q = __builtin_elementwise_fma(splat2(-2.992485764e-05f), u, splat2(7.398797018e-04f));
    q = __builtin_elementwise_fma(q, u, splat2(-7.977479093e-03f));
    q = __builtin_elementwise_fma(q, u, splat2(5.323820859e-02f));
    q = __builtin_elementwise_fma(q, u, splat2(4.589156733e-01f));
    q = __builtin_elementwise_fma(q, u, splat2(1.151147085e+00f));
#endif
    const float2v t = __builtin_elementwise_fma(q, u, splat2(1.f));              // the factor 1/2 rides in the exponent: 0.5 * 2^-qu = 2^-(qu + 1)
    const float2v e = {__builtin_amdgcn_exp2f(-t[0]), __builtin_amdgcn_exp2f(-t[1])};
    const float2v m = {fmaxf(x[0], 0.f), fmaxf(x[1], 0.f)};
    return __builtin_elementwise_fma(-u, e, m);
}
#endif

// ---- lane exchanges
// The row swaps and the DPP sums below are inline asm because nothing else gives their shape: v_permlane16/32_swap exchange TWO registers between the
// 16-lane rows (or the halves) of a wave, so one instruction serves a value and its copy, and v_add_f32 with a DPP operand does in one instruction what
// the compiler emits as v_mov_dpp + v_add for v += dpp(v).  Nothing inside an asm statement is padded by the compiler, so each sequence carries its own
// wait states: two after the VALU write a swap or a DPP operand reads (three when the value comes straight from a v_dot2c chain - the leading s_nop 2),
// one before a VALU reads a swap's result.  Where several independent values go through together their chains are interleaved and fill each other's
// wait states; what is left is an s_nop.  v_max_f32 is used as is (fmaxf() would canonicalise both swap results first).
__device__ __forceinline__ void swap16(float& a, float& b) { asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 0" : "+v"(a), "+v"(b)); }
// sums over the two lanes (l, l ^ 32) that hold one token row, for two values at once (inputs straight from v_dot2c chains)
__device__ __forceinline__ void halves_sum2(float& a0, float& a1) {
    float b0, b1;
    asm volatile(
        "s_nop 2\n\tv_mov_b32 %2, %0\n\tv_mov_b32 %3, %1\n\ts_nop 0\n\t"
        "v_permlane32_swap_b32 %0, %2\n\tv_permlane32_swap_b32 %1, %3\n\t"
        "v_add_f32 %0, %0, %2\n\tv_add_f32 %1, %1, %3"
        : "+v"(a0), "+v"(a1), "=&v"(b0), "=&v"(b1));
}
// maximum over the four 16-lane rows of a wave (lanes fr, fr + 16, fr + 32, fr + 48: the four lanes that hold one query column) for three values at once
__device__ __forceinline__ void rows_max3(float& a0, float& a1, float& a2) {
    float b0, b1, b2;
    asm volatile(
        "v_mov_b32 %3, %0\n\tv_mov_b32 %4, %1\n\tv_mov_b32 %5, %2\n\t"
        "v_permlane16_swap_b32 %0, %3\n\tv_permlane16_swap_b32 %1, %4\n\tv_permlane16_swap_b32 %2, %5\n\t"
        "v_max_f32 %0, %0, %3\n\tv_max_f32 %1, %1, %4\n\tv_max_f32 %2, %2, %5\n\t"
        "v_mov_b32 %3, %0\n\tv_mov_b32 %4, %1\n\tv_mov_b32 %5, %2\n\t"
        "v_permlane32_swap_b32 %0, %3\n\tv_permlane32_swap_b32 %1, %4\n\tv_permlane32_swap_b32 %2, %5\n\t"
        "v_max_f32 %0, %0, %3\n\tv_max_f32 %1, %1, %4\n\tv_max_f32 %2, %2, %5"
        : "+v"(a0), "+v"(a1), "+v"(a2), "=&v"(b0), "=&v"(b1), "=&v"(b2));
}
// one v_add_f32 step with a DPP operand on one / four / six registers of an asm statement (the group sums of the attention kernels)
#define W2X_DPP1(R, CTRL) "v_add_f32_dpp " R ", " R ", " R " " CTRL " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
#define W2X_DPP4(CTRL) W2X_DPP1("%0", CTRL) W2X_DPP1("%1", CTRL) W2X_DPP1("%2", CTRL) W2X_DPP1("%3", CTRL)
#define W2X_DPP6(CTRL) W2X_DPP4(CTRL) W2X_DPP1("%4", CTRL) W2X_DPP1("%5", CTRL)
// sum over aligned groups of 16 lanes (a row) with DPP: xor 1, xor 2, half-row mirror, row mirror; over groups of 32 lanes: one row swap across on top
__device__ __forceinline__ float group_sum16(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
    return v;
}
__device__ __forceinline__ float group_sum32(float v) {
    float a = group_sum16(v), b = a;
    swap16(a, b);
    return a + b;
}

// ---- phases of a wave
// The MLP kernels hand data from lane to lane through the wave's own LDS slab.  The hardware executes a wave's LDS instructions in order, so no
// s_barrier / s_waitcnt is needed between the phases; the compiler-level fence (no instruction emitted) keeps hipcc from forwarding a lane's own store to
// its later load or moving slab accesses across a phase boundary.
// History: a first version exchanged per-row LayerNorm statistics through a small float table in the slab
// (ds_write_b64 by lane = row, ds_read_b64 by the fragment lanes a few instructions later).  That exchange returned stale
// values on the second wave of a SIMD at full problem size (tools/ab/mlp_ab.hip reproduces it: first workgroup per CU always
// right, co-resident ones wrong, not cured by s_waitcnt / s_barrier) and was replaced by register swaps.
#define W2X_PHASE_FENCE() asm volatile("" ::: "memory")
#define W2X_RING_FENCE() asm volatile("" ::: "memory")   // keeps a ring refill where it is written (the scheduler would sink it to its use)

// slab row of token t of a 6 x 6 window (attention kernels): tokens 0..31 in order, tokens 32..35 on rows 32, 36, 40, 44, so that left-over key 32 + g sits
// on row 4g of the third key tile
__device__ __forceinline__ int slab_row(int t) { return t < 32 ? t : 32 + 4 * (t - 32); }

// ---- launchers: a pass in runs (host)
// run(q) for consecutive runs of at most max_rows rows of the MLP pass p: q is p with M, x, y and stats_out of the run and the run's first row in the whole
// pass as the origin of the dead-skip rows (live_row0) and of the image head's rows (ti_row0).  Both origins are set for every pass: mlp2_kernel and
// mlp96q_kernel read live_row0 only where p.live is set, and ti_row0 is read by mlp96q_kernel<true> alone, the image-head instantiation.
template <class Run>
hipError_t for_mlp_runs(const MlpParams& p, long max_rows, Run&& run) {
    const size_t row_bytes = (size_t)p.C * 2;
    for (long r0 = 0; r0 < p.M; r0 += max_rows) {
        MlpParams q = p;
        q.M = std::min(max_rows, p.M - r0);
        q.x = (const char*)p.x + (size_t)r0 * row_bytes; q.y = (char*)p.y + (size_t)r0 * row_bytes;
        if (p.stats_out) q.stats_out = p.stats_out + 2 * r0;
        q.live_row0 = p.live_row0 + r0;
        q.ti_row0 = r0;
        if (hipError_t e = run(q); e != hipSuccess) return e;
    }
    return hipSuccess;
}
// run(q) for consecutive runs of whole images of the attention pass p (token maps of nwin windows of ntok tokens of C channels), as many images as max_bytes
// hold: windows never cross an image, the statistics rows follow the pixels and the dead-skip table has one entry per image
template <class Run>
hipError_t for_attn_runs(const SwinAttnParams& p, int ntok, int C, size_t max_bytes, Run&& run) {
    const size_t img_rows = (size_t)p.nwin * ntok, img_bytes = img_rows * C * 2;
    if (img_bytes == 0 || img_bytes > max_bytes) return hipErrorInvalidValue;
    const int per_run = (int)std::min<size_t>((size_t)p.B, max_bytes / img_bytes);
    for (int b0 = 0; b0 < p.B; b0 += per_run) {
        SwinAttnParams q = p;
        q.B = std::min(per_run, p.B - b0);
        q.x = (const char*)p.x + (size_t)b0 * img_bytes;
        q.y = (char*)p.y + (size_t)b0 * img_bytes;
        if (p.stats_out) q.stats_out = p.stats_out + (size_t)b0 * img_rows * 2;
        if (p.live) q.live = p.live + b0;
        if (hipError_t e = run(q); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace
}  // namespace w2x
