// Fused transformer MLP branch for gfx950, wave-private rows:   y = x + W2 * gelu(W1 * LayerNorm(x) + b1) + b2
// Every wave owns 16*TT token rows from the first load to the last store:
//   * x rows arrive as one flat, fully coalesced stream into the wave's LDS slab; each lane then reads the 16-byte pieces it
//     uses as MFMA fragments, LayerNorm statistics are the lane's own sums plus two row swaps, and the normalised pieces are
//     the operand registers of GEMM1 as they stand (LDS program order is the only ordering needed inside a wave, see
//     W2X_PHASE_FENCE);
//   * weights: the four waves of a workgroup stage each 32-hidden-unit chunk once into LDS by LDS-DMA (global_load_lds: the
//     fragment-major copy of engine.cpp makes a fragment one contiguous KiB = one wave instruction, no registers in between),
//     double-buffered, one workgroup barrier per chunk - per-wave weight streams from L2 were 56 % of the C = 192 kernel's time -
//     and read them into a ring of six registers, each fragment six fragments ahead of its use;
//   * GEMM1 is computed transposed (rows = 32 hidden units of the chunk, columns = tokens) so that the GELU'd accumulators
//     are, as they stand, the B fragments of GEMM2 with a permuted k order (W2 is stored with the same permutation) - no LDS
//     round trip between the two products; GEMM2 is transposed too (rows = output channels), so a lane ends with 4 consecutive
//     channels of a token: b2 is the initial accumulator and the tile reaches the slab in 8-byte stores;
//   * the result tile goes through the slab once so that residual add and stores are flat 16-byte pieces again; at C = 96 the
//     raw x rows are still in the slab at that point (the weight buffers sit behind the slabs), so x is read from HBM once.
// TT = 2 for both widths, which leaves C = 96 at 3 waves per SIMD.
#include "transformer_device.h"

#include <cstdlib>

// C = 192 geometry (tools/ab/mlp192_variants.sh times the alternatives): token tiles of 16 rows per wave, waves per workgroup, and
// the workgroups per CU the register budget is set for
#ifndef W2X_MLP192_TT
#define W2X_MLP192_TT 2
#endif
#ifndef W2X_MLP192_NW
#define W2X_MLP192_NW 4
#endif
#ifndef W2X_MLP192_WPS
#define W2X_MLP192_WPS 2
#endif
#ifndef W2X_MLP192_KEEP
#define W2X_MLP192_KEEP 0     // 1: weight buffers behind the slabs, the raw rows stay in LDS for the residual add (no second fetch); needs 8 waves per
#endif                        // workgroup to fit the CU (one workgroup of 150 KB instead of two of 51 KB)

namespace w2x {
namespace {

constexpr size_t kMaxBufBytes = 0xFFF00000u;   // the longest run of a pass (for_mlp_runs): 32-bit byte offsets, with room for a last tile's pieces past the end, whose offsets must not wrap

// sum over the four 16-lane rows of a wave (swap16 and why the swaps are inline asm on two registers: transformer_device.h)
__device__ __forceinline__ void swap32(float& a, float& b) { asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 0" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ float rows_sum(float v) { float a = v, b = v; swap16(a, b); v = a + b; a = v; b = v; swap32(a, b); return a + b; }

template <int C, int TT, int NW>
struct Mlp2Cfg {
    static constexpr int RW = 16 * TT;           // rows per wave
    static constexpr int NWV = NW;               // waves per workgroup
    static constexpr int BM = NWV * RW;          // rows per workgroup
    static constexpr int LDX = C + 8;            // slab row stride in halves: 16-byte pieces rotate over the banks
    static constexpr int PPR = C / 8;            // 16-byte pieces per row
    static constexpr int KS = C / 32;            // k-steps of GEMM1
    static constexpr int NT = C / 16;            // output n-tiles of GEMM2
    static constexpr int NCH = 2 * C / 32;       // hidden chunks of 32
    static constexpr int NP = RW * PPR / 64;     // flat 16-byte pieces per lane
    static constexpr int SLAB = RW * LDX * 2;    // bytes per wave
    static constexpr int NF = 2 * KS + NT;       // weight fragments (KiB) per hidden chunk
    static constexpr int WBUF = NF * 1024;       // one staged chunk, two buffers
    static constexpr int RING = 6;               // weight-fragment registers of a wave
    // KEEP (C = 96): the weight buffers sit behind the slabs (50.6 KB per workgroup, still 3 workgroups per CU), so the raw x rows stay
    // in the slab and serve the residual add - x is read from HBM once.  Otherwise the buffers alias the slabs (x lives in
    // registers by then) and the residual rows are fetched a second time.
    static constexpr bool KEEP = C == 96 || (W2X_MLP192_KEEP && NW != 4);   // (four waves cannot: W2X_MLP192_KEEP above)
    static constexpr int WORK = KEEP ? NWV * SLAB + 2 * WBUF : (NWV * SLAB > 2 * WBUF ? NWV * SLAB : 2 * WBUF);
    // b1 [2C] | b2 [C] as fp32 behind the work area: the per-chunk bias reads are LDS reads.  As global loads they shared the vector
    // memory counter with the LDS-DMA staging of the NEXT chunk, and the wait for a chunk's two bias vectors (s_waitcnt vmcnt(0), in
    // order) was a wait for that staging: the double buffering did not overlap anything.
    static constexpr int BIAS_OFF = WORK;
    static constexpr int SMEM = WORK + 3 * C * 4;
    static_assert(NF % NWV == 0 && NF % RING == 0 && 2 * KS >= RING, "fragments per wave / ring slots");
    static_assert(RW * PPR % 64 == 0, "flat piece count");
};

template <int C, int TT, int NW>
// (the second launch bound is hipcc's minimum number of waves per SIMD, not blocks per CU)
__global__ __launch_bounds__(NW * 64, (C == 96 ? 3 : W2X_MLP192_WPS) * NW / 4) void mlp2_kernel(const MlpParams p) {
    using K = Mlp2Cfg<C, TT, NW>;
    constexpr int RW = K::RW, LDX = K::LDX, PPR = K::PPR, KS = K::KS, NT = K::NT, NCH = K::NCH, NP = K::NP, NF = K::NF, RING = K::RING;
    constexpr int NFW = NF / K::NWV;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, g = lane >> 4;
    _Float16* Xw = (_Float16*)(smem + wv * K::SLAB);          // [RW][LDX]
    unsigned char* const WBb = smem + (K::KEEP ? K::NWV * K::SLAB : 0);   // two weight buffers of NF fragments [64 lanes][8]

    // dead-skip (kernels.h LiveExt): a workgroup none of whose rows a kept output pixel depends on ends here - its waves share the staged weights and the
    // barriers, so the row group is the workgroup's BM rows.  Scalar table reads, uniform over the workgroup.
    if (p.live) {
        const long g0 = (long)blockIdx.x * K::BM, left = p.M - g0;
        if (!live_rows(p.live, p.live_row0 + g0, left < K::BM ? (int)left : K::BM, p.live_W, p.live_H)) return;
    }
    const long row0 = ((long)blockIdx.x * K::NWV + wv) * RW;       // first row of this wave
    const long nrows = p.M - row0 < RW ? p.M - row0 : RW;     // may be <= 0: the wave then only runs dead arithmetic
    // rows through buffer resources (32-bit byte offsets, bounds-checked: pieces past the last row read zeros, their stores are dropped;
    // the launcher cuts passes of more than kMaxBufBytes into runs)
    const unsigned xbytes = (unsigned)(p.M * (C * 2));
    const __amdgpu_buffer_rsrc_t XB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t YB = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, xbytes, 0x00020000);
    const unsigned vo = nrows > 0 ? (unsigned)row0 * (C * 2) + lane * 16u : 0xFFFFC000u;   // (no rows: every piece past the end, without wrapping)
    const _Float16* __restrict__ W1 = (const _Float16*)p.w1_frag + lane * 8;   // [NCH*2 row tiles][KS][64][8]
    const _Float16* __restrict__ W2 = (const _Float16*)p.w2_frag + lane * 8;   // [NCH][NT][64][8], k order of the GELU'd accumulators

    // ---- weights: the four waves stage each 32-hidden-unit chunk once into LDS (fragment-major: a fragment is one contiguous KiB,
    //      which is exactly what one LDS-DMA instruction of a wave moves - global_load_lds, 16 bytes per lane, no registers, no
    //      ds_write), two buffers, wave w brings fragments w*NFW .. of the next chunk while the current one is consumed.
    auto frag_src = [&](int ch, int f) { return f < 2 * KS ? W1 + (size_t)(ch * 2 * KS + f) * 512 : W2 + (size_t)(ch * NT + (f - 2 * KS)) * 512; };
    auto stage = [&](int ch) {
#pragma unroll
        for (int i = 0; i < NFW; ++i) {
            const int f = wv * NFW + i;
            __builtin_amdgcn_global_load_lds((const void*)frag_src(ch, f), (__attribute__((address_space(3))) void*)(WBb + (size_t)(ch & 1) * K::WBUF + (size_t)f * 1024), 16, 0, 0);
        }
    };
    // fragment j of a chunk in the order the products consume them: GEMM1 (k-step j / 2, hidden half j & 1), then GEMM2 (n-tile j - 2 KS)
    auto lds_frag = [&](int ch, int j) {
        const int f = j < 2 * KS ? (j & 1) * KS + (j >> 1) : j;
        return *(const half8*)(WBb + (size_t)(ch & 1) * K::WBUF + (size_t)f * 1024 + lane * 16);
    };
    if (K::KEEP) stage(0);                     // separate buffers: under the row loads and the LayerNorm
    for (int i = tid; i < 3 * C; i += K::NWV * 64) ((float*)(smem + K::BIAS_OFF))[i] = i < 2 * C ? p.b1[i] : p.b2[i - 2 * C];   // (first read after two barriers)
    const float* B1s = (const float*)(smem + K::BIAS_OFF) + g * 4;
    const float* B2s = B1s + 2 * C;

    // ---- x rows: flat coalesced load -> slab
    {
        half8 xr[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) xr[k] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(XB, vo + k * 1024u, 0, 0));
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int idx = k * 64 + lane, r = idx / PPR, c = idx - r * PPR;
            *(half8*)(Xw + r * LDX + c * 8) = xr[k];
        }
    }
    W2X_PHASE_FENCE();
    // ---- LayerNorm in fragment layout: lane (fr, g) holds channels ks*32 + 8g .. +7 of row 16tt + fr, so the row sums are the
    //      lane's own KS pieces plus the three other lane groups (two row swaps); the normalised pieces are the operand registers
    //      of GEMM1 as they stand (rows without data hold zeros: 0 * rstd - 0)
    half8 xreg[TT][KS];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
        half8 raw[KS];
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { raw[ks] = *(const half8*)(Xw + (tt * 16 + fr) * LDX + ks * 32 + g * 8); sum_sq8_acc(raw[ks], s, q); }
        s = rows_sum(s);
        q = rows_sum(q);
        const float mean = s * (1.f / C);
        const float rstd = __builtin_amdgcn_rsqf(fmaxf(q * (1.f / C) - mean * mean, 0.f) + p.eps);   // the argument is >= eps
        const float nm = -mean * rstd;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) xreg[tt][ks] = norm8(raw[ks], rstd, nm);
    }
    W2X_PHASE_FENCE();
    if (!K::KEEP) {
        __syncthreads();                       // every wave holds its rows in registers: the slab area becomes weight buffers
        stage(0);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);        // vmcnt(0): this wave's share of chunk 0 has landed
    __syncthreads();

    // Weight fragments reach the MFMAs through a ring of six registers: a fragment is requested from LDS right after the last MFMA
    // that used its register, six fragments (12 MFMAs) ahead of its use, so no product waits on an LDS round trip.  (Reads placed at
    // their point of use made the compiler wait for each one.)
    half8 wr[RING];
#pragma unroll
    for (int i = 0; i < RING; ++i) wr[i] = lds_frag(0, i);

    // GEMM2 is computed transposed as well (rows = output channels, columns = tokens): a lane ends with 4 consecutive channels of
    // one token (8-byte slab stores) and b2 is the initial accumulator
    float4v acc2[TT][NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const float4v b2v = *(const float4v*)(B2s + j * 16);
#pragma unroll
        for (int i = 0; i < TT; ++i) acc2[i][j] = b2v;
    }

    half8 xres[NP];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {   // fully unrolled: the ring registers are renamed statically
        if (ch + 1 < NCH) stage(ch + 1);       // into the other buffer (last read before the previous barrier); in flight under this chunk
        // GEMM1 (transposed): acc1[ht][tt] = W1[32ch + 16ht ..][:] * Xn[16tt ..][:]^T   (rows = hidden, columns = tokens), from b1
        float4v acc1[2][TT];
        {
            const float4v be = *(const float4v*)(B1s + ch * 32);
            const float4v bo = *(const float4v*)(B1s + ch * 32 + 16);
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) { acc1[0][tt] = be; acc1[1][tt] = bo; }
        }
#pragma unroll
        for (int j = 0; j < 2 * KS; ++j) {
            const int ks = j >> 1, ht = j & 1;
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) acc1[ht][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wr[j % RING], xreg[tt][ks], acc1[ht][tt], 0, 0, 0);
            wr[j % RING] = lds_frag(ch, j + RING);
            W2X_RING_FENCE();
        }
        if (!K::KEEP && ch == NCH - 1) {   // the residual rows, requested as soon as the normalised copies have served their last product:
#pragma unroll                           // they travel under the last GELU and second-layer products (round 2 fetched them in the epilogue and waited)
            for (int k = 0; k < NP; ++k) xres[k] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(XB, vo + k * 1024u, 0, W2X_LD_LAST_AUX));
        }
        // GELU in place; lane holds hidden rows 16ht + 4g + j of token column fr -> B fragment of GEMM2 for the
        // k order (ht 0: slots 0..3, ht 1: slots 4..7)
        half8 a2[TT];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
            const float4v e = acc1[0][tt], o = acc1[1][tt];
            const float2v g0 = gelu_fast2((float2v){e[0], e[1]});
            const float2v g1 = gelu_fast2((float2v){e[2], e[3]});
            const float2v g2 = gelu_fast2((float2v){o[0], o[1]});
            const float2v g3 = gelu_fast2((float2v){o[2], o[3]});
            a2[tt] = (half8){(_Float16)g0[0], (_Float16)g0[1], (_Float16)g1[0], (_Float16)g1[1],
                             (_Float16)g2[0], (_Float16)g2[1], (_Float16)g3[0], (_Float16)g3[1]};
        }
        // GEMM2 (transposed): acc2[tt][nt] += W2[16nt ..][chunk] * H[tokens][chunk]^T
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int j = 2 * KS + nt;
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) acc2[tt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wr[j % RING], a2[tt], acc2[tt][nt], 0, 0, 0);
            if (j + RING < NF) { wr[j % RING] = lds_frag(ch, j + RING); W2X_RING_FENCE(); }
        }
        if (ch + 1 < NCH) __builtin_amdgcn_s_waitcnt(0x0F70);    // vmcnt(0): this wave's share of the next chunk has landed
        __syncthreads();                       // (after the last chunk: every wave is done with the weight buffers the slabs alias)
        if (ch + 1 < NCH) {
#pragma unroll
            for (int i = 0; i < RING; ++i) wr[i] = lds_frag(ch + 1, i);
        }
    }

    W2X_PHASE_FENCE();
    // ---- epilogue: residual pieces first (KEEP: from the slab, which still holds the raw rows; otherwise a second fetch),
    //      accumulators -> fp16 tile in the slab, then flat pieces
    if (K::KEEP) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int idx = k * 64 + lane, r = idx / PPR, c = idx - r * PPR;
            xres[k] = *(const half8*)(Xw + r * LDX + c * 8);
        }
    }
    W2X_PHASE_FENCE();
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
            *(half4*)(Xw + (tt * 16 + fr) * LDX + nt * 16 + g * 4) = (half4){(_Float16)acc2[tt][nt][0], (_Float16)acc2[tt][nt][1], (_Float16)acc2[tt][nt][2], (_Float16)acc2[tt][nt][3]};
    W2X_PHASE_FENCE();
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int idx = k * 64 + lane, r = idx / PPR, c = idx - r * PPR;
        const half8 o = *(const half8*)(Xw + r * LDX + c * 8) + xres[k];     // fp16 + fp16 rounded once == fp32 add rounded to fp16
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4v, o), YB, vo + k * 1024u, 0, W2X_ST_AUX);
        if (p.stats_out) *(half8*)(Xw + r * LDX + c * 8) = o;
    }
    W2X_PHASE_FENCE();
    if (p.stats_out && lane < nrows) {   // LayerNorm statistics of the produced rows for an un-fused consumer
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int c = 0; c < PPR; ++c) sum_sq8_acc(*(const half8*)(Xw + lane * LDX + c * 8), s, q);
        const float mean = s * (1.f / C);
        p.stats_out[2 * (row0 + lane)] = mean;
        p.stats_out[2 * (row0 + lane) + 1] = __builtin_amdgcn_rsqf(fmaxf(q * (1.f / C) - mean * mean, 0.f) + p.eps_out);
    }
}

template <int C, int TT, int NW>
hipError_t launch_mlp2_c(const MlpParams& p, hipStream_t s) {
    using K = Mlp2Cfg<C, TT, NW>;
    static unsigned lds_ok = 0;   // per-device bit: kernels.h ensure_dynamic_lds
    if (hipError_t e = ensure_dynamic_lds((const void*)mlp2_kernel<C, TT, NW>, K::SMEM, lds_ok); e != hipSuccess) return e;
    // the kernel addresses x / y with 32-bit byte offsets: longer passes run in pieces of whole workgroups
    const long max_rows = (long)((kMaxBufBytes / (C * 2)) / K::BM) * K::BM;
    return for_mlp_runs(p, max_rows, [&](const MlpParams& q) {
        dim3 grid((unsigned)((q.M + K::BM - 1) / K::BM));
        hipLaunchKernelGGL((mlp2_kernel<C, TT, NW>), grid, dim3(K::NWV * 64), K::SMEM, s, q);
        return hipGetLastError();
    });
}

}  // namespace

bool mlp96q_supported(const MlpParams& p);                        // k_mlp96q.hip: C = 96 with both matrices resident in LDS
hipError_t launch_mlp96q(const MlpParams& p, hipStream_t s);

hipError_t launch_mlp2(const MlpParams& p, hipStream_t s) {
    // C = 96: the resident-weight kernel on 32x32 tiles (k_mlp96q.hip; the engine stores its weights in that kernel's fragment order,
    // fragorder.h frag32_*).  This file's chunked schedule at C = 96 (frag_major / frag_w2 order) remains for tools/ab/mlp_ab.hip.
    // C = 192 (weights 288 KiB): shared-weight schedule, 32 rows per wave, 4 waves per workgroup.
    // Measured alternatives: 8 waves per workgroup (a chunk staged once per 256 rows, one workgroup per CU) 2.0 ms of C = 192 MLP time
    // per frame against 1.77; in round 1 6 / 12 waves per workgroup 2.45 / 1.86 ms of MLP time per frame against 1.58; a per-wave
    // register ring straight from L2 (TT = 4) and 64 rows per wave with shared weights were slower as well.  The same schedule on 32x32x16 tiles
    // (mlp2q_kernel, the engine's C = 192 kernel of rounds 3 - 5) is tools/ab/k_mlp192q.hip, an alternative source of this object.
    if (p.C == 96 && p.frag32) return mlp96q_supported(p) ? launch_mlp96q(p, s) : hipErrorInvalidValue;
    if (p.C == 96) return launch_mlp2_c<96, 2, 4>(p, s);
    if (p.C == 192 && p.frag32) return hipErrorInvalidValue;   // the 32x32x16 fragment order at C = 192: tools/ab/k_mlp192q.hip, retired in round 6
    if (p.C == 192) return launch_mlp2_c<192, W2X_MLP192_TT, W2X_MLP192_NW>(p, s);
    return hipErrorInvalidValue;
}

}  // namespace w2x
