// Fused transformer MLP branch, C = 192, on v_mfma_f32_32x32x16_f16 tiles:   y = x + W2 * gelu(W1 * LayerNorm(x) + b1) + b2
// The engine's C = 192 kernel of rounds 3 - 5 (mlp2q_kernel<192, 4> of csrc/k_mlp2.hip then), retired in round 6 when the 16x16x32 kernel mlp2_kernel<192, 2, 4>
// took the same time per launch for less energy per product (profiles/r6_kernels/lib_mlp192_tile16_frame_level.txt, mlp192_tile_shape_power.txt).
// The schedule of csrc/k_mlp2.hip - a wave owns 32 token rows from the first load to the last store, the four waves of a workgroup stage each
// 32-hidden-unit chunk of the weights once into LDS by LDS-DMA, double-buffered, one barrier per chunk, a ring of six fragment registers - on the tile
// shape of csrc/k_mlp96q.hip (why: there): a chunk is ONE 32 x 32 accumulator of the transposed first product (12 k-steps of 16 channels), whose registers
// 8s .. 8s+7 are the B fragment of k-step s of the second product as they stand (W2 stored in that k order: fragorder.h frag32_w2); the second product is
// 6 tiles of 32 output channels x 2 k-steps.  Same FLOP, same 24 KiB of fragments per chunk, half the matrix instructions, LayerNorm sums with one lane swap.
// The weight buffers alias the row slabs (the rows are in registers by then), so the residual rows are fetched a second time.  No dead-skip: the kernel
// predates it and runs every row.
//
// This file is an alternative source of the library's object k_mlp2.o: it defines launch_mlp2, for weights in the 32x32x16 fragment order only (C = 96
// goes to csrc/k_mlp96q.hip as in the product, C = 192 to the kernel below, anything else is an error).  Two ways to run it:
//   kernel alone, against the shipped 16x16x32 kernel as variant 0 (then tools/ab/mlp192_variants [rows] on the GPU):
//     FRAG32_MASK=0b10 tools/ab/mlp192_variants.sh "" "SRC=<root>/tools/ab/k_mlp192q.hip"
//   whole library, the engine built to store the C = 192 weights in this order (support.h):
//     tools/ab/lib_variants.sh "engine.cpp:-DW2X_MLP192_TILE32+k_mlp2.hip@tools/ab/k_mlp192q.hip"
// tests/test_gpu_kernel_ab.py runs the first.
#include "transformer_device.h"

// W2X_MLP2Q_EXP, timing experiments (results are wrong; tools/ab/mlp192_variants.sh): bit 0 no barrier per chunk, bit 1 no weight staging after
// chunk 0 (and no wait for it), bit 2 GELU replaced by the bare conversion, bit 3 no matrix products, bit 4 every wave fetches its rows (and the residual
// rows) from the first 12 KiB of x (cache hits: no HBM latency or bandwidth on the way in), bit 5 no stores.
#ifndef W2X_MLP2Q_PIPE
#define W2X_MLP2Q_PIPE 0     // 1: the chunk loop software-pipelined (first-layer products of chunk c + 1 between the pieces of chunk c's GELU), see mlp2q_kernel
#endif
#ifndef W2X_MLP2Q_EXP
#define W2X_MLP2Q_EXP 0
#endif
// 1: the first chunk's weights get a buffer of their own behind the slabs (78 KB per workgroup, still two per CU) and are staged when the workgroup starts,
// under the row fetch and the LayerNorm; 0: both buffers alias the slabs, chunk 0 is staged after the rows are in registers and waited for on the spot.
// Measured equal (0.3025 / 0.0794 against 0.3004 / 0.0790 ms, profiles/r3_kernels/mlp2q_early0.txt): the CU's other workgroup already covers the wait.  Off.
#ifndef W2X_MLP2Q_EARLY0
#define W2X_MLP2Q_EARLY0 0
#endif
// 1: the odd k-steps of the first layer on a second accumulator - two chains of six dependent products instead of one of twelve.  -1.6 % per launch, within
// noise (LEDGER, round 3): it is not the dependent chain.  Off.
#ifndef W2X_MLP2Q_SPLITACC
#define W2X_MLP2Q_SPLITACC 0
#endif

namespace w2x {
namespace {

constexpr size_t kMaxBufBytes = 0xFFF00000u;   // the longest run of a pass: 32-bit byte offsets, with room for a last tile's pieces past the end, whose offsets must not wrap

// the <192, 2, 4> geometry of csrc/k_mlp2.hip's Mlp2Cfg
constexpr int C = 192, RW = 32, NWV = 4, NTHR = NWV * 64, BM = NWV * RW;   // 32 rows per wave, 4 waves = 128 rows per workgroup
constexpr int LDX = C + 8, PPR = C / 8;      // slab row stride in halves (16-byte pieces rotate over the banks), 16-byte pieces per row
constexpr int NP = RW * PPR / 64;            // flat 16-byte pieces per lane (12)
constexpr int SLAB = RW * LDX * 2;           // bytes per wave
constexpr int KS = C / 16, NT = C / 32, NCH = 2 * C / 32;   // 12 k-steps of 16 channels, 6 output tiles of 32 channels, 12 chunks of 32 hidden units
constexpr int NF = KS + 2 * NT, NFW = NF / NWV;             // weight fragments (KiB) per chunk (24), per wave (6)
constexpr int WBUF = NF * 1024;              // one staged chunk, two buffers
constexpr int RING = 6;                      // weight-fragment registers of a wave
constexpr int WORK = NWV * SLAB > 2 * WBUF ? NWV * SLAB : 2 * WBUF;   // the buffers alias the slabs
constexpr int BIAS_OFF = WORK;               // b1 [2C] | b2 [C] as fp32 behind the work area: the per-chunk bias reads are LDS reads (csrc/k_mlp2.hip)
constexpr int SMEM = WORK + 3 * C * 4;
constexpr int SMEMQ = W2X_MLP2Q_EARLY0 ? NWV * SLAB + WBUF + 3 * C * 4 : SMEM;
static_assert(NF % NWV == 0 && NF % RING == 0 && KS >= RING, "fragments per wave / ring slots");
static_assert(RW * PPR % 64 == 0, "flat piece count");

// (the second launch bound is hipcc's minimum number of waves per SIMD, not blocks per CU: two workgroups of four waves per CU)
__global__ __launch_bounds__(NTHR, 2) void mlp2q_kernel(const MlpParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, h = lane >> 5;
    _Float16* Xw = (_Float16*)(smem + wv * SLAB);          // [RW][LDX]
    // two weight buffers of NF fragments [64 lanes][8]: odd chunks in the slab area (the rows are in registers by then), even chunks behind it (EARLY0) or there as well
    constexpr int BUF0 = W2X_MLP2Q_EARLY0 ? NWV * SLAB : 0, BUF1 = W2X_MLP2Q_EARLY0 ? 0 : WBUF;
    constexpr int BIASQ = W2X_MLP2Q_EARLY0 ? NWV * SLAB + WBUF : BIAS_OFF;
    auto wbuf = [&](int ch) { return smem + ((ch & 1) ? BUF1 : BUF0); };

    const long row0 = ((long)blockIdx.x * NWV + wv) * RW;
    const long nrows = p.M - row0 < RW ? p.M - row0 : RW;
    const unsigned xbytes = (unsigned)(p.M * (C * 2));
    const __amdgpu_buffer_rsrc_t XB = make_rsrc(p.x, xbytes);
    const __amdgpu_buffer_rsrc_t YB = make_rsrc(p.y, xbytes);
    const unsigned vo = nrows > 0 ? (unsigned)row0 * (C * 2) + lane * 16u : 0xFFFFC000u;
    const unsigned vl = (W2X_MLP2Q_EXP & 16) ? lane * 16u : vo;     // (timing experiment: where the rows are read from)
    const _Float16* __restrict__ W1 = (const _Float16*)p.w1_frag + lane * 8;   // frag32_major: [NCH row tiles of 32][KS][64][8]
    const _Float16* __restrict__ W2 = (const _Float16*)p.w2_frag + lane * 8;   // frag32_w2:    [NCH][NT][2][64][8]
    auto frag_src = [&](int ch, int f) { return f < KS ? W1 + (size_t)(ch * KS + f) * 512 : W2 + (size_t)(ch * 2 * NT + (f - KS)) * 512; };
    auto stage = [&](int ch) {
#pragma unroll
        for (int i = 0; i < NFW; ++i) {
            const int f = wv * NFW + i;
            __builtin_amdgcn_global_load_lds((const void*)frag_src(ch, f), (__attribute__((address_space(3))) void*)(wbuf(ch) + (size_t)f * 1024), 16, 0, 0);
        }
    };
    auto lds_frag = [&](int ch, int j) { return *(const half8*)(wbuf(ch) + (size_t)j * 1024 + lane * 16); };   // consumption order = storage order
#if W2X_MLP2Q_EARLY0
    stage(0);                                  // the oldest requests of the wave: they land under the row fetch
#endif
    for (int i = tid; i < 3 * C; i += NWV * 64) ((float*)(smem + BIASQ))[i] = i < 2 * C ? p.b1[i] : p.b2[i - 2 * C];
    const float* B1s = (const float*)(smem + BIASQ) + h * 4;
    const float* B2s = B1s + 2 * C;

    // ---- x rows: flat coalesced pieces -> slab -> LayerNorm in fragment layout (lane (r32, h): channels ks*16 + 8h .. +7 of row r32)
    {
        half8 xr[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) xr[k] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(XB, vl + k * 1024u, 0, 0));
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int idx = k * 64 + lane, r = idx / PPR, c = idx - r * PPR;
            *(half8*)(Xw + r * LDX + c * 8) = xr[k];
        }
    }
    W2X_PHASE_FENCE();
    half8 xreg[KS];
    {
        half8 raw[KS];
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { raw[ks] = *(const half8*)(Xw + r32 * LDX + ks * 16 + h * 8); sum_sq8_acc(raw[ks], s, q); }
        halves_sum2(s, q);
        const float mean = s * (1.f / C);
        const float rstd = __builtin_amdgcn_rsqf(fmaxf(q * (1.f / C) - mean * mean, 0.f) + p.eps);
        const float nm = -mean * rstd;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) xreg[ks] = norm8(raw[ks], rstd, nm);
    }
#if W2X_MLP2Q_PIPE
    // ---- software-pipelined chunk loop (round 4).  Per chunk a wave issues 24 matrix instructions (12 first-layer, 12 second-layer) and ~130 vector
    // instructions (the GELU of 16 values per lane), and as written above they come in separate runs: a 32 x 32 product lets about four vector
    // instructions issue for free while it occupies the pipe (tools/issue_model.hip: 23.4 ticks alone, 31.6 with eight), but a run of products has none to
    // hide and the GELU run has no product to hide behind.  Here the FIRST-layer products of chunk c + 1 (they depend on nothing of chunk c) are issued
    // one by one between the pieces of chunk c's GELU.  What it takes: a second first-layer accumulator (16 registers), and the staged chunks skewed by
    // half a chunk - buffer c holds W1 of chunk c + 1 and W2 of chunk c (fragments 0 .. KS-1 / KS .. NF-1, consumption order = storage order as before).
    W2X_PHASE_FENCE();
    auto skew_src = [&](int c, int f) { return f < KS ? W1 + (size_t)((c + 1) * KS + f) * 512 : W2 + (size_t)(c * 2 * NT + (f - KS)) * 512; };
    auto stage_skew = [&](int c) {               // c = -1: only W1 of chunk 0; c = NCH - 1: only W2 of the last chunk
#pragma unroll
        for (int i = 0; i < NFW; ++i) {
            const int f = wv * NFW + i;
            if ((f < KS && c + 1 >= NCH) || (f >= KS && c < 0)) continue;
            __builtin_amdgcn_global_load_lds((const void*)skew_src(c, f), (__attribute__((address_space(3))) void*)(wbuf(c & 1) + (size_t)f * 1024), 16, 0, 0);
        }
    };
    __syncthreads();                           // every wave holds its rows in registers: the slab area becomes weight buffers
    stage_skew(-1);
    __builtin_amdgcn_s_waitcnt(0x0F70);        // vmcnt(0)
    __syncthreads();
    stage_skew(0);                             // lands under the first chunk's first-layer products
    float16v acc1n;
    {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4v b = *(const float4v*)(B1s + q * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc1n[4 * q + j] = b[j];
        }
        half8 w0[RING];
#pragma unroll
        for (int i = 0; i < RING; ++i) w0[i] = lds_frag(-1, i);
#pragma unroll
        for (int j = 0; j < KS; ++j) {
            acc1n = __builtin_amdgcn_mfma_f32_32x32x16_f16(w0[j % RING], xreg[j], acc1n, 0, 0, 0);
            if (j + RING < KS) { w0[j % RING] = lds_frag(-1, j + RING); W2X_RING_FENCE(); }
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);        // vmcnt(0): this wave's share of buffer 0
    __syncthreads();
    half8 wr[RING];
    float16v acc2[NT];                         // rows = output channels 32nt + 8q + 4h + j in register 4q + j, columns = tokens; from b2
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4v b = *(const float4v*)(B2s + nt * 32 + q * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc2[nt][4 * q + j] = b[j];
        }
    half8 xres[NP];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const bool more = ch + 1 < NCH;        // there is a next chunk whose first-layer products run under this chunk's GELU
        if (more) stage_skew(ch + 1);
        const int f0 = more ? 0 : KS;          // first fragment consumed from this buffer
#pragma unroll
        for (int i = 0; i < RING; ++i) wr[i] = lds_frag(ch, f0 + i);
        const float16v acc1 = acc1n;
        if (more) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4v b = *(const float4v*)(B1s + (ch + 1) * 32 + q * 8);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc1n[4 * q + j] = b[j];
            }
        }
        // GELU of chunk ch in eight pieces of one value pair each, a first-layer product of chunk ch + 1 in front of every piece (and of the
        // four conversions); the scheduling barriers keep the pieces between the products
        float2v gp[8];
        half8 a2[2];
        // ten pieces - pairs 0..3, pack a2[0], pairs 4..7, pack a2[1] - spread over the KS product slots: slot j takes pieces [10 j / KS, 10 (j + 1) / KS)
#pragma unroll
        for (int j = 0; j < KS; ++j) {
            if (more) {
                acc1n = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr[j % RING], xreg[j], acc1n, 0, 0, 0);
                wr[j % RING] = lds_frag(ch, j + RING);          // (f0 = 0 here: fragments KS .. KS + RING - 1 are the first of the second layer)
                W2X_RING_FENCE();
            }
#pragma unroll
            for (int e = 10 * j / KS; e < 10 * (j + 1) / KS; ++e) {
                if (e == 4 || e == 9) {
                    const int s2 = e == 4 ? 0 : 1;
                    a2[s2] = (half8){(_Float16)gp[4 * s2][0], (_Float16)gp[4 * s2][1], (_Float16)gp[4 * s2 + 1][0], (_Float16)gp[4 * s2 + 1][1],
                                     (_Float16)gp[4 * s2 + 2][0], (_Float16)gp[4 * s2 + 2][1], (_Float16)gp[4 * s2 + 3][0], (_Float16)gp[4 * s2 + 3][1]};
                } else {
                    const int w = e < 4 ? e : e - 1;             // value pair w = registers 2w, 2w + 1 of the accumulator
                    gp[w] = gelu_fast2((float2v){acc1[2 * w], acc1[2 * w + 1]});
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (ch == NCH - 1) {   // the residual rows, requested as soon as the normalised copies have served their last product
#pragma unroll
            for (int k = 0; k < NP; ++k) xres[k] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(XB, vl + k * 1024u, 0, W2X_LD_LAST_AUX));
        }
#pragma unroll
        for (int i = 0; i < 2 * NT; ++i) {     // second layer: fragment KS + i = (output tile i >> 1, k-step i & 1)
            const int k = (more ? KS : 0) + i; // position in this chunk's consumption order
            acc2[i >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr[k % RING], a2[i & 1], acc2[i >> 1], 0, 0, 0);
            if (f0 + k + RING < NF) { wr[k % RING] = lds_frag(ch, f0 + k + RING); W2X_RING_FENCE(); }
        }
        if (more) __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();
    }
#else
    W2X_PHASE_FENCE();
#if W2X_MLP2Q_EARLY0
    __builtin_amdgcn_s_waitcnt(0x0F70);        // vmcnt(0): this wave's share of chunk 0 (requested first) has landed
    __syncthreads();                           // every wave holds its rows in registers: the slab area becomes the odd chunks' buffer
#else
    __syncthreads();                           // every wave holds its rows in registers: the slab area becomes weight buffers
    stage(0);
    __builtin_amdgcn_s_waitcnt(0x0F70);        // vmcnt(0): this wave's share of chunk 0 has landed
    __syncthreads();
#endif

    half8 wr[RING];
#pragma unroll
    for (int i = 0; i < RING; ++i) wr[i] = lds_frag(0, i);
    float16v acc2[NT];                         // rows = output channels 32nt + 8q + 4h + j in register 4q + j, columns = tokens; from b2
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4v b = *(const float4v*)(B2s + nt * 32 + q * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc2[nt][4 * q + j] = b[j];
        }
    half8 xres[NP];
#if defined(W2X_MLP2Q_PRIO) && W2X_MLP2Q_PRIO == 1   // s_setprio by phase: 1 = the chunk loop at priority 1, row phases at 0; 2 = the reverse; 3 = only the GELU at 1
    __builtin_amdgcn_s_setprio(1);
#elif defined(W2X_MLP2Q_PRIO) && W2X_MLP2Q_PRIO == 2
    __builtin_amdgcn_s_setprio(0);
#endif
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        if (ch + 1 < NCH && !(W2X_MLP2Q_EXP & 2)) stage(ch + 1);
        float16v acc1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4v b = *(const float4v*)(B1s + ch * 32 + q * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc1[4 * q + j] = b[j];
        }
#if W2X_MLP2Q_SPLITACC
        float16v acc1b = {};                   // odd k-steps on a second accumulator: two chains of six dependent products instead of one of twelve
#endif
#pragma unroll
        for (int j = 0; j < KS; ++j) {
#if W2X_MLP2Q_SPLITACC
            if (j & 1) acc1b = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr[j % RING], xreg[j], acc1b, 0, 0, 0);
            else
#endif
            if (!(W2X_MLP2Q_EXP & 8)) acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr[j % RING], xreg[j], acc1, 0, 0, 0);
            else acc1[j % 16] += (float)wr[j % RING][0] + (float)xreg[j][0];
            wr[j % RING] = lds_frag(ch, j + RING);
            W2X_RING_FENCE();
        }
#if W2X_MLP2Q_SPLITACC
        acc1 += acc1b;
#endif
        if (ch == NCH - 1) {   // the residual rows, requested as soon as the normalised copies have served their last product
#pragma unroll
            for (int k = 0; k < NP; ++k) xres[k] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(XB, vl + k * 1024u, 0, W2X_LD_LAST_AUX));
        }
        half8 a2[2];
#if defined(W2X_MLP2Q_PRIO) && W2X_MLP2Q_PRIO == 3
        __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            auto act2 = [](float2v v) { return (W2X_MLP2Q_EXP & 4) ? v : gelu_fast2(v); };
            const float2v g0 = act2((float2v){acc1[8 * s2 + 0], acc1[8 * s2 + 1]});
            const float2v g1 = act2((float2v){acc1[8 * s2 + 2], acc1[8 * s2 + 3]});
            const float2v g2 = act2((float2v){acc1[8 * s2 + 4], acc1[8 * s2 + 5]});
            const float2v g3 = act2((float2v){acc1[8 * s2 + 6], acc1[8 * s2 + 7]});
            a2[s2] = (half8){(_Float16)g0[0], (_Float16)g0[1], (_Float16)g1[0], (_Float16)g1[1],
                             (_Float16)g2[0], (_Float16)g2[1], (_Float16)g3[0], (_Float16)g3[1]};
        }
#if defined(W2X_MLP2Q_PRIO) && W2X_MLP2Q_PRIO == 3
        __builtin_amdgcn_s_setprio(0);
#endif
#pragma unroll
        for (int i = 0; i < 2 * NT; ++i) {     // fragment KS + i = (output tile i >> 1, k-step i & 1)
            const int j = KS + i;
            if (!(W2X_MLP2Q_EXP & 8)) acc2[i >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr[j % RING], a2[i & 1], acc2[i >> 1], 0, 0, 0);
            else acc2[i >> 1][i % 16] += (float)wr[j % RING][0] + (float)a2[i & 1][0];
            if (j + RING < NF) { wr[j % RING] = lds_frag(ch, j + RING); W2X_RING_FENCE(); }
        }
        if (ch + 1 < NCH && !(W2X_MLP2Q_EXP & 2)) __builtin_amdgcn_s_waitcnt(0x0F70);
        if (!(W2X_MLP2Q_EXP & 1)) __syncthreads();
        if (ch + 1 < NCH) {
#pragma unroll
            for (int i = 0; i < RING; ++i) wr[i] = lds_frag(ch + 1, i);
        }
    }
#if defined(W2X_MLP2Q_PRIO) && W2X_MLP2Q_PRIO == 1
    __builtin_amdgcn_s_setprio(0);
#elif defined(W2X_MLP2Q_PRIO) && W2X_MLP2Q_PRIO == 2
    __builtin_amdgcn_s_setprio(1);
#endif

#endif
    W2X_PHASE_FENCE();
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *(half4*)(Xw + r32 * LDX + nt * 32 + q * 8 + h * 4) = (half4){(_Float16)acc2[nt][4 * q], (_Float16)acc2[nt][4 * q + 1], (_Float16)acc2[nt][4 * q + 2], (_Float16)acc2[nt][4 * q + 3]};
    W2X_PHASE_FENCE();
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int idx = k * 64 + lane, r = idx / PPR, c = idx - r * PPR;
        const half8 o = *(const half8*)(Xw + r * LDX + c * 8) + xres[k];
        if (!(W2X_MLP2Q_EXP & 32) || o[0] == (_Float16)12345.f) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4v, o), YB, vo + k * 1024u, 0, 0);
        if (p.stats_out) *(half8*)(Xw + r * LDX + c * 8) = o;
    }
    W2X_PHASE_FENCE();
    if (p.stats_out && lane < nrows) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int c = 0; c < PPR; ++c) sum_sq8_acc(*(const half8*)(Xw + lane * LDX + c * 8), s, q);
        const float mean = s * (1.f / C);
        p.stats_out[2 * (row0 + lane)] = mean;
        p.stats_out[2 * (row0 + lane) + 1] = __builtin_amdgcn_rsqf(fmaxf(q * (1.f / C) - mean * mean, 0.f) + p.eps_out);
    }
}

}  // namespace

bool mlp96q_supported(const MlpParams& p);                        // csrc/k_mlp96q.hip
hipError_t launch_mlp96q(const MlpParams& p, hipStream_t s);

hipError_t launch_mlp2(const MlpParams& p, hipStream_t s) {
    if (p.C == 96 && p.frag32) return mlp96q_supported(p) ? launch_mlp96q(p, s) : hipErrorInvalidValue;
    if (p.C != C || !p.frag32) return hipErrorInvalidValue;
    static unsigned lds_ok = 0;   // per-device bit: kernels.h ensure_dynamic_lds
    if (hipError_t e = ensure_dynamic_lds((const void*)mlp2q_kernel, SMEMQ, lds_ok); e != hipSuccess) return e;
    // the kernel addresses x / y with 32-bit byte offsets: longer passes run in pieces of whole workgroups
    const long max_rows = (long)((kMaxBufBytes / (C * 2)) / BM) * BM;
    return for_mlp_runs(p, max_rows, [&](const MlpParams& q) {
        hipLaunchKernelGGL(mlp2q_kernel, dim3((unsigned)((q.M + BM - 1) / BM)), dim3(NTHR), SMEMQ, s, q);
        return hipGetLastError();
    });
}

}  // namespace w2x
