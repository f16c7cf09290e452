// Launch interface of the HIP kernels (gfx950).  Plain C structs, no torch types.
#pragma once
#include <hip/hip_runtime.h>

#include "support.h"
#include "switches.h"
#include "dither.h"
#include "light.h"
#include "edge.h"
#include <cstdint>

namespace w2x {

constexpr int kGemmBM = 128;   // rows per GEMM workgroup tile (every instantiation)

// The opt-in to more than 64 KiB of dynamic LDS is a per-device attribute of a kernel: every launcher calls this with its own
// static mask before launching, so that engines on several devices of one process (one host thread each) all get it.
inline hipError_t ensure_dynamic_lds(const void* fn, int bytes, unsigned& done_mask) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned bit = 1u << (dev & 31);
    if (__atomic_load_n(&done_mask, __ATOMIC_ACQUIRE) & bit) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) __atomic_fetch_or(&done_mask, bit, __ATOMIC_RELEASE);
    return e;
}

// Cache policy of the kernels' OUTPUT stores (round 6).  What a launch produces is read by the next launch, never by itself: with the nt (streaming) policy the rows
// stay out of L2, which they would only pass through, and leave it to the weights and to the rows a launch fetches a second time.  The four transformer kernels together:
// -0.9 % per frame in five alternating runs on two boxes (profiles/r6_kernels/lib_nt_stores_frame_level.txt).  W2X_ST_AUX = the aux operand of the buffer stores
// (2 = nt, 0 = default policy; per file: tools/ab/lib_variants.sh "<file>:-DW2X_ST_AUX=0"); w2x_store_out() is the same choice for stores through a plain pointer.
#ifndef W2X_ST_AUX
#define W2X_ST_AUX 2
#endif
// cache policy of a kernel's LAST read of its input rows (the residual fetch of the transformer kernels; the C = 96 MLP reads its rows once)
#ifndef W2X_LD_LAST_AUX
#define W2X_LD_LAST_AUX 2
#endif
#ifdef __HIPCC__
template <class T> __device__ __forceinline__ void w2x_store_out(T* p, const T v) {
#if W2X_ST_AUX == 2
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}
#endif

// Dead-skip extents (liveness.h): per (plan op, pass slot) the part of the op's row map (W x H tokens) that some kept output pixel of the slot's tile
// depends on - columns [0, cx) U [W - wx, W), rows [0, cy) U [H - wy, H); cx >= W and cy >= H: everything.  The engine keeps one table per op in device memory and
// rewrites it with the slot table of every frame; a kernel reads its slot's entry once per workgroup / tile through the scalar data cache (a uniform load from
// the constant address space) and skips units whose rows are all dead.  A null table means "all" (w2x_infer, the tools).
struct LiveExt { uint16_t cx, wx, cy, wy; };
#ifdef __HIPCC__
__device__ __forceinline__ LiveExt live_ext_load(const LiveExt* t, int slot) {
    typedef const unsigned long long __attribute__((address_space(4)))* cptr;
    const unsigned long long v = ((cptr)(unsigned long long)t)[slot];
    return LiveExt{(uint16_t)v, (uint16_t)(v >> 16), (uint16_t)(v >> 32), (uint16_t)(v >> 48)};
}
__device__ __forceinline__ bool live_token(const LiveExt e, int x, int y, int W, int H) { return (x < e.cx || x >= W - e.wx) && (y < e.cy || y >= H - e.wy); }
// rows [r0, r0 + n) of a pass of row-major W x H token maps (n <= W H, wave-uniform arguments): false when none of them is live
__device__ __forceinline__ bool live_rows(const LiveExt* t, long r0, int n, int W, int H) {
    const int HW = W * H;
    if (n > HW) return true;
    const int img = (int)(r0 / HW);
    int r = (int)(r0 - (long)img * HW);
    LiveExt e = live_ext_load(t, img);
    for (int left = n; left > 0;) {
        if (r >= HW) { r -= HW; e = live_ext_load(t, img + 1); }      // (the run crosses into the next image; past the last image nothing is stored: harmless)
        const int y = r / W, x0 = r - y * W, x1 = x0 + left < W ? x0 + left : W;      // the piece [x0, x1) of token row y
        if ((y < e.cy || y >= H - e.wy) && (x0 < e.cx || x1 > W - e.wx)) return true;
        left -= x1 - x0; r += x1 - x0;
    }
    return false;
}
#endif

struct TView {           // device view of a channel-last tensor
    void* p = nullptr;
    int Hs = 0, Ws = 0, Cs = 0;  // stored dims
    int y0 = 0, x0 = 0;          // origin of the logical window
};

struct GemmParams {
    TView a;
    int amode = 0, kh = 1, kw = 1, stride = 1;
    int B = 0, Mrows = 0, aW = 0;
    const int* win_table = nullptr;
    int K = 0, N = 0, Kw = 0;       // Kw: row stride of wt (K rounded up to 8, zero padded)
    const void* wt = nullptr;       // fp16 [N][Kw]
    const void* wt_frag = nullptr;  // fragment-major copy (fragorder.h) for k_pixgemm.hip, or null
    const void* wt_perm = nullptr;  // fragorder.h frag_conv3b copy for k_conv3.hip's conv3b_kernel, or null
    const float* bias = nullptr;    // [N]
    const float* csum = nullptr;    // [N] (ln)
    const float* stats_in = nullptr;  // [pixels of a][2]
    int ln = 0;
    int act = 0; float alpha = 0.f;
    int has_clip = 0; float clip_lo = 0.f, clip_hi = 0.f;
    const float* a_scale = nullptr;   // fp32 [B][a.Cs]: squeeze-excite gate of the input map, applied to A on load (rounded to fp16 like the in-place pass)
    const float* res_scale = nullptr; // fp32 [B][res.Cs]: the same for the first residual
    TView res, res2;                // p == nullptr: none
    TView out;
    int omode = 0, r = 1, Cout = 0;
    float* stats_out = nullptr; float ln_eps = 1e-5f;
    float* pool_out = nullptr;      // [B][ceil(Mrows/kGemmBM)][out.Cs] per-workgroup column sums (squeeze-excite)
};

struct AttnParams {
    const void* qkv = nullptr; void* out = nullptr;
    int B = 0, nwin = 0, heads = 0, hd = 0, ntok = 0;
    float scale = 1.f;
    const void* bias = nullptr;     // fp16 [nmask][heads][ntok][ntok]
    const int* maskid = nullptr;    // [nwin]
};

struct MlpParams {               // y = x + W2 gelu(W1 LN(x) + b1) + b2 on contiguous rows [M][C]
    const void* x = nullptr; void* y = nullptr;
    long M = 0; int C = 0;
    const void* w1 = nullptr;      // fp16 [2C][C], LayerNorm gamma folded in
    const float* b1 = nullptr;     // [2C], LayerNorm beta folded in
    const void* w2 = nullptr;      // fp16 [C][2C]
    const float* b2 = nullptr;     // [C]
    float eps = 1e-5f;
    float* stats_out = nullptr; float eps_out = 1e-5f;
    // fragment-major copies for k_mlp2.hip (engine.cpp): w1 as [hidden tile][k-step][lane][8]; w2 as
    // [chunk of 32 hidden][n-tile][lane][8] with the k order of the GELU'd accumulators (slots 0..3: hidden 4g+j, 4..7: 16+4g+j)
    const void* w1_frag = nullptr; const void* w2_frag = nullptr;
    // true: the fragment copies are in the 32x32x16 order of k_mlp96q.hip (fragorder.h frag32_major / frag32_w2; C = 96 in the engine)
    bool frag32 = false;
    // Image head folded into the launch (engine.cpp: the plan's last MLP followed by Linear 96 -> 64 = 4x4 sub-pixels x 4 stored channels, DepthToSpace(4), Clip):
    // y is not stored; every produced row goes through the head instead, out[b][4 oy + dy][4 ox + dx][0..3] = clip(fp16(y_row W^T + bias)) - the arithmetic of
    // toimage_kernel (k_pixgemm.hip), bit for bit.  ti_w = null: no head.
    const void* ti_w = nullptr;    // fp16 fragment-major [4 n-tiles][3 k-steps][64 lanes][8] (the head's GemmParams::wt_frag)
    const float* ti_b = nullptr;   // fp32 [64]
    void* ti_out = nullptr; int ti_Hs = 0, ti_Ws = 0, ti_Mrows = 0, ti_aW = 0;   // output map [B][Hs][Ws][4], rows per image, row width of the token map
    int ti_clip = 0; float ti_lo = 0.f, ti_hi = 0.f;
    long ti_row0 = 0;              // (set by the launcher when it cuts a pass into runs: global index of this run's first row)
    // dead-skip (LiveExt above): the op's table entry of the pass's first image, the token map of an image; null: every row runs
    const LiveExt* live = nullptr; int live_W = 0, live_H = 0;
    long live_row0 = 0;            // (set by the launcher like ti_row0)
};

struct SwinAttnParams {          // y = x + proj(W-MSA(LN(x))) on token maps [B][H][W][C], window 6x6
    const void* x = nullptr; void* y = nullptr;
    const int* table = nullptr;    // int32[H*W]: window-order row -> pixel (shift + partition); also the scatter map
    int H = 0, W = 0, ry = -1, rx = -1;   // ry >= 0: closed form of the table, pixel = ((y+ry)%H)*W + (x+rx)%W (no lookup)
    int B = 0, nwin = 0, C = 0, hd = 0;
    const void* wqkv = nullptr;    // fp16 [3C][C], LayerNorm gamma folded in
    const float* bqkv = nullptr;   // [3C], LayerNorm beta folded in
    float scale = 1.f;
    const float* bias32 = nullptr; // fp32 [nmask][heads][3][576]: (rel-pos bias + shift mask) * log2(e) in the kernel's lane order (lower.cpp)
    const int* maskid = nullptr;   // [nwin]
    const void* wproj = nullptr;   // fp16 [C][C]
    const float* bproj = nullptr;  // [C]
    float eps = 1e-5f;
    float* stats_out = nullptr; float eps_out = 1e-5f;
    // the same two matrices in MFMA-fragment order (engine.cpp frag_major): [16-row tile][32-column k-step][lane][8], so a
    // wave's fragment load is one contiguous KiB.  Required by k_swinattn96.hip / k_swinattn192u.hip.
    const void* wqkv_frag = nullptr; const void* wproj_frag = nullptr;
    const LiveExt* live = nullptr; // dead-skip (LiveExt above): the op's table entry of the pass's first image; null: every window runs
};

struct SeParams {
    const float* pool = nullptr; float* scale = nullptr;   // pool: [B][nblocks][Cs] partial sums from the producing GEMM (nblocks row tiles per batch item)
    int B = 0, C = 0, Cs = 0, Cmid = 0; float inv_count = 0.f;
    int nblocks = 0, Mrows = 0;
    const float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
};

struct TileSlot { int x, y, aug, valid; };   // input rect origin (may be negative), augmentation 0..7, 0 = zero-pad slot

struct GatherParams {
    const uint8_t* frame = nullptr; int rows = 0, cols = 0; size_t step = 0;  // u8 BGR interleaved (deep: u16 samples; step in bytes)
    int deep = 0;
    void* out = nullptr;            // fp16 (fp32 engines: fp32) [B][T][T][4]
    int fp32 = 0;
    const TileSlot* slots = nullptr;
    int B = 0, T = 0;
};

struct ComposeParams {
    const void* tiles = nullptr;    // fp16 (fp32 engines: fp32) [slots][To][To][4], slot = tile*steps + aug
    int fp32 = 0;
    uint8_t* dst = nullptr; size_t dst_step = 0;    // u8 BGR (deep: u16 samples; step in bytes)
    int deep = 0;
    int outW = 0, outH = 0;
    int To = 0;
    int nx = 0, ny = 0;
    int stride_x = 0, stride_y = 0;   // To - outOverlap
    int ovx = 0, ovy = 0;             // blend ramp lengths (0: no blending)
    const float* ramp_x = nullptr;    // [ovx] left ramp, fl32(double(i+1)/(ovx+1))
    const float* ramp_y = nullptr;
    int tta = 0;
    int tta_bug_compat = 0;
    // strip rendering (one GPU of several composes only its columns): output columns [x0, x1) and the global index of
    // the tile held by slot 0 (x1 = 0: the whole canvas)
    int x0 = 0, x1 = 0; long first_tile = 0;
    // shard rendering (renderSharded): additionally output rows [y0, y1) (y1 = 0: all rows)
    int y0 = 0, y1 = 0;
};

// (a pass whose maps reach 2^31 halves of a, or pixels of res / res2 / out, is issued as runs of whole images; one image past that is hipErrorInvalidValue)
hipError_t launch_gemm(const GemmParams& p, hipStream_t s);
bool pixgemm_supported(const GemmParams& p);                    // k_pixgemm.hip: streaming kernel for pixel-shuffle projections
hipError_t launch_pixgemm(const GemmParams& p, hipStream_t s);
int pixgemm_rows_per_workgroup(const GemmParams& p);            // rows (2 x 2 branch: output pixels) per workgroup of the kernel launch_pixgemm picks; 0: none
bool conv3_supported(const GemmParams& p);                      // k_conv3.hip: LDS-tiled direct 3x3 convolution
// k_stem.hip: first 3x3 convolution on the 4-halves-per-pixel input tile (no LDS, weights in registers)
bool stem_supported(const GemmParams& p);
hipError_t launch_stem(const GemmParams& p, hipStream_t s);
hipError_t launch_conv3(const GemmParams& p, hipStream_t s);
bool conv3h_supported(const GemmParams& p);                     // k_conv3h.hip: direct 3x3 convolution onto 4 stored channels (cunet's image heads)
hipError_t launch_conv3h(const GemmParams& p, hipStream_t s);
bool conv48_supported(const GemmParams& p);                     // k_conv48.hip: direct 3x3 convolution 48 -> 96 channels (swin_unet's patch convolution)
hipError_t launch_conv48(const GemmParams& p, hipStream_t s);
bool conv48_stem_supported(const GemmParams& p, const GemmParams& ps);   // k_conv48.hip: the stem launch ps folded into the patch convolution p that alone reads its output
hipError_t launch_conv48_stem(const GemmParams& p, const GemmParams& ps, hipStream_t s);
bool conv3_stem_supported(const GemmParams& p, const GemmParams& ps);    // k_conv3.hip: the same for cunet's stem (4 -> 32) in front of its 32 -> 64 convolution
hipError_t launch_conv3_stem(const GemmParams& p, const GemmParams& ps, hipStream_t s);
bool conv3_up_supported(const GemmParams& p, const GemmParams& q);       // k_conv3.hip: cunet's ConvTranspose (pixel-shuffle projection q, LeakyReLU, skip add) computed in the halo stage of the 64 -> 64 convolution p behind it
hipError_t launch_conv3_up(const GemmParams& p, const GemmParams& q, hipStream_t s);
int conv3_tiles(const GemmParams& p);                           // workgroups (= pooling partials) per image of launch_conv3
hipError_t launch_attn(const AttnParams& p, hipStream_t s);
// k_f32.hip: the fp32 engine's kernels (Plan::elt == 4): general GEMM / convolution and the window attention core on fp32 rows
hipError_t launch_gemm_f32(const GemmParams& p, hipStream_t s, bool exact);      // exact: fp32 products (Precision::FP32); else three bf16 products per k-step (Precision::TF32)
hipError_t launch_attn_f32(const AttnParams& p, hipStream_t s);
// Fused MLP branch on fp32 rows with split-bf16 products (Precision::TF32; k_f32.hip mlp32_kernel): y = x + W2 gelu(W1 ((x - mean) rstd) + b1) + b2, the row statistics
// from the producer's stats tensor.  w1h / w1l, w2h / w2l: the bf16 hi / lo planes of W1 [2C][C] (LayerNorm gamma folded) and W2 [C][2C] in fragment-major order
// (fragorder.h frag_major of each plane).  The engine launches it in place of an fc1 / fc2 pair of gemm32 launches.
struct Mlp32Params {
    const float* x = nullptr; float* y = nullptr;
    long M = 0; int C = 0;
    const float* stats_in = nullptr;     // [M][2]: mean, rstd
    const void *w1h = nullptr, *w1l = nullptr, *w2h = nullptr, *w2l = nullptr;
    const float *b1 = nullptr, *b2 = nullptr;
    float* stats_out = nullptr; float eps_out = 1e-5f;
};
hipError_t launch_mlp32(const Mlp32Params& p, hipStream_t s);
// Fused Swin attention branch on fp32 rows with split-bf16 products (Precision::TF32; k_f32.hip swinattn32_kernel): y = res + proj(W-MSA((x - mean) rstd)), in place of the
// un-fused plan's qkv gemm -> attention core -> proj gemm.  Rows are pixels of plain [pixels][C] maps; table_in / table_out: window-order row -> pixel inside a batch item
// (the qkv op's gather table and the proj op's scatter table); weights as bf16 hi / lo planes, fragment-major (frag_major of each plane of W [3C][C] / [C][C]).
struct SwinAttn32Params {
    const float* x = nullptr; float* y = nullptr; const float* res = nullptr;
    int B = 0, nwin = 0, C = 0;
    long pix_per_item = 0;
    const int* table_in = nullptr; const int* table_out = nullptr;
    const float* stats_in = nullptr;
    const void *wqkv_h = nullptr, *wqkv_l = nullptr, *wproj_h = nullptr, *wproj_l = nullptr;
    const float *bqkv = nullptr, *bproj = nullptr;
    float scale = 1.f;
    const float* bias = nullptr; const int* maskid = nullptr;      // fp32 [nmask][6][36][36], [nwin]
    float* stats_out = nullptr; float eps_out = 1e-5f;
};
hipError_t launch_swinattn32(const SwinAttn32Params& p, hipStream_t s);
hipError_t launch_mlp(const MlpParams& p, hipStream_t s);
hipError_t launch_swin_attn(const SwinAttnParams& p, hipStream_t s);
// swin_attn_supported / mlp_supported / mlp32_supported / swinattn32_supported / gemm_row_stats_supported / attn_supported: support.h
// Dithered output (dither.h states the rule): what a dithered launch gets beside its parameters.  dx / dy: the pattern's offset per plane index c
// (R, G, B / Y, U, V = 0, 1, 2; gray = 1), already reduced mod 64; table: the device's copy of the 64 x 64 blue-noise ranks (dither_table_device(), BlueNoise
// only).  Every launcher below takes one as its last argument; mode None - the default - launches the kernel of the undithered engine, whose argument list and
// instructions do not know about any of this; a mode it has no kernel for is hipErrorInvalidValue.
struct DitherArgs {
    int mode = kDitherNone;
    int dx[3] = {0, 0, 0}, dy[3] = {0, 0, 0};
    const uint16_t* table = nullptr;
};
inline DitherArgs dither_args(int mode, unsigned phase, const uint16_t* table) {
    DitherArgs d;
    d.mode = mode; d.table = table;
    for (int c = 0; c < 3; ++c) { d.dx[c] = (int)dither_dx(phase, c); d.dy[c] = (int)dither_dy(phase, c); }
    return d;
}
inline bool dither_args_ok(const DitherArgs& d) { return dither_mode_ok(d.mode) && (d.mode != kDitherBlueNoise || d.table); }
// k_dither.hip: the blue-noise table in the current device's memory (part of the code object: nothing is uploaded); nullptr and *err on failure
const uint16_t* dither_table_device(hipError_t* err = nullptr);
// k_dither.hip dither_planes_kernel (test hook, Img2Img::ditherPlanes): n planes of rows x cols fp32 values (src, steps in bytes) quantised into the planes of
// dst (8 .. 16 bits) by the store of the compose / resample kernels (store4): V = v * (2^bits - 1), plane k with plane index k (one plane: 1)
struct PlanarPlanes;
hipError_t launch_dither_planes(const PlanarPlanes& src, const PlanarPlanes& dst, const DitherArgs& d, hipStream_t s);
// Resize in linear light (light.h states the rule): LightArgs, the curve as data.  The canvas launchers (launch_compose_canvas*) and the resample
// launchers take one as their last argument; mode Gamma - the default - launches the kernel of the engine that never heard of it, whose argument list and
// instructions do not know about any of this.  A canvas launch decodes the colour planes (never the alpha plane), a resample launch encodes them.
// k_light.hip light_decode_planes_kernel (test hook, Img2Img::resizePlanes): n fp32 values in place, v = decode(sat01(v)) by the device function the canvas
// kernels call; mode Gamma: no launch
hipError_t launch_light_decode_planes(float* v, size_t n, const LightArgs& l, hipStream_t s);
hipError_t launch_se(const SeParams& p, hipStream_t s);
hipError_t launch_scale(void* x, const float* scale, int B, int HW, int Cs, bool fp32, hipStream_t s);
// edge (every gather launcher of the RGB family): the rule that replaces the two clamp lines, a template parameter of the kernel; kEdgeReplicate - the
// default - launches the kernel that never heard of it; an unknown mode is hipErrorInvalidValue
hipError_t launch_gather(const GatherParams& p, hipStream_t s, int edge = kEdgeReplicate);
hipError_t launch_compose(const ComposeParams& p, hipStream_t s, const DitherArgs& d = DitherArgs());
// k_prepost.hip compose_canvas_kernel: compose_kernel's per-pixel sums for the same rect of p (x0..x1, y0..y1; p.dst / p.deep unused) left
// unquantised as fp32 RGB planes: canvas[c][Y][X], plane stride outW * outH (the input of the resize, renderResized)
hipError_t launch_compose_canvas(const ComposeParams& p, float* canvas, hipStream_t s, const LightArgs& l = LightArgs());
// k_resample.hip resample_kernel: an antialiased separable resize of the fp32 RGB canvas (three planes of inH x inW) to outH x outW, quantised like
// compose (sat(rint(x * 255)), 16-bit: 65535) and stored as BGR.  The tap tables (tiles.h resize_taps) live on the device: fx / wx per output column,
// fy / wy per output row; rows_max = the input rows an output tile of kResampleRows rows reads at most (resample_rows_max).  Every resize kernel
// below (RGBA, planes, YUV) is this one with another store: the two passes and the launch sequence are shared (pixel_device.h)
struct ResampleParams {
    const float* canvas = nullptr; int inW = 0, inH = 0;
    uint8_t* dst = nullptr; size_t dst_step = 0; int deep = 0;
    int outW = 0, outH = 0;
    const int* fx = nullptr; const float* wx = nullptr; int kx = 0;
    const int* fy = nullptr; const float* wy = nullptr; int ky = 0;
    int rows_max = 0;
};
constexpr int kResampleRows = 16, kResampleCols = 64;
// compose_kernel's launch shape (k_prepost.hip, where the choice is measured), also compose_planes_kernel's: rows a thread walks, threads per workgroup
#ifndef W2X_COMPOSE_ROWS
#define W2X_COMPOSE_ROWS 4
#endif
#ifndef W2X_COMPOSE_THREADS
#define W2X_COMPOSE_THREADS 64
#endif
constexpr int kComposeRows = W2X_COMPOSE_ROWS, kComposeThreads = W2X_COMPOSE_THREADS;
// host: the largest input row span of an output row tile; rows_above = 1: of the tile and the output row above it (top-left sited 4:2:0 chroma)
int resample_rows_max(const int* fy, int outH, int inH, int ky, int rows_above = 0);
// the same for the tables of an edged resize (resize_taps_edge: full support, rows below 0 and past inH): nothing is cut at inH
int resample_rows_max_edge(const int* fy, int outH, int ky);
// e (launch_resample, _rgba, _planar, _planar_rgba): mode Wrap or Mirror - the tables are resize_taps_edge's, rows_max resample_rows_max_edge's, and
// every input index of pass 1 goes through the rule; Replicate - the default - launches the kernel that never heard of it
hipError_t launch_resample(const ResampleParams& p, hipStream_t s, const DitherArgs& d = DitherArgs(), const LightArgs& l = LightArgs(), const EdgeArgs& e = EdgeArgs());
// YUV 4:2:0 frames (Img2Img::renderYuv): three planes - Y of rows x cols, U and V of ceil(rows/2) x ceil(cols/2) - with 8-bit (uint8) or 10-bit
// (uint16, low 10 bits) samples; steps in bytes.  Chroma siting (siting): kYuvLeft, MPEG-2 "left", chroma (i, j) at luma (x = 2j, y = 2i + 1/2);
// kYuvCenter (JPEG, MPEG-1) at (2j + 1/2, 2i + 1/2); kYuvTopLeft (BT.2020) at (2j, 2i).  Per subsampled axis a siting is one of two rules, co-sited or centred:
// Left = co-sited columns, centred rows; Center = both centred; TopLeft = both co-sited.  I422 has the column rule only, I444 none.
// layout (YuvLayout): kYuvI420 the above; kYuvI422 U and V of rows x ceil(cols/2) (chroma row y serves luma row y); kYuvI444 U and V of
// rows x cols; kYuvNV12 I420 with U and V interleaved in p[1] (ceil(rows/2) rows of 2 * ceil(cols/2) samples, U first; p[2] unused) and, at 10 bits,
// the code in the high 10 bits of each uint16 of Y and UV (P010: read >> 6, written << 6).
constexpr int kYuvI420 = 0, kYuvI422 = 1, kYuvI444 = 2, kYuvNV12 = 3;
struct YuvPlanes {
    uint8_t* p[3] = {nullptr, nullptr, nullptr}; size_t step[3] = {0, 0, 0};
    int rows = 0, cols = 0, bits = 8;
    int layout = kYuvI420;
    int siting = 0;                                             // kYuvLeft
};
constexpr int kYuvLeft = 0, kYuvCenter = 1, kYuvTopLeft = 2;
// the 1-D rule of a siting along the columns / the rows: true = centred, false = co-sited
constexpr bool yuv_cols_centred(int siting) { return siting == kYuvCenter; }
constexpr bool yuv_rows_centred(int siting) { return siting != kYuvTopLeft; }
// the chroma plane's rows and samples per row (NV12: both components) of a rows x cols frame
inline int yuv_chroma_rows(int rows, int layout) { return layout == kYuvI420 || layout == kYuvNV12 ? (rows + 1) / 2 : rows; }
inline int yuv_chroma_samples(int cols, int layout) { return layout == kYuvI444 ? cols : layout == kYuvNV12 ? 2 * ((cols + 1) / 2) : (cols + 1) / 2; }
// The code <-> normalised value maps of one (matrix, range, bits) (yuv_coefs): Y' = (Y - y_off) * y_mul, C' = (C - c_off) * c_mul on input,
// Y = y_off + Y' / y_mul, C = c_off + C' / c_mul on output; kr, kb, kg the matrix
struct YuvCoefs {
    float y_off = 0.f, y_mul = 0.f, c_off = 0.f, c_mul = 0.f;   // input: code -> normalised
    float y_scale = 0.f, c_scale = 0.f;                         // output: normalised -> code (before y_off / c_off are added)
    float kr = 0.f, kg = 0.f, kb = 0.f;
    float r_cr = 0.f, g_cb = 0.f, g_cr = 0.f, b_cb = 0.f;       // R = Y' + r_cr Cr', G = Y' + g_cb Cb' + g_cr Cr', B = Y' + b_cb Cb'
    float cb_div = 0.f, cr_div = 0.f;                           // Cb' = (B - Y') * cb_div, Cr' = (R - Y') * cr_div
    int maxcode = 255;
};
// matrix 0 BT.601, 1 BT.709, 2 BT.2020 non-constant; full_range 0 limited ("tv"), 1 full ("pc"); bits 8 or 10 (host, in double, rounded once to float)
inline YuvCoefs yuv_coefs(int matrix, int full_range, int bits) {
    const double kr = matrix == 0 ? 0.299 : matrix == 1 ? 0.2126 : 0.2627, kb = matrix == 0 ? 0.114 : matrix == 1 ? 0.0722 : 0.0593, kg = 1.0 - kr - kb;
    const double q = (double)(1 << (bits - 8)), top = (double)((1 << bits) - 1);
    const double y_off = full_range ? 0.0 : 16.0 * q, y_scale = full_range ? top : 219.0 * q;
    const double c_off = full_range ? (double)(1 << (bits - 1)) : 128.0 * q, c_scale = full_range ? top : 224.0 * q;
    YuvCoefs k;
    k.y_off = (float)y_off; k.y_mul = (float)(1.0 / y_scale); k.c_off = (float)c_off; k.c_mul = (float)(1.0 / c_scale);
    k.y_scale = (float)y_scale; k.c_scale = (float)c_scale;
    k.kr = (float)kr; k.kg = (float)kg; k.kb = (float)kb;
    k.r_cr = (float)(2.0 * (1.0 - kr)); k.b_cb = (float)(2.0 * (1.0 - kb));
    k.g_cb = (float)(-2.0 * (1.0 - kb) * kb / kg); k.g_cr = (float)(-2.0 * (1.0 - kr) * kr / kg);
    k.cb_div = (float)(1.0 / (2.0 * (1.0 - kb))); k.cr_div = (float)(1.0 / (2.0 * (1.0 - kr)));
    k.maxcode = (1 << bits) - 1;
    return k;
}
// k_prepost.hip gather_yuv_kernel: gather_kernel's tiles (same slots, replicate padding, TTA source index) from a YUV frame - Y and the 2 x 2
// chroma neighbours of the source pixel, chroma upsampled to the luma grid, the matrix inverted in fp32, R, G, B clamped to [0, 1].  One instantiation
// per src.layout: I422 interpolates columns only, I444 reads the pixel's own chroma, NV12 is I420 on de-interleaved samples.
struct GatherYuvParams {
    YuvPlanes src; YuvCoefs k;
    void* out = nullptr; int fp32 = 0;
    const TileSlot* slots = nullptr;
    int B = 0, T = 0;
};
hipError_t launch_gather_yuv(const GatherYuvParams& p, hipStream_t s);
// k_prepost.hip compose_yuv_kernel: compose_pixel_sums over the whole canvas (p.c: p.c.dst / deep / x0..y1 unused), R, G, B clamped to [0, 1],
// written as YUV 4:2:0 planes of p.c.outH x p.c.outW: Y per pixel, Cb / Cr of the RGB filtered (1/4, 1/2, 1/4) x (1/2, 1/2) onto each chroma site
struct ComposeYuvParams {
    ComposeParams c;
    YuvPlanes dst; YuvCoefs k;
};
constexpr int kYuvSites = 4, kYuvThreads = 64;   // chroma sites (8 luma columns, 2 rows) per thread, threads per workgroup (one wave)
// dst.siting kYuvTopLeft, I420 / NV12: the chroma rows a workgroup walks with the luma row above carried in registers.  One luma row is computed
// twice per band: (2 * 12 + 1) / (2 * 12) = 1.042 of kYuvLeft's pixel sums
#ifndef W2X_YUV_BAND
#define W2X_YUV_BAND 12
#endif
constexpr int kYuvBand = W2X_YUV_BAND;   // (a build switch like W2X_COMPOSE_ROWS, for A/B runs of k_prepost.hip: profiles/yuv_siting/compose_band.txt)
// dst.layout picks the kernel: I420 and NV12 compose_yuv_kernel (NV12: U and V stored interleaved, P010 codes << 6), I422 the same kernel
// without the vertical pair (a thread owns four sites of ONE luma row), I444 compose_yuv444_kernel (compose_kernel's shape: four pixels of a row per
// thread, its four-pixel fast path, no chroma filter)
hipError_t launch_compose_yuv(const ComposeYuvParams& p, hipStream_t s, const DitherArgs& d = DitherArgs());
// RGBA frames (renderRgba; k_rgba.hip).
// alpha_bleed_kernel: the uploaded BGRA frame split into the BGR frame gather reads and the alpha plane, with the colour of every pixel of alpha > 0
// spread `radius` pixels (0..16) outward under the pixels of alpha == 0 (tiles.h alpha_bleed states the arithmetic), all iterations in one launch.
// minmax: two device words the launch reduces max(A) and max(255 - A) into with vector atomics (the caller zeroes them first).
struct AlphaBleedParams {
    const uint8_t* bgra = nullptr; size_t step = 0; int rows = 0, cols = 0;   // u8 BGRA interleaved, rows 4-byte aligned
    int radius = 0;
    uint8_t* bgr = nullptr; size_t bgr_step = 0;                              // out: u8 BGR interleaved
    uint8_t* alpha = nullptr; size_t alpha_step = 0;                          // out: u8 plane
    unsigned* minmax = nullptr;
};
constexpr int kBleedTileW = 64, kBleedTileH = 32, kBleedMaxRadius = 16;
// wrap (kEdgeWrap): the eight neighbours are taken through the rule, so all eight always exist; false: a neighbour outside the frame does not exist
hipError_t launch_alpha_bleed(const AlphaBleedParams& p, hipStream_t s, bool wrap = false);
// gather_rgba_kernel: gather_kernel on the two planes of an RGBA frame.  A slot of this table says which plane it reads in `valid`: 1 the BGR frame
// (exactly gather_kernel), 2 the alpha plane as the gray pixel (a, a, a, 0), a = u8 * fl32(1/255); 0 stays the zero-pad slot.
struct GatherRgbaParams {
    const uint8_t* bgr = nullptr; size_t bgr_step = 0;
    const uint8_t* alpha = nullptr; size_t alpha_step = 0;
    int rows = 0, cols = 0;
    void* out = nullptr; int fp32 = 0;
    const TileSlot* slots = nullptr;
    int B = 0, T = 0;
};
constexpr int kSlotColour = 1, kSlotAlpha = 2;
hipError_t launch_gather_rgba(const GatherRgbaParams& p, hipStream_t s, int edge = kEdgeReplicate);
// compose_rgba_kernel: compose_pixel_sums over the colour tiles (c.tiles) quantised to B, G, R, and over the alpha tiles (alpha_tiles, the same grid, slot 0 =
// tile 0) whose green sum quantised the same way is A; one dword B | G << 8 | R << 16 | A << 24 per pixel into c.dst (c.dst_step bytes per row, 4-byte
// aligned).  alpha_tiles == nullptr: A = alpha_value everywhere (a uniform plane whose tiles were not run).
struct ComposeRgbaParams {
    ComposeParams c;
    const void* alpha_tiles = nullptr;
    unsigned alpha_value = 255;
};
hipError_t launch_compose_rgba(const ComposeRgbaParams& p, hipStream_t s, const DitherArgs& d = DitherArgs());
// Resized RGBA frames (renderRgbaResized; k_rgba.hip).
// compose_canvas_rgba_kernel: compose_canvas_kernel over both tile sets of an RGBA frame - the colour tiles' sums as the fp32 planes R, G, B (what
// compose_canvas_kernel writes for the colour frame) and the green sum of the alpha tiles as a fourth plane A (what it writes into plane 1 for the gray
// image): canvas[c][Y][X], plane stride outW * outH, whole canvas (c.x0..y1, c.dst, c.deep unused).  alpha_tiles == nullptr: three planes.
struct ComposeCanvasRgbaParams {
    ComposeParams c;
    const void* alpha_tiles = nullptr;
    float* canvas = nullptr;
};
hipError_t launch_compose_canvas_rgba(const ComposeCanvasRgbaParams& p, hipStream_t s, const LightArgs& l = LightArgs());
// resample_rgba_kernel: resample_kernel's resize (same tap tables, same rows_max, same accumulation per plane) over the four planes of that canvas, each
// quantised sat(rint(x * 255)) and stored as one dword B | G << 8 | R << 16 | A << 24 per pixel into dst (dst_step bytes per row, a multiple of 4).
// uniform != 0: the canvas has three planes, none is filtered for alpha and A = alpha_value everywhere.
struct ResampleRgbaParams {
    const float* canvas = nullptr; int inW = 0, inH = 0;
    uint8_t* dst = nullptr; size_t dst_step = 0;
    int outW = 0, outH = 0;
    const int* fx = nullptr; const float* wx = nullptr; int kx = 0;
    const int* fy = nullptr; const float* wy = nullptr; int ky = 0;
    int rows_max = 0;
    int uniform = 0; unsigned alpha_value = 255;
};
hipError_t launch_resample_rgba(const ResampleRgbaParams& p, hipStream_t s, const DitherArgs& d = DitherArgs(), const LightArgs& l = LightArgs(), const EdgeArgs& e = EdgeArgs());
// Frames of planes (k_planar.hip): `n` planes of rows x cols samples - uint8 (bits 8), little-endian uint16 with the code in the low bits (10 / 12 / 16) or
// float32 of nominal [0, 1] (32) - each with its own pointer and step in bytes; u16 / f32 samples aligned to their size.  n = 3: planar RGB frames (renderPlanar,
// DESIGN 9h), planes R, G, B.  n = 1: gray frames (renderGray) of 8 or 16 bits: one sample per pixel on both sides, the result the green channel of
// the BGR path on B = G = R = g - the planar frame whose three planes are the one.
struct PlanarPlanes {
    uint8_t* p[3] = {nullptr, nullptr, nullptr}; size_t step[3] = {0, 0, 0};
    int rows = 0, cols = 0, bits = 8;
    int n = 3;
};
inline bool planar_bits_ok(int bits) { return bits == 8 || bits == 10 || bits == 12 || bits == 16 || bits == 32; }
inline size_t planar_sample_bytes(int bits) { return bits == 32 ? 4 : bits > 8 ? 2 : 1; }
// gather_planes_kernel: gather_kernel's tiles (same slots, replicate padding, TTA source index) from the planes: the tile pixel is make_px(r, g, b) - one plane:
// (a, a, a, 0) -, each sample min(code, 2^bits - 1) * fl32(1 / (2^bits - 1)) - at 8 and 16 bits gather_kernel's own constants - or, float, min(max(x, 0), 1)
// with NaN -> 0
struct GatherPlanarParams {
    PlanarPlanes src;
    void* out = nullptr; int fp32 = 0;
    const TileSlot* slots = nullptr;
    int B = 0, T = 0;
};
hipError_t launch_gather_planar(const GatherPlanarParams& p, hipStream_t s, int edge = kEdgeReplicate);
// compose_planes_kernel: compose_kernel over the whole canvas of c (c.dst / c.deep / x0..y1 unused): the three sums of compose_pixel_sums - one plane: the
// green sum - into the planes of dst (c.outH x c.outW), integer sat(rint(x * (2^bits - 1))), float min(max(x, 0), 1) stored as fp32
struct ComposePlanarParams {
    ComposeParams c;
    PlanarPlanes dst;
};
hipError_t launch_compose_planar(const ComposePlanarParams& p, hipStream_t s, const DitherArgs& d = DitherArgs());
// The hand-off of a chained render (k_chain.hip): the frame between two stages is [rows][cols][4] tile pixels of the CONSUMING engine's type - half4
// (frame_fp32 / fp32 = 0) or float4v -, values in [0, 1], lane 3 zero, 8- / 16-byte aligned.
// compose_px_kernel: compose_kernel over the whole canvas of c (c.dst / c.deep / x0..y1 unused): the three sums of compose_pixel_sums, each min(max(x, 0), 1), rounded
// once to the frame's type, one vector store per pixel into frame[c.outH][c.outW]
struct ComposePxParams {
    ComposeParams c;
    void* frame = nullptr; int frame_fp32 = 0;
};
hipError_t launch_compose_px(const ComposePxParams& p, hipStream_t s);
// gather_px_kernel: gather_kernel's tiles (same slots, replicate padding, TTA source index) copied out of such a frame: one vector load and one vector store per
// tile pixel, no conversion (fp32: the type of frame and tiles alike)
struct GatherPxParams {
    const void* frame = nullptr; int rows = 0, cols = 0;
    void* out = nullptr; int fp32 = 0;
    const TileSlot* slots = nullptr;
    int B = 0, T = 0;
};
hipError_t launch_gather_px(const GatherPxParams& p, hipStream_t s, int edge = kEdgeReplicate);
// compose_canvas_gray_kernel: the green sums of compose_pixel_sums over the whole canvas of p (x0..y1, dst, deep unused) unquantised as one fp32 plane
// canvas[Y][X] of outH x outW: the canvas of a resized gray frame (a resized planar frame has compose_canvas_kernel's)
hipError_t launch_compose_canvas_gray(const ComposeParams& p, float* canvas, hipStream_t s, const LightArgs& l = LightArgs());
// resample_planes_kernel: resample_kernel's resize (same tap tables, same rows_max, same accumulation) of the fp32 canvas of dst.n planes, the accumulators
// quantised like compose_planes_kernel into the planes of dst (outH x outW)
struct ResamplePlanarParams {
    const float* canvas = nullptr; int inW = 0, inH = 0;
    int outW = 0, outH = 0;
    const int* fx = nullptr; const float* wx = nullptr; int kx = 0;
    const int* fy = nullptr; const float* wy = nullptr; int ky = 0;
    int rows_max = 0;
    PlanarPlanes dst;
};
hipError_t launch_resample_planar(const ResamplePlanarParams& p, hipStream_t s, const DitherArgs& d = DitherArgs(), const LightArgs& l = LightArgs(), const EdgeArgs& e = EdgeArgs());
// Planar RGBA frames (renderPlanarRgba; k_planar_rgba.hip): four planes R, G, B, A of one sample type, laid out like PlanarPlanes' three.
struct RgbaPlanes {
    uint8_t* p[4] = {nullptr, nullptr, nullptr, nullptr}; size_t step[4] = {0, 0, 0, 0};
    int rows = 0, cols = 0, bits = 8;
};
// alpha_bleed_planes_kernel: alpha_bleed_kernel on planes of any integer depth (tiles.h alpha_bleed_planes states the arithmetic): the colour planes of src with
// every code clamped to 2^bits - 1 and the colours of the visible pixels (clamped alpha > 0) spread `radius` pixels (0 .. kBleedMaxRadius) under the others into
// colour[0..2], the alpha plane copied into alpha (steps in bytes, planes of src.bits samples).  Float planes: radius 0 only, both copied bit for bit.
// minmax: two device words (zeroed by the caller) that receive max(key) and max(top - key) over the frame, key the clamped alpha code and top 2^bits - 1 - float:
// the bits of min(max(a, 0), 1) (NaN, -0.0: 0) and top 0x3F800000, which order as the values do -: the plane is one value iff the two add up to top.
struct AlphaBleedPlanesParams {
    RgbaPlanes src;
    int radius = 0;
    uint8_t* colour[3] = {nullptr, nullptr, nullptr}; size_t colour_step = 0;
    uint8_t* alpha = nullptr; size_t alpha_step = 0;
    unsigned* minmax = nullptr;
};
inline unsigned alpha_key_top(int bits) { return bits == 32 ? 0x3F800000u : (1u << bits) - 1u; }
hipError_t launch_alpha_bleed_planes(const AlphaBleedPlanesParams& p, hipStream_t s, bool wrap = false);
// gather_planes_rgba_kernel: gather_rgba_kernel's slots (kSlotColour / kSlotAlpha) over those planes with gather_planes_kernel's samples: a colour slot reads
// make_px(r, g, b) from colour[0..2], an alpha slot (a, a, a) from the alpha plane
struct GatherPlanarRgbaParams {
    const uint8_t* colour[3] = {nullptr, nullptr, nullptr}; size_t colour_step = 0;
    const uint8_t* alpha = nullptr; size_t alpha_step = 0;
    int rows = 0, cols = 0, bits = 8;
    void* out = nullptr; int fp32 = 0;
    const TileSlot* slots = nullptr;
    int B = 0, T = 0;
};
hipError_t launch_gather_planar_rgba(const GatherPlanarRgbaParams& p, hipStream_t s, int edge = kEdgeReplicate);
// compose_planes_rgba_kernel: compose_planes_kernel's three sums over the colour tiles (c.tiles) into dst.p[0..2] and its green sum over the alpha tiles (the same
// grid, slot 0 = tile 0) into dst.p[3], quantised alike; alpha_tiles == nullptr: the plane is alpha_value (in [0, 1]) quantised like a sum.
struct ComposePlanarRgbaParams {
    ComposeParams c;
    const void* alpha_tiles = nullptr;
    float alpha_value = 1.f;
    RgbaPlanes dst;
};
hipError_t launch_compose_planar_rgba(const ComposePlanarRgbaParams& p, hipStream_t s, const DitherArgs& d = DitherArgs());
// resample_planes_rgba_kernel: resample_planes_kernel over the four planes of compose_canvas_rgba_kernel's canvas; uniform != 0: the canvas has three planes and
// dst.p[3] is alpha_value quantised like an accumulator
struct ResamplePlanarRgbaParams {
    const float* canvas = nullptr; int inW = 0, inH = 0;
    int outW = 0, outH = 0;
    const int* fx = nullptr; const float* wx = nullptr; int kx = 0;
    const int* fy = nullptr; const float* wy = nullptr; int ky = 0;
    int rows_max = 0;
    RgbaPlanes dst;
    int uniform = 0; float alpha_value = 1.f;
};
hipError_t launch_resample_planar_rgba(const ResamplePlanarRgbaParams& p, hipStream_t s, const DitherArgs& d = DitherArgs(), const LightArgs& l = LightArgs(), const EdgeArgs& e = EdgeArgs());
// k_resample_yuv.hip: resample_kernel's resize of the fp32 RGB canvas (same tap tables, same rows_max, the same two passes) with compose_yuv_kernel's
// encoding behind it instead of the BGR quantisation: the resized R, G, B clamped to [0, 1] and written as the YUV planes of dst (outH x outW =
// dst.rows x dst.cols), Y per pixel; 4:2:0: Cb / Cr of the RGB filtered (1/4, 1/2, 1/4) x (1/2, 1/2) onto each chroma site (renderYuvResized)
struct ResampleYuvParams {
    const float* canvas = nullptr; int inW = 0, inH = 0;
    int outW = 0, outH = 0;
    const int* fx = nullptr; const float* wx = nullptr; int kx = 0;
    const int* fy = nullptr; const float* wy = nullptr; int ky = 0;
    int rows_max = 0;
    YuvPlanes dst; YuvCoefs k;
};
// dst.layout picks the kernel: I420 resample_yuv_kernel, a thread per chroma site; NV12 / P010 resample_yuv_nv12_kernel, the same body and so
// I420's samples, with U and V interleaved in plane 1 and, at 10 bits, every code << 6; I444 resample_kernel's pass 2 with each pixel's own Cb / Cr; I422 the
// same shape with the chroma filter along the row alone
// rows_max_above: resample_rows_max(.., 1) of the same tables.  The launcher, which knows what the destination's siting dispatches, sizes the LDS and the kernel's
// row pitch by it where the kernel reads the row above its tile (top-left sited I420 / NV12) and by p.rows_max everywhere else; a top-left launch
// without it is an error, not a launch with too little LDS.
hipError_t launch_resample_yuv(const ResampleYuvParams& p, int rows_max_above, hipStream_t s, const DitherArgs& d = DitherArgs(), const LightArgs& l = LightArgs());
// debug/test helpers used by w2x_infer (mirrors blobFromImages / imagesFromBlob, img2img_infer.cpp:5-39)
hipError_t launch_blob_to_nhwc(const float* nchw, void* out_nhwc4, int B, int T, bool fp32, hipStream_t s);
hipError_t launch_nhwc_to_blob(const void* in_nhwc4, float* nchw, int B, int T, bool fp32, hipStream_t s);

#ifdef __HIPCC__
namespace gate {
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
// x * s on 8 halves, s fp32 per channel (cunet's squeeze-excite gates: the in-place pass scale_kernel and the gated operand loads of
// k_gemm / k_pixgemm all go through this, so folding a gate never changes a bit): v_fma_mixlo / mixhi read the f16 halves directly,
// multiply by the fp32 gate and write f16 - one instruction per element
typedef unsigned gate_u4 __attribute__((ext_vector_type(4)));
typedef float gate_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ half8 gate8(const half8 v, const float* sc) {
    const gate_f4 s0 = *(const gate_f4*)sc, s1 = *(const gate_f4*)(sc + 4);
    const float s[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
    gate_u4 x = __builtin_bit_cast(gate_u4, v), o;
    const float zero = 0.f;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        unsigned r;
        asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(x[d]), "v"(s[2 * d]), "v"(zero));
        asm("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(r) : "v"(x[d]), "v"(s[2 * d + 1]), "v"(zero));
        o[d] = r;
    }
    return __builtin_bit_cast(half8, o);
}
}  // namespace gate
#endif

}  // namespace w2x
