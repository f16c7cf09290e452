/* C ABI of libw2x.so - the FFI boundary for the hot path.
 *
 * Each entry point names the reference interface it replaces (paths relative to /root/reference/src/tensorrt/):
 *   w2x_create / w2x_destroy      trt::Img2Img::Img2Img / ~Img2Img            img2img.h:16-17, img2img_base.cpp:4-10
 *   w2x_set_message_callback      trt::Img2Img::setMessageCallback            img2img.h:21, logger.h:20
 *   w2x_set_progress_callback     trt::Img2Img::setProgressCallback           img2img.h:22, logger.h:21
 *   w2x_build                     trt::Img2Img::build(path, BuildConfig)      img2img.h:18, img2img_build.cpp:54-173
 *   w2x_load                      trt::Img2Img::load(path, RenderConfig)      img2img.h:19, img2img_load.cpp:117-291
 *   w2x_render                    trt::Img2Img::render(cv::Mat, cv::Mat&)     img2img.h:20, img2img_render.cpp:224-352
 *   w2x_infer                     trt::Img2Img::infer (private)               img2img.h:25, img2img_infer.cpp:41-93
 *   w2x_render_sharded            (extension) one frame over N engines         img2img_render.cpp:43-44, 329-330
 *   w2x_calculate_tiles           calculateTiles (file-static)                img2img_render.cpp:7-66
 *   w2x_tile_weights              createTileWeights (file-static)             img2img_load.cpp:29-52
 * Return convention: 1 = true, 0 = false (after the message callback received the error text), like the reference's
 * bool returns.  Plain pointers and sizes only.
 */
#ifndef W2X_C_API_H
#define W2X_C_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct w2x_engine w2x_engine;

enum { W2X_PRECISION_TF32 = 0, W2X_PRECISION_FP16 = 1, W2X_PRECISION_FP32 = 2 };  /* config.h:7-10; CLI map main.cpp:76-84; FP32: an addition (include/w2x/config.h) */

enum { W2X_RESIZE_BICUBIC = 0, W2X_RESIZE_BILINEAR = 1 };   /* extension: the filter of the resized renders (include/w2x/config.h ResizeFilter) */
/* extension: the matrix and range of the YUV renders (include/w2x/img2img.h YuvMatrix / YuvRange) */
enum { W2X_YUV_BT601 = 0, W2X_YUV_BT709 = 1, W2X_YUV_BT2020 = 2 };
enum { W2X_YUV_LIMITED = 0, W2X_YUV_FULL = 1 };
/* extension: the plane layouts of the YUV renders (include/w2x/img2img.h YuvLayout): yuv420p, yuv422p, yuv444p (10 bits: ...p10le) and nv12 (10 bits: p010le) */
enum { W2X_YUV_I420 = 0, W2X_YUV_I422 = 1, W2X_YUV_I444 = 2, W2X_YUV_NV12 = 3 };

typedef struct w2x_build_config {   /* trt::BuildConfig, config.h:12-31 */
    int deviceId, precision;
    int minBatchSize, optBatchSize, maxBatchSize;
    int minChannels, optChannels, maxChannels;
    int minWidth, optWidth, maxWidth;
    int minHeight, optHeight, maxHeight;
} w2x_build_config;

typedef struct w2x_render_config {  /* trt::RenderConfig, config.h:33-43 */
    int deviceId, precision, batchSize, channels, height, width, scaling;
    double overlapX, overlapY;
    int tta;
    int ttaBugCompat;               /* extension, see include/w2x/config.h */
} w2x_render_config;

typedef void (*w2x_message_fn)(int severity, const char* message, void* user);        /* logger.h:20 */
typedef void (*w2x_progress_fn)(int current, int total, double speed, void* user);    /* logger.h:21 */

w2x_engine* w2x_create(void);
void w2x_destroy(w2x_engine* e);
void w2x_set_message_callback(w2x_engine* e, w2x_message_fn fn, void* user);
void w2x_set_progress_callback(w2x_engine* e, w2x_progress_fn fn, void* user);
int w2x_build(w2x_engine* e, const char* onnx_path, const w2x_build_config* cfg);
int w2x_load(w2x_engine* e, const char* onnx_path, const w2x_render_config* cfg);
/* src/dst: interleaved 8-bit BGR, `step` bytes per row; dst must be rows*scaling x cols*scaling. */
int w2x_render(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, size_t dst_step);
/* The same on 16-bit samples (extension; the reference reads and writes 8-bit frames only, capture.cpp:96-99, and lists deeper images as a
 * TODO, README.md:88): interleaved BGR uint16, steps in BYTES; x = u16 * float(1/65535) into the network, sat(rint(x * 65535)) out. */
int w2x_render16(w2x_engine* e, const uint16_t* src, int rows, int cols, size_t src_step, uint16_t* dst, size_t dst_step);
/* Extension (Img2Img::renderResized): the frame w2x_render gives, resized on the device to dst_rows x dst_cols with an antialiased filter
 * (W2X_RESIZE_BICUBIC / _BILINEAR: torch.nn.functional.interpolate(antialias=True) on the fp32 canvas, then quantised).  Each target dimension must lie
 * in [input dim, input dim * scaling]; other sizes return 0 through the message callback.  At the scaled size the bytes are w2x_render's. */
int w2x_render_resized(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, int dst_rows, int dst_cols, size_t dst_step, int filter);
int w2x_render16_resized(w2x_engine* e, const uint16_t* src, int rows, int cols, size_t src_step, uint16_t* dst, int dst_rows, int dst_cols, size_t dst_step, int filter);
/* Multi-GPU split of ONE frame (no reference counterpart: main.cpp:70-74 is single-device): strip `part` of
 * `parts` = a contiguous range of the reference's column-major tile order (img2img_render.cpp:43-44) plus the output columns
 * it alone composes.  w2x_strip_plan is pure host logic: out[0..3] = first_tile, tile_count, x0, x1 (x in output pixels). */
int w2x_render_strip(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, size_t dst_step, int part, int parts);
/* ONE frame over `count` engines of this process with every tile computed once (no reference counterpart; SURVEY.md 8e, seam exchange):
 * engine k renders part k of w2x_shard_plan - a contiguous range of the reference's column-major tile order (img2img_render.cpp:43-44) -
 * the blend bands of the ny + 1 tiles in front of a range are copied device-to-device from the engine(s) that computed them, and each
 * engine composes and downloads the canvas cells of its own tiles.  Same bytes as w2x_render.  w2x_shard_plan is pure host logic:
 * out[0..3] = first_tile, tile_count, halo_first, nrect; out[4 + 4r ..] = x, y, w, h of rectangle r (r < 3) in output pixels. */
int w2x_render_sharded(w2x_engine* const* engines, int count, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, size_t dst_step);
int w2x_shard_plan(int in_w, int in_h, int out_w, int out_h, int tile_in, int tile_out, int scaling, double overlap_x, double overlap_y,
                   int part, int parts, int* out16);
/* The same split with ONE PROCESS PER GPU: rank r calls w2x_shard_compute (its own tiles into its slab, complete on return), exports w2x_shard_slab with
 * w2x_ipc_export (a 64-byte handle, hipIpcGetMemHandle) and hands it to its peers by whatever channel the caller has (bench.py: gloo all_gather - the
 * exchange is also the barrier); w2x_shard_finish takes the w2x_ipc_open'ed slabs of the parts in front of `part` (slabs[q] for q < part that own tiles;
 * other entries are ignored; devices[q] = the logical device the slab lives on, or NULL), copies the seam bands device to device, composes and writes this
 * part's canvas cells of dst (dst rows x cols = the OUTPUT size).  No collective on the data path. */
int w2x_shard_compute(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, int part, int parts);
const void* w2x_shard_slab(w2x_engine* e, size_t* bytes);
int w2x_shard_finish(w2x_engine* e, uint8_t* dst, int out_rows, int out_cols, size_t dst_step, int part, int parts, const void* const* slabs, const int* devices);
int w2x_ipc_export(const void* device_ptr, uint8_t* out64);
void* w2x_ipc_open(const uint8_t* handle64, int device);
void w2x_ipc_close(void* p);
/* Frame sequence with the PCIe copies overlapped (no reference counterpart: main.cpp:263-269 renders frame by frame): srcs/dsts are
 * arrays of `count` frame pointers of one size.  The copies run by DMA beside the kernels only for page-locked memory: take the
 * frame buffers from w2x_alloc_host (engine-owned, w2x_free_host or w2x_destroy releases them).  w2x_pin_host page-locks caller
 * memory in place and accepts whole pages only (data and bytes multiples of 4096). */
int w2x_render_sequence(w2x_engine* e, const uint8_t* const* srcs, int rows, int cols, size_t src_step, uint8_t* const* dsts, size_t dst_step, int count);
/* w2x_render_sequence with every frame resized like w2x_render_resized (one target size for the sequence, 8-bit frames) */
int w2x_render_sequence_resized(w2x_engine* e, const uint8_t* const* srcs, int rows, int cols, size_t src_step, uint8_t* const* dsts, int dst_rows, int dst_cols, size_t dst_step,
                                int count, int filter);
/* Extension (Img2Img::renderYuv): render on planar YUV 4:2:0 frames (ffmpeg yuv420p / yuv420p10le; an AVFrame's data[0..2] and linesize[0..2]).
 * planes[0..2] = Y, U (Cb), V (Cr); steps[0..2] in BYTES; Y is rows x cols, U and V (rows + 1) / 2 x (cols + 1) / 2.  bits 8 (uint8 samples) or 10
 * (little-endian uint16, low 10 bits), chosen independently for src and dst.  matrix W2X_YUV_BT601 / _BT709 / _BT2020 (non-constant luminance), range
 * W2X_YUV_LIMITED ("tv") / _FULL ("pc"), one pair for both directions; chroma sited MPEG-2 "left".  dst_rows x dst_cols must be the scaled size.
 * Invalid depths, matrices, ranges, missing planes, short steps and other sizes return 0 through the message callback. */
int w2x_render_yuv(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                   void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int matrix, int range);
/* w2x_render_sequence over YUV frames: src_planes / dst_planes hold 3 * count pointers (frame i at [3i .. 3i + 2]); one set of steps, one size and one
 * pair of depths for the sequence */
int w2x_render_sequence_yuv(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                            void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int count, int matrix, int range);
/* Extension (YuvImage::layout): w2x_render_yuv / w2x_render_sequence_yuv on frames of any W2X_YUV_I420 .. _NV12 layout, chosen independently for
 * src and dst like the depths (nv12 in, yuv444p10le out).  Plane arrays stay three pointers and three steps per frame.  I422: U and V are rows x (cols + 1) / 2;
 * I444: rows x cols; NV12: planes[1] holds (rows + 1) / 2 rows of 2 * ((cols + 1) / 2) samples U, V, U, V, ... and planes[2] / steps[2] are ignored (may be NULL /
 * 0); NV12 at 10 bits is P010: each uint16 of Y and UV carries its code in the HIGH 10 bits (read v >> 6, written code << 6; the planar layouts keep the low 10).
 * With both layouts W2X_YUV_I420 the bytes are w2x_render_yuv's.  Unknown layouts, a missing plane or a step shorter than the layout's row return 0 through
 * the message callback, with whatever w2x_render_yuv refuses.  (The resized calls below take I420 only; resized frames of the other layouts:
 * c_api_yuv_resized.h.) */
int w2x_render_yuv_layout(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits, int src_layout,
                          void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int dst_layout, int matrix, int range);
int w2x_render_sequence_yuv_layout(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits, int src_layout,
                                   void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int dst_layout, int count, int matrix, int range);
/* Extension (Img2Img::renderYuvResized): w2x_render_yuv with the canvas resized on the device to dst_rows x dst_cols before it is encoded (the filter and
 * the size rule of w2x_render_resized: each target dimension in [input dim, input dim * scaling], the two independent, odd sizes allowed; the resized RGB
 * is clamped and coded as w2x_render_yuv codes the canvas).  At the scaled size the bytes are w2x_render_yuv's.  What w2x_render_yuv refuses, other
 * sizes and unknown filters return 0 through the message callback. */
int w2x_render_yuv_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                           void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int matrix, int range, int filter);
/* w2x_render_sequence_yuv with every frame resized like w2x_render_yuv_resized (one target size for the sequence) */
int w2x_render_sequence_yuv_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                                    void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int count, int matrix, int range, int filter);
/* Extension (Img2Img::renderRgba): w2x_render on interleaved 8-bit BGRA frames (CV_8UC4; steps in bytes, >= cols * 4; dst rows*scaling x cols*scaling) in one
 * call: one upload, the colour bleed on the device (bleed = radius 0..16: the colours of the pixels with alpha > 0 spread that far under alpha == 0, see
 * w2x_alpha_bleed), colour and alpha tiles in one schedule, one download.  Colour bytes: w2x_render of w2x_alpha_bleed(BGR, A, bleed); alpha bytes: the green
 * channel of w2x_render of the gray image B = G = R = A.  skip_uniform_alpha != 0: a frame whose alpha plane is one value v runs no alpha tiles and gets
 * alpha v everywhere.  A bleed outside [0, 16], empty images and short steps return 0 through the message callback. */
int w2x_render_rgba(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, size_t dst_step, int bleed, int skip_uniform_alpha);
/* Extension (Img2Img::renderRgbaResized): w2x_render_rgba with the output resized on the device to dst_rows x dst_cols - the targets and filters of
 * w2x_render_resized (each dimension in [src dim, src dim * scaling]; filter 0 bicubic, 1 bilinear).  Colour bytes: w2x_render_resized of the bled colour frame;
 * alpha bytes: the green channel of w2x_render_resized of the gray image B = G = R = A.  At the scaled size it is w2x_render_rgba. */
int w2x_render_rgba_resized(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, int dst_rows, int dst_cols, size_t dst_step, int bleed,
                            int skip_uniform_alpha, int filter);
/* Extension (Img2Img::renderSequenceRgba): count BGRA frames of one size with one set of options, upload / compute / download overlapped as in
 * w2x_render_sequence (page-locked buffers: w2x_alloc_host); output i is the bytes of w2x_render_rgba on frame i. */
int w2x_render_sequence_rgba(w2x_engine* e, const uint8_t* const* srcs, int rows, int cols, size_t src_step, uint8_t* const* dsts, size_t dst_step, int count, int bleed,
                             int skip_uniform_alpha);
/* w2x_render_sequence_rgba with every frame resized like w2x_render_rgba_resized (one target size for the sequence) */
int w2x_render_sequence_rgba_resized(w2x_engine* e, const uint8_t* const* srcs, int rows, int cols, size_t src_step, uint8_t* const* dsts, int dst_rows, int dst_cols,
                                     size_t dst_step, int count, int bleed, int skip_uniform_alpha, int filter);
/* Test hook (Img2Img::alphaBleed): the device bleed alone - BGRA frame in, the BGR frame the tiles would be read from out (rows x cols, bgr_step >= cols * 3) */
int w2x_alpha_bleed_device(w2x_engine* e, const uint8_t* bgra, int rows, int cols, size_t bgra_step, uint8_t* bgr, size_t bgr_step, int radius);
void* w2x_alloc_host(w2x_engine* e, size_t bytes);
void w2x_free_host(w2x_engine* e, void* data);
int w2x_pin_host(w2x_engine* e, void* data, size_t bytes);
void w2x_unpin_host(w2x_engine* e, void* data);
int w2x_strip_plan(int in_w, int in_h, int out_w, int out_h, int tile_in, int tile_out, int scaling, double overlap_x, double overlap_y,
                   int part, int parts, int* out4);
int w2x_infer(w2x_engine* e, const float* input_nchw, float* output_nchw);
int w2x_output_tile_size(w2x_engine* e);
double w2x_plan_flops(w2x_engine* e);   /* algorithmic FLOP of one network pass */
int w2x_pass_tiles(w2x_engine* e);      /* tiles per network pass (batchSize x super-batch factor) */
float w2x_last_render_ms(w2x_engine* e);
float w2x_bench_resident(w2x_engine* e, int iters);
/* the output frame the last w2x_bench_resident step left in device memory -> dst (bytes = rows*s * cols*s * 3 samples) */
int w2x_resident_output(w2x_engine* e, void* dst, size_t bytes);
/* out[5*k+{0,1,2}] = {ms, launches, algorithmic FLOP} for k = 0 gemm, 1 attention, 2 se/scale, 3 gather, 4 compose, 5 fused mlp;
   out[30] = frame ms; cap >= 31 */
int w2x_profile_frame(w2x_engine* e, double* out, int cap);
/* ms per plan op (same order as w2x_describe_plan) of the last w2x_profile_frame; returns the op count */
int w2x_op_times(w2x_engine* e, double* out, int cap);

/* Host-only helpers (no GPU needed). */
/* rects: 4 ints (x,y,w,h) per tile, column-major tile order; returns tile count (or -1 if cap is too small). */
int w2x_calculate_tiles(int in_w, int in_h, int out_w, int out_h, int tile_in, int tile_out, int scaling,
                        double overlap_x, double overlap_y, int* in_rects, int* out_rects, int cap);
/* which: 0 top, 1 right, 2 bottom, 3 left (weights[] index, img2img_load.cpp:30-51); out: size*size floats. */
int w2x_tile_weights(int which, int overlap_x, int overlap_y, int size, float* out);
/* Tap tables of the resized renders along one axis, `in` -> `out` samples: first[i] = first input index of output i, weights[i * taps + k] its weights
 * (normalised, zero past the taps it has).  Returns taps per output; 0 for invalid arguments; with first / weights NULL only the count; -taps (nothing
 * written) when cap < out * taps. */
int w2x_resize_weights(int in, int out, int filter, int* first, float* weights, int cap);
/* The planes of a packed YUV 4:2:0 frame of rows x cols at `bits` (8 or 10): plane_rows[k], plane_cols[k] (samples) and plane_bytes[k] = rows * cols *
 * bytes per sample, k = Y, U, V.  Returns 1; 0 (nothing written) for an empty frame or other depths.  Any output pointer may be NULL. */
int w2x_yuv_plane_sizes(int rows, int cols, int bits, int* plane_rows, int* plane_cols, size_t* plane_bytes);
/* The same for a frame of `layout` (W2X_YUV_I420 .. _NV12): *nplanes = 3, or 2 for NV12 (Y, UV); plane_cols[k] counts the SAMPLES of a row (NV12's UV plane:
 * 2 * ((cols + 1) / 2)); the three-entry arrays get 0 in the entries past *nplanes.  Returns 1; 0 (nothing written) for an empty frame, other depths or an
 * unknown layout.  Any output pointer may be NULL. */
int w2x_yuv_layout_plane_sizes(int rows, int cols, int bits, int layout, int* nplanes, int* plane_rows, int* plane_cols, size_t* plane_bytes);
/* The colour bleed on the host (tiles.h alpha_bleed): bgr rows x cols interleaved 8-bit BGR, alpha rows x cols bytes, radius in [0, 16]; out (not aliasing bgr)
 * receives the frame with the colours of the pixels of alpha > 0 spread `radius` pixels outward under the pixels of alpha == 0: `radius` Jacobi iterations in
 * which an unknown pixel with n > 0 known neighbours among its eight takes (their sum + (n >> 1)) / n per channel and becomes known.  1 on success, 0 (nothing
 * written) for invalid arguments. */
int w2x_alpha_bleed(const uint8_t* bgr, size_t bgr_step, const uint8_t* alpha, size_t alpha_step, int rows, int cols, int radius, uint8_t* out, size_t out_step);
/* Lower an ONNX file at [batch,3,tile,tile] and write a textual description of the plan (ops, FLOPs) into buf. */
int w2x_describe_plan(const char* onnx_path, int batch, int tile, char* buf, size_t cap);
/* the same for any precision (W2X_PRECISION_FP16 / _TF32 / _FP32: the plan build() would write for that BuildConfig::precision; TF32 and FP32 share one) */
int w2x_describe_plan_precision(const char* onnx_path, int batch, int tile, int precision, char* buf, size_t cap);
/* Host-only halves of build() / load() for tools and tests: lower an ONNX file and write the plan (no .json side file, no
 * device); read a plan file back and run the consistency checks load() runs (img2img_load.cpp:149-154 "Failed to deserialize
 * engine"), writing "ok" or the reason into buf. */
int w2x_write_engine_file(const char* onnx_path, int batch, int tile, const char* out_path);
int w2x_validate_engine_file(const char* path, char* buf, size_t cap);
/* Dead-skip extents (csrc/liveness.h), host only: lower the ONNX file at [batch,3,tile,tile] (fp16) and report, for tile `tile_index` (column-major,
 * w2x_calculate_tiles order) of an in_w x in_h frame, the part of every plan op's row map that some kept output pixel of that tile depends on.  A launch that
 * computes several plan ops (the stem, the image head) takes its LAST op's entry.  tile_index < 0 (w2x_infer: tile outputs consumed whole) and tta != 0: "all".
 * Per op W2X_EXTENT_INTS ints: 0 op kind (0 gemm, 4 mlp, 5 window attention), 1-2 row map W, H, 3-6 cx, wx, cy, wy - the live columns are [0, cx) U [W - wx, W),
 * the live rows [0, cy) U [H - wy, H), all: cx = W, wx = 0, cy = H, wy = 0 - 7-9 attention roll rx, ry and window size (else -1, -1, 0), 10-12 the tensors the
 * op reads, writes and adds as a residual (-1: none), 13-15 convolution kh, kw, stride (else 1), 16-17 origin x0, y0 of the input view in its tensor, 18 the
 * pixel-shuffle factor r (the row map is the INPUT token map; else 1), 19-22 W, H of the read and the written tensor, 23-24 live and total units of the launch
 * (windows for attention, rows otherwise).  Returns the op count; -count when cap < count * W2X_EXTENT_INTS (nothing written); 0 on error. */
enum { W2X_EXTENT_INTS = 25 };
int w2x_dead_skip_extents(const char* onnx_path, int batch, int tile, int in_w, int in_h, int scaling, double overlap_x, double overlap_y, int tile_index, int tta,
                          int* out, int cap);
/* PCI bus id ("0000:c1:00.0") of HIP device `device` of this process (after W2X_DEVICE_MAP), for callers that place their host threads and
 * page-locked buffers on the GPU's NUMA node (/sys/bus/pci/devices/<id>/local_cpulist); 1 on success. */
int w2x_device_pci_bus_id(int device, char* buf, size_t cap);
/* sha256 hex digest (names engine files; utilities/sha256.h:39-94). out: 65 bytes. */
void w2x_sha256_hex(const void* data, size_t len, char* out);
const char* w2x_version(void);
/* Test hook, process-wide: the reference paths the A/B tests compare the shipped kernels and plans with - un-fused lowering ("no_fuse", "no_fuse_attn",
 * "no_se_fold"; read by build), separate launches ("no_fuse_head", "no_fuse_stem", "no_fuse_up"; read by load), the general kernel instead of a shape-specialised one
 * ("no_pixgemm", "no_conv3", "no_conv3h", "no_conv3h_walk", "no_conv48", "no_stem", "attn_valu"; read per launch), every tile slot's dead-skip extents "all"
 * ("no_dead_skip"; read per frame set-up, where the slot table of a render call is written - and by w2x_dead_skip_extents).  Which ops share a launch is fixed at load:
 * a switch set after load() changes the kernel of a launch of its own, never a folded launch (the stem, the transposed convolution, the image head).  They have no environment names.  The operational
 * switches (W2X_GROUPS, W2X_NO_GRAPH, ... - csrc/switches.h) can be set here too, by field name, but are re-read from the environment by
 * every build / load.  1 = set, 0 = no such switch. */
int w2x_debug_set(const char* name, int value);

#ifdef __cplusplus
}
#endif
#endif
