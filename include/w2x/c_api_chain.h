/* Chained renders through the flat C ABI (Img2Img::renderChained and its neighbours): ONE frame through 2 to 4 engines one after the other - x4 from
 * two x2 models, x8, x16 - with the frame staying on the device between them.  The entries live in this header of their own and not in c_api.h: the recorded
 * call log of the bindings (tests/golden/binding_calls.json) pins the set of names c_api.h declares.  Everything else - the engine handle, the callbacks,
 * W2X_RESIZE_BICUBIC / _BILINEAR, w2x_alloc_host - is c_api.h's; a planar frame travels as in c_api_planar.h (three planes R, G, B, their steps, bits 8, 10, 12,
 * 16 or 32).  The planar entries say "planes": c_api_planar.h owns every exported name that holds the word "planar".
 *
 * engines[0 .. count): loaded engines of this process on one device; the same handle may appear more than once.  The total factor S is the product of their
 * scale factors.  engines[0] owns the message and progress callbacks of the call.  quantize 0: the frame between two stages is the canvas clamped to [0, 1],
 * unrounded, in the tile type of the consuming engine - the bytes of w2x_render_planar(dst_bits 32) followed by w2x_render_planar(src_bits 32); quantize 1: it is
 * rounded to the source's depth - the bytes of calling the single entries one after the other.  The last engine's dither and resize-light settings apply, to the
 * last stage only.  Every entry returns 1 on success and 0 after a refusal, which engines[0]'s message callback receives at severity error: a count outside
 * 2 .. 4, a null engine or a null array (no message), an engine that was never loaded, engines on differing devices, a destination of another size, quantize on
 * float planes, an unknown filter, whatever the single entries refuse of the source and the destination. */
#ifndef W2X_C_API_CHAIN_H
#define W2X_C_API_CHAIN_H

#include "c_api.h"

#ifdef __cplusplus
extern "C" {
#endif

/* refusal codes of w2x_chain_plan */
#define W2X_CHAIN_OK 0
#define W2X_CHAIN_COUNT 1      /* count outside 2 .. 4, or a null array */
#define W2X_CHAIN_SCALING 2    /* a scale factor outside 1 .. 4 */
#define W2X_CHAIN_SOURCE 3     /* an empty source */
#define W2X_CHAIN_TOO_LARGE 4  /* a frame of the chain beyond 65536 samples per side */
#define W2X_CHAIN_TARGET 5     /* a target dimension outside [source dim, source dim * S] */
#define W2X_CHAIN_SHRINK 6     /* a target dimension below a quarter of the last stage's canvas */

/* Host only; the one place the size rules live.  A rows x cols frame through stages of scalings[0 .. count): out[2k], out[2k + 1] = rows, cols of the frame stage
 * k reads (k = 0: the source), out[2 count], out[2 count + 1] = the last stage's canvas, then the target's rows and cols, then S: 2 count + 5 ints.  dst_rows =
 * dst_cols = 0 asks for the canvas itself.  Returns W2X_CHAIN_OK or the refusal; out is written on W2X_CHAIN_OK only. */
int w2x_chain_plan(int rows, int cols, const int* scalings, int count, int dst_rows, int dst_cols, int* out);

/* Img2Img::renderChained: interleaved BGR frames of `depth` 8 or 16 (uint16 samples; steps in bytes) on both sides; dst is rows * S x cols * S.  Progress:
 * engines[0]'s callback, total = the sum over the stages of their batches. */
int w2x_render_chained(w2x_engine* const* engines, int count, const void* src, int rows, int cols, size_t src_step, void* dst, size_t dst_step, int depth, int quantize);
/* Img2Img::renderChainedResized: the last stage's canvas resized on the device to dst_rows x dst_cols (filter 0 bicubic, 1 bilinear) */
int w2x_render_chained_resized(w2x_engine* const* engines, int count, const void* src, int rows, int cols, size_t src_step, void* dst, int dst_rows, int dst_cols,
                               size_t dst_step, int depth, int quantize, int filter);
/* Img2Img::renderSequenceChained: `frames` 8-bit frames of one size and one pair of steps, upload / stages / download overlapped (page-locked buffers:
 * w2x_alloc_host on any engine); output i is the bytes of w2x_render_chained on frame i.  frames 0: 1, nothing done. */
int w2x_render_sequence_chained(w2x_engine* const* engines, int count, const void* const* srcs, int rows, int cols, size_t src_step, void* const* dsts, size_t dst_step,
                                int frames, int quantize);
int w2x_render_sequence_chained_resized(w2x_engine* const* engines, int count, const void* const* srcs, int rows, int cols, size_t src_step, void* const* dsts,
                                        int dst_rows, int dst_cols, size_t dst_step, int frames, int quantize, int filter);
/* Img2Img::renderChainedPlanar / renderChainedPlanarResized: src_bits and dst_bits independent; dst_rows x dst_cols is rows * S x cols * S for the plain entry */
int w2x_render_chained_planes(w2x_engine* const* engines, int count, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                              void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int quantize);
int w2x_render_chained_planes_resized(w2x_engine* const* engines, int count, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                                      void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int quantize, int filter);

#ifdef __cplusplus
}
#endif
#endif
