/* Gray frames through the flat C ABI (Img2Img::renderGray and its three neighbours).  The entries live in this header of their own and not in
 * c_api.h: the recorded call log of the bindings (tests/golden/binding_calls.json) pins the set of names c_api.h declares.  Everything else - the engine
 * handle, the callbacks, W2X_RESIZE_BICUBIC / _BILINEAR, w2x_alloc_host - is c_api.h's.
 *
 * A gray frame is ONE sample per pixel: rows x cols samples of 8 bits (uint8_t) or 16 bits (uint16_t), steps in bytes, src_step >= cols * bytes per sample.
 * The contract: for rep(g) the BGR frame with B = G = R = g,
 *   w2x_render_gray(g)            is the green channel of w2x_render(rep(g)),
 *   w2x_render_gray_resized(g)    is the green channel of w2x_render_resized(rep(g)) to the same target with the same filter,
 * byte for byte, at 8 and at 16 bits - the rule w2x_render_rgba states for its alpha plane.  One sample per pixel travels each way; nothing is replicated.
 * Every entry returns 1 on success and 0 after a refusal, which the message callback receives at severity error: a null engine (no message), an engine that
 * was never loaded, empty frames, short steps, a destination of another size, an unknown filter. */
#ifndef W2X_C_API_GRAY_H
#define W2X_C_API_GRAY_H

#include "c_api.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Img2Img::renderGray on 8-bit samples: dst is rows * scaling x cols * scaling samples, dst_step >= cols * scaling.  Progress as w2x_render reports it. */
int w2x_render_gray(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, size_t dst_step);
/* the same on 16-bit samples (u16 * float(1/65535) in, sat(rint(x * 65535)) out, as w2x_render16); steps stay in bytes */
int w2x_render_gray16(w2x_engine* e, const uint16_t* src, int rows, int cols, size_t src_step, uint16_t* dst, size_t dst_step);
/* Img2Img::renderGrayResized: w2x_render_gray resized on the device to dst_rows x dst_cols, each in [src dim, src dim * scaling] (the targets and filters of
 * w2x_render_resized; filter 0 bicubic, 1 bilinear).  At the scaled size it is w2x_render_gray. */
int w2x_render_gray_resized(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, int dst_rows, int dst_cols, size_t dst_step, int filter);
int w2x_render_gray16_resized(w2x_engine* e, const uint16_t* src, int rows, int cols, size_t src_step, uint16_t* dst, int dst_rows, int dst_cols, size_t dst_step, int filter);
/* Img2Img::renderSequenceGray: count 8-bit gray frames of one size and one pair of steps, upload / compute / download overlapped as in w2x_render_sequence
 * (page-locked buffers: w2x_alloc_host); output i is the bytes of w2x_render_gray on frame i.  count 0: 1, nothing done; negative counts and null arrays: 0. */
int w2x_render_sequence_gray(w2x_engine* e, const uint8_t* const* srcs, int rows, int cols, size_t src_step, uint8_t* const* dsts, size_t dst_step, int count);
/* w2x_render_sequence_gray with every frame resized like w2x_render_gray_resized (one target size for the sequence) */
int w2x_render_sequence_gray_resized(w2x_engine* e, const uint8_t* const* srcs, int rows, int cols, size_t src_step, uint8_t* const* dsts, int dst_rows, int dst_cols,
                                     size_t dst_step, int count, int filter);

#ifdef __cplusplus
}
#endif
#endif
