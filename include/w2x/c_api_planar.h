/* Planar RGB frames through the flat C ABI (Img2Img::renderPlanar and its three neighbours).  The entries live in this header of their own and not
 * in c_api.h: the recorded call log of the bindings (tests/golden/binding_calls.json) pins the set of names c_api.h declares.  Everything else - the engine
 * handle, the callbacks, W2X_RESIZE_BICUBIC / _BILINEAR, w2x_alloc_host - is c_api.h's.
 *
 * A planar frame is three planes of rows x cols samples: planes[0] = R, planes[1] = G, planes[2] = B (a gbrp AVFrame: data[2], data[0], data[1]; the order
 * carries no meaning of its own), steps[k] the bytes per row of plane k.  bits: 8 (uint8_t), 10 / 12 / 16 (little-endian uint16_t, the code in the LOW bits),
 * 32 (IEEE float, nominal [0, 1]); u16 / float samples aligned to their size.  src_bits and dst_bits are independent.
 *   in, integer:  min(code, 2^bits - 1) * float(1 / (2^bits - 1))     (8 / 16 bits: w2x_render / w2x_render16's own constants)
 *   in, float:    min(max(x, 0), 1), NaN -> 0
 *   out, integer: sat(rint(x * (2^bits - 1)))                          out, float: min(max(x, 0), 1), never rounded to a code
 * The contract: at 8 / 8 bits w2x_render_planar gives the planes of w2x_render of the interleaved frame, byte for byte, at 16 / 16 bits those of w2x_render16;
 * w2x_render_planar_resized stands to w2x_render_resized / w2x_render16_resized the same way; at the scaled size the resized call is the plain one.
 * Every entry returns 1 on success and 0 after a refusal, which the message callback receives at severity error: a null engine (no message), an engine that
 * was never loaded, other depths, empty frames, missing planes, short steps, misaligned samples, a destination of another size, an unknown filter. */
#ifndef W2X_C_API_PLANAR_H
#define W2X_C_API_PLANAR_H

#include "c_api.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Img2Img::renderPlanar: dst is rows * scaling x cols * scaling.  Progress as w2x_render reports it. */
int w2x_render_planar(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                      void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits);
/* Img2Img::renderPlanarResized: resized on the device to dst_rows x dst_cols, each in [src dim, src dim * scaling] (the targets and filters of
 * w2x_render_resized; filter 0 bicubic, 1 bilinear). */
int w2x_render_planar_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                              void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int filter);
/* Img2Img::renderSequencePlanar: count frames of one size, one pair of depths and one set of steps per side; frame i's planes at src_planes[3i .. 3i + 2] /
 * dst_planes[3i .. 3i + 2]; upload / compute / download overlapped as w2x_render_sequence overlaps them (page-locked buffers: w2x_alloc_host); output i is the bytes of
 * w2x_render_planar on frame i.  count 0: 1, nothing done; negative counts and null arrays: 0. */
int w2x_render_sequence_planar(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                               void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int count);
/* w2x_render_sequence_planar with every frame resized like w2x_render_planar_resized (one target size for the sequence) */
int w2x_render_sequence_planar_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                                       void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int count, int filter);
/* host helper: the bytes of one packed plane of rows x cols samples of `bits`; 0 for an empty plane or a depth the entries refuse */
size_t w2x_planar_plane_bytes(int rows, int cols, int bits);

#ifdef __cplusplus
}
#endif
#endif
