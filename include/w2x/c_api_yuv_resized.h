/* Resized YUV frames of any layout through the flat C ABI (Img2Img::renderYuvResized / renderSequenceYuvResized on YuvImages whose layout is not I420,
 * DESIGN 9j).  The two entries live in this header of their own and not in c_api.h: the recorded call log of the bindings (tests/golden/binding_calls.json)
 * pins the set of names c_api.h declares.  Everything else - the engine handle, the callbacks, W2X_YUV_I420 .. _NV12, W2X_YUV_BT601 .., W2X_RESIZE_BICUBIC /
 * _BILINEAR, w2x_alloc_host, w2x_yuv_layout_plane_sizes - is c_api.h's.
 *
 * The frames are those of w2x_render_yuv_layout: three pointers and three steps (bytes) per frame, the planes of src_layout / dst_layout (NV12: planes[1] holds
 * U, V, U, V, ...; planes[2] / steps[2] are ignored and may be NULL / 0; NV12 at 10 bits is P010, the code in the HIGH 10 bits), bits 8 or 10 per side.  Layout
 * and depth of source and destination are independent.  The target dst_rows x dst_cols follows w2x_render_yuv_resized: each dimension in [input dim, input dim
 * * scaling], the two independent, odd sizes allowed; filter W2X_RESIZE_BICUBIC / _BILINEAR.  The fp32 canvas is resized unclamped, the resized R, G, B are
 * clamped to [0, 1] and coded as w2x_render_yuv_layout codes the canvas: I420 / NV12 chroma of the colour filtered (1/4, 1/2, 1/4) x (1/2, 1/2) onto each site,
 * I422 (1/4, 1/2, 1/4) along the row, I444 each pixel's own.
 * The contract, all of it equality: with both layouts W2X_YUV_I420 the bytes are w2x_render_yuv_resized's; at the scaled size they are
 * w2x_render_yuv_layout's; the Y plane does not depend on dst_layout; an NV12 destination holds the I420 destination's samples (P010: << 6); an NV12 source
 * gives what its samples give as I420.
 * Both return 1 on success and 0 after a refusal, which the message callback receives at severity error: a null engine (no message), an engine that was never
 * loaded, an unknown filter, layout, matrix or range, other depths, an empty frame, a missing plane, a step shorter than the layout's row, a target outside the
 * range above. */
#ifndef W2X_C_API_YUV_RESIZED_H
#define W2X_C_API_YUV_RESIZED_H

#include "c_api.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Img2Img::renderYuvResized: w2x_render_yuv_layout's arguments and the filter */
int w2x_render_yuv_layout_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits, int src_layout,
                                  void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int dst_layout, int matrix, int range,
                                  int filter);
/* Img2Img::renderSequenceYuvResized: w2x_render_sequence_yuv_layout's arguments and the filter - count frames of one size, one pair of depths, one pair of
 * layouts, one set of steps per side and one target; frame i's planes at src_planes[3i .. 3i + 2] / dst_planes[3i .. 3i + 2]; output i is the bytes of
 * w2x_render_yuv_layout_resized on frame i.  count 0: nothing is rendered; negative counts and null arrays: 0. */
int w2x_render_sequence_yuv_layout_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits, int src_layout,
                                           void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int dst_layout, int count,
                                           int matrix, int range, int filter);

#ifdef __cplusplus
}
#endif
#endif
