/* YUV frames with a chroma siting per side through the flat C ABI (YuvImage::siting).  The two entries live in this header of their own and not in
 * c_api.h for the reason c_api_yuv_resized.h gives: the recorded call log of the bindings (tests/golden/binding_calls.json) pins the set of names c_api.h
 * declares.  Everything else - the engine handle, the callbacks, W2X_YUV_I420 .. _NV12, W2X_YUV_BT601 .., W2X_RESIZE_BICUBIC / _BILINEAR, w2x_alloc_host,
 * w2x_yuv_layout_plane_sizes - is c_api.h's.
 *
 * A siting says where the chroma samples of a 4:2:0 / 4:2:2 frame sit on the luma grid; per subsampled axis it is one of two rules, co-sited (the sample lies
 * on an even luma sample) or centred (between two):
 *   W2X_YUV_SITING_LEFT     columns co-sited, rows centred   MPEG-2, H.264 default (AVCHROMA_LOC_LEFT); what every other entry of the ABI assumes
 *   W2X_YUV_SITING_CENTER   columns centred, rows centred    JPEG, MJPEG, MPEG-1 (AVCHROMA_LOC_CENTER)
 *   W2X_YUV_SITING_TOPLEFT  columns co-sited, rows co-sited  BT.2020 / UHD / HDR10 (AVCHROMA_LOC_TOPLEFT)
 * Source and destination sitings are independent, like layouts and depths (centre-sited MJPEG in, left-sited H.264 out is one call).  I422 and NV12 / I420
 * follow the table; I422 has the column rule only, so TOPLEFT gives LEFT's bytes there; I444 has no subsampled axis and gives the same bytes for all three.
 *
 * The frames, the target and the filter are those of w2x_render_yuv_layout_resized (c_api_yuv_resized.h); at dst = rows * scaling x cols * scaling the call is
 * the plain render (w2x_render_yuv_layout with the sitings), as the resized contract says.  With both sitings W2X_YUV_SITING_LEFT the bytes are
 * w2x_render_yuv_layout_resized's.  The Y plane does not depend on any siting of the destination.
 * Both return 1 on success and 0 after a refusal, which the message callback receives at severity error: what w2x_render_yuv_layout_resized refuses, and an
 * unknown siting on either side (refused by the engine in its own words, "[renderYuvResized@line] Unknown YUV chroma siting N.": on an engine that was never loaded
 * the refusal is that of the missing load). */
#ifndef W2X_C_API_YUV_SITING_H
#define W2X_C_API_YUV_SITING_H

#include "c_api.h"

#ifdef __cplusplus
extern "C" {
#endif

#define W2X_YUV_SITING_LEFT 0
#define W2X_YUV_SITING_CENTER 1
#define W2X_YUV_SITING_TOPLEFT 2

/* Img2Img::renderYuvResized on YuvImages with a siting: w2x_render_yuv_layout_resized's arguments, src_siting behind src_layout, dst_siting behind dst_layout */
int w2x_render_yuv_sited(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits, int src_layout, int src_siting,
                         void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int dst_layout, int dst_siting, int matrix, int range,
                         int filter);
/* Img2Img::renderSequenceYuvResized likewise: w2x_render_sequence_yuv_layout_resized's arguments and the two sitings, which hold for every frame of the
 * sequence.  count 0: nothing is rendered; negative counts and null arrays: 0. */
int w2x_render_sequence_yuv_sited(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits, int src_layout, int src_siting,
                                  void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int dst_layout, int dst_siting, int count,
                                  int matrix, int range, int filter);

#ifdef __cplusplus
}
#endif
#endif
