/* Resize in linear light through the flat C ABI (Img2Img::setResizeLight).  The entries live in this header of their own and not in c_api.h: the
 * recorded call log of the bindings (tests/golden/binding_calls.json) pins the set of names c_api.h declares.  The engine handle and the callbacks are c_api.h's.
 *
 * The rule.  Every resized frame (w2x_render_resized and its siblings of every frame format, the resized sequences) resizes the network's fp32 canvas to a
 * smaller raster by an antialiased filter, that is by averaging.  W2X_LIGHT_GAMMA, the default, averages the encoded values as they are.  The two other modes
 * average light.  A curve is four constants (t, k, a, g):
 *
 *     decode(e) = e / k    for e < t,        else ((e + a) / (1 + a))^g
 *     encode(l) = k l      for l < t / k,    else (1 + a) l^(1/g) - a
 *
 *     W2X_LIGHT_SRGB   (IEC 61966-2-1):                                                  t = 0.04045,      k = 12.92, a = 0.055,        g = 2.4
 *     W2X_LIGHT_BT709  (the Rec.709 / BT.2020 camera curve inverted, as zimg does):      t = 0.0812428583, k = 4.5,   a = 0.0992968268, g = 1 / 0.45
 *
 * Both curves have a linear toe, so the slope of encode is bounded (12.92 and 4.5).  A pure power (BT.1886) has an unbounded slope at black and is left out on
 * purpose; PQ and HLG are out of scope.  With a curve set, a resized frame is
 *
 *     1. L = decode(sat01(canvas value)), per colour sample, where the canvas is written;
 *     2. the existing resize of L: the same tap tables, tap order, tile and LDS layout;
 *     3. V = encode(sat01(L')) where the kernels otherwise clamp or quantise;
 *     4. everything behind that, on V, as it is: quantisation, dither threshold, BGR packing, the Y'CbCr matrix, the chroma-site filters, the NV12 interleave.
 *
 * Y'CbCr and its chroma subsampling stay on encoded values, as the standards define them.  Consequences:
 *   - alpha is coverage and is never decoded or encoded (BGRA's A, the planar A plane, the uniform-alpha shortcut): alpha bytes do not depend on the setting;
 *   - float destinations hold V;
 *   - decode(0) = 0, decode(1) = 1, encode(0) = 0 and encode(1) = 1 exactly: flat black and flat white stay exact;
 *   - at the scaled size a resized call is the plain call, with no round trip through the curves;
 *   - W2X_LIGHT_GAMMA gives the bytes of an engine that was never told about the setting.
 * The arithmetic is fp32 with every rounding stated: decode = e < t ? e * fl(1/k) : exp2(g * log2(fma(e - 1, fl(1/(1+a)), 1))), encode = l < fl(t/k) ? k * l :
 * fma(a, p - 1, p) with p = exp2(fl(1/g) * log2(l)); the constants are made in double and rounded once.  The device takes log2 / exp2 from the hardware.
 *
 * The setting belongs to the engine like the dither and the callbacks: allowed before w2x_load, kept until changed, read by every following frame call, single
 * calls and sequences alike. */
#ifndef W2X_C_API_RESIZE_LIGHT_H
#define W2X_C_API_RESIZE_LIGHT_H

#include "c_api.h"

#ifdef __cplusplus
extern "C" {
#endif

#define W2X_LIGHT_GAMMA 0
#define W2X_LIGHT_SRGB 1
#define W2X_LIGHT_BT709 2

/* Img2Img::setResizeLight.  1, or 0 for a null engine (no message) and for an unknown mode (message callback), which leaves the previous setting in place. */
int w2x_set_resize_light(w2x_engine* e, int mode);
/* Img2Img::resizeLight: the current mode, or -1 for a null engine. */
int w2x_get_resize_light(const w2x_engine* e);
/* The host statement of the two functions, for tests: v clamped to [0, 1], then decoded / encoded by the curve of `mode` in the fp32 arithmetic above
 * (W2X_LIGHT_GAMMA: the clamped value itself).  NaN for an unknown mode.  No engine needed. */
float w2x_light_decode(int mode, float v);
float w2x_light_encode(int mode, float v);
/* Test hook (Img2Img::resizePlanes): three planes of rows x cols float32 values (steps in bytes) are taken as the canvas of a resized frame and go the
 * production way - the device decode function the canvas kernels call (in a kernel of its own), the resize kernel of planar frames, its store - under the
 * engine's current light and dither settings, into three planes of dst_rows x dst_cols samples of `bits` (8: uint8; 10, 12, 16: uint16; 32: float).  The
 * target lies between a quarter of the source size and the source size per axis.  filter: W2X_RESIZE_BICUBIC or W2X_RESIZE_BILINEAR.  No network and no tiles
 * are involved; the engine must be loaded. */
int w2x_resize_planes(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols,
                      void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int bits, int filter);

#ifdef __cplusplus
}
#endif
#endif
