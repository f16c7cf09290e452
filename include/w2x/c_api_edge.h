/* Edge modes through the flat C ABI (Img2Img::setEdge).  The entries live in this header of their own and not in c_api.h: the recorded call log of
 * the bindings (tests/golden/binding_calls.json) pins the set of names c_api.h declares.  The engine handle and the callbacks are c_api.h's.
 *
 * The rule.  A tile that reaches over the frame edge, the colour bleed of an RGBA frame and the taps of a resize all read samples that do not exist.  The mode
 * says which sample stands in: the source index of coordinate i in a dimension of n samples, for ANY integer i (a tile border may be several times a small frame):
 *
 *     W2X_EDGE_REPLICATE   min(max(i, 0), n - 1)      the default: the reference's BORDER_REPLICATE, and the bytes of an engine never told about the setting
 *     W2X_EDGE_WRAP        ((i % n) + n) % n          the frame is one period of a texture that tiles ("seamless")
 *     W2X_EDGE_MIRROR      reflection that does not repeat the edge sample (numpy's "reflect": -1 -> 1, n -> n - 2), period 2 (n - 1); n == 1 gives 0
 *
 * Where it acts, for every frame format of the RGB family (BGR, gray, planar, BGRA, planar RGBA; single calls, resized calls, sequences, chains):
 *   - tiles:  the gather's source index;
 *   - bleed:  under WRAP a pixel's eight neighbours are taken through the rule, so all eight exist and colour spreads across the joint; MIRROR keeps REPLICATE's
 *             rule, in which a neighbour outside the frame does not exist (a reflected neighbour carries no new information);
 *   - resize: under WRAP and MIRROR the taps are not cut off and renormalised at the border: every output sample has its full support, read through the rule.
 * Dither and linear light are per sample and do not know about it.  A chained render's stage gathers under its own engine's mode; the last engine's mode governs
 * the resize.  Not built under WRAP / MIRROR, and refused by name through the message callback with nothing written: every YUV call, strips and shards.
 *
 * The setting belongs to the engine like the dither and the callbacks: allowed before w2x_load, kept until changed, read by every following frame call. */
#ifndef W2X_C_API_EDGE_H
#define W2X_C_API_EDGE_H

#include "c_api.h"

#ifdef __cplusplus
extern "C" {
#endif

#define W2X_EDGE_REPLICATE 0
#define W2X_EDGE_WRAP 1
#define W2X_EDGE_MIRROR 2

/* Img2Img::setEdge.  1, or 0 for a null engine (no message) and for an unknown mode (message callback), which leaves the previous setting in place. */
int w2x_set_edge(w2x_engine* e, int mode);
/* Img2Img::edge: the current mode, or -1 for a null engine. */
int w2x_get_edge(const w2x_engine* e);
/* The rule itself, host only: the source index of coordinate i in a dimension of n samples under `mode`.  -1 for an unknown mode or n <= 0.  No engine needed. */
int w2x_edge_index(int mode, long long i, int n);
/* w2x_resize_weights under a mode.  REPLICATE: that table, to the bit.  WRAP / MIRROR: every output sample has its full support - first[i] may be negative and
 * first[i] + k may pass `in`; tap k reads the sample w2x_edge_index(mode, first[i] + k, in) - and the weights are normalised over all taps.  Returns like
 * w2x_resize_weights: the taps per output sample (first / weights null: a query), minus that for a cap below out * taps, 0 for invalid arguments, an unknown
 * mode included. */
int w2x_resize_weights_edge(int in, int out, int filter, int mode, int* first, float* weights, int cap);
/* w2x_alpha_bleed under a mode (host).  WRAP: the eight neighbours through the rule.  REPLICATE and MIRROR: w2x_alpha_bleed.  0 for invalid arguments, an
 * unknown mode included; nothing is written then. */
int w2x_alpha_bleed_edge(const uint8_t* bgr, size_t bgr_step, const uint8_t* alpha, size_t alpha_step, int rows, int cols, int radius, uint8_t* out, size_t out_step,
                         int mode);
/* The same on four planes R, G, B, A of 8, 10, 12 or 16 bits (the arguments of the host bleed of frames of planes, steps in bytes): three colour planes out. */
int w2x_alpha_bleed_planes_edge(const void* const* planes, const size_t* steps, int rows, int cols, int bits, int radius, void* const* out_planes, const size_t* out_steps,
                                int mode);

#ifdef __cplusplus
}
#endif
#endif
