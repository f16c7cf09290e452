/* Dithered output through the flat C ABI (Img2Img::setDither).  The entries live in this header of their own and not in c_api.h: the recorded call
 * log of the bindings (tests/golden/binding_calls.json) pins the set of names c_api.h declares.  The engine handle and the callbacks are c_api.h's.
 *
 * The rule.  Without dither every integer sample the engine writes is sat(rint(V)) of an fp32 value V.  With it, the destination sample of an integer depth
 * (8, 10, 12 or 16 bits) in plane c at position (x, y) of that plane is
 *
 *     code = min(max(floor_to_int(fl32(V + t)), 0), maxcode),      t = (rank + 0.5) / N
 *
 * V is exactly the value the undithered kernel rounds; V + t is one rounded fp32 addition, never fused into the product that made V; t is exact in fp32.
 *   W2X_DITHER_ORDERED:   N = 64,   rank = B8[(y + dy) & 7][(x + dx) & 7], the recursive 8 x 8 Bayer matrix (first rows 0 32 8 40 2 34 10 42 / 48 16 56 24 50 18
 *                         58 26): with u = (x + dx) & 7, v = (y + dy) & 7 and q_b = ((u_b ^ v_b) << 1) | v_b for the bits b = 0, 1, 2, rank = q_0 << 4 | q_1 << 2 | q_2.
 *   W2X_DITHER_BLUENOISE: N = 4096, rank = T[(y + dy) & 63][(x + dx) & 63], T a 64 x 64 void-and-cluster table holding every rank 0 .. 4095 once
 *                         (w2x_dither_table).
 *   dx = 17 c + 23 phase, dy = 29 c + 41 phase: the planes are decorrelated and a caller moves the pattern per frame.
 * Plane index c: R, G, B = 0, 1, 2 whatever the memory order; a gray frame is plane 1, so that w2x_render_gray(g) stays the green channel of
 * w2x_render(rep(g)); Y, U, V = 0, 1, 2, a chroma sample with the coordinates of its own plane, NV12 / P010 chroma with those of the I420 samples they are.
 * (x, y) are absolute positions in the destination frame, never relative to a strip, a shard or a workgroup.  Alpha is never dithered (BGRA's A, the planar A
 * plane, the uniform-alpha shortcut): it keeps rint.  Float destinations are untouched.  Consequences: W2X_DITHER_NONE gives the bytes of an engine that was
 * never told about dither; and where V is an integer the code is that integer, so flat exact areas are unchanged - as long as fl32(V + t) stays below V + 1 for
 * the largest t, 1 - 1 / (2N): always for ORDERED; for BLUENOISE below code 2048 (from there on fp32 keeps fewer than 13 fraction bits and the few top
 * thresholds round up to V + 1: 1 position in 4096 at code 2048, 8 in 4096 at code 65535).
 *
 * The setting belongs to the engine like the callbacks: allowed before w2x_load, kept until changed, read by every following frame call.  Frame i of a
 * sequence entry is dithered as the single call with phase + i * advance would be (advance 0: a still pattern; 1: temporal dither).  w2x_render_strip and
 * w2x_render_sharded keep their byte equality with w2x_render. */
#ifndef W2X_C_API_DITHER_H
#define W2X_C_API_DITHER_H

#include "c_api.h"

#ifdef __cplusplus
extern "C" {
#endif

#define W2X_DITHER_NONE 0
#define W2X_DITHER_ORDERED 1
#define W2X_DITHER_BLUENOISE 2

/* Img2Img::setDither.  1, or 0 for a null engine (no message) and for an unknown mode (message callback), which leaves the previous setting in place. */
int w2x_set_dither(w2x_engine* e, int mode, unsigned phase, unsigned advance);
/* Img2Img::dither: the current setting into whichever of the three pointers are not null.  0 for a null engine. */
int w2x_get_dither(const w2x_engine* e, int* mode, unsigned* phase, unsigned* advance);
/* The rank table of a mode, row-major: W2X_DITHER_ORDERED the 8 x 8 Bayer matrix (*side = 8, 64 values), W2X_DITHER_BLUENOISE the 64 x 64 table (*side = 64,
 * 4096 values).  out may be null to ask for the side alone; else it holds side * side values.  0 for W2X_DITHER_NONE and unknown modes.  No engine needed. */
int w2x_dither_table(int mode, uint16_t* out, int* side);
/* The rank of sample (x, y) of plane c at `phase` as the device computes it (dither.h dither_rank), or -1: mode none or unknown, c outside 0 .. 2, x or y < 0. */
int w2x_dither_rank(int mode, unsigned phase, int c, int x, int y);
/* Test hook (Img2Img::ditherPlanes): three planes of rows x cols float32 values v (steps in bytes) quantised on the device from V = v * (2^bits - 1) by the
 * store of the compose and resample kernels, with the engine's current setting (none: sat(rint(V))), into three planes of `bits` (8: uint8; 10, 12, 16:
 * uint16, code in the low bits).  Plane k has plane index k.  No network and no tiles are involved; the engine must be loaded. */
int w2x_dither_planes(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, void* const* dst_planes, const size_t* dst_steps, int bits);

#ifdef __cplusplus
}
#endif
#endif
