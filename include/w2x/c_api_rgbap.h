/* Planar RGBA frames through the flat C ABI (Img2Img::renderPlanarRgba and its three neighbours).  The entries live in this header of their own and
 * not in c_api.h: the recorded call log of the bindings (tests/golden/binding_calls.json) pins the set of names c_api.h declares; and their names say "rgbap",
 * since the headers c_api_planar.h and c_api_gray.h own every exported name that holds their word.  Everything else - the engine handle, the callbacks,
 * W2X_RESIZE_BICUBIC / _BILINEAR, w2x_alloc_host - is c_api.h's.
 *
 * A frame is four planes of rows x cols samples: planes[0] = R, planes[1] = G, planes[2] = B, planes[3] = A (a gbrap AVFrame: data[2], data[0], data[1],
 * data[3]), steps[k] the bytes per row of plane k.  bits: 8 (uint8_t), 10 / 12 / 16 (little-endian uint16_t, the code in the LOW bits), 32 (IEEE float,
 * nominal [0, 1]); u16 / float samples aligned to their size.  src_bits and dst_bits are independent.  Alpha is straight (not premultiplied) and every sample,
 * alpha included, is read and written as c_api_planar.h states; a pixel is visible iff its alpha sample read that way is > 0.
 * The contract, all of it equality:
 *   colour planes: w2x_render_planar / _resized of the planes w2x_alpha_bleed_rgbap gives for (R, G, B), A and `bleed`, at the same depths;
 *   alpha plane:   the G plane of w2x_render_planar / _resized of the frame (A, A, A) at the same depths;
 *   8 / 8 bits:    the planes interleaved as B, G, R, A are the bytes of w2x_render_rgba / w2x_render_rgba_resized with the same options.
 * bleed: 0 .. 16, and 0 for float samples (a float bleed is not built).  skip_uniform_alpha != 0 and every alpha sample one value v: no alpha tiles run, every
 * output alpha is sat(rint(v * (2^dst_bits - 1))) - float: v -, progress counts the colour tiles alone.
 * Every entry returns 1 on success and 0 after a refusal, which the message callback receives at severity error: a null engine (no message), an engine that
 * was never loaded, other depths, empty frames, missing planes, short steps, misaligned samples, a destination of another size, an unknown filter, a bleed
 * outside [0, 16] or on float samples. */
#ifndef W2X_C_API_RGBAP_H
#define W2X_C_API_RGBAP_H

#include "c_api.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Img2Img::renderPlanarRgba: dst is rows * scaling x cols * scaling.  Progress as w2x_render_rgba reports it. */
int w2x_render_rgbap(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                     void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int bleed, int skip_uniform_alpha);
/* Img2Img::renderPlanarRgbaResized: resized on the device to dst_rows x dst_cols, each in [src dim, src dim * scaling] (the targets and filters of
 * w2x_render_resized; filter 0 bicubic, 1 bilinear). */
int w2x_render_rgbap_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                             void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int bleed, int skip_uniform_alpha, int filter);
/* Img2Img::renderSequencePlanarRgba: count frames of one size, one pair of depths, one set of steps per side and one set of options; frame i's planes at
 * src_planes[4i .. 4i + 3] / dst_planes[4i .. 4i + 3]; upload / compute / download overlapped as w2x_render_sequence overlaps them (page-locked buffers:
 * w2x_alloc_host); output i is the bytes of w2x_render_rgbap on frame i.  count 0: 1, nothing done; negative counts and null arrays: 0. */
int w2x_render_sequence_rgbap(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                              void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int count, int bleed, int skip_uniform_alpha);
/* w2x_render_sequence_rgbap with every frame resized like w2x_render_rgbap_resized (one target size for the sequence) */
int w2x_render_sequence_rgbap_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                                      void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int count, int bleed,
                                      int skip_uniform_alpha, int filter);
/* host helper, no engine: the colour bleed on planes of integer codes (tiles.h alpha_bleed_planes).  planes / steps: the four planes R, G, B, A of bits 8, 10,
 * 12 or 16; out_planes / out_steps: three planes of the same samples, none aliasing an input.  Every code, alpha included, counts as min(code, 2^bits - 1).
 * 0 (nothing written) for invalid arguments. */
int w2x_alpha_bleed_rgbap(const void* const* planes, const size_t* steps, int rows, int cols, int bits, int radius, void* const* out_planes, const size_t* out_steps);
/* test hook (Img2Img::alphaBleedPlanes): the device bleed alone on the same arguments (float planes: radius 0, copied).  words: null, or two words that receive
 * max(key) and max(top - key) over the alpha plane, key the clamped code and top 2^bits - 1 (float: the bits of the clamped value, top 0x3F800000). */
int w2x_alpha_bleed_rgbap_device(w2x_engine* e, const void* const* planes, const size_t* steps, int rows, int cols, int bits, int radius,
                                 void* const* out_planes, const size_t* out_steps, unsigned* words);

#ifdef __cplusplus
}
#endif
#endif
