// Dithered output, host side: the modes, the threshold of a destination sample, the blue-noise table and the parsing of the option.  No HIP: it builds
// with plain g++ (make asan) and is what the tests state the device code against.
//
// The rule.  A destination sample of an integer depth in plane c at position (x, y) of that plane is
//     code = min(max(floor_to_int(fl32(V + t)), 0), maxcode),   t = (rank + 0.5) / N,
// V the fp32 value the kernel would otherwise round to nearest, V + t one rounded fp32 addition.  t is exact in fp32.
//     Ordered:   N = 64,   rank = B8[(y + dy) & 7][(x + dx) & 7], the recursive 8 x 8 Bayer matrix: with u = (x + dx) & 7, v = (y + dy) & 7 and
//                q_b = ((u_b ^ v_b) << 1) | v_b for the bits b = 0, 1, 2, rank = q_0 << 4 | q_1 << 2 | q_2.
//     BlueNoise: N = 4096, rank = T[(y + dy) & 63][(x + dx) & 63], T the 64 x 64 void-and-cluster table of dither_table.h (tools/blue_noise.py).
//     dx = 17 c + 23 phase, dy = 29 c + 41 phase: the planes are decorrelated, and a caller moves the pattern per frame with the phase.
// Plane index c: R, G, B = 0, 1, 2 whatever the memory order; a gray frame is plane 1; Y, U, V = 0, 1, 2.  (x, y) are absolute positions in the destination
// plane.  Alpha is never dithered and float destinations are not touched.  Where V is an integer the code is V: t < 1.
#pragma once
#include <cstdint>

namespace w2x {

constexpr int kDitherNone = 0, kDitherOrdered = 1, kDitherBlueNoise = 2;
constexpr int kDitherSide = 64;                                   // the blue-noise table's side; the Bayer matrix's 8 divides it

inline bool dither_mode_ok(int mode) { return mode >= kDitherNone && mode <= kDitherBlueNoise; }
// N of a mode: 64, 4096; 0: nothing is added
inline unsigned dither_levels(int mode) { return mode == kDitherOrdered ? 64u : mode == kDitherBlueNoise ? 4096u : 0u; }
// the pattern's offset for plane c at `phase`, reduced mod 64 (unsigned arithmetic: 64 divides 2^32, so a wrapped phase gives the offset of the exact sum)
inline unsigned dither_dx(unsigned phase, int c) { return (17u * (unsigned)c + 23u * phase) & (kDitherSide - 1); }
inline unsigned dither_dy(unsigned phase, int c) { return (29u * (unsigned)c + 41u * phase) & (kDitherSide - 1); }
inline unsigned bayer8_rank(unsigned u, unsigned v) {
    unsigned r = 0;
    for (int b = 0; b < 3; ++b) {
        const unsigned ub = (u >> b) & 1u, vb = (v >> b) & 1u;
        r |= (((ub ^ vb) << 1) | vb) << (4 - 2 * b);
    }
    return r;
}
// the 64 x 64 ranks, row-major
const uint16_t* dither_table();
// rank of sample (x, y) of plane c (x, y >= 0; c in 0 .. 2); -1: mode None or unknown, c outside
int dither_rank(int mode, unsigned phase, int c, int x, int y);
// (rank + 0.5) / N as the float the device adds; 0 where dither_rank gives -1
float dither_threshold(int mode, unsigned phase, int c, int x, int y);
// "none" | "ordered" | "bluenoise" <-> the mode; parse: false for anything else (mode untouched); name: nullptr for an unknown mode
bool dither_parse_mode(const char* name, int& mode);
const char* dither_mode_name(int mode);

}  // namespace w2x
