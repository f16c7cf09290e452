// Dithered output, host side (dither.h).
#include "dither.h"

#include <cstring>

namespace w2x {

namespace {
const uint16_t kBlueNoiseRanks[kDitherSide * kDitherSide] = {
#include "dither_table.h"
};
}  // namespace

const uint16_t* dither_table() { return kBlueNoiseRanks; }

int dither_rank(int mode, unsigned phase, int c, int x, int y) {
    if (c < 0 || c > 2 || x < 0 || y < 0) return -1;
    const unsigned u = (unsigned)x + dither_dx(phase, c), v = (unsigned)y + dither_dy(phase, c);
    if (mode == kDitherOrdered) return (int)bayer8_rank(u & 7u, v & 7u);
    if (mode == kDitherBlueNoise) return (int)kBlueNoiseRanks[(v & (kDitherSide - 1)) * kDitherSide + (u & (kDitherSide - 1))];
    return -1;
}

float dither_threshold(int mode, unsigned phase, int c, int x, int y) {
    const int r = dither_rank(mode, phase, c, x, y);
    if (r < 0) return 0.f;
    return ((float)r + 0.5f) / (float)dither_levels(mode);        // exact: rank + 0.5 has at most 13 bits, N is a power of two
}

bool dither_parse_mode(const char* name, int& mode) {
    if (!name) return false;
    for (int m = kDitherNone; m <= kDitherBlueNoise; ++m)
        if (std::strcmp(name, dither_mode_name(m)) == 0) { mode = m; return true; }
    return false;
}

const char* dither_mode_name(int mode) {
    switch (mode) {
        case kDitherNone: return "none";
        case kDitherOrdered: return "ordered";
        case kDitherBlueNoise: return "bluenoise";
        default: return nullptr;
    }
}

}  // namespace w2x
