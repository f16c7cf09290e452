// Edge modes (Img2Img::setEdge), host side: the modes and the one rule.  No HIP: it builds with plain g++ (make asan) and is what the tests state the
// device code against (prepost_device.h edge_src / edge_index_dev are the same statements).
//
// The rule.  The source index of frame coordinate i in a dimension of n samples, for ANY integer i (a tile border may be several times a small frame):
//     Replicate: min(max(i, 0), n - 1)                      - the default, the reference's BORDER_REPLICATE and what the engine always did;
//     Wrap:      ((i % n) + n) % n                          - the frame is one period of a texture that tiles;
//     Mirror:    reflection that does not repeat the edge sample (numpy's "reflect": -1 -> 1, n -> n - 2), period 2 (n - 1), applied as often as needed; n == 1: 0.
// Who reads it: the gather of every RGB-family frame (the two clamp lines), the eight neighbours of the colour bleed under Wrap, and the taps of the resize,
// which under Wrap and Mirror are no longer cut off and renormalised at the border.
#pragma once
#include <cstring>

namespace w2x {

constexpr int kEdgeReplicate = 0, kEdgeWrap = 1, kEdgeMirror = 2;
inline bool edge_mode_ok(int mode) { return mode >= kEdgeReplicate && mode <= kEdgeMirror; }

// n >= 1; an unknown mode is read as Replicate (the callers check the mode first)
inline int edge_index(int mode, long long i, int n) {
    if (n <= 1) return 0;
    if (mode == kEdgeWrap) { const long long r = i % n; return (int)(r < 0 ? r + n : r); }
    if (mode == kEdgeMirror) {
        const long long p = 2LL * (n - 1);
        long long r = i % p;
        if (r < 0) r += p;
        return (int)(r < n ? r : p - r);
    }
    return (int)(i < 0 ? 0 : i > n - 1 ? n - 1 : i);
}

// What an edged resize launch gets beside its parameters (the kernels' trailing pack, like DitherArgs and LightArgs): the mode as data - one instantiation
// serves Wrap and Mirror.  Replicate launches take no such argument and are the kernels that never heard of it.
struct EdgeArgs { int mode = kEdgeReplicate; };

// "replicate" | "wrap" | "mirror" <-> the mode; parse: false for anything else (mode untouched); name: nullptr for an unknown mode
inline const char* edge_mode_name(int mode) { return mode == kEdgeReplicate ? "replicate" : mode == kEdgeWrap ? "wrap" : mode == kEdgeMirror ? "mirror" : nullptr; }
inline bool edge_parse_mode(const char* name, int& mode) {
    if (!name) return false;
    for (int m = kEdgeReplicate; m <= kEdgeMirror; ++m)
        if (std::strcmp(name, edge_mode_name(m)) == 0) { mode = m; return true; }
    return false;
}

}  // namespace w2x
