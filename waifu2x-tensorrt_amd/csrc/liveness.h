// Dead-skip extents: for every plan op, the rows of its row map that some KEPT output pixel of a tile depends on.
// A tile at the right / bottom edge of a frame keeps only the part of its output that calculate_tiles' clipped rect (TileGrid::out)
// covers; everything else it computes lies on replicate padding and compose never reads it.  Host-only.
//
// The set of an op is a product of two axis sets of the form [0, c) U [n - w, n) over the op's ROW MAP - the map its launch walks:
// the token map of an MLP or attention op, the output pixels of a convolution, the INPUT tokens of a pixel-shuffle projection.
// It is found by walking the ops backwards from the kept rect, each op widening the set by its own footprint:
//   per-token ops (MLP, 1 x 1 rows, the image head)   nothing (a pixel-shuffle projection by r: token x is needed when one of its r outputs is)
//   window attention                                   whole windows under the op's cyclic roll (ry, rx): a window is needed as soon as one of its
//                                                      tokens is, and then needs ALL its tokens as keys, masked ones included
//   k x k stride-s convolutions                        their taps: output x reads inputs s x .. s x + k - 1 of its (cropped) input view
//   a tensor read by several ops (skip connections)    the union of its readers' sets, per axis
// A set that is not of that form on an axis becomes the whole axis.  Plans with anything else in them (fp32, un-fused attention,
// LayerNorm statistics passed between ops, squeeze-excite, window tables without a closed form) get "all" for every op.
#pragma once
#include <vector>

#include "plan.h"

namespace w2x {

struct AxisExt { int n = 0, c = 0, w = 0; };          // [0, c) U [n - w, n); all: c == n, w == 0
struct OpExtent {
    AxisExt x, y;                                     // over the op's row map (W x H)
    int ry = -1, rx = -1, ws = 0;                     // window attention: roll and window size (else -1, -1, 0)
    bool all() const { return x.c >= x.n && y.c >= y.n; }
    // units of the launch that run / exist (windows for attention, rows else): what the profile records price
    long live_units() const;
    long total_units() const;
};

// kept_w x kept_h: the tile's clipped output rect (output pixels, from the tile's origin).  kept >= Tout on both axes, `force_all`
// (TTA slots, w2x_infer, the no_dead_skip switch) or an unsupported plan: every op "all".
std::vector<OpExtent> dead_skip_extents(const Plan& plan, int kept_w, int kept_h, bool force_all = false);

}  // namespace w2x
