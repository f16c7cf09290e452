// Host-side tile geometry: bit-exact restatement of calculateTiles / createTileWeights
// (/root/reference/src/tensorrt/img2img_render.cpp:7-66, img2img_load.cpp:29-52, 262-265), and everything the engine derives from the grid by integer
// arithmetic alone: the strips and shards of a frame spread over devices, the step schedule (batches, passes, slots) and the pipelined parts of a render()
// call.  Host-only: the CPU suite runs it under the sanitizers (w2x_parse_check tiles / parts, tests/test_render_parts_host.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "edge.h"

namespace w2x {

struct Rect { int x, y, w, h; };

struct TileGrid {
    int count = 0, nx = 0, ny = 0;
    std::vector<Rect> in, out;        // column-major: index = i*ny + j (img2img_render.cpp:43-44)
    int scaledInW = 0, scaledInH = 0; // input stride before overlap
    int inOvX = 0, inOvY = 0, outOvX = 0, outOvY = 0;
};

TileGrid calculate_tiles(int inW, int inH, int outW, int outH, int tileInW, int tileInH, int tileOutW, int tileOutH,
                         int scaling, double overlapX, double overlapY);

// One GPU's share of a single frame (tile-column strips): tiles are column-major, so part p of n owns the tile
// columns [p*nx/n, (p+1)*nx/n) and composes the output columns [x0, x1) = from its first tile's origin to the next part's.
// Pixels of that range are also covered by the tail of earlier tile columns (the blend band), so those columns are
// computed redundantly: tiles [first_tile, first_tile + tile_count) are a contiguous range of the reference's tile order,
// and every output pixel receives the same contributions in the same order as in a whole-frame render (bit-identical).
struct StripPlan { int first_tile = 0, tile_count = 0, x0 = 0, x1 = 0; };
StripPlan strip_plan(const TileGrid& g, int outW, int tileOutW, int part, int parts);

// One GPU's share of a single frame with EVERY TILE COMPUTED ONCE (second option: seam exchange instead of redundant columns).
// Part p of n takes the contiguous range [p * count / n, (p + 1) * count / n) of the reference's column-major tile order
// (img2img_render.cpp:43-44), so a range may begin and end inside a tile column.  The canvas is partitioned into one CELL per tile -
// cell (i, j) = x in [i * stride_x, (i + 1) * stride_x), y in [j * stride_y, (j + 1) * stride_y), the last column / row running to the canvas
// edge - and a part composes the cells of its own tiles: at most three rectangles (the tail of its first tile column, its whole columns, the
// head of its last one).  A pixel of cell (i, j) receives contributions from tiles (i-1..i, j-1..j) only (overlap < stride), added in
// ascending tile index like the reference's canvas add (img2img_render.cpp:329-330): besides its own tiles a part needs the blend bands of
// the ny + 1 tiles in front of its range - [halo_first, first_tile), computed by the preceding part(s) and copied over (the seam exchange).
struct ShardPlan {
    int first_tile = 0, tile_count = 0;   // own tiles (global indices)
    int halo_first = 0;                   // first tile whose bands are needed from the preceding parts (== first_tile: none)
    int nrect = 0;
    Rect rect[3];                         // output rectangles this part composes (x, y, w, h in canvas pixels)
};
ShardPlan shard_plan(const TileGrid& g, int outW, int outH, int tileOutW, int tileOutH, int part, int parts);
// The canvas cells of the contiguous tile range [t0, t1) into out[0..2]; returns how many rectangles (0 for an empty range or a grid without cells).
int tile_range_cells(const TileGrid& g, int outW, int outH, int tileOutW, int tileOutH, int t0, int t1, Rect out[3]);
// shard_plan() of every part into `plans`; false when the plans do not own every tile (shard_plan() hands out nothing when the blend bands are as wide as
// the tile stride).
bool shard_plans(const TileGrid& g, int outW, int outH, int tileOut, int parts, std::vector<ShardPlan>& plans);
// the slab slots a part keeps in front of its own tiles for the blend bands of the preceding parts' tiles [halo_first, first_tile)
inline size_t halo_slots(const ShardPlan& sp, int steps) { return (size_t)(sp.first_tile - sp.halo_first) * steps; }

// The step schedule of a frame's tiles (img2img_render.cpp:246-267): slot = step index, tile = step / steps, augmentation = step % steps (steps = 8 under TTA,
// else 1), zero pad slots at the end.  batch_count(): the reference batches (of userB steps) of `tiles` tiles (:249); pass_slots(): the slots of the whole
// network passes (of B slots, B / userB batches) those batches round up to; last_pass_live(): the live slots of the last of those passes.
int batch_count(int tiles, int steps, int userB);
size_t pass_slots(int tiles, int steps, int userB, int B);
int last_pass_live(int tiles, int steps, int B);

// A whole frame (render()) runs as a few PARTS one after the other: a part's tiles, its canvas cells composed and handed to the download
// stream, then the next part's while those cells travel to the host - the synchronous contract of img2img_render.cpp:226-344 with most of
// the 100 MB download of a 4K frame off the critical path: only the last part's cells travel after the last kernel (config 3: 9.9 ms per
// call as one part, 8.4 as three, profiles/r4_kernels/render_parts_*.txt).  The parts are those of shard_plan() (contiguous tile ranges, canvas cells of their
// tiles; a part reads the tiles in front of its range from the same slab), cut at multiples of the batch size so that batches, their order
// and the progress schedule (:246-250, 336-338) are the reference's.
constexpr int kMaxRenderParts = 4;
struct RenderParts {
    struct Part {
        int first = 0, tiles = 0;             // tiles [first, first + tiles) of the strip
        int batches = 0, batches_before = 0;  // reference batches of the part, and of the parts in front of it
        size_t slots_off = 0, slots = 0;      // where the part's steps begin in the slot table, and its pass_slots()
        int nrect = 0;
        Rect rect[3];                         // the cells of the part's tiles (tile_range_cells)
    };
    int n = 1;
    Part part[kMaxRenderParts];
    int batch_total = 0;
    size_t slot_total = 0;
    // the frame columns [0, x_split) are what the first part's tiles read: they are uploaded first, the rest while that part computes (tiles are ordered by
    // column, :43-44, so a part reads a column range).  == cols: the frame travels in one piece
    int x_split = 0;
    // the slab holds the frame's tiles in tile order: the last part's passes end at most a pass beyond them, and the frame as ONE part (what a resident replay
    // runs) ends at most a pass beyond its tiles - slots for both
    size_t slab_slots = 0;
};
// The parts of `strip` (tiles of `grid`, T x T in, Tout x Tout out) of a frame of `cols` columns and an outW x outH canvas.  `want`: how many parts the call
// may use (1 for a strip of several, a resized frame or a switched-off pipeline); a frame of fewer than 16 tiles or with an overlap that reaches the stride
// is one part, every other at most min(want, kMaxRenderParts, tiles / 8).
RenderParts render_parts(const TileGrid& grid, const StripPlan& strip, int cols, int outW, int outH, int T, int Tout, int steps, int userB, int B, int want);

// The frames of a chained render (Img2Img::renderChained*): `count` stages (kChainMinStages .. kChainMaxStages) with the scale factors scalings[k]
// take a rows x cols frame to rows * S x cols * S, S their product; stage k reads a frame of rows[k] x cols[k] (rows[0] = the source's) and the last stage's
// canvas, rows[count] x cols[count], is resized to the target dst_rows x dst_cols (0 x 0: the canvas itself).  This is the one place the size rules live:
// every scaling in 1 .. kChainMaxScaling, no frame beyond kChainMaxDim samples per side, the target per axis in [source dim, source dim * S] - the two axes
// independent - and no smaller than the last canvas over kChainMaxShrink (the resize kernels' tile holds the input rows of a shrink by 4 at most).
constexpr int kChainMinStages = 2, kChainMaxStages = 4, kChainMaxScaling = 4, kChainMaxDim = 1 << 16, kChainMaxShrink = 4;
enum ChainRefusal { kChainOk = 0, kChainCount = 1, kChainScaling = 2, kChainSource = 3, kChainTooLarge = 4, kChainTarget = 5, kChainShrink = 6 };
struct ChainPlan {
    int count = 0, S = 0;
    int rows[kChainMaxStages + 1] = {}, cols[kChainMaxStages + 1] = {};
    int out_rows = 0, out_cols = 0;                                      // the target
    bool resized = false;                                                // the target is not the last canvas
};
ChainRefusal chain_plan(int rows, int cols, const int* scalings, int count, int dst_rows, int dst_cols, ChainPlan& plan);
const char* chain_refusal_text(ChainRefusal why);

// left/top ramp: w[i] = float(double(i+1)/(ov+1)), i < ov  (img2img_load.cpp:34-45)
std::vector<float> blend_ramp(int ov);

// full mask like the reference builds it; which: 0 top, 1 right, 2 bottom, 3 left
std::vector<float> tile_weight_mask(int which, int ovx, int ovy, int size);

// Tap tables of an antialiased separable resize of one axis, `in` -> `out` samples: PIL's convolution resampler as
// torch.nn.functional.interpolate(mode=bilinear / bicubic, antialias=True, align_corners=False) computes it.  Output i is centred on
// (i + 0.5) * scale (scale = in / out); the filter support grows by `scale` when scale > 1; the taps are clipped at the border and
// normalised to sum 1; bicubic uses a = -0.5.  Computed in double, stored as float: first[i] = the first input index, w[i * taps + k]
// its k-th weight (zero past the taps output i has).  filter: 0 bicubic, 1 bilinear.  taps = 0 for invalid arguments.
struct ResizeTaps { int taps = 0; std::vector<int> first; std::vector<float> w; };
ResizeTaps resize_taps(int in, int out, int filter);
// The same under an edge mode (edge.h).  kEdgeReplicate: resize_taps, to the bit.  kEdgeWrap / kEdgeMirror: the taps are NOT clipped at the border -
// every output has its full support, first[i] = floor(centre - support + 0.5) may be negative and first[i] + k may pass `in`; tap k reads the sample
// edge_index(mode, first[i] + k, in); the weights are normalised over all taps.  This is the table torch's resampler has in the interior of a frame padded with
// np.pad(mode = "wrap" / "reflect").  taps = 0 for invalid arguments, an unknown mode included.
ResizeTaps resize_taps_edge(int in, int out, int filter, int mode);

// Colour bleed under transparent pixels (RGBA frames), integer and exact.  bgr: rows x cols interleaved 8-bit BGR, alpha: rows x cols
// bytes, radius R in [0, 16].  known_0(p) = alpha(p) > 0, col_0 = bgr.  Iteration it = 1..R reads state it - 1 and writes state it (Jacobi): a pixel unknown in
// state it - 1 with n > 0 neighbours among its eight that lie inside the frame and are known in state it - 1 takes, per channel, (their sum + (n >> 1)) / n
// and becomes known; every other pixel keeps colour and flag.  out = col_R (a pixel still unknown keeps its colour; R = 0, an all-zero and an all-non-zero
// plane leave the frame unchanged; a known pixel never changes).  out may not alias bgr.  false (nothing written) for invalid arguments.
// edge: kEdgeWrap - the eight neighbours are taken through edge_index (all eight always exist; colour spreads across the joint of a texture that
// tiles); kEdgeReplicate and kEdgeMirror - the rule above, a neighbour outside the frame does not exist (a reflected neighbour carries no new information).  An
// unknown mode is an invalid argument.  The same for alpha_bleed_planes.
bool alpha_bleed(const uint8_t* bgr, size_t bgr_step, const uint8_t* alpha, size_t alpha_step, int rows, int cols, int radius, uint8_t* out, size_t out_step,
                 int edge = kEdgeReplicate);

// alpha_bleed restated on planes of codes of any integer depth (planar RGBA frames).  colour[0..2] and alpha: planes of rows x cols samples of
// sample_bytes (1: uint8, 2: uint16) with steps in bytes; maxcode = 2^bits - 1 (at most 65535, and 255 for one-byte samples).  Every code is first clamped to
// maxcode, alpha included: known_0(p) = min(alpha(p), maxcode) > 0.  The iterations, the neighbourhood and the mean (sum + (n >> 1)) / n are alpha_bleed's - eight
// 16-bit codes fit a 32-bit sum.  out[0..2]: the three planes of state R (no plane of out may alias an input).  At one byte and maxcode 255 the planes are those
// of alpha_bleed.  false (nothing written) for invalid arguments.
bool alpha_bleed_planes(const void* const colour[3], const size_t colour_steps[3], const void* alpha, size_t alpha_step, int rows, int cols, int sample_bytes,
                        unsigned maxcode, int radius, void* const out[3], const size_t out_steps[3], int edge = kEdgeReplicate);

}  // namespace w2x
