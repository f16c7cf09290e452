#include "tiles.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace w2x {

TileGrid calculate_tiles(int inW, int inH, int outW, int outH, int tileInW, int tileInH, int tileOutW, int tileOutH,
                         int scaling, double overlapX, double overlapY) {
    TileGrid g;
    // img2img_render.cpp:11-14 - the width is used for both dimensions
    const int sOutW = tileInW * scaling, sOutH = tileInW * scaling;
    // :16-19
    const int sInW = (int)std::lround((double)tileOutW / sOutW * tileInW);
    const int sInH = (int)std::lround((double)tileOutH / sOutH * tileInH);
    // :21-24
    g.inOvX = (int)std::lround(tileInW * overlapX);
    g.inOvY = (int)std::lround(tileInH * overlapY);
    // :26-29
    g.outOvX = (int)std::lround(sOutW * overlapX);
    g.outOvY = (int)std::lround(sOutH * overlapY);
    // degenerate geometry (overlap >= stride): the reference divides by zero here; report an empty grid instead
    if (sInW - g.inOvX <= 0 || sInH - g.inOvY <= 0 || sOutW <= 0) return g;
    // :31-34
    g.nx = (int)std::lround(std::ceil((double)(inW - g.inOvX) / (sInW - g.inOvX)));
    g.ny = (int)std::lround(std::ceil((double)(inH - g.inOvY) / (sInH - g.inOvY)));
    g.count = g.nx * g.ny;
    g.scaledInW = sInW; g.scaledInH = sInH;
    g.in.reserve(g.count > 0 ? g.count : 0); g.out.reserve(g.count > 0 ? g.count : 0);
    for (int i = 0; i < g.nx; ++i) {
        for (int j = 0; j < g.ny; ++j) {
            // :46-51
            g.in.push_back(Rect{-((tileInW - sInW) / 2) + i * sInW - i * g.inOvX,
                                -((tileInH - sInH) / 2) + j * sInH - j * g.inOvY, tileInW, tileInH});
            // :54-61
            const int x = i * tileOutW - i * g.outOvX;
            const int y = j * tileOutH - j * g.outOvY;
            g.out.push_back(Rect{x, y, x + tileOutW > outW ? outW - x : tileOutW, y + tileOutH > outH ? outH - y : tileOutH});
        }
    }
    return g;
}

std::vector<float> blend_ramp(int ov) {
    std::vector<float> r(ov > 0 ? ov : 0);
    const int d = ov + 1;
    for (int i = 1; i < d; ++i) r[i - 1] = (float)((double)i / d);
    return r;
}

std::vector<float> tile_weight_mask(int which, int ovx, int ovy, int size) {
    std::vector<float> m((size_t)size * size, 1.f);
    if (which == 0 || which == 2) {
        auto r = blend_ramp(ovy);
        for (int i = 0; i < ovy && i < size; ++i) {
            int row = which == 0 ? i : size - 1 - i;
            for (int x = 0; x < size; ++x) m[(size_t)row * size + x] = r[i];
        }
    } else {
        auto r = blend_ramp(ovx);
        for (int i = 0; i < ovx && i < size; ++i) {
            int col = which == 3 ? i : size - 1 - i;
            for (int y = 0; y < size; ++y) m[(size_t)y * size + col] = r[i];
        }
    }
    return m;
}

StripPlan strip_plan(const TileGrid& g, int outW, int tileOutW, int part, int parts) {
    StripPlan sp;
    if (parts <= 0 || part < 0 || part >= parts || g.nx <= 0) return sp;
    const int stride = tileOutW - g.outOvX;                   // output origin of tile column i = i * stride (img2img_render.cpp:54-55)
    // Every strip but the first also renders the k earlier tile columns whose blend band reaches into its pixels (k = 1 for every
    // blend setting of the command line, 0 without overlap), so the strips are balanced by the columns they RENDER, nx + (parts - 1) k
    // in all: strip p ends at column floor((p + 1) (nx + (parts - 1) k) / parts) - p k.  (Equal shares of own columns left the first
    // strip short and the others a column over: 20 / 30 tiles instead of 25 / 25 for nx = 9, two strips.)
    const int k = g.outOvX > 0 && stride > 0 ? (g.outOvX + stride - 1) / stride : 0;
    auto end_col = [&](int p) {
        const long t = (long)g.nx + (long)(parts - 1) * k;
        long c = (long)(p + 1) * t / parts - (long)p * k;
        if (p + 1 == parts) c = g.nx;
        return (int)std::min<long>(std::max<long>(c, 0), g.nx);
    };
    int c0 = 0;
    for (int p = 0; p < part; ++p) c0 = std::max(c0, end_col(p));
    const int c1 = std::max(c0, end_col(part));
    if (c0 >= c1) return sp;                                  // more parts than tile columns: nothing to do
    sp.x0 = c0 * stride;
    sp.x1 = c1 < g.nx ? c1 * stride : outW;
    int cc0 = c0;                                             // first tile column whose extent reaches x0
    while (cc0 > 0 && (cc0 - 1) * stride + tileOutW > sp.x0) --cc0;
    sp.first_tile = cc0 * g.ny;
    sp.tile_count = (c1 - cc0) * g.ny;
    return sp;
}

ShardPlan shard_plan(const TileGrid& g, int outW, int outH, int tileOutW, int tileOutH, int part, int parts) {
    ShardPlan sp;
    if (parts <= 0 || part < 0 || part >= parts || g.count <= 0 || g.ny <= 0) return sp;
    const int sx = tileOutW - g.outOvX, sy = tileOutH - g.outOvY;
    // a cell sees tiles (i-1..i, j-1..j) only if a tile's blend band does not reach past its neighbour: overlap < stride (every blend setting of
    // the command line: overlap <= 1/8 of the tile)
    if (sx <= 0 || sy <= 0 || g.outOvX >= sx || g.outOvY >= sy) return sp;
    const long t0 = (long)part * g.count / parts, t1 = (long)(part + 1) * g.count / parts;
    if (t0 >= t1) return sp;                                           // more parts than tiles
    sp.first_tile = (int)t0; sp.tile_count = (int)(t1 - t0);
    sp.halo_first = (int)std::max<long>(0, t0 - g.ny - 1);
    sp.nrect = tile_range_cells(g, outW, outH, tileOutW, tileOutH, sp.first_tile, sp.first_tile + sp.tile_count, sp.rect);
    return sp;
}

int tile_range_cells(const TileGrid& g, int outW, int outH, int tileOutW, int tileOutH, int t0, int t1, Rect out[3]) {
    if (g.ny <= 0 || t0 < 0 || t0 >= t1 || t1 > g.count) return 0;
    const int sx = tileOutW - g.outOvX, sy = tileOutH - g.outOvY;
    int n = 0;
    auto x_of = [&](int i) { return i >= g.nx ? outW : i * sx; };
    auto y_of = [&](int j) { return j >= g.ny ? outH : j * sy; };
    auto add = [&](int i0, int i1, int j0, int j1) {                   // cells of columns [i0, i1) x rows [j0, j1)
        if (i0 >= i1 || j0 >= j1) return;
        out[n++] = Rect{x_of(i0), y_of(j0), x_of(i1) - x_of(i0), y_of(j1) - y_of(j0)};
    };
    const int c0 = t0 / g.ny, r0 = t0 % g.ny, c1 = t1 / g.ny, r1 = t1 % g.ny;
    if (c0 == c1) add(c0, c0 + 1, r0, r1);                             // inside one column
    else {
        int full0 = c0;
        if (r0 != 0) { add(c0, c0 + 1, r0, g.ny); full0 = c0 + 1; }    // the tail of the first column
        add(full0, c1, 0, g.ny);                                       // whole columns
        if (r1 != 0) add(c1, c1 + 1, 0, r1);                           // the head of the last column
    }
    return n;
}

bool shard_plans(const TileGrid& g, int outW, int outH, int tileOut, int parts, std::vector<ShardPlan>& plans) {
    plans.assign(std::max(parts, 0), ShardPlan{});
    int owned = 0;
    for (int k = 0; k < parts; ++k) { plans[k] = shard_plan(g, outW, outH, tileOut, tileOut, k, parts); owned += plans[k].tile_count; }
    return owned == g.count;
}

int batch_count(int tiles, int steps, int userB) { return (int)std::lround(std::ceil((double)(tiles * steps) / userB)); }

size_t pass_slots(int tiles, int steps, int userB, int B) {
    const int S = B / userB;
    return (size_t)((batch_count(tiles, steps, userB) + S - 1) / S) * B;
}

int last_pass_live(int tiles, int steps, int B) { return tiles * steps - (tiles * steps - 1) / B * B; }

RenderParts render_parts(const TileGrid& grid, const StripPlan& strip, int cols, int outW, int outH, int T, int Tout, int steps, int userB, int B, int want) {
    RenderParts rp;
    const int tiles = strip.tile_count;
    int first_of[kMaxRenderParts + 1] = {0, tiles, 0, 0, 0};            // part k = tiles [first_of[k], first_of[k + 1]) of the strip
    if (want > 1 && tiles >= 16 && grid.outOvX < Tout - grid.outOvX && grid.outOvY < Tout - grid.outOvY) {
        int q = 1; while ((q * steps) % userB) ++q;                     // part boundaries: whole reference batches
        want = std::min({want, kMaxRenderParts, tiles / 8});
        // the LAST part is the small one - its cells are the only ones that travel after the last kernel (a fifth of the tiles, at least 8: smaller passes no longer
        // fill the device) - and the tiles in front of it split evenly: config 3's 45 tiles run as 16 + 20 + 9 (8.4 ms per call; as 15 + 15 + 15: 8.8, 12 + 12 + 12 + 9: 8.45)
        int n = 0;
        const int body = want >= 2 ? (tiles - std::max(8, tiles / 5)) / q * q : 0;
        for (int k = 1; k < want; ++k) {
            const int t = k + 1 == want ? body : (int)((long)k * body / (want - 1)) / q * q;
            if (t > first_of[n] && t < tiles) first_of[++n] = t;
        }
        first_of[++n] = tiles;
        rp.n = n;
    }
    for (int k = 0; k < rp.n; ++k) {
        RenderParts::Part& p = rp.part[k];
        p.first = first_of[k]; p.tiles = first_of[k + 1] - first_of[k];
        p.batches = batch_count(p.tiles, steps, userB);
        p.batches_before = rp.batch_total; rp.batch_total += p.batches;
        p.slots_off = rp.slot_total;
        p.slots = pass_slots(p.tiles, steps, userB, B);                 // reference batches rounded up to whole network passes
        rp.slot_total += p.slots;
        p.nrect = tile_range_cells(grid, outW, outH, Tout, Tout, strip.first_tile + p.first, strip.first_tile + p.first + p.tiles, p.rect);
    }
    rp.x_split = cols;
    if (rp.n > 1) {
        int xm = 0;
        for (int t = 0; t < first_of[1]; ++t) xm = std::max(xm, grid.in[strip.first_tile + t].x + T);
        if (xm > 0 && xm < cols - 64) rp.x_split = xm;
    }
    const RenderParts::Part& last = rp.part[rp.n - 1];
    rp.slab_slots = std::max((size_t)last.first * steps + last.slots, pass_slots(tiles, steps, userB, B));
    return rp;
}

ResizeTaps resize_taps(int in, int out, int filter) {
    ResizeTaps t;
    if (in <= 0 || out <= 0 || (filter != 0 && filter != 1)) return t;
    const double scale = (double)in / out;
    const double half = filter == 0 ? 2.0 : 1.0;                       // interp_size / 2: bicubic 4 taps, bilinear 2 at scale 1
    const double support = scale >= 1.0 ? half * scale : half;
    const double inv = scale >= 1.0 ? 1.0 / scale : 1.0;
    t.taps = (int)std::ceil(support) * 2 + 1;
    t.first.assign(out, 0); t.w.assign((size_t)out * t.taps, 0.f);
    auto f = [&](double x) {
        x = std::fabs(x);
        if (filter == 1) return x < 1.0 ? 1.0 - x : 0.0;
        const double a = -0.5;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
        if (x < 2.0) return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a;
        return 0.0;
    };
    std::vector<double> w(t.taps);
    for (int i = 0; i < out; ++i) {
        const double center = scale * (i + 0.5);
        const long x0 = std::max<long>((long)(center - support + 0.5), 0);
        const long n = std::min<long>(std::min<long>((long)(center + support + 0.5), in) - x0, t.taps);
        double total = 0.0;
        for (long k = 0; k < n; ++k) { w[k] = f((k + x0 - center + 0.5) * inv); total += w[k]; }
        t.first[i] = (int)x0;
        for (long k = 0; k < n; ++k) t.w[(size_t)i * t.taps + k] = (float)(total != 0.0 ? w[k] / total : w[k]);
    }
    return t;
}

ResizeTaps resize_taps_edge(int in, int out, int filter, int mode) {
    if (!edge_mode_ok(mode)) return ResizeTaps();
    if (mode == kEdgeReplicate) return resize_taps(in, out, filter);
    ResizeTaps t;
    if (in <= 0 || out <= 0 || (filter != 0 && filter != 1)) return t;
    const double scale = (double)in / out;
    const double half = filter == 0 ? 2.0 : 1.0;
    const double support = scale >= 1.0 ? half * scale : half;
    const double inv = scale >= 1.0 ? 1.0 / scale : 1.0;
    t.taps = (int)std::ceil(support) * 2 + 1;
    t.first.assign(out, 0); t.w.assign((size_t)out * t.taps, 0.f);
    auto f = [&](double x) {                                          // (resize_taps' two filters)
        x = std::fabs(x);
        if (filter == 1) return x < 1.0 ? 1.0 - x : 0.0;
        const double a = -0.5;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
        if (x < 2.0) return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a;
        return 0.0;
    };
    std::vector<double> w(t.taps);
    for (int i = 0; i < out; ++i) {
        const double center = scale * (i + 0.5);
        const long x0 = (long)std::floor(center - support + 0.5);      // (resize_taps truncates, which is floor where it does not clip)
        const long n = std::min<long>((long)std::floor(center + support + 0.5) - x0, t.taps);
        double total = 0.0;
        for (long k = 0; k < n; ++k) { w[k] = f((k + x0 - center + 0.5) * inv); total += w[k]; }
        t.first[i] = (int)x0;
        for (long k = 0; k < n; ++k) t.w[(size_t)i * t.taps + k] = (float)(total != 0.0 ? w[k] / total : w[k]);
    }
    return t;
}

bool alpha_bleed(const uint8_t* bgr, size_t bgr_step, const uint8_t* alpha, size_t alpha_step, int rows, int cols, int radius, uint8_t* out, size_t out_step, int edge) {
    if (!bgr || !alpha || !out || rows <= 0 || cols <= 0 || radius < 0 || radius > 16 || !edge_mode_ok(edge)) return false;
    const bool wrap = edge == kEdgeWrap;
    if (bgr_step < (size_t)cols * 3 || out_step < (size_t)cols * 3 || alpha_step < (size_t)cols) return false;
    const size_t n_px = (size_t)rows * cols;
    std::vector<uint8_t> col(n_px * 3), col2, known(n_px), known2;
    for (int y = 0; y < rows; ++y) {
        memcpy(&col[(size_t)y * cols * 3], bgr + (size_t)y * bgr_step, (size_t)cols * 3);
        for (int x = 0; x < cols; ++x) known[(size_t)y * cols + x] = alpha[(size_t)y * alpha_step + x] > 0;
    }
    for (int it = 1; it <= radius; ++it) {
        col2 = col; known2 = known;                    // state it starts as state it - 1; only pixels that become known change
        bool changed = false;
        for (int y = 0; y < rows; ++y)
            for (int x = 0; x < cols; ++x) {
                const size_t i = (size_t)y * cols + x;
                if (known[i]) continue;
                unsigned n = 0, sum[3] = {0, 0, 0};
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        int yy = y + dy, xx = x + dx;
                        if (dy == 0 && dx == 0) continue;
                        if (wrap) { yy = edge_index(kEdgeWrap, yy, rows); xx = edge_index(kEdgeWrap, xx, cols); }
                        else if (yy < 0 || yy >= rows || xx < 0 || xx >= cols) continue;
                        const size_t q = (size_t)yy * cols + xx;
                        if (!known[q]) continue;
                        ++n;
                        for (int ch = 0; ch < 3; ++ch) sum[ch] += col[q * 3 + ch];
                    }
                if (!n) continue;
                for (int ch = 0; ch < 3; ++ch) col2[i * 3 + ch] = (uint8_t)((sum[ch] + (n >> 1)) / n);
                known2[i] = 1; changed = true;
            }
        if (!changed) break;                           // nothing left to reach: the later states are this one
        col.swap(col2); known.swap(known2);
    }
    for (int y = 0; y < rows; ++y) memcpy(out + (size_t)y * out_step, &col[(size_t)y * cols * 3], (size_t)cols * 3);
    return true;
}

namespace {
// alpha_bleed's loop on three planes of samples T (the state: three packed planes of clamped codes and the flags)
template <typename T>
void bleed_planes(const void* const colour[3], const size_t colour_steps[3], const void* alpha, size_t alpha_step, int rows, int cols, unsigned maxcode, int radius,
                  void* const out[3], const size_t out_steps[3], bool wrap) {
    const size_t n_px = (size_t)rows * cols;
    auto at = [](const void* base, size_t step, int y, int x) { return ((const T*)((const uint8_t*)base + (size_t)y * step))[x]; };
    std::vector<T> col(n_px * 3), col2;
    std::vector<uint8_t> known(n_px), known2;
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            const size_t i = (size_t)y * cols + x;
            for (int ch = 0; ch < 3; ++ch) col[i * 3 + ch] = (T)std::min<unsigned>(at(colour[ch], colour_steps[ch], y, x), maxcode);
            known[i] = std::min<unsigned>(at(alpha, alpha_step, y, x), maxcode) > 0;
        }
    for (int it = 1; it <= radius; ++it) {
        col2 = col; known2 = known;
        bool changed = false;
        for (int y = 0; y < rows; ++y)
            for (int x = 0; x < cols; ++x) {
                const size_t i = (size_t)y * cols + x;
                if (known[i]) continue;
                uint32_t n = 0, sum[3] = {0, 0, 0};
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        int yy = y + dy, xx = x + dx;
                        if (dy == 0 && dx == 0) continue;
                        if (wrap) { yy = edge_index(kEdgeWrap, yy, rows); xx = edge_index(kEdgeWrap, xx, cols); }
                        else if (yy < 0 || yy >= rows || xx < 0 || xx >= cols) continue;
                        const size_t q = (size_t)yy * cols + xx;
                        if (!known[q]) continue;
                        ++n;
                        for (int ch = 0; ch < 3; ++ch) sum[ch] += col[q * 3 + ch];
                    }
                if (!n) continue;
                for (int ch = 0; ch < 3; ++ch) col2[i * 3 + ch] = (T)((sum[ch] + (n >> 1)) / n);
                known2[i] = 1; changed = true;
            }
        if (!changed) break;
        col.swap(col2); known.swap(known2);
    }
    for (int ch = 0; ch < 3; ++ch)
        for (int y = 0; y < rows; ++y) {
            T* d = (T*)((uint8_t*)out[ch] + (size_t)y * out_steps[ch]);
            for (int x = 0; x < cols; ++x) d[x] = col[((size_t)y * cols + x) * 3 + ch];
        }
}
}  // namespace

bool alpha_bleed_planes(const void* const colour[3], const size_t colour_steps[3], const void* alpha, size_t alpha_step, int rows, int cols, int sample_bytes,
                        unsigned maxcode, int radius, void* const out[3], const size_t out_steps[3], int edge) {
    if (!colour || !colour_steps || !alpha || !out || !out_steps || rows <= 0 || cols <= 0 || radius < 0 || radius > 16 || !edge_mode_ok(edge)) return false;
    const bool wrap = edge == kEdgeWrap;
    if ((sample_bytes != 1 && sample_bytes != 2) || maxcode == 0 || maxcode > (sample_bytes == 1 ? 255u : 65535u)) return false;
    const size_t row = (size_t)cols * sample_bytes, mis = (size_t)sample_bytes - 1;
    if (alpha_step < row || ((((size_t)alpha) | alpha_step) & mis)) return false;
    for (int ch = 0; ch < 3; ++ch) {
        if (!colour[ch] || !out[ch] || colour_steps[ch] < row || out_steps[ch] < row) return false;
        if ((((size_t)colour[ch]) | colour_steps[ch] | ((size_t)out[ch]) | out_steps[ch]) & mis) return false;
    }
    if (sample_bytes == 1) bleed_planes<uint8_t>(colour, colour_steps, alpha, alpha_step, rows, cols, maxcode, radius, out, out_steps, wrap);
    else bleed_planes<uint16_t>(colour, colour_steps, alpha, alpha_step, rows, cols, maxcode, radius, out, out_steps, wrap);
    return true;
}

ChainRefusal chain_plan(int rows, int cols, const int* scalings, int count, int dst_rows, int dst_cols, ChainPlan& plan) {
    plan = ChainPlan{};
    if (count < kChainMinStages || count > kChainMaxStages || !scalings) return kChainCount;
    for (int k = 0; k < count; ++k) if (scalings[k] < 1 || scalings[k] > kChainMaxScaling) return kChainScaling;
    if (rows <= 0 || cols <= 0) return kChainSource;
    plan.count = count; plan.S = 1;
    long r = rows, c = cols;
    plan.rows[0] = rows; plan.cols[0] = cols;
    for (int k = 0; k < count; ++k) {
        r *= scalings[k]; c *= scalings[k]; plan.S *= scalings[k];
        if (r > kChainMaxDim || c > kChainMaxDim) { plan = ChainPlan{}; return kChainTooLarge; }
        plan.rows[k + 1] = (int)r; plan.cols[k + 1] = (int)c;
    }
    const bool full = dst_rows == 0 && dst_cols == 0;
    plan.out_rows = full ? (int)r : dst_rows; plan.out_cols = full ? (int)c : dst_cols;
    ChainRefusal why = kChainOk;
    if (plan.out_rows < rows || plan.out_rows > r || plan.out_cols < cols || plan.out_cols > c) why = kChainTarget;
    else if ((long)plan.out_rows * kChainMaxShrink < r || (long)plan.out_cols * kChainMaxShrink < c) why = kChainShrink;
    if (why != kChainOk) { plan = ChainPlan{}; return why; }
    plan.resized = plan.out_rows != r || plan.out_cols != c;
    return kChainOk;
}
const char* chain_refusal_text(ChainRefusal why) {
    switch (why) {
        case kChainOk: return "";
        case kChainCount: return "A chain takes 2 to 4 stages.";
        case kChainScaling: return "A stage of the chain has a scale factor outside 1..4.";
        case kChainSource: return "Input image is empty.";
        case kChainTooLarge: return "A frame of the chain is larger than 65536 samples per side.";
        case kChainTarget: return "Output image has invalid size for the chain: each dimension must lie between the input's and the input's times the product of the stages' scale factors.";
        case kChainShrink: return "Output image has invalid size for the chain: the last stage's canvas can shrink by a factor of 4 at most.";
    }
    return "Unknown chain refusal.";
}

}  // namespace w2x
