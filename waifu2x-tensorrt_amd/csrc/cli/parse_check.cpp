// Sanitizer driver for everything in this tree that parses files or command lines: the hand-written ONNX protobuf reader
// (onnx_pb.cpp), constant folding and lowering (fold.cpp, lower.cpp), the engine-file reader (plan.cpp), the tile grid (tiles.cpp),
// the built-in image / video codecs (cli/imageio.cpp) and the option parser (cli/args.cpp) - and for the pass schedule of a lowered plan (schedule.cpp).  `make asan` builds it with
// g++ -fsanitize=address,undefined -fno-sanitize-recover=all - host code only, no HIP - and tests/test_malformed_inputs.py feeds it
// truncated and bit-flipped files.  The reference has no such target (CMakeLists.txt:49-68).
//   w2x_parse_check onnx  FILE BATCH TILE [fp32]    load_onnx -> fold_graph -> lower_graph -> serialize -> deserialize
//   w2x_parse_check plan  FILE                      Plan::deserialize (+ validate), what load() runs on an engine file
//   w2x_parse_check image FILE [deep]               read_image, then write_image to /dev/null-like temp names in every format it allows
//   w2x_parse_check avi   FILE                      AviReader::open + every frame
//   w2x_parse_check args  ARGS...                   cli::parse
//   w2x_parse_check tiles W H T S TOUT OVX OVY      calculate_tiles, then strip_plan, shard_plans, tile_range_cells and render_parts over the grid
//   w2x_parse_check parts W H T S TOUT OVX OVY [STEPS USERB B WANT]...   the grid, its tiles and its shard plans for 1-8 parts beside tile_range_cells of the same
//                                                           ranges, then render_parts (tiles.h) of the whole frame per schedule: one line per case and per part;
//                                                           tests/test_render_parts_host.py judges them
//   w2x_parse_check bleed FILE RADIUS               read_image, then alpha_bleed of its colour under its alpha plane (an opaque plane without one), padded rows
//   w2x_parse_check planes BITS ROWS COLS RADIUS SEED OUT   alpha_bleed_planes on a seeded frame of four planes of BITS (8, 10, 12, 16), padded rows; OUT receives
//                                                           the four planes and the three bled ones, packed, for the test to compare with its own statement
//   w2x_parse_check schedule FILE BATCH TILE {fp16|tf32|fp32} [switch=value ...]   lower_for_shape -> candidate_launches -> layout_arena (schedule.h), printed: one line
//                                                           per plan, op, launch and tensor and one for the arena; tests/test_schedule_host.py judges them
//   w2x_parse_check dither {ordered|bluenoise} PHASE PLANE X0 Y0 W H   dither_rank / dither_threshold (dither.h) over a W x H window of plane PLANE at PHASE:
//                                                           one line of ranks per row and, behind a line "thresholds", one of thresholds; "table" in place of the
//                                                           mode prints the 64 x 64 table.  tests/test_dither_host.py compares them with its own statement
// Exit code: 0 = accepted, 2 = rejected with a message on stderr (the clean `false` of the product path); anything else is a crash
// or a sanitizer report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../dither.h"
#include "../lower.h"
#include "../schedule.h"
#include "../switches.h"
#include "../tiles.h"
#include "args.h"
#include "imageio.h"

using namespace w2x;

static int run(int argc, char** argv) {
    if (argc < 3) throw std::runtime_error("usage: w2x_parse_check {onnx|plan|image|avi|args|tiles|parts|bleed|planes|schedule|dither} ...");
    const std::string mode = argv[1];
    if (mode == "onnx") {
        if (argc < 5) throw std::runtime_error("onnx FILE BATCH TILE [fp32]");
        const int batch = atoi(argv[3]), tile = atoi(argv[4]);
        Plan plan = build_plan(argv[2], batch, 3, tile, tile, argc > 5);
        plan.userB = batch;
        const std::vector<uint8_t> bytes = plan.serialize();
        const Plan back = Plan::deserialize(bytes.data(), bytes.size());
        printf("ok: %zu ops, %zu tensors, %zu bytes of engine file, %s\n", back.ops.size(), back.tensors.size(), bytes.size(), onnx_op_histogram(argv[2]).substr(0, 60).c_str());
    } else if (mode == "plan") {
        std::ifstream f(argv[2], std::ios::binary | std::ios::ate);
        if (!f.is_open()) throw std::runtime_error("could not open engine file");
        std::vector<char> bytes((size_t)f.tellg());
        f.seekg(0); f.read(bytes.data(), (std::streamsize)bytes.size());
        const Plan p = Plan::deserialize((const uint8_t*)bytes.data(), bytes.size());
        printf("ok: %zu ops\n", p.ops.size());
    } else if (mode == "image") {
        const cli::Bitmap b = cli::read_image(argv[2], argc > 3);
        const std::string tmp = std::string(argv[2]) + ".rewritten";
        cli::write_image(tmp + ".png", b);
        if (b.bgr16.empty()) { cli::write_image(tmp + ".bmp", b); cli::Bitmap c = b; c.alpha.clear(); cli::write_image(tmp + ".ppm", c); }
        printf("ok: %d x %d%s%s\n", b.cols, b.rows, b.alpha.empty() ? "" : " +alpha", b.bgr16.empty() ? "" : " 16-bit");
    } else if (mode == "avi") {
        cli::AviReader rd; std::string why;
        if (!rd.open(argv[2], &why)) throw std::runtime_error("not an AVI this reader takes: " + why);
        std::vector<uint8_t> frame((size_t)rd.info().width * rd.info().height * 3);
        int n = 0;
        while (rd.read(frame.data())) ++n;
        printf("ok: %d x %d, %d of %d frames\n", rd.info().width, rd.info().height, n, rd.info().frames);
    } else if (mode == "args") {
        const cli::Options o = cli::parse(argc - 1, argv + 1);
        printf("ok: %s\n", cli::to_json(o).c_str());
    } else if (mode == "tiles") {
        if (argc < 9) throw std::runtime_error("tiles W H T S TOUT OVX OVY");
        const int W = atoi(argv[2]), H = atoi(argv[3]), T = atoi(argv[4]), S = atoi(argv[5]), TO = atoi(argv[6]);
        const TileGrid g = calculate_tiles(W, H, W * S, H * S, T, T, TO, TO, S, atof(argv[7]), atof(argv[8]));
        for (int parts = 1; parts <= 8 && parts <= g.nx; ++parts) for (int p = 0; p < parts; ++p) (void)strip_plan(g, W * S, TO, p, parts);
        // the shards, the cells of every tile range that begins at tile 0 or ends at the last, and the pipelined parts of the frame under a few schedules
        std::vector<ShardPlan> plans;
        for (int parts = 1; parts <= 8; ++parts) (void)shard_plans(g, W * S, H * S, TO, parts, plans);
        Rect cells[3];
        for (int t = 0; t <= g.count; ++t) { (void)tile_range_cells(g, W * S, H * S, TO, TO, 0, t, cells); (void)tile_range_cells(g, W * S, H * S, TO, TO, t, g.count, cells); }
        if (g.count > 0)
            for (int steps : {1, 8}) for (int userB = 1; userB <= 4; ++userB) for (int want = 1; want <= kMaxRenderParts + 1; ++want) {
                const RenderParts rp = render_parts(g, strip_plan(g, W * S, TO, 0, 1), W, W * S, H * S, T, TO, steps, userB, 4 * userB, want);
                (void)last_pass_live(rp.part[rp.n - 1].tiles, steps, 4 * userB);
            }
        printf("ok: %d tiles (%d x %d)\n", g.count, g.nx, g.ny);
    } else if (mode == "parts") {
        if (argc < 9 || (argc - 9) % 4) throw std::runtime_error("parts W H T S TOUT OVX OVY [STEPS USERB B WANT]...");
        const int W = atoi(argv[2]), H = atoi(argv[3]), T = atoi(argv[4]), S = atoi(argv[5]), TO = atoi(argv[6]);
        const TileGrid g = calculate_tiles(W, H, W * S, H * S, T, T, TO, TO, S, atof(argv[7]), atof(argv[8]));
        if (g.count <= 0) throw std::runtime_error("parts: the tile grid is empty");
        auto rects = [](const Rect* r, int n) { std::string s; for (int k = 0; k < n; ++k) s += (k ? ";" : "") + std::to_string(r[k].x) + "," + std::to_string(r[k].y) + "," + std::to_string(r[k].w) + "," + std::to_string(r[k].h); return s.empty() ? std::string("-") : s; };
        printf("grid nx=%d ny=%d count=%d ovx=%d ovy=%d\n", g.nx, g.ny, g.count, g.outOvX, g.outOvY);
        for (int t = 0; t < g.count; ++t) printf("tile %d x=%d y=%d\n", t, g.in[t].x, g.in[t].y);
        for (int parts = 1; parts <= 8; ++parts) {
            std::vector<ShardPlan> plans;
            const bool all = shard_plans(g, W * S, H * S, TO, parts, plans);
            for (int p = 0; p < parts; ++p) {
                Rect cells[3];
                const int n = tile_range_cells(g, W * S, H * S, TO, TO, plans[p].first_tile, plans[p].first_tile + plans[p].tile_count, cells);
                printf("shard parts=%d part=%d owned=%d first=%d tiles=%d halo=%zu plan=%s cells=%s\n", parts, p, all ? 1 : 0, plans[p].first_tile, plans[p].tile_count, halo_slots(plans[p], 1),
                       rects(plans[p].rect, plans[p].nrect).c_str(), rects(cells, n).c_str());
            }
        }
        const StripPlan whole = strip_plan(g, W * S, TO, 0, 1);
        for (int a = 9; a + 3 < argc; a += 4) {
            const int steps = atoi(argv[a]), userB = atoi(argv[a + 1]), B = atoi(argv[a + 2]), want = atoi(argv[a + 3]);
            if ((steps != 1 && steps != 8) || userB <= 0 || B < userB || B > 4096) throw std::runtime_error("parts: STEPS is 1 or 8, 0 < USERB <= B <= 4096");
            const RenderParts rp = render_parts(g, whole, W, W * S, H * S, T, TO, steps, userB, B, want);
            printf("case steps=%d userB=%d B=%d want=%d parts=%d batches=%d slots=%zu x_split=%d slab=%zu\n", steps, userB, B, want, rp.n, rp.batch_total, rp.slot_total, rp.x_split, rp.slab_slots);
            for (int k = 0; k < rp.n; ++k) {
                const RenderParts::Part& p = rp.part[k];
                printf("part %d first=%d tiles=%d batches=%d before=%d slots_off=%zu slots=%zu live=%d rects=%s\n", k, p.first, p.tiles, p.batches, p.batches_before, p.slots_off, p.slots,
                       last_pass_live(p.tiles, steps, B), rects(p.rect, p.nrect).c_str());
            }
        }
    } else if (mode == "bleed") {
        if (argc < 4) throw std::runtime_error("bleed FILE RADIUS");
        const cli::Bitmap b = cli::read_image(argv[2]);
        const int radius = atoi(argv[3]);
        if (b.bgr.size() != (size_t)b.rows * b.cols * 3) throw std::runtime_error("not an 8-bit image");
        // exact-size heap blocks with padded steps: a read or write past a row or the frame is a sanitizer report
        const size_t cs = (size_t)b.cols * 3 + 5, as = (size_t)b.cols + 3;
        std::vector<uint8_t> c(cs * b.rows), a(as * b.rows, 255), out(cs * b.rows, 0xEE);
        for (int y = 0; y < b.rows; ++y) {
            std::copy(b.bgr.begin() + (size_t)y * b.cols * 3, b.bgr.begin() + (size_t)(y + 1) * b.cols * 3, c.begin() + y * cs);
            if (!b.alpha.empty()) std::copy(b.alpha.begin() + (size_t)y * b.cols, b.alpha.begin() + (size_t)(y + 1) * b.cols, a.begin() + y * as);
        }
        if (!alpha_bleed(c.data(), cs, a.data(), as, b.rows, b.cols, radius, out.data(), cs)) throw std::runtime_error("alpha_bleed refused " + std::to_string(b.cols) + "x" + std::to_string(b.rows) + " at radius " + std::to_string(radius));
        size_t changed = 0;
        for (int y = 0; y < b.rows; ++y) {
            for (size_t x = 0; x < (size_t)b.cols * 3; ++x) changed += out[y * cs + x] != c[y * cs + x];
            for (size_t x = (size_t)b.cols * 3; x < cs; ++x) if (out[y * cs + x] != 0xEE) throw std::runtime_error("alpha_bleed wrote into the row padding");
        }
        printf("ok: %d x %d at radius %d, %zu bytes changed\n", b.cols, b.rows, radius, changed);
    } else if (mode == "planes") {
        if (argc < 8) throw std::runtime_error("planes BITS ROWS COLS RADIUS SEED OUT");
        const int bits = atoi(argv[2]), rows = atoi(argv[3]), cols = atoi(argv[4]), radius = atoi(argv[5]);
        if (!(bits == 8 || bits == 10 || bits == 12 || bits == 16) || rows <= 0 || cols <= 0 || rows > 4096 || cols > 4096) throw std::runtime_error("planes: BITS in {8,10,12,16}, a frame of at most 4096 x 4096");
        const int bps = bits > 8 ? 2 : 1;
        const unsigned maxcode = (1u << bits) - 1u;
        // exact-size heap blocks, every plane with a padded step of its own: a read or write past a row or a plane is a sanitizer report.  The samples: a
        // 64-bit LCG; about half the alpha plane zero; at 10 and 12 bits some codes above the depth
        uint64_t state = (uint64_t)atoll(argv[6]) * 2862933555777941757ull + 3037000493ull;
        auto next = [&] { state = state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(state >> 33); };
        std::vector<std::vector<uint8_t>> in(4), out(3);
        size_t steps[4], osteps[3];
        auto put = [&](std::vector<uint8_t>& v, size_t step, int y, int x, unsigned code) { if (bps == 1) v[y * step + x] = (uint8_t)code; else { v[y * step + 2 * x] = (uint8_t)code; v[y * step + 2 * x + 1] = (uint8_t)(code >> 8); } };
        auto get = [&](const std::vector<uint8_t>& v, size_t step, int y, int x) { return bps == 1 ? (unsigned)v[y * step + x] : (unsigned)v[y * step + 2 * x] | (unsigned)v[y * step + 2 * x + 1] << 8; };
        for (int k = 0; k < 4; ++k) {
            steps[k] = (size_t)(cols + k + 1) * bps;
            in[k].assign(steps[k] * rows, 0xEE);
            for (int y = 0; y < rows; ++y)
                for (int x = 0; x < cols; ++x) {
                    unsigned code = next() % ((bps == 1 ? 256u : bits == 16 ? 65536u : maxcode + 1u + maxcode / 8u));
                    if (k == 3 && (next() & 1u)) code = 0;
                    put(in[k], steps[k], y, x, code);
                }
        }
        for (int k = 0; k < 3; ++k) { osteps[k] = (size_t)(cols + 2 * k + 2) * bps; out[k].assign(osteps[k] * rows, 0xEE); }
        const void* cp[3] = {in[0].data(), in[1].data(), in[2].data()};
        void* op[3] = {out[0].data(), out[1].data(), out[2].data()};
        if (!alpha_bleed_planes(cp, steps, in[3].data(), steps[3], rows, cols, bps, maxcode, radius, op, osteps)) throw std::runtime_error("alpha_bleed_planes refused the frame");
        for (int k = 0; k < 3; ++k)
            for (int y = 0; y < rows; ++y)
                for (size_t x = (size_t)cols * bps; x < osteps[k]; ++x) if (out[k][y * osteps[k] + x] != 0xEE) throw std::runtime_error("alpha_bleed_planes wrote into the row padding");
        std::ofstream f(argv[7], std::ios::binary);
        if (!f.is_open()) throw std::runtime_error("could not open the output file");
        size_t changed = 0;
        for (int k = 0; k < 7; ++k)
            for (int y = 0; y < rows; ++y)
                for (int x = 0; x < cols; ++x) {
                    const unsigned code = k < 4 ? get(in[k], steps[k], y, x) : get(out[k - 4], osteps[k - 4], y, x);
                    if (k >= 4) changed += code != std::min(get(in[k - 4], steps[k - 4], y, x), maxcode);
                    const char b[2] = {(char)code, (char)(code >> 8)};
                    f.write(b, bps);
                }
        printf("ok: %d x %d of %d bits at radius %d, %zu samples changed\n", cols, rows, bits, radius, changed);
    } else if (mode == "schedule") {
        if (argc < 6) throw std::runtime_error("schedule FILE BATCH TILE {fp16|tf32|fp32} [switch=value ...]");
        const int batch = atoi(argv[3]), tile = atoi(argv[4]);
        const std::string word = argv[5];
        if (word != "fp16" && word != "tf32" && word != "fp32") throw std::runtime_error("schedule: precision " + word + " is none of fp16, tf32, fp32");
        const Precision prec = word == "fp16" ? Precision::FP16 : word == "tf32" ? Precision::TF32 : Precision::FP32;
        for (int k = 6; k < argc; ++k) {
            const std::string a = argv[k];
            const size_t eq = a.find('=');
            if (eq == std::string::npos || !set_switch(a.substr(0, eq).c_str(), atol(a.c_str() + eq + 1))) throw std::runtime_error("schedule: no switch " + a.substr(0, eq));
        }
        const Plan plan = lower_for_shape(argv[2], batch, 3, tile, tile, prec != Precision::FP16);
        const std::vector<Launch> ls = candidate_launches(plan, prec, switches().check_general);
        const Lifetimes lt = lifetimes(plan, ls);
        const ArenaLayout lay = layout_arena(plan, ls);
        static const char* const kOp[] = {"gemm", "attn", "se", "scale_add", "mlp", "swinattn"};
        static const char* const kLaunch[] = {"op", "head", "stem", "up", "mlp32", "attn32"};
        auto ids = [](const auto& v) { std::string s; for (int t : v) if (t >= 0) s += (s.empty() ? "" : ",") + std::to_string(t); return s.empty() ? std::string("-") : s; };
        printf("plan ops=%zu tensors=%zu B=%d userB=%d in=%d out=%d\n", plan.ops.size(), plan.tensors.size(), plan.B, plan.userB, plan.in_tensor, plan.out_tensor);
        for (size_t i = 0; i < plan.ops.size(); ++i) {
            const Op& op = plan.ops[i];
            const TensorUse u = tensor_use(op);
            printf("op %zu kind=%s rd=%s wr=%s name=%s\n", i, op.kind >= 0 && op.kind < 6 ? kOp[op.kind] : "?", ids(u.rd).c_str(), ids(u.wr).c_str(), op.name.c_str());
        }
        for (const Launch& L : ls) printf("launch kind=%s first=%d last=%d timed=%d family=%d label=%s\n", kLaunch[L.kind], L.first, L.last, L.timed, L.family, launch_label(plan, L).c_str());
        for (size_t t = 0; t < plan.tensors.size(); ++t)
            printf("tensor %zu bytes=%lld first=%d last=%d placed=%d off=%zu\n", t, (long long)plan.tensors[t].bytes(), lt.first[t], lt.last[t], lay.placed[t] ? 1 : 0, lay.off[t]);
        printf("arena bytes=%zu part2=%zu part3=%zu part4=%zu\n", lay.bytes, arena_part_bytes(lay.bytes, 2), arena_part_bytes(lay.bytes, 3), arena_part_bytes(lay.bytes, 4));
    } else if (mode == "dither") {
        const std::string what = argv[2];
        if (what == "table") {
            const uint16_t* t = dither_table();
            for (int y = 0; y < kDitherSide; ++y) { for (int x = 0; x < kDitherSide; ++x) printf(x ? " %d" : "%d", (int)t[y * kDitherSide + x]); printf("\n"); }
            return 0;
        }
        if (argc < 9) throw std::runtime_error("dither {ordered|bluenoise} PHASE PLANE X0 Y0 W H  |  dither table");
        int m = kDitherNone;
        if (!dither_parse_mode(what.c_str(), m) || m == kDitherNone) throw std::runtime_error("dither: mode " + what + " is none of ordered, bluenoise");
        const unsigned phase = (unsigned)strtoul(argv[3], nullptr, 10);
        const int c = atoi(argv[4]), x0 = atoi(argv[5]), y0 = atoi(argv[6]), w = atoi(argv[7]), h = atoi(argv[8]);
        if (argc > 9 || c < 0 || c > 2 || x0 < 0 || y0 < 0 || w <= 0 || h <= 0 || w > 4096 || h > 4096) throw std::runtime_error("dither: PLANE in 0..2, a window of at most 4096 x 4096 at a non-negative origin");
        std::vector<int> ranks((size_t)w * h);                           // (an exact-size heap block: an index past the window is a sanitizer report)
        for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) ranks[(size_t)y * w + x] = dither_rank(m, phase, c, x0 + x, y0 + y);
        for (int y = 0; y < h; ++y) { for (int x = 0; x < w; ++x) printf(x ? " %d" : "%d", ranks[(size_t)y * w + x]); printf("\n"); }
        printf("thresholds\n");
        for (int y = 0; y < h; ++y) { for (int x = 0; x < w; ++x) printf(x ? " %.17g" : "%.17g", (double)dither_threshold(m, phase, c, x0 + x, y0 + y)); printf("\n"); }
    } else throw std::runtime_error("unknown mode " + mode);
    return 0;
}

int main(int argc, char** argv) {
    try { return run(argc, argv); }
    catch (const std::exception& e) { fprintf(stderr, "rejected: %s\n", e.what()); return 2; }
}
