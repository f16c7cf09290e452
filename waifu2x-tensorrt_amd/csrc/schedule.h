// The pass schedule of a loaded plan: which ops one launch computes, every tensor's lifetime under those launches, and where the activation arena puts it.
// Facts of the plan, the load's switches and its precision alone - no HIP types, no device pointers: like support.h and liveness.h this builds with a plain host
// compiler for the sanitizer target (`make asan`), where w2x_parse_check's `schedule` mode prints it and tests/test_schedule_host.py states its invariants.
// The engine (engine.cpp upload_plan) asks for the candidates and the layout, allocates, and confirms or splits each candidate with its prepared launch parameters.
#pragma once
#include <array>
#include <cstddef>
#include <string>
#include <vector>

#include "../../include/w2x/config.h"
#include "plan.h"

namespace w2x {

// Lowering of a model for one input shape, shared by build() (which writes the result to disk) and by load() when the render
// configuration lies inside an engine's [min, max] range but is not the shape that engine was specialised for.
// Super-batching: tiles are independent, so one network pass may carry several reference batches (S x batchSize tiles); results
// are bit-identical, launches per frame drop S-fold and the low-resolution stages fill all 256 CUs.  W2X_SUPERBATCH (switches.h) overrides;
// the default targets the pixel count of 48 tiles of 256x256 per pass (one 1080p frame at config 3), capped at 64 tiles.  Small
// tiles gain the most: at tile 64 / batch 1 a pass of one tile is ~40 launches of a few microseconds of work each (a 1080p frame:
// 1100 passes, 650 ms, hipGraph replay or not); 64 tiles per pass make it 18 passes.
Plan lower_for_shape(const std::string& onnxModelPath, int batch, int channels, int height, int width, bool fp32);

// The launches of one network pass, decided once per load() (engine.cpp upload_plan) and walked by run_network().  A fold computes several neighbouring plan ops
// in one launch; the map between them is neither stored nor read:
//  head   - a C = 96 MLP and the image head behind it (k_mlp96q.hip)
//  stem   - a stem convolution and the 3x3 convolution behind it, which computes the 48- / 32-channel map in its halo stage (k_conv48.hip; k_conv3.hip for cunet)
//  up     - cunet's pixel-shuffle projection (ConvTranspose) and the 64 -> 64 3x3 convolution behind it, which computes it in its halo stage (k_conv3.hip UP)
//  mlp32  - fp32 plans at Precision::TF32: LayerNorm + fc1 + GELU and fc2 + residual (k_f32.hip mlp32_kernel)
//  attn32 - the same: LayerNorm + window gather + qkv, attention core, proj + window scatter + residual (k_f32.hip swinattn32_kernel)
enum LaunchKind { L_OP, L_HEAD, L_STEM, L_UP, L_MLP32, L_ATTN32 };
struct Launch {
    LaunchKind kind = L_OP;
    int first = 0, last = 0;      // the plan ops it computes
    int timed = 0;                // the op whose op_ms slot receives its time (profileFrame / opTimes)
    double flops = 0;
    int family = 0;               // profileFrame's kernel family (stamp_begin)
};

// The tensors an op reads and writes: the one table behind the arena's lifetimes and the fold tests
struct TensorUse { std::array<int, 6> rd; std::array<int, 3> wr; };
TensorUse tensor_use(const Op& op);
// Every tensor's lifetime [first op, last op] when the pass runs as the launches `ls`: everything a launch touches is live across the whole launch (a fold
// writes its last op's outputs while other workgroups still read its first op's inputs).  The input is written before op 0 (gather), the output read after the last op.
struct Lifetimes { std::vector<int> first, last; };
Lifetimes lifetimes(const Plan& plan, const std::vector<Launch>& ls);
// t is op i's output and only op i + 1 reads it (over the plan's own lifetimes: no other op touches it, and it is not the pass's output)
bool passes_on(const Lifetimes& lt, int t, int i);
Launch make_launch(const Plan& plan, LaunchKind kind, int first, int last);

// The candidate launches of a pass: the folds that plan facts, the load's switches and its precision allow.  The engine lays the arena out for them and then
// confirms or splits each with the prepared launch parameters.  No op but a launch's last may write the pass's output (out_override replaces the last op's).
std::vector<Launch> candidate_launches(const Plan& plan, Precision prec, bool check_general);
// "12 [name]", or "12-13 [name + name]" for a fold: the roctx range and the error messages of a launch
std::string launch_label(const Plan& plan, const Launch& L);

// Activation arena: tensors whose lifetimes (first writer .. last reader, in op order) do not overlap share
// memory.  An op's outputs are placed before its inputs are released, so no op reads and writes one address.
// With the lifetimes of the candidate launches, a candidate that the engine splits back into its ops keeps a layout that covers what they need.
struct ArenaLayout {
    std::vector<size_t> off;      // per tensor id: byte offset in the arena (0 where not placed)
    std::vector<char> placed;     // per tensor id: non-zero when some op touches it
    size_t bytes = 0;             // the arena's size
};
ArenaLayout layout_arena(const Plan& plan, const std::vector<Launch>& ls);

// A pass cut into NG tile groups gives each group its own PART of the arena, laid out like the whole one at 1/NG of the size: a tensor of B tiles at offset o
// becomes B/NG tiles at o/NG inside part grp (offsets are multiples of 3072 bytes = 256 x 12, so they stay 256-byte aligned for NG = 2, 3, 4).
inline size_t arena_part_bytes(size_t arena_bytes, int ng) { return ((arena_bytes / ng) + 255) / 256 * 256; }
inline size_t arena_group_offset(size_t arena_bytes, int ng, int grp, size_t off) { return (size_t)grp * arena_part_bytes(arena_bytes, ng) + off / ng; }

}  // namespace w2x
