#include "schedule.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

#include "lower.h"
#include "support.h"
#include "switches.h"

namespace w2x {

Plan lower_for_shape(const std::string& onnxModelPath, int batch, int channels, int height, int width, bool fp32) {
    int S = 1;
    if (switches().superbatch > 0) S = switches().superbatch;
    else {
        const double want = 48.0 * 256 * 256 / ((double)batch * height * width);
        S = std::max(1, (int)std::lround(want));
        while (S > 1 && S * batch > 64) --S;
    }
    Plan plan;
    try {
        plan = build_plan(onnxModelPath, batch * S, channels, height, width, fp32);
    } catch (const std::exception&) {
        if (S == 1) throw;
        plan = build_plan(onnxModelPath, batch, channels, height, width, fp32);   // e.g. a graph with a static batch dimension
    }
    plan.userB = batch;
    return plan;
}

TensorUse tensor_use(const Op& op) {
    TensorUse u; u.rd.fill(-1); u.wr.fill(-1);
    switch (op.kind) {
        case OP_GEMM: u.rd = {{op.g.a.t, op.g.res.t, op.g.res2.t, op.g.stats_in, op.g.se_scale, op.g.res_scale}}; u.wr = {{op.g.out.t, op.g.stats_out, op.g.pool_out}}; break;
        case OP_ATTN: u.rd[0] = op.at.qkv; u.wr[0] = op.at.out; break;
        case OP_SE: u.rd[0] = op.se.pool; u.wr[0] = op.se.scale; break;
        case OP_SCALE_ADD: u.rd = {{op.se.pool, op.se.scale, -1, -1, -1, -1}}; u.wr[0] = op.se.pool; break;      // (in place)
        case OP_MLP: u.rd[0] = op.m.x; u.wr = {{op.m.y, op.m.stats_out, -1}}; break;
        case OP_SWINATTN: u.rd[0] = op.sa.x; u.wr = {{op.sa.y, op.sa.stats_out, -1}}; break;
        default: break;
    }
    return u;
}

Lifetimes lifetimes(const Plan& plan, const std::vector<Launch>& ls) {
    const int nops = (int)plan.ops.size();
    Lifetimes lt{std::vector<int>(plan.tensors.size(), nops), std::vector<int>(plan.tensors.size(), -1)};
    for (const Launch& L : ls)
        for (int i = L.first; i <= L.last; ++i) {
            const TensorUse u = tensor_use(plan.ops[i]);
            auto touch = [&](int t) { if (t >= 0) { lt.first[t] = std::min(lt.first[t], L.first); lt.last[t] = std::max(lt.last[t], L.last); } };
            for (int t : u.rd) touch(t);
            for (int t : u.wr) touch(t);
        }
    lt.first[plan.in_tensor] = -1;
    lt.last[plan.out_tensor] = nops;
    return lt;
}

bool passes_on(const Lifetimes& lt, int t, int i) { return t >= 0 && lt.first[t] == i && lt.last[t] == i + 1; }

Launch make_launch(const Plan& plan, LaunchKind kind, int first, int last) {
    static constexpr int kFamily[] = {0, 1, 2, 2, 5, 1};   // per OpKind: gemm, attention, se / scale, fused mlp (profileFrame's out[5 * k])
    Launch L; L.kind = kind; L.first = first; L.last = last;
    L.timed = kind == L_STEM || kind == L_UP ? first + 1 : first;     // (the convolution's launch computes the op in front of it)
    const int k = plan.ops[first].kind;
    L.family = kind == L_ATTN32 ? 1 : k >= 0 && k < 6 ? kFamily[k] : 0;
    if (L.family != 2) for (int i = first; i <= last; ++i) L.flops += plan.ops[i].flops;   // (squeeze-excite launches are not priced)
    return L;
}

namespace {

// fp32 plans, Precision::TF32: which runs of un-fused ops one fused launch of k_f32.hip serves.  Facts of the plan alone (lower.cpp's fuse_mlp() / fuse_attn() state
// the same patterns for the fp16 plan); the plan itself stays un-fused - one lowering serves TF32 and FP32, and Precision::FP32 runs every launch.
bool whole_view(const Plan& plan, const View& v) { if (v.t < 0) return false; const TensorDesc& t = plan.tensors[v.t]; return v.y0 == 0 && v.x0 == 0 && v.H == t.H && v.W == t.W; }
bool mlp32_pair(const Plan& plan, size_t i, const Lifetimes& lt) {
    if (plan.elt != 4 || switches().no_fuse || i + 1 >= plan.ops.size() || plan.ops[i].kind != OP_GEMM || plan.ops[i + 1].kind != OP_GEMM) return false;
    const GemmOp& g1 = plan.ops[i].g; const GemmOp& g2 = plan.ops[i + 1].g;
    const int Cm = g1.K;
    auto whole_view = [&](const View& v) { return w2x::whole_view(plan, v); };
    return mlp32_supported(Cm) && g1.amode == A_ROWS && g1.ln && g1.stats_in >= 0 && g1.act == ACT_GELU && g1.omode == O_ROWS && g1.res.t < 0 && g1.res2.t < 0 && !g1.has_clip &&
           g1.N == 2 * Cm && g1.stats_out < 0 && g1.pool_out < 0 && g1.se_scale < 0 && whole_view(g1.a) && whole_view(g1.out) && plan.tensors[g1.a.t].C == Cm && plan.tensors[g1.out.t].C == 2 * Cm &&
           g1.Mrows == plan.tensors[g1.a.t].H * plan.tensors[g1.a.t].W &&
           g2.amode == A_ROWS && !g2.ln && g2.act == ACT_NONE && g2.omode == O_ROWS && g2.a.t == g1.out.t && g2.K == 2 * Cm && g2.N == Cm && g2.res.t == g1.a.t && g2.res2.t < 0 &&
           !g2.has_clip && g2.pool_out < 0 && g2.se_scale < 0 && g2.res_scale < 0 && whole_view(g2.a) && whole_view(g2.res) && whole_view(g2.out) && plan.tensors[g2.out.t].C == Cm && g2.Mrows == g1.Mrows &&
           passes_on(lt, g1.out.t, (int)i) &&
           plan.blobs[g1.w].data.size() == (size_t)2 * Cm * Cm * 4 && plan.blobs[g2.w].data.size() == (size_t)2 * Cm * Cm * 4;      // fp32 [2C][C] and [C][2C], rows unpadded
}
bool attn32_triple(const Plan& plan, size_t i, const Lifetimes& lt) {
    if (plan.elt != 4 || switches().no_fuse || switches().no_fuse_attn || i + 2 >= plan.ops.size() || plan.ops[i].kind != OP_GEMM || plan.ops[i + 1].kind != OP_ATTN || plan.ops[i + 2].kind != OP_GEMM) return false;
    const GemmOp& g1 = plan.ops[i].g; const AttnOp& a = plan.ops[i + 1].at; const GemmOp& g2 = plan.ops[i + 2].g;
    const int Cm = g1.K;
    auto whole_view = [&](const View& v) { return w2x::whole_view(plan, v); };
    return swinattn32_supported(Cm, a.heads, a.hd, a.ws * a.ws) && a.heads * a.hd == Cm &&
           g1.amode == A_WIN && g1.win_table >= 0 && g1.ln && g1.stats_in >= 0 && g1.act == ACT_NONE && g1.omode == O_ROWS && g1.res.t < 0 && g1.res2.t < 0 && !g1.has_clip && g1.N == 3 * Cm &&
           g1.stats_out < 0 && g1.pool_out < 0 && g1.se_scale < 0 && whole_view(g1.a) && whole_view(g1.out) && plan.tensors[g1.a.t].C == Cm && plan.tensors[g1.out.t].C == 3 * Cm &&
           g1.Mrows == a.nwin * a.ws * a.ws && g1.Mrows == plan.tensors[g1.a.t].H * plan.tensors[g1.a.t].W &&
           a.qkv == g1.out.t && a.bias >= 0 && a.maskid >= 0 &&
           g2.amode == A_ROWS && g2.a.t == a.out && !g2.ln && g2.act == ACT_NONE && g2.omode == O_WIN && g2.win_table >= 0 && g2.K == Cm && g2.N == Cm && g2.res.t == g1.a.t && g2.res2.t < 0 &&
           !g2.has_clip && g2.pool_out < 0 && g2.se_scale < 0 && g2.res_scale < 0 && whole_view(g2.a) && whole_view(g2.res) && whole_view(g2.out) && plan.tensors[g2.out.t].C == Cm &&
           plan.tensors[g2.out.t].H * plan.tensors[g2.out.t].W == g1.Mrows && g2.Mrows == g1.Mrows &&
           passes_on(lt, g1.out.t, (int)i) && passes_on(lt, a.out, (int)i + 1) &&
           plan.blobs[g1.w].data.size() == (size_t)3 * Cm * Cm * 4 && plan.blobs[g2.w].data.size() == (size_t)Cm * Cm * 4;
}

}  // namespace

std::vector<Launch> candidate_launches(const Plan& plan, Precision prec, bool check_general) {
    const int nops = (int)plan.ops.size();
    std::vector<Launch> ls;
    for (int i = 0; i < nops; ++i) ls.push_back(make_launch(plan, L_OP, i, i));
    const Lifetimes lt = lifetimes(plan, ls);
    ls.clear();
    const bool fp16 = plan.elt == 2 && !check_general, tf32 = plan.elt == 4 && prec == Precision::TF32;   // (W2X_CHECK_GENERAL compares every shape-specialised launch alone)
    // the image head (Linear 96 -> 4x4 sub-pixels x 4 channels) behind a C = 96 MLP: it rides on k_mlp96q.hip's launch only
    auto head = [&](const Op& a, const Op& b, int i) {
        return !switches().no_fuse_head && mlp_frag32(96) && a.kind == OP_MLP && b.kind == OP_GEMM && a.m.C == 96 && a.m.stats_out < 0 && b.g.a.t == a.m.y && passes_on(lt, a.m.y, i) &&
               b.g.amode == A_ROWS && b.g.K == 96 && b.g.N == 64 && b.g.r == 4 && b.g.omode == O_PIXSHUF && b.g.res.t < 0 && b.g.res2.t < 0 && b.g.act == ACT_NONE && !b.g.ln &&
               b.g.se_scale < 0 && b.g.res_scale < 0 && b.g.stats_out < 0 && b.g.pool_out < 0;
    };
    // the stem (3x3, 4 -> 48 / 32 channels) in front of the 3x3 convolution that alone reads it
    auto stem = [&](const Op& a, const Op& b, int i) {
        return a.kind == OP_GEMM && b.kind == OP_GEMM && a.g.a.t >= 0 && plan.tensors[a.g.a.t].C == 4 && ((a.g.N == 48 && b.g.K == 9 * 48) || (a.g.N == 32 && b.g.K == 9 * 32 && b.g.N == 64 && b.g.pool_out < 0)) &&
               b.g.a.t == a.g.out.t && passes_on(lt, a.g.out.t, i) && a.g.stats_out < 0 && a.g.pool_out < 0;
    };
    // cunet's ConvTranspose 2x2 stride 2 (a pixel-shuffle projection with a skip add) in front of the 64 -> 64 3x3 convolution that alone reads it
    auto up = [&](const Op& a, const Op& b, int i) {
        return a.kind == OP_GEMM && b.kind == OP_GEMM && a.g.omode == O_PIXSHUF && a.g.r == 2 && a.g.K == 64 && a.g.N == 256 && a.g.res.t >= 0 && a.g.res2.t < 0 && a.g.res_scale < 0 && !a.g.ln &&
               a.g.stats_out < 0 && a.g.pool_out < 0 && b.g.amode == A_CONV && b.g.kh == 3 && b.g.kw == 3 && b.g.stride == 1 && b.g.K == 9 * 64 && b.g.N == 64 && b.g.pool_out < 0 &&
               b.g.a.t == a.g.out.t && passes_on(lt, a.g.out.t, i);
    };
    auto writes_output = [&](int j) { const auto wr = tensor_use(plan.ops[j]).wr; return std::find(wr.begin(), wr.end(), plan.out_tensor) != wr.end(); };
    for (int i = 0; i < nops;) {
        const Op& a = plan.ops[i]; const Op& b = plan.ops[std::min(i + 1, nops - 1)];
        LaunchKind k = tf32 && attn32_triple(plan, i, lt) ? L_ATTN32 : tf32 && mlp32_pair(plan, i, lt) ? L_MLP32 : i + 1 == nops || !fp16 ? L_OP :
                       head(a, b, i) ? L_HEAD : stem(a, b, i) ? L_STEM : up(a, b, i) ? L_UP : L_OP;
        int last = i + (k == L_OP ? 0 : k == L_ATTN32 ? 2 : 1);
        for (int j = i; j < last; ++j) if (writes_output(j)) { k = L_OP; last = i; }
        ls.push_back(make_launch(plan, k, i, last));
        i = last + 1;
    }
    return ls;
}

std::string launch_label(const Plan& plan, const Launch& L) {
    std::string m = std::to_string(L.first) + (L.last > L.first ? "-" + std::to_string(L.last) : "") + " [";
    for (int i = L.first; i <= L.last; ++i) m += (i > L.first ? " + " : "") + plan.ops[i].name;
    return m + "]";
}

ArenaLayout layout_arena(const Plan& plan, const std::vector<Launch>& ls) {
    const int nt = (int)plan.tensors.size(), nops = (int)plan.ops.size();
    const Lifetimes lt = lifetimes(plan, ls);
    const std::vector<int>& first = lt.first; const std::vector<int>& last = lt.last;
    struct Block { size_t off, size; };
    std::vector<Block> free_list;
    std::vector<size_t> off(nt, 0);
    size_t arena = 0;
    // 256 bytes x 12: offsets stay 256-byte aligned when the arena is cut into 2, 3 or 4 group parts (arena_group_offset).
    constexpr size_t unit = 3072;
    auto align = [](size_t v) { return (v + unit - 1) / unit * unit; };
    auto alloc = [&](size_t bytes) -> size_t {
        bytes = align(bytes);
        int best = -1;
        for (int k = 0; k < (int)free_list.size(); ++k) if (free_list[k].size >= bytes && (best < 0 || free_list[k].size < free_list[best].size)) best = k;
        if (best >= 0) { size_t o = free_list[best].off; free_list[best].off += bytes; free_list[best].size -= bytes; if (!free_list[best].size) free_list.erase(free_list.begin() + best); return o; }
        if (!free_list.empty()) {   // grow the last free block if it touches the end of the arena
            for (int k = 0; k < (int)free_list.size(); ++k) if (free_list[k].off + free_list[k].size == arena) { size_t o = free_list[k].off; arena = o + bytes; free_list.erase(free_list.begin() + k); return o; }
        }
        size_t o = arena; arena += bytes; return o;
    };
    auto release = [&](size_t o, size_t bytes) {
        bytes = align(bytes);
        free_list.push_back({o, bytes});
        std::sort(free_list.begin(), free_list.end(), [](const Block& a, const Block& b) { return a.off < b.off; });
        for (size_t k = 0; k + 1 < free_list.size();) { if (free_list[k].off + free_list[k].size == free_list[k + 1].off) { free_list[k].size += free_list[k + 1].size; free_list.erase(free_list.begin() + k + 1); } else ++k; }
    };
    std::vector<char> placed(nt, 0);
    for (int step = -1; step <= nops; ++step) {
        for (int t = 0; t < nt; ++t) if (!placed[t] && first[t] == step && last[t] >= 0) { off[t] = alloc((size_t)plan.tensors[t].bytes()); placed[t] = 1; }
        for (int t = 0; t < nt; ++t) if (placed[t] == 1 && last[t] == step) { release(off[t], (size_t)plan.tensors[t].bytes()); placed[t] = 2; }
    }
    // (tensors no op touches - the q / k / v, score and hidden maps inside the fused attention and MLP ops - get no memory: at config 3 they
    //  were 19 of the arena's 20.7 GiB until round 3)
    ArenaLayout lay;
    lay.off = std::move(off); lay.placed = std::move(placed); lay.bytes = arena;
    return lay;
}

}  // namespace w2x
