#include "liveness.h"

#include <algorithm>

namespace w2x {

namespace {

using Axis = std::vector<char>;

Axis expand(const AxisExt& e) {
    Axis a(e.n, 0);
    for (int i = 0; i < e.n; ++i) a[i] = i < e.c || i >= e.n - e.w;
    return a;
}
// the form [0, c) U [n - w, n) of a set, or the whole axis when the set is not of that form
AxisExt to_ext(const Axis& a) {
    const int n = (int)a.size();
    AxisExt e; e.n = n;
    while (e.c < n && a[e.c]) ++e.c;
    if (e.c == n) return e;
    while (e.w < n - e.c && a[n - 1 - e.w]) ++e.w;
    for (int i = e.c; i < n - e.w; ++i) if (a[i]) { e.c = n; e.w = 0; break; }
    return e;
}
int count(const AxisExt& e) { return e.c >= e.n ? e.n : e.c + e.w; }
// window k of an axis under roll r holds tokens (ws k + j + r) % n: live when its first token is (sets of attention ops are whole windows)
int live_windows(const AxisExt& e, int r, int ws) {
    int k = 0;
    for (int i = 0; i < e.n / ws; ++i) { const int t = (ws * i + r) % e.n; k += t < e.c || t >= e.n - e.w; }
    return k;
}
void unite(Axis& into, const Axis& a) {
    if (into.empty()) { into = a; return; }
    for (size_t i = 0; i < into.size() && i < a.size(); ++i) into[i] |= a[i];
}

struct Unsupported {};

}  // namespace

long OpExtent::live_units() const { return ws > 0 ? (long)live_windows(x, rx, ws) * live_windows(y, ry, ws) : (long)count(x) * count(y); }
long OpExtent::total_units() const { return ws > 0 ? (long)(x.n / ws) * (y.n / ws) : (long)x.n * y.n; }

std::vector<OpExtent> dead_skip_extents(const Plan& plan, int kept_w, int kept_h, bool force_all) {
    const int nops = (int)plan.ops.size(), nt = (int)plan.tensors.size();
    std::vector<OpExtent> ext(nops);
    // the row map of every op (also what "all" reports)
    auto row_map = [&](const Op& op, int& W, int& H) {
        W = H = 0;
        if (op.kind == OP_GEMM) { W = op.g.aW; H = op.g.aW > 0 ? op.g.Mrows / op.g.aW : 0; }
        else if (op.kind == OP_MLP && op.m.x >= 0 && op.m.x < nt) { W = plan.tensors[op.m.x].W; H = plan.tensors[op.m.x].H; }
        else if (op.kind == OP_SWINATTN) { W = op.sa.W; H = op.sa.H; }
    };
    auto set_all = [&] {
        for (int i = 0; i < nops; ++i) {
            int W, H; row_map(plan.ops[i], W, H);
            OpExtent e; e.x = AxisExt{W, W, 0}; e.y = AxisExt{H, H, 0};
            if (plan.ops[i].kind == OP_SWINATTN) { e.ry = plan.ops[i].sa.ry; e.rx = plan.ops[i].sa.rx; e.ws = plan.ops[i].sa.ws; }
            ext[i] = e;
        }
    };
    set_all();
    if (force_all || nops == 0 || plan.elt != 2 || plan.out_tensor < 0 || plan.out_tensor >= nt) return ext;
    if (kept_w >= plan.Tout && kept_h >= plan.Tout) return ext;
    if (kept_w <= 0 || kept_h <= 0) return ext;
    try {
        std::vector<Axis> nx(nt), ny(nt);      // per tensor: the pixels its readers need (empty: none yet), over the stored map
        auto whole = [&](const View& v) { if (v.t < 0 || v.t >= nt) throw Unsupported{}; const TensorDesc& d = plan.tensors[v.t]; return v.y0 == 0 && v.x0 == 0 && v.H == d.H && v.W == d.W; };
        auto need = [&](int t, const Axis& ax, const Axis& ay) {
            if (t < 0 || t >= nt || (int)ax.size() != plan.tensors[t].W || (int)ay.size() != plan.tensors[t].H) throw Unsupported{};
            unite(nx[t], ax); unite(ny[t], ay);
        };
        {
            const TensorDesc& d = plan.tensors[plan.out_tensor];
            if (d.W != plan.Tout || d.H != plan.Tout) throw Unsupported{};
            Axis ax(d.W, 0), ay(d.H, 0);
            for (int i = 0; i < std::min(kept_w, d.W); ++i) ax[i] = 1;
            for (int i = 0; i < std::min(kept_h, d.H); ++i) ay[i] = 1;
            need(plan.out_tensor, ax, ay);
        }
        for (int i = nops - 1; i >= 0; --i) {
            const Op& op = plan.ops[i];
            int W, H; row_map(op, W, H);
            if (W <= 0 || H <= 0) throw Unsupported{};
            OpExtent e; Axis rx_, ry_;
            if (op.kind == OP_GEMM) {
                const GemmOp& g = op.g;
                if (g.ln || g.stats_in >= 0 || g.stats_out >= 0 || g.pool_out >= 0 || g.se_scale >= 0 || g.res_scale >= 0 || g.res2.t >= 0 || g.amode == A_WIN || g.omode == O_WIN ||
                    (long)W * H != g.Mrows || !whole(g.out)) throw Unsupported{};
                const int r = g.omode == O_PIXSHUF ? g.r : 1;
                if (r < 1 || g.out.W != W * r || g.out.H != H * r) throw Unsupported{};
                const Axis& ox = nx[g.out.t]; const Axis& oy = ny[g.out.t];
                if (ox.empty() || oy.empty()) throw Unsupported{};            // an op nobody reads
                rx_.assign(W, 0); ry_.assign(H, 0);
                for (int k = 0; k < W * r; ++k) if (ox[k]) rx_[k / r] = 1;
                for (int k = 0; k < H * r; ++k) if (oy[k]) ry_[k / r] = 1;
                e.x = to_ext(rx_); e.y = to_ext(ry_);
                rx_ = expand(e.x); ry_ = expand(e.y);
                if (g.res.t >= 0) {      // the residual has the output's geometry: the output pixels of the live rows
                    if (!whole(g.res) || g.res.W != W * r || g.res.H != H * r) throw Unsupported{};
                    Axis ax(W * r), ay(H * r);
                    for (int k = 0; k < W * r; ++k) ax[k] = rx_[k / r];
                    for (int k = 0; k < H * r; ++k) ay[k] = ry_[k / r];
                    need(g.res.t, ax, ay);
                }
                // the A side: row x reads pixels s x .. s x + k - 1 of its view (rows: s = k = 1), the view sits at (x0, y0) of the stored map
                const int s = g.amode == A_CONV ? g.stride : 1, kw = g.amode == A_CONV ? g.kw : 1, kh = g.amode == A_CONV ? g.kh : 1;
                if (g.a.t < 0 || g.a.t >= nt || s < 1 || kw < 1 || kh < 1) throw Unsupported{};
                const TensorDesc& d = plan.tensors[g.a.t];
                if (g.a.x0 < 0 || g.a.y0 < 0 || g.a.x0 + (W - 1) * s + kw > d.W || g.a.y0 + (H - 1) * s + kh > d.H) throw Unsupported{};   // (a valid convolution: every tap inside the map)
                Axis ax(d.W, 0), ay(d.H, 0);
                for (int k = 0; k < W; ++k) if (rx_[k]) for (int j = 0; j < kw; ++j) ax[g.a.x0 + s * k + j] = 1;
                for (int k = 0; k < H; ++k) if (ry_[k]) for (int j = 0; j < kh; ++j) ay[g.a.y0 + s * k + j] = 1;
                need(g.a.t, ax, ay);
            } else if (op.kind == OP_MLP) {
                const MlpOp& m = op.m;
                if (m.stats_out >= 0 || m.y < 0 || m.y >= nt || plan.tensors[m.y].W != W || plan.tensors[m.y].H != H || nx[m.y].empty()) throw Unsupported{};
                e.x = to_ext(nx[m.y]); e.y = to_ext(ny[m.y]);
                need(m.x, expand(e.x), expand(e.y));
            } else if (op.kind == OP_SWINATTN) {
                const SwinAttnOp& a = op.sa;
                if (a.stats_out >= 0 || a.ry < 0 || a.rx < 0 || a.ws <= 0 || W % a.ws || H % a.ws || a.y < 0 || a.y >= nt || plan.tensors[a.y].W != W || plan.tensors[a.y].H != H ||
                    a.x < 0 || a.x >= nt || plan.tensors[a.x].W != W || plan.tensors[a.x].H != H || nx[a.y].empty()) throw Unsupported{};
                auto windows = [&](const Axis& o, int n, int roll) {
                    Axis out(n, 0);
                    for (int k = 0; k < n / a.ws; ++k) {
                        bool any = false;
                        for (int j = 0; j < a.ws; ++j) any = any || o[(a.ws * k + j + roll) % n];
                        if (any) for (int j = 0; j < a.ws; ++j) out[(a.ws * k + j + roll) % n] = 1;
                    }
                    return out;
                };
                e.x = to_ext(windows(nx[a.y], W, a.rx)); e.y = to_ext(windows(ny[a.y], H, a.ry));
                // (an axis that fell back to "all" is still a union of whole windows)
                e.ry = a.ry; e.rx = a.rx; e.ws = a.ws;
                need(a.x, expand(e.x), expand(e.y));
            } else throw Unsupported{};
            ext[i] = e;
        }
    } catch (const Unsupported&) {
        set_all();
    }
    return ext;
}

}  // namespace w2x
