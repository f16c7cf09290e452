// w2x::Img2Img - the MI355X engine behind the reference's trt::Img2Img interface
// (/root/reference/src/tensorrt/img2img.h:14-50).  build(): ONNX -> plan file; load(): plan -> HBM; render(): frame ->
// tiles -> fused HIP kernels -> blended frame.  Everything on the device is HIP; there is no CPU fallback.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <filesystem>
#include <fstream>
#include <map>
#include <sstream>
#include <tuple>

#include "../../include/w2x/img2img.h"
#include "common.h"
#include "fragorder.h"
#include "kernels.h"
#include "liveness.h"
#include "lower.h"
#include "plan.h"
#include "schedule.h"
#include "sha256.h"
#include "switches.h"
#include "tiles.h"

#define W2X_LOG(sev, message) impl->log(sev, message, __FUNCTION__, __LINE__)
#define W2X_LOG_AS(who, sev, message) impl->log(sev, message, who, __LINE__)

namespace w2x {

namespace {

// helper.h:13-17 (cudaAssert): a failed runtime call becomes an exception carrying the runtime's message
inline void hipAssert(hipError_t e) {
    if (e != hipSuccess) throw std::runtime_error(hipGetErrorString(e));
}

// helper.h:27-46
std::string hipGetDeviceName(int deviceId) {
    hipDeviceProp_t prop{};
    hipAssert(hipGetDeviceProperties(&prop, deviceId));
    // The marketing name depends on which libdrm data file the process finds (empty or generic on some boxes, and different
    // between the ROCm runtime and the copy bundled with PyTorch); a plan is tied to the ISA and the CU count, so that is the key.
    std::string arch = prop.gcnArchName;
    return arch + " x" + std::to_string(prop.multiProcessorCount);
}

// Logical -> physical device ordinal.  W2X_DEVICE_MAP="0,0,1" makes logical devices 0 and 1 share physical device 0 (test hook:
// the multi-device code paths - one engine and one host thread per logical device - can then run on a single-GPU box).
int physical_device(int logical) {   // called by build() and load() only
    std::vector<int> map;
    if (const char* e = getenv("W2X_DEVICE_MAP")) { std::stringstream ss(e); std::string tok; while (std::getline(ss, tok, ',')) if (!tok.empty()) map.push_back(atoi(tok.c_str())); }
    return logical >= 0 && logical < (int)map.size() ? map[logical] : logical;
}

// One instance = one device (img2img_load.cpp:129 cudaSetDevice in load only).  The reference is driven from one thread; here
// several engines may live in one process, each on its own host thread, so every public entry that allocates, copies or launches
// makes the engine's device current for its own duration and restores the caller's on the way out.
struct DeviceGuard {
    int prev = -1, dev = -1;
    explicit DeviceGuard(int d) : dev(d) {
        if (d < 0) return;
        if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
        if (prev != d) hipAssert(hipSetDevice(d));
    }
    ~DeviceGuard() { if (dev >= 0 && prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// "" when `physical` is a device of this process, else the sentence build() / load() log (a raw "invalid device ordinal" names neither the
// count nor the map that produced the ordinal)
std::string device_ordinal_problem(int logical, int physical) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) { (void)hipGetLastError(); count = 0; }
    if (count <= 0) return "no HIP device is visible to this process (hipGetDeviceCount = 0): this library has no CPU path";
    if (physical >= 0 && physical < count) return "";
    std::string m = "device id " + std::to_string(logical);
    if (physical != logical) m += " (W2X_DEVICE_MAP -> " + std::to_string(physical) + ")";
    return m + " does not exist: this process sees " + std::to_string(count) + " HIP device" + (count == 1 ? "" : "s") + " (valid ids 0.." + std::to_string(count - 1) + ")";
}

}  // namespace
bool device_pci_bus_id(int deviceId, char* buf, size_t cap) {
    const int dev = physical_device(deviceId);
    if (!device_ordinal_problem(deviceId, dev).empty()) return false;
    const bool ok = hipDeviceGetPCIBusId(buf, (int)cap, dev) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    return ok;
}
namespace {

std::string precision_name(Precision p) { return p == Precision::FP16 ? "FP16" : p == Precision::FP32 ? "FP32" : "TF32"; }

// img2img_build.cpp:8-27
std::string getConfigHash(const BuildConfig& c, std::string deviceName) {
    deviceName.erase(std::remove_if(deviceName.begin(), deviceName.end(), ::isspace), deviceName.end());
    std::ostringstream oss;
    oss << deviceName << "." << precision_name(c.precision) << "."
        << c.minBatchSize << "." << c.optBatchSize << "." << c.maxBatchSize << "."
        << c.minChannels << "." << c.optChannels << "." << c.maxChannels << "."
        << c.minWidth << "." << c.optWidth << "." << c.maxWidth << "."
        << c.minHeight << "." << c.optHeight << "." << c.maxHeight;
    std::string s = oss.str();
    return sha256_hex(s.data(), s.size());
}

// img2img_build.cpp:29-50 - same keys, same order, 4-space indent
void serializeConfig(const std::string& path, const BuildConfig& c, const std::string& deviceName) {
    std::ofstream f(path);
    if (!f.is_open()) throw std::runtime_error("could not open config \"" + path + "\"");
    auto esc = [](const std::string& s) { std::string o; for (char ch : s) { if (ch == '"' || ch == '\\') o.push_back('\\'); o.push_back(ch); } return o; };
    f << "{\n"
      << "    \"deviceName\": \"" << esc(deviceName) << "\",\n"
      << "    \"precision\": \"" << precision_name(c.precision) << "\",\n"
      << "    \"minBatchSize\": " << c.minBatchSize << ",\n    \"optBatchSize\": " << c.optBatchSize << ",\n    \"maxBatchSize\": " << c.maxBatchSize << ",\n"
      << "    \"minChannels\": " << c.minChannels << ",\n    \"optChannels\": " << c.optChannels << ",\n    \"maxChannels\": " << c.maxChannels << ",\n"
      << "    \"minWidth\": " << c.minWidth << ",\n    \"optWidth\": " << c.optWidth << ",\n    \"maxWidth\": " << c.maxWidth << ",\n"
      << "    \"minHeight\": " << c.minHeight << ",\n    \"optHeight\": " << c.optHeight << ",\n    \"maxHeight\": " << c.maxHeight << "\n}";
}

// img2img_load.cpp:54-77 (flat object of strings and integers)
void deserializeConfig(const std::string& path, BuildConfig& c, std::string& deviceName) {
    std::ifstream f(path);
    if (!f.is_open()) throw std::runtime_error("could not open config \"" + path + "\"");
    std::stringstream ss; ss << f.rdbuf();
    const std::string j = ss.str();
    auto find_value = [&](const std::string& key) -> size_t {
        size_t k = j.find("\"" + key + "\"");
        if (k == std::string::npos) throw std::runtime_error("config key \"" + key + "\" missing");
        size_t c2 = j.find(':', k);
        if (c2 == std::string::npos) throw std::runtime_error("config malformed");
        ++c2; while (c2 < j.size() && isspace((unsigned char)j[c2])) ++c2;
        return c2;
    };
    auto get_str = [&](const std::string& key) {
        size_t p = find_value(key);
        if (j[p] != '"') throw std::runtime_error("config value of \"" + key + "\" is not a string");
        std::string o; ++p;
        while (p < j.size() && j[p] != '"') { if (j[p] == '\\' && p + 1 < j.size()) ++p; o.push_back(j[p++]); }
        return o;
    };
    auto get_int = [&](const std::string& key) { return (int)std::strtol(j.c_str() + find_value(key), nullptr, 10); };
    deviceName = get_str("deviceName");
    const std::string prec = get_str("precision");
    c.precision = prec == "FP16" ? Precision::FP16 : prec == "FP32" ? Precision::FP32 : Precision::TF32;
    c.minBatchSize = get_int("minBatchSize"); c.optBatchSize = get_int("optBatchSize"); c.maxBatchSize = get_int("maxBatchSize");
    c.minChannels = get_int("minChannels"); c.optChannels = get_int("optChannels"); c.maxChannels = get_int("maxChannels");
    c.minWidth = get_int("minWidth"); c.optWidth = get_int("optWidth"); c.maxWidth = get_int("maxWidth");
    c.minHeight = get_int("minHeight"); c.optHeight = get_int("optHeight"); c.maxHeight = get_int("maxHeight");
}

// img2img_load.cpp:9-20; quirk Q12 fixed: the device is compared by name, not by the index of the first device with that name
bool isCompatible(const RenderConfig& r, const BuildConfig& b, const std::string& builtOn, const std::string& runningOn) {
    return builtOn == runningOn && r.precision == b.precision &&
           r.batchSize >= b.minBatchSize && r.batchSize <= b.maxBatchSize &&
           r.channels >= b.minChannels && r.channels <= b.maxChannels &&
           r.width >= b.minWidth && r.width <= b.maxWidth && r.height >= b.minHeight && r.height <= b.maxHeight;
}
// img2img_load.cpp:22-27
bool isOptimized(const RenderConfig& r, const BuildConfig& b) {
    return r.batchSize == b.optBatchSize && r.channels == b.optChannels && r.width == b.optWidth && r.height == b.optHeight;
}

constexpr const char* kEngineExt = ".w2x";

// the filter of a resized call as resize_taps() and resize_problem() number it: 0 bicubic, 1 bilinear; any other value is 2, which resize_problem() refuses
int filter_id(ResizeFilter filter) { return filter == ResizeFilter::Bilinear ? 1 : filter == ResizeFilter::Bicubic ? 0 : 2; }

// what Impl::entry() logs for a call before a successful load, and in front of the message of an exception
constexpr const char* kNotLoaded = "Render called before a successful load.";
constexpr const char* kRenderFailed = "Render failed unexpectedly: ";

}  // namespace

struct Img2Img::Impl {
    MessageCallback messageCallback{};
    ProgressCallback progressCallback{};

    // logger.cpp:14-22
    void log(Severity s, const std::string& m) { if (messageCallback) messageCallback(s, m); }
    void log(Severity s, const std::string& m, const std::string& fn, int line) { if (messageCallback) messageCallback(s, "[" + fn + "@" + std::to_string(line) + "] " + m); }
    void log(int current, int total, double speed) { Impl* const to = report_to ? report_to : this; if (to->progressCallback) to->progressCallback(current, total, speed); }
    Impl* report_to = nullptr;           // a stage of a chained render: the engine whose progress callback hears of its batches (engines[0]); else null

    bool loaded = false;
    int device = -1;                   // physical HIP ordinal this engine lives on (set by load)
    // copies of the operational switches (switches.h), taken once per load(), never read from the environment on the launch path
    bool poison = false;               // W2X_POISON: stale activations become fp16 NaNs before every frame (tests)
    bool check_general = false;        // W2X_CHECK_GENERAL: every shape-specialised launch is compared with the general kernel
    bool use_graphs = true;            // W2X_NO_GRAPH switches the hipGraph replay of network passes off
    Plan plan;
    RenderConfig cfg;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // W2X_ROCTX=1 (read at load): roctxRangePushA / roctxRangePop around the launches of every plan op, resolved from libroctx64.so at run time (no link dependency)
    int (*roctx_push)(const char*) = nullptr; int (*roctx_pop)() = nullptr;
    hipEvent_t ev_shard = nullptr;       // renderSharded(): this engine's tiles are in its slab
    hipEvent_t ev_part[kMaxRenderParts] = {nullptr, nullptr, nullptr, nullptr};
    int pipeline_parts = 3;              // W2X_RENDER_PARTS (read at load): parts a render() call runs a frame in (1 = one part; at most kMaxRenderParts)
    size_t shard_halo_slots = 0;         // renderSharded(): slab slots in front of this engine's own tiles (the bands copied from the preceding parts)
    int shard_rows = 0, shard_cols = 0;  // shardCompute(): the frame shardFinish() completes
    hipStream_t gstream[3] = {nullptr, nullptr, nullptr};   // further tile groups of a pass (run_frame)
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    int groups = 2;                      // W2X_GROUPS (1..4; W2X_NO_SPLIT = 1): tile groups a pass is cut into
    std::vector<void*> tensors, blobs;   // tensors point into one arena
    std::vector<void*> frag_blobs;       // per blob id: fragment-major copy of a weight matrix (or null)
    std::vector<void*> perm_blobs;       // per blob id: frag_conv3b copy of a 3x3 convolution's weights (or null)
    std::vector<int> pool_blocks;        // per tensor id: pooling partials per image written by the last producer (0: plan default)
    void* arena_base = nullptr; size_t arena_bytes = 0;
    std::vector<GemmParams> gemm;      // per op (kind == OP_GEMM)
    int final_op = -1;
    // The launches of one network pass (schedule.h), decided once per load() (upload_plan) and walked by run_network(); launch_planes[k]: launch k's device side -
    // mlp32 / attn32: bf16 hi / lo planes of both matrices, fragment-major (freed by release())
    std::vector<Launch> launches;
    std::vector<std::array<void*, 4>> launch_planes;

    // frame-level buffers (grown on demand, reused across frames like the reference's input/output GpuMats, img2img.h:37-38)
    bool deep = false;                   // the frame in d_frame / d_out has 16-bit samples (Image::depth == 16)
    uint8_t* d_frame = nullptr; size_t frame_cap = 0;
    uint8_t* d_out = nullptr; size_t out_cap = 0;
    void* d_slab = nullptr; size_t slab_cap = 0;
    void* d_slab2 = nullptr; size_t slab2_cap = 0;      // second tile slab of a rolling sequence (run_rolling_frame)
    hipEvent_t ev_g0[2] = {nullptr, nullptr}, ev_cmp[2] = {nullptr, nullptr};   // rolling sequence: first group's passes of a frame issued / its compose done
    bool rolling = false;                               // inside run_rolling_frame: split passes do not join their streams
    bool rolling_ok = true;                             // W2X_NO_ROLLING switches the frame-to-frame pipeline of benchResident / renderSequence off
    TileSlot* d_slots = nullptr; size_t slots_cap = 0;
    // Dead-skip extents (liveness.h, kernels.h LiveExt): d_live[op * live_stride + slot] for the slots of d_slots, rewritten by upload_live() wherever a slot
    // table is uploaded (a frame's set-up: render / renderStrip parts, shardCompute, sequences, RGBA schedules, one_part_slots).  Captured passes hold addresses
    // into it: it only moves through ensure(), which drops them.  The no_dead_skip switch (read here, per frame set-up), W2X_CHECK_GENERAL (whole maps are compared)
    // and TTA slots (the kept rect would have to go through the slot's dihedral map) get "all"; the profiling pass honours the table like any pass.
    LiveExt* d_live = nullptr; size_t live_cap = 0, live_stride = 0;
    std::vector<LiveExt> h_live;
    std::map<std::pair<int, int>, std::vector<OpExtent>> live_cache;     // per kept rect (w, h) of this load's plan
    void upload_live(const TileGrid& grid, size_t count, hipStream_t on) {
        const size_t nops = plan.ops.size();
        if (!count || !nops) return;
        if (count > live_stride) {
            ensure(d_live, live_cap, (nops * count + 8) * sizeof(LiveExt));      // (slack: a kernel may read the entry behind a run's last image)
            live_stride = count;
        }
        const bool all = switches().no_dead_skip || check_general || cfg.tta;
        std::map<std::pair<int, int>, int> tile_at;                              // tile origins are distinct
        if (!all) for (int t = 0; t < grid.count; ++t) tile_at[{grid.in[t].x, grid.in[t].y}] = t;
        auto extents = [&](int w, int h) -> const std::vector<OpExtent>& {
            auto it = live_cache.find({w, h});
            if (it == live_cache.end()) it = live_cache.emplace(std::make_pair(w, h), dead_skip_extents(plan, w, h, false)).first;
            return it->second;
        };
        const std::vector<OpExtent>& whole = extents(plan.Tout, plan.Tout);
        h_live.resize(nops * count);
        for (size_t st = 0; st < count; ++st) {
            const TileSlot& sl = h_slots[st];
            const std::vector<OpExtent>* e = &whole;
            if (!all && sl.valid && sl.aug == 0) {
                const auto it = tile_at.find({sl.x, sl.y});
                if (it != tile_at.end()) e = &extents(grid.out[it->second].w, grid.out[it->second].h);
            }
            for (size_t i = 0; i < nops; ++i) {
                const OpExtent& x = (*e)[i];
                auto u16 = [](int v) { return (uint16_t)std::min(std::max(v, 0), 65535); };
                h_live[i * count + st] = x.all() ? LiveExt{65535, 0, 65535, 0} : LiveExt{u16(x.x.c), u16(x.x.w), u16(x.y.c), u16(x.y.w)};
            }
        }
        hipAssert(hipMemcpy2DAsync(d_live, live_stride * sizeof(LiveExt), h_live.data(), count * sizeof(LiveExt), count * sizeof(LiveExt), nops, hipMemcpyHostToDevice, on));
    }
    float *d_rampx = nullptr, *d_rampy = nullptr;
    int ovx = 0, ovy = 0;
    float* d_blob_in = nullptr; float* d_blob_out = nullptr;
    // renderSequence(): second frame/output buffer and the copy streams
    uint8_t* d_frame2 = nullptr; size_t frame2_cap = 0;
    uint8_t* d_out2 = nullptr; size_t out2_cap = 0;
    hipStream_t s_up = nullptr, s_dn = nullptr;
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_comp[2] = {nullptr, nullptr}, ev_dn[2] = {nullptr, nullptr};
    // renderResized() / renderSequenceResized(): the fp32 RGB canvas compose_canvas_kernel writes and resample_kernel reads (allocated on the first
    // resized frame, so render() callers pay nothing; not a captured address: growing it keeps the pass graphs) and the device tap tables, uploaded
    // once per (canvas size, target size, filter).
    float* d_canvas = nullptr; size_t canvas_cap = 0;
    struct ResizeTables {
        int inW = 0, inH = 0, outW = 0, outH = 0, filter = 0, edge = kEdgeReplicate;
        int *fx = nullptr, *fy = nullptr; float *wx = nullptr, *wy = nullptr;
        int kx = 0, ky = 0, rows_max = 0;
        int rows_max_above = 0;                                              // rows_max of a tile and the output row above it (top-left sited 4:2:0 output)
    };
    std::deque<ResizeTables> rs_tables;
    // YUV frames (renderYuv / renderSequenceYuv): d_frame / d_out hold the planes of in_layout / out_layout (yuv_layout; kernels.h kYuvI420 ..) and the gather /
    // compose launches are gather_yuv_kernel / compose_yuv_kernel (4:4:4 output: compose_yuv444_kernel); `key` tells the captured passes of each input format -
    // depth, range, matrix, layout - apart.  Resized (renderYuvResized) the frame ends with compose_canvas_kernel and the resample kernel of out_layout
    // (launch_resample_yuv, k_resample_yuv.hip), and d_out holds out_layout's planes of the target size.
    // in_siting / out_siting: where the chroma samples of each side sit (kYuvLeft ..); the kernels are instantiated per siting, and the source's is
    // part of `key` (a captured pass bakes its gather kernel in).
    struct YuvJob { YuvCoefs in, out; int in_bits = 8, out_bits = 8, key = 0, in_layout = kYuvI420, out_layout = kYuvI420, in_siting = kYuvLeft, out_siting = kYuvLeft; };
    // RGBA frames (renderRgba, renderRgbaResized, renderSequenceRgba*): d_frame holds the uploaded BGRA frame, alpha_bleed_kernel writes the BGR frame and the alpha
    // plane the passes gather from (gather_rgba_kernel), d_minmax receives max(A) and max(255 - A), read back into the page-locked h_minmax behind the kernel.  The
    // frame step is rgba_frame(); resized it ends with compose_canvas_rgba_kernel and resample_rgba_kernel.
    uint8_t* d_bgr = nullptr; size_t bgr_cap = 0;
    uint8_t* d_alpha = nullptr; size_t alpha_cap = 0;
    unsigned* d_minmax = nullptr; unsigned* h_minmax = nullptr;
    hipEvent_t ev_minmax = nullptr;
    // (alpha_slot0, uniform, value: what rgba_frame() found out about the frame's alpha plane, for the launches that end the frame)
    struct RgbaJob { int bleed = 0; bool skip = false; size_t alpha_slot0 = 0; bool uniform = false; unsigned value = 255; };
    // Gray frames (renderGray, renderGrayResized, renderSequenceGray*): d_frame / d_out hold ONE sample per pixel (8 or 16 bits, rows padded to 16 bytes:
    // planar_step) - a planar frame of one plane, through the planar launches below; resized, its canvas is compose_canvas_gray_kernel's one fp32 plane.  The
    // sample depth is the job's, not `deep`: nothing of a gray call is replayable.
    struct GrayJob { bool deep = false; };
    // Planar RGB frames (renderPlanar, renderPlanarResized, renderSequencePlanar*): d_frame / d_out hold three planes R, G, B one after the other, each
    // of in_bits / out_bits samples (8; 10, 12, 16 as uint16; 32 as float) with rows padded to 16 bytes (planar_layout).  The gather launch is gather_planes_kernel,
    // the frame ends with compose_planes_kernel - resized with compose_canvas_kernel (the BGR path's own canvas) and resample_planes_kernel.
    struct PlanarJob { int in_bits = 8, out_bits = 8; };
    // Planar RGBA frames (renderPlanarRgba, renderPlanarRgbaResized, renderSequencePlanarRgba*): an RGBA frame on planar samples.  Its options are the
    // two jobs above - job.planar the depths, job.rgba bleed, skip, alpha_slot0, uniform and value (the key of the uniform plane: its clamped code, float: the bits of
    // its clamped value) - and its frame step is rgba_frame().  d_frame / d_out hold four planes R, G, B, A (planar_layout); alpha_bleed_planes_kernel writes the three
    // colour planes into d_bgr and the alpha plane into d_alpha (planes of in_bits samples, rows padded as in planar_layout), which gather_planes_rgba_kernel reads.
    // A stage of a chained render (runChained) keeps the kind of the chain's frames and replaces one side or both: src set - the stage's tiles are
    // gathered from a device frame of tile pixels (gather_px_kernel; [rows][cols][4] of THIS engine's tile type) instead of d_frame; dst set - the frame ends with
    // compose_px_kernel into that frame (of the NEXT engine's tile type, dst_fp32) instead of the format's compose into d_out.  A quantised chain sets neither: its
    // stages run the format's own kernels with d_frame / d_out pointed at the chain's buffers.
    struct ChainJob { const void* src = nullptr; void* dst = nullptr; bool dst_fp32 = false; };
    // The kind of frame the running entry point renders.  Only the block "the frame formats" below branches on it: the key of the captured passes, the
    // gather (gather_tiles), the end of a frame (finish_frame), the device layout of a frame, the slot tables of a call.  The default is a plain BGR frame, not
    // resized.  The kind is set in three places - runSequenceYuv, the RGBA calls (rgba_call), runGray, runPlanar, runPlanarRgba - between the call's checks and run_call();
    // entry() puts the default back on every exit, exceptions included.  `rs`: the tap tables of a resized frame's target (job_resize), else null.
    // (`deep` is not part of it: it describes the replayable frame in d_frame / d_out and outlives the call.)
    struct Job {
        enum Kind { BGR, YUV, RGBA, GRAY, PLANAR, PLANAR_RGBA } kind = BGR;
        const ResizeTables* rs = nullptr;
        YuvJob yuv;
        RgbaJob rgba;
        GrayJob gray;
        PlanarJob planar;
        ChainJob chain;
    };
    // Dithered output (setDither): a setting of the engine like the callbacks, NOT part of the job - it outlives the call that follows it and every
    // load().  The launches that end a frame (finish_frame, outside the captured passes) read it through dither_now(), so a changed setting acts on the very
    // next frame, replayed passes or not.  seq_frame: the index of the frame a sequence call is issuing (run_sequence), 0 everywhere else - frame i of a
    // sequence is dithered like a single call at phase + i * advance.
    DitherOptions dither;
    unsigned seq_frame = 0;
    const uint16_t* d_noise = nullptr;                                   // the blue-noise table on this engine's device, looked up once per load (release() forgets it)
    DitherArgs dither_now() {
        const int mode = (int)dither.mode;
        if (mode == kDitherNone) return DitherArgs();
        if (mode == kDitherBlueNoise && !d_noise) {                      // (the caller holds the engine's DeviceGuard)
            hipError_t e = hipSuccess;
            d_noise = dither_table_device(&e);
            hipAssert(e);
        }
        return dither_args(mode, dither.phase + seq_frame * dither.advance, mode == kDitherBlueNoise ? d_noise : nullptr);
    }
    // Resize in linear light (setResizeLight): an engine-wide setting like the dither, read by the two launches that end a resized frame - the canvas
    // compose decodes, the resample encodes - through light_now().  Nothing else reads it: a frame that is not resized (job.rs null, the scaled size included)
    // never passes through the curves.
    ResizeLight light = ResizeLight::Gamma;
    LightArgs light_now() const { return light_args((int)light); }
    // Edge modes (setEdge): an engine-wide setting like the two above.  Unlike them it is read INSIDE the captured passes - the gather launch is part
    // of a pass's graph - so it is part of the pass key (sample_format()); the bleed and the resize of a frame read it outside them.  A chained render's stage
    // gathers under its own engine's mode, and the resize at its end is the last engine's.
    int edge = kEdgeReplicate;
    // What is not built under Wrap and Mirror - YUV frames, strips and shards - is refused by name before anything else is looked at: true, and
    // the message names setEdge.  Replicate: false, the call goes on as it always did.
    bool edge_refuses(const char* who, const char* what) {
        if (edge == kEdgeReplicate) return false;
        log(Severity::error, std::string(what) + " not built under setEdge(" + edge_mode_name(edge) + "): only setEdge(replicate) serves this call.", who, __LINE__);
        return true;
    }
    Job job;
    struct JobScope { Impl* im; ~JobScope() { im->job = Job{}; } };
    // Chained renders (runChained).  On engines[0]: the frames between the stages (d_chain[k]: stage k's output) and the events that order the
    // stages' streams - ev_chain_done[k]: stage k's frame is whole; ev_chain_read[k]: stage k + 1 has gathered its tiles out of d_chain[k] (a sequence's next
    // frame may overwrite it).  Plain allocations: no captured pass of THIS engine is tied to them beyond its key, which holds the address.
    // On every engine, per stage index it runs: slot and liveness tables of that stage's own grid (an engine that appears twice runs two grids in one call, and
    // the host side of an upload must stay untouched until the stream has taken it), swapped into d_slots / d_live / h_slots / h_live for the stage's duration.
    static constexpr int kChainStages = 4;
    void* d_chain[kChainStages - 1] = {nullptr, nullptr, nullptr}; size_t chain_cap[kChainStages - 1] = {0, 0, 0};
    hipEvent_t ev_chain_done[kChainStages] = {nullptr, nullptr, nullptr, nullptr}, ev_chain_read[kChainStages - 1] = {nullptr, nullptr, nullptr};
    struct StageTables { TileSlot* d_slots = nullptr; size_t slots_cap = 0; LiveExt* d_live = nullptr; size_t live_cap = 0, live_stride = 0; std::vector<LiveExt> h_live; std::vector<TileSlot> h_slots; };
    StageTables chain_tables[kChainStages];
    void swap_tables(int k) {
        StageTables& t = chain_tables[k];
        std::swap(d_slots, t.d_slots); std::swap(slots_cap, t.slots_cap); std::swap(d_live, t.d_live); std::swap(live_cap, t.live_cap); std::swap(live_stride, t.live_stride);
        h_live.swap(t.h_live); h_slots.swap(t.h_slots);
    }
    void ensure_chain(int k, size_t bytes) {
        if (bytes <= chain_cap[k]) return;
        if (d_chain[k]) hipAssert(hipFree(d_chain[k]));
        d_chain[k] = nullptr; chain_cap[k] = 0;
        hipAssert(hipMalloc(&d_chain[k], bytes));
        chain_cap[k] = bytes;
    }
    std::vector<void*> pinned;
    std::vector<void*> host_allocs;     // allocHost(): page-locked buffers handed to the caller
    std::vector<TileSlot> h_slots;

    // per-launch HIP-event profiling (profileFrame): events recorded on the compute stream around every launch
    bool profiling = false;
    struct Stamp { int kind; hipEvent_t a, b; double flops; int op; };
    std::vector<double> op_ms;   // per plan op, summed over the batches of the profiled frame
    std::vector<Stamp> stamps;
    void stamp_begin(int kind, double flops, int op = -1) {
        if (!profiling) return;
        Stamp st{kind, nullptr, nullptr, flops, op};
        hipAssert(hipEventCreate(&st.a)); hipAssert(hipEventCreate(&st.b));
        hipAssert(hipEventRecord(st.a, stream));
        stamps.push_back(st);
    }
    void stamp_end() { if (profiling) hipAssert(hipEventRecord(stamps.back().b, stream)); }

    // The copy streams of renderSequence() (upload, download) and of a two-part render() (download): ONE pair, created in one place and in one
    // order - the runtime spreads streams over its hardware queues in creation order, and a further stream in between moved the copy streams
    // onto the compute streams' queues (host-to-host 7.6 -> 9.8 ms per frame, profiles/r4_kernels/render_parts_ab.txt, first run).
    void ensure_copy_streams() {
        if (s_up) return;
        hipAssert(hipStreamCreateWithFlags(&s_up, hipStreamNonBlocking));
        hipAssert(hipStreamCreateWithFlags(&s_dn, hipStreamNonBlocking));
        for (int b = 0; b < 2; ++b) { hipAssert(hipEventCreateWithFlags(&ev_up[b], hipEventDisableTiming)); hipAssert(hipEventCreateWithFlags(&ev_comp[b], hipEventDisableTiming)); hipAssert(hipEventCreateWithFlags(&ev_dn[b], hipEventDisableTiming)); }
    }

    // last frame (for benchResident / profileFrame, which replay it as ONE part)
    bool one_part_stale = false;          // the last render() ran in parts: d_slots holds the parts' slot tables
    void one_part_slots() {
        if (!one_part_stale) return;
        const size_t stepCount = pass_slots(last_strip.tile_count);
        fill_slots(last_grid, last_strip.first_tile, last_strip.tile_count, 1, 0, stepCount);
        upload_slots(last_grid, stepCount, stepCount);      // (the slab is already that large: renderPart sizes it for both layouts)
        hipAssert(hipStreamSynchronize(stream));
        one_part_stale = false;
    }
    // the step schedule of a frame's tiles (tiles.h) under this engine's plan and configuration
    int batch_count(int tiles) const { return w2x::batch_count(tiles, cfg.tta ? 8 : 1, plan.userB); }
    size_t pass_slots(int tiles) const { return w2x::pass_slots(tiles, cfg.tta ? 8 : 1, plan.userB, plan.B); }
    // h_slots[at, at + count): the steps of the tiles [first, first + tiles) of the grid, pad slots behind them.  `valid`: 1, or kSlotColour / kSlotAlpha (RGBA)
    void fill_slots(const TileGrid& grid, int first, int tiles, int valid, size_t at, size_t count) {
        const int steps = cfg.tta ? 8 : 1;
        if (h_slots.size() < at + count) h_slots.resize(at + count);
        for (size_t st = 0; st < count; ++st) {
            const int ti = (int)(st / steps), aug = (int)(st % steps);
            TileSlot sl{0, 0, aug, 0};
            if (ti < tiles) { sl.x = grid.in[first + ti].x; sl.y = grid.in[first + ti].y; sl.valid = valid; }
            h_slots[at + st] = sl;
        }
    }
    // h_slots[0, count) into d_slots and their dead-skip extents into d_live, both on `stream` (not waited for), and a slab that holds `slab_slots` tiles
    void upload_slots(const TileGrid& grid, size_t count, size_t slab_slots) {
        ensure(d_slots, slots_cap, count * sizeof(TileSlot));
        hipAssert(hipMemcpyAsync(d_slots, h_slots.data(), count * sizeof(TileSlot), hipMemcpyHostToDevice, stream));
        upload_live(grid, count, stream);
        ensure(d_slab, slab_cap, slab_slots * plan.Tout * plan.Tout * 4 * plan.elt);
    }
    int last_rows = 0, last_cols = 0, last_batches = 0;
    TileGrid last_grid;
    StripPlan last_strip;
    float last_ms = 0.f;

    // One network pass (gather + every plan op) captured as a hipGraph: the reference's whole network is a single
    // enqueueV3 (img2img_infer.cpp:80); here a pass is ~40 launches, which the host cannot issue fast enough for small tiles.
    // A pass is captured the second time it is met (the first run stays eager so that one-time attribute calls are out of the
    // way) and replayed from then on.  The key holds everything the captured launches bake in.
    static constexpr int kRgbaKey = 64;   // (YuvJob::key stays below 50 for left-sited sources and is 100 .. 149 / 200 .. 249 for centre / top-left sited ones)
    static constexpr int kGrayKey = 65;   // 65 / 66: gray frames of 8 / 16 bits
    static constexpr int kPlanarKey = 67; // 67 .. 71: planar frames whose input samples have 8 / 10 / 12 / 16 / 32 bits
    static constexpr int kPlanarRgbaKey = 72; // 72 .. 76: planar RGBA frames, by input depth likewise
    static constexpr int kChainKey = 80;      // a stage of a chained render that gathers from a frame of tile pixels (whatever the chain's frame format)
    using GraphKey = std::tuple<const void*, const void*, const void*, const void*, int, int, int, int>;   // frame, slots, slab out, arena, rows, cols, live, sample format (1: 16-bit, >= 2: YuvJob::key)
    // A pass that runs as NG tile groups is NG graphs, one per group, each a straight line of launches replayed on that group's OWN stream (fork / join
    // events between the streams are issued around the replays): a single captured graph with NG branches runs its side branches on streams the runtime
    // creates at instantiation, which land on whichever hardware queue has the fewest users at that moment - sometimes the copy streams' queue, where the
    // next download or upload then waits behind a whole pass (render() in three parts 10.1 ms, in two or four 9.0 / 8.6, same work).
    struct PassGraphs { hipGraphExec_t g[4] = {nullptr, nullptr, nullptr, nullptr}; int n = 0; };
    std::map<GraphKey, PassGraphs> graphs;
    std::map<GraphKey, int> graph_seen;
    long graph_replays = 0, eager_passes = 0;
    void drop_graphs() {
        for (auto& kv : graphs) for (int k = 0; k < kv.second.n; ++k) if (kv.second.g[k]) (void)hipGraphExecDestroy(kv.second.g[k]);
        graphs.clear(); graph_seen.clear();
    }

    ~Impl() {
        release();
        for (void* h : host_allocs) if (hipHostFree(h) != hipSuccess) (void)hipGetLastError();
    }

    void release() {
        std::unique_ptr<DeviceGuard> guard;
        if (device >= 0) { try { guard.reset(new DeviceGuard(device)); } catch (...) {} }
        drop_graphs();
        // img2img_base.cpp:6-10 frees the IO buffers; here everything the engine owns
        if (arena_base) { (void)hipFree(arena_base); arena_base = nullptr; }
        for (void* p : blobs) if (p) (void)hipFree(p);
        for (void* p : frag_blobs) if (p) (void)hipFree(p);
        frag_blobs.clear();
        for (void* p : perm_blobs) if (p) (void)hipFree(p);
        perm_blobs.clear();
        for (const auto& planes : launch_planes) for (void* p : planes) if (p) (void)hipFree(p);
        launch_planes.clear(); launches.clear();
        tensors.clear(); blobs.clear(); gemm.clear();
        for (void* h : pinned) if (hipHostUnregister(h) != hipSuccess) (void)hipGetLastError();
        pinned.clear();
        // (allocHost() buffers belong to the caller's frames and outlive a re-load: they go in the destructor)
        for (hipEvent_t* e : {&ev_up[0], &ev_up[1], &ev_comp[0], &ev_comp[1], &ev_dn[0], &ev_dn[1]}) if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
        if (s_up) { (void)hipStreamDestroy(s_up); s_up = nullptr; }
        if (s_dn) { (void)hipStreamDestroy(s_dn); s_dn = nullptr; }
        frame2_cap = out2_cap = 0;
        for (ResizeTables& t : rs_tables) for (void* q : {(void*)t.fx, (void*)t.fy, (void*)t.wx, (void*)t.wy}) if (q) (void)hipFree(q);
        rs_tables.clear(); job = Job{}; d_noise = nullptr;
        if (d_canvas) { (void)hipFree(d_canvas); d_canvas = nullptr; }
        canvas_cap = 0;
        for (int k = 0; k + 1 < kChainStages; ++k) { if (d_chain[k]) (void)hipFree(d_chain[k]); d_chain[k] = nullptr; chain_cap[k] = 0; if (ev_chain_read[k]) { (void)hipEventDestroy(ev_chain_read[k]); ev_chain_read[k] = nullptr; } }
        for (hipEvent_t& e : ev_chain_done) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        for (StageTables& t : chain_tables) { if (t.d_slots) (void)hipFree(t.d_slots); if (t.d_live) (void)hipFree(t.d_live); t = StageTables{}; }
        report_to = nullptr;
        for (void** q : {(void**)&d_bgr, (void**)&d_alpha, (void**)&d_minmax}) if (*q) { (void)hipFree(*q); *q = nullptr; }
        bgr_cap = alpha_cap = 0;
        if (h_minmax) { if (hipHostFree(h_minmax) != hipSuccess) (void)hipGetLastError(); h_minmax = nullptr; }
        if (ev_minmax) { (void)hipEventDestroy(ev_minmax); ev_minmax = nullptr; }
        for (void** p : {(void**)&d_frame, (void**)&d_out, (void**)&d_frame2, (void**)&d_out2, &d_slab, &d_slab2, (void**)&d_slots, (void**)&d_live, (void**)&d_rampx, (void**)&d_rampy, (void**)&d_blob_in, (void**)&d_blob_out})
            if (*p) { (void)hipFree(*p); *p = nullptr; }
        frame_cap = out_cap = slab_cap = slab2_cap = slots_cap = 0;
        live_cap = live_stride = 0; live_cache.clear();
        shard_rows = shard_cols = 0; shard_halo_slots = 0; rolling = false; one_part_stale = false;
        last_rows = last_cols = last_batches = 0;      // (benchResident / profileFrame replay the last frame of THIS load)
        if (ev0) { (void)hipEventDestroy(ev0); ev0 = nullptr; }
        if (ev1) { (void)hipEventDestroy(ev1); ev1 = nullptr; }
        if (ev_shard) { (void)hipEventDestroy(ev_shard); ev_shard = nullptr; }
        for (hipEvent_t& e : ev_part) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        for (hipEvent_t& e : ev_g0) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        for (hipEvent_t& e : ev_cmp) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        if (ev_fork) { (void)hipEventDestroy(ev_fork); ev_fork = nullptr; }
        for (hipEvent_t& e : ev_join) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        for (hipStream_t& st : gstream) if (st) { (void)hipStreamDestroy(st); st = nullptr; }
        if (stream) { (void)hipStreamDestroy(stream); stream = nullptr; }
        loaded = false;
    }

    TView tview(const View& v) const {
        TView t;
        if (v.t < 0) return t;
        const TensorDesc& d = plan.tensors[v.t];
        t.p = tensors[v.t]; t.Hs = d.H; t.Ws = d.W; t.Cs = d.C; t.y0 = v.y0; t.x0 = v.x0;
        return t;
    }

    // the bf16 hi / lo planes of an fp32 matrix [N][K] in fragment-major order (split4 of k_f32.hip on the host: hi = bf16(x), lo = bf16(x - hi), round to nearest even)
    void upload_planes(const std::vector<uint8_t>& w, int N, int K, void*& dh, void*& dl) {
        std::vector<uint16_t> hi((size_t)N * K), lo((size_t)N * K);
        const float* f = (const float*)w.data();
        auto bf = [](float x) { uint32_t u; memcpy(&u, &x, 4); return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); };
        for (size_t k = 0; k < hi.size(); ++k) {
            const uint16_t h = bf(f[k]);
            const uint32_t hu = (uint32_t)h << 16; float hf; memcpy(&hf, &hu, 4);
            hi[k] = h; lo[k] = bf(f[k] - hf);
        }
        for (int pl = 0; pl < 2; ++pl) {
            const std::vector<uint16_t> fr = frag_major(pl ? lo.data() : hi.data(), N, K);
            void*& d = pl ? dl : dh;
            hipAssert(hipMalloc(&d, fr.size() * 2 + 256));
            hipAssert(hipMemcpy(d, fr.data(), fr.size() * 2, hipMemcpyHostToDevice));
        }
    }

    // load(): the plan on the device, in four steps.  The order of the allocations and copies is part of it (load() says why).
    void upload_plan(Precision prec) {
        const std::vector<Launch> candidates = candidate_launches(plan, prec, check_general);
        place_tensors(layout_arena(plan, candidates));
        upload_weights();
        prepare_gemm_params();
        confirm_launches(candidates);
        hipAssert(hipStreamSynchronize(stream));
    }
    // step 1: the activation arena for the layout of the candidate launches (schedule.h): one allocation, tensors[] from the offsets
    void place_tensors(const ArenaLayout& lay) {
        const int nt = (int)plan.tensors.size();
        const size_t arena = lay.bytes;
        hipAssert(hipMalloc(&arena_base, arena + 1024));   // slack: vector reads past a table's last row; the group parts rounded up to 256 bytes
        hipAssert(hipMemsetAsync(arena_base, 0, arena + 1024, stream));
        arena_bytes = arena;
        pool_blocks.assign(nt, 0);
        tensors.assign(nt, nullptr);
        for (int t = 0; t < nt; ++t) tensors[t] = lay.placed[t] ? (uint8_t*)arena_base + lay.off[t] : nullptr;
    }
    // step 2: the weights and tables, and the fragment-major / permuted copies of the matrices that kernels read in that order
    void upload_weights() {
        blobs.assign(plan.blobs.size(), nullptr);
        for (size_t i = 0; i < plan.blobs.size(); ++i) {
            const auto& d = plan.blobs[i].data;
            hipAssert(hipMalloc(&blobs[i], d.size() + 256));   // slack: kernels may read a vector past a table's last row
            hipAssert(hipMemcpy(blobs[i], d.data(), d.size(), hipMemcpyHostToDevice));
        }
        // fragment-major copies (fragorder.h) of the weights that kernels read straight from L2
        frag_blobs.assign(plan.blobs.size(), nullptr);
        auto upload_frag = [&](int blob, const std::vector<uint16_t>& f) {
            hipAssert(hipMalloc(&frag_blobs[blob], f.size() * 2 + 256));
            hipAssert(hipMemcpy(frag_blobs[blob], f.data(), f.size() * 2, hipMemcpyHostToDevice));
        };
        auto frag_major_blob = [&](int blob, int N, int K) {
            if (frag_blobs[blob]) return;
            const auto& d = plan.blobs[blob].data;
            if (d.size() != (size_t)N * K * 2) throw std::runtime_error("plan: weight shape");
            upload_frag(blob, frag_major((const uint16_t*)d.data(), N, K));
        };
        auto frag_w2_blob = [&](int blob, int Cc) {
            if (frag_blobs[blob]) return;
            const auto& d = plan.blobs[blob].data;
            if (d.size() != (size_t)Cc * Cc * 4) throw std::runtime_error("plan: mlp weight shape");
            upload_frag(blob, frag_w2((const uint16_t*)d.data(), Cc));
        };
        for (const Op& op : plan.ops)   // pixel-shuffle projections served by k_pixgemm.hip
            if (plan.elt == 2 && op.kind == OP_GEMM && ((op.g.omode == 2 && (op.g.amode == 0 || (op.g.amode == 2 && op.g.kh == 1 && op.g.kw == 1))) || (op.g.amode == 2 && op.g.kh == 2 && op.g.kw == 2 && op.g.stride == 2)) && op.g.K % 32 == 0 && op.g.N % 16 == 0 &&
                plan.blobs[op.g.w].data.size() == (size_t)op.g.N * op.g.K * 2) frag_major_blob(op.g.w, op.g.N, op.g.K);
        perm_blobs.assign(plan.blobs.size(), nullptr);
        for (const Op& op : plan.ops)   // plain 3x3 convolutions onto 64 / 128 / 256 channels (k_conv3.hip)
            if (plan.elt == 2 && op.kind == OP_GEMM && op.g.amode == 2 && op.g.kh == 3 && op.g.kw == 3 && op.g.stride == 1 && op.g.omode == 0 && op.g.K % 32 == 0 && op.g.N % 64 == 0 &&
                plan.blobs[op.g.w].data.size() == (size_t)op.g.N * op.g.K * 2 && !perm_blobs[op.g.w]) {
                const std::vector<uint16_t> f = frag_conv3b((const uint16_t*)plan.blobs[op.g.w].data.data(), op.g.N, op.g.K);
                hipAssert(hipMalloc(&perm_blobs[op.g.w], f.size() * 2 + 256));
                hipAssert(hipMemcpy(perm_blobs[op.g.w], f.data(), f.size() * 2, hipMemcpyHostToDevice));
            }
        for (const Op& op : plan.ops)   // 48 -> 96 channel 3x3 convolution (k_conv48.hip): K = 432 padded with zero columns to 14 k-steps of 32
            if (plan.elt == 2 && op.kind == OP_GEMM && op.g.amode == 2 && op.g.kh == 3 && op.g.kw == 3 && op.g.stride == 1 && op.g.omode == 0 && op.g.K == 432 && op.g.N == 96 &&
                plan.tensors[op.g.a.t].C == 48 && !frag_blobs[op.g.w]) {
                const auto& d = plan.blobs[op.g.w].data;
                const int Kw = round_up(op.g.K, 8), Kp = 448;
                if (d.size() != (size_t)op.g.N * Kw * 2) throw std::runtime_error("plan: weight shape");
                std::vector<uint16_t> padded((size_t)op.g.N * Kp, 0);
                for (int n = 0; n < op.g.N; ++n) memcpy(&padded[(size_t)n * Kp], d.data() + (size_t)n * Kw * 2, (size_t)op.g.K * 2);
                upload_frag(op.g.w, frag_major(padded.data(), op.g.N, Kp));
            }
        for (const Op& op : plan.ops)
            if (plan.elt == 2 && op.kind == OP_MLP && mlp_supported(op.m.C)) {
                const int Cm = op.m.C;
                const auto& w1 = plan.blobs[op.m.w1].data; const auto& w2 = plan.blobs[op.m.w2].data;
                if (w1.size() != (size_t)2 * Cm * Cm * 2 || w2.size() != w1.size()) throw std::runtime_error("plan: MLP weight size");
                // C = 96: 32x32x16 fragments (k_mlp96q.hip).  C = 192: 16x16x32 fragments (mlp2_kernel<192,2,4> in k_mlp2.hip) since round 6 - the 32x32x16 kernel of
                // rounds 3-5 (mlp2q_kernel, now tools/ab/k_mlp192q.hip; -DW2X_MLP192_TILE32 here and that file in place of k_mlp2.hip) takes the same time per launch but more energy per product, and the frame runs at the
                // board's power cap: 7.272 / 7.274 against 7.306 / 7.312 / 7.307 ms per frame in alternating pairs (profiles/r6_kernels/lib_mlp192_tile16_frame_level.txt)
                if (!mlp_frag32(Cm)) {
                    if (!frag_blobs[op.m.w1]) upload_frag(op.m.w1, frag_major((const uint16_t*)w1.data(), 2 * Cm, Cm));
                    if (!frag_blobs[op.m.w2]) upload_frag(op.m.w2, frag_w2((const uint16_t*)w2.data(), Cm));
                    continue;
                }
                if (!frag_blobs[op.m.w1]) upload_frag(op.m.w1, frag32_major((const uint16_t*)w1.data(), 2 * Cm, Cm));
                if (!frag_blobs[op.m.w2]) upload_frag(op.m.w2, frag32_w2((const uint16_t*)w2.data(), Cm));
            }
        for (const Op& op : plan.ops)
            if (plan.elt == 2 && op.kind == OP_SWINATTN) { frag_major_blob(op.sa.wqkv, 3 * op.sa.C, op.sa.C); frag_major_blob(op.sa.wproj, op.sa.C, op.sa.C); }
    }
    // step 3: every GEMM op's launch parameters for a whole pass (run_network() adjusts a copy per pass and group)
    void prepare_gemm_params() {
        gemm.assign(plan.ops.size(), GemmParams{}); final_op = -1;
        for (size_t i = 0; i < plan.ops.size(); ++i) {
            const Op& op = plan.ops[i];
            if (op.kind != OP_GEMM) continue;
            const GemmOp& g = op.g;
            GemmParams& p = gemm[i];
            p.a = tview(g.a); p.amode = g.amode; p.kh = g.kh; p.kw = g.kw; p.stride = g.stride;
            p.B = plan.B; p.Mrows = g.Mrows; p.aW = g.aW;
            p.win_table = g.win_table >= 0 ? (const int*)blobs[g.win_table] : nullptr;
            p.K = g.K; p.N = g.N; p.Kw = round_up(g.K, 8);
            p.wt = blobs[g.w]; p.wt_frag = frag_blobs[g.w]; p.wt_perm = perm_blobs[g.w]; p.bias = (const float*)blobs[g.bias];
            p.ln = g.ln; p.csum = g.csum >= 0 ? (const float*)blobs[g.csum] : nullptr;
            p.stats_in = g.stats_in >= 0 ? (const float*)tensors[g.stats_in] : nullptr;
            p.act = g.act; p.alpha = g.alpha; p.has_clip = g.has_clip; p.clip_lo = g.clip_lo; p.clip_hi = g.clip_hi;
            p.res = tview(g.res); p.res2 = tview(g.res2); p.out = tview(g.out);
            p.omode = g.omode; p.r = g.r; p.Cout = g.Cout;
            p.stats_out = g.stats_out >= 0 ? (float*)tensors[g.stats_out] : nullptr; p.ln_eps = g.ln_eps;
            p.pool_out = g.pool_out >= 0 ? (float*)tensors[g.pool_out] : nullptr;
            p.a_scale = g.se_scale >= 0 ? (const float*)tensors[g.se_scale] : nullptr;
            p.res_scale = g.res_scale >= 0 ? (const float*)tensors[g.res_scale] : nullptr;
            if ((p.a_scale || p.res_scale) && plan.elt != 2) throw std::runtime_error("plan: folded gates in an fp32 plan");
            if (g.out.t == plan.out_tensor) final_op = (int)i;
            // shape checks the kernels rely on (a wrong shape would fault on the device)
            if (p.ln && (!p.stats_in || !p.csum)) throw std::runtime_error("plan: LayerNorm op without statistics");
            if (p.stats_out && p.Cout != p.out.Cs) throw std::runtime_error("plan: statistics over padded rows");
            if (p.pool_out && p.omode != O_ROWS) throw std::runtime_error("plan: pooling on a scattered output");
            if (p.omode == O_PIXSHUF && p.N != p.r * p.r * p.out.Cs) throw std::runtime_error("plan: pixel-shuffle width mismatch");
            if (p.omode != O_PIXSHUF && p.N != p.out.Cs) throw std::runtime_error("plan: output width mismatch");
            if ((p.amode == A_WIN || p.omode == O_WIN) && !p.win_table) throw std::runtime_error("plan: missing window table");
            if (p.a.Cs != 4 && (p.a.Cs % 8)) throw std::runtime_error("plan: unaligned input channels");
        }
        if (final_op < 0) throw std::runtime_error("plan: the output tensor is not produced by a fused op");
    }
    // step 4: the launch list.  The candidates are what plan facts allow (schedule.h); what the kernels take of the prepared parameters - which compare device pointers - is decided here.
    void confirm_launches(const std::vector<Launch>& candidates) {
        // Each fold confirmed with the prepared launch parameters, or split back into its ops.  The image head: k_mlp96q.hip takes a 32-row tile inside one image, at most
        // two token rows, and clip bounds that fp16 holds exactly.  The stem and the transposed convolution: k_conv48.hip conv48_kernel<true> / k_conv3.hip conv3_kernel
        // (switches.h no_fuse_head / no_fuse_stem / no_fuse_up keep the launches apart).
        auto head_supported = [&](const GemmParams& g) {
            return g.wt_frag && g.out.Cs == 4 && g.a.y0 == 0 && g.a.x0 == 0 && g.a.Ws == g.aW && (long)g.a.Hs * g.a.Ws == g.Mrows && g.Mrows % 32 == 0 && g.aW >= 32 && pixgemm_supported(g) &&
                   (!g.has_clip || (f16_to_f32(f32_to_f16(g.clip_lo)) == g.clip_lo && f16_to_f32(f32_to_f16(g.clip_hi)) == g.clip_hi));
        };
        launches.clear();
        for (const Launch& L : candidates) {
            const GemmParams& p = gemm[L.last]; const GemmParams& q = gemm[L.first];
            const bool ok = L.kind == L_HEAD ? head_supported(p) : L.kind == L_STEM ? conv48_stem_supported(p, q) || conv3_stem_supported(p, q) : L.kind == L_UP ? conv3_up_supported(p, q) : true;
            if (ok) launches.push_back(L);
            else for (int i = L.first; i <= L.last; ++i) launches.push_back(make_launch(plan, L_OP, i, i));
        }
        // fp32 plans at Precision::TF32: the weights of the fused launches as bf16 hi / lo planes
        launch_planes.assign(launches.size(), {{nullptr, nullptr, nullptr, nullptr}});
        for (size_t k = 0; k < launches.size(); ++k) {
            const Launch& L = launches[k]; std::array<void*, 4>& planes = launch_planes[k];
            if (L.kind == L_MLP32 || L.kind == L_ATTN32) {
                const GemmOp& g1 = plan.ops[L.first].g; const GemmOp& g2 = plan.ops[L.last].g;
                upload_planes(plan.blobs[g1.w].data, g1.N, g1.K, planes[0], planes[1]);
                upload_planes(plan.blobs[g2.w].data, g2.N, g2.K, planes[2], planes[3]);
            }
        }
    }

    // one pass of the network over the tiles currently in plan.in_tensor; the last op writes to `out_override`
    // `live` = tiles of this pass that carry image data; the zero-pad slots the reference appends to fill its last batch
    // (img2img_render.cpp:281) are never read back (:298-299), so they are not computed at all.
    // `grp` / `s`: the pass may be cut into NG tile groups that run side by side on NG streams (run_frame).  Tensors with disjoint
    // lifetimes share arena memory, which only holds while the ops run one after the other - so each group gets its own PART of the
    // arena, laid out like the whole one at 1/NG of the size (schedule.h arena_part_bytes / arena_group_offset): group grp of up to B/NG tiles
    // runs the plan on arena_base + grp * arena_part.  out_override is the slab address of the group's first tile.
    int ng_now = 1;                      // NG of the pass being issued
    size_t arena_part() const { return arena_part_bytes(arena_bytes, ng_now); }
    uint8_t* group_ptr(const void* full, int grp) const {
        return full ? (uint8_t*)arena_base + arena_group_offset(arena_bytes, ng_now, grp, (size_t)((const uint8_t*)full - (const uint8_t*)arena_base)) : nullptr;
    }
    void run_network(void* out_override, int live = -1, int grp = -1, hipStream_t s = nullptr, const LiveExt* ext = nullptr) {
        if (!s) s = stream;
        const int cap = grp < 0 ? plan.B : plan.B / ng_now;
        if (live < 0 || live > cap) live = cap;
        auto tp = [&](int t) -> uint8_t* { return t < 0 ? nullptr : grp < 0 ? (uint8_t*)tensors[t] : group_ptr(tensors[t], grp); };
        // `ext`: the dead-skip entry of this pass's (group's) first slot in op 0's table, or null ("all": w2x_infer); op i's table lies i * live_stride entries on
        auto lv = [&](int i) -> const LiveExt* { return ext ? ext + (size_t)i * live_stride : nullptr; };
        // op i's prepared parameters for this pass: `live` tiles, the group's part of the arena, the pass's output where op i writes it
        auto gp = [&](int i) {
            GemmParams p = gemm[i];
            p.B = live;
            if (grp >= 0) {
                auto shift = [&](auto*& ptr) { ptr = (std::remove_reference_t<decltype(ptr)>)group_ptr(ptr, grp); };
                shift(p.a.p); shift(p.res.p); shift(p.res2.p); shift(p.out.p); shift(p.stats_in); shift(p.stats_out); shift(p.pool_out); shift(p.a_scale); shift(p.res_scale);
            }
            if (i == final_op && out_override) p.out.p = out_override;
            return p;
        };
        for (const Launch& L : launches) try {
            const std::array<void*, 4>& planes = launch_planes[&L - launches.data()];
            const Op& op = plan.ops[L.first];
            struct Range { Impl* e; bool on; ~Range() { if (on) e->roctx_pop(); } } range{this, roctx_push != nullptr};   // W2X_ROCTX=1: a roctx range per launch (rocprofv3 --marker-trace)
            if (range.on) roctx_push(launch_label(plan, L).c_str());
            auto issue = [&](auto&& f) { stamp_begin(L.family, L.flops, L.timed); hipAssert(f()); stamp_end(); };   // (profileFrame: events around the launch alone)
            switch (L.kind) {
                case L_HEAD: {      // the image head rides on the MLP launch
                    const GemmParams g = gp(L.last);
                    MlpParams p = mlp_params(op, live, tp);
                    p.live = lv(L.last);      // (the head is per token: its rows are the MLP's)
                    p.ti_w = g.wt_frag; p.ti_b = g.bias; p.ti_out = g.out.p; p.ti_Hs = g.out.Hs; p.ti_Ws = g.out.Ws; p.ti_Mrows = g.Mrows; p.ti_aW = g.aW;
                    p.ti_clip = g.has_clip; p.ti_lo = g.clip_lo; p.ti_hi = g.clip_hi;
                    issue([&] { return launch_mlp(p, s); });
                    break;
                }
                case L_STEM: case L_UP: {      // the convolution computes the op in front of it in its halo stage (the stem: k_conv48.hip onto 48 channels, k_conv3.hip onto 32)
                    const GemmParams p = gp(L.last), q = gp(L.first);
                    issue([&] { return L.kind == L_UP ? launch_conv3_up(p, q, s) : q.N == 48 ? launch_conv48_stem(p, q, s) : launch_conv3_stem(p, q, s); });
                    break;
                }
                case L_MLP32: {      // fc1 + GELU + fc2 + residual on fp32 rows
                    const GemmParams p = gp(L.first), q = gp(L.last);
                    Mlp32Params m;
                    m.x = (const float*)p.a.p; m.y = (float*)q.out.p; m.M = (long)live * p.Mrows; m.C = p.K; m.stats_in = p.stats_in;
                    m.w1h = planes[0]; m.w1l = planes[1]; m.w2h = planes[2]; m.w2l = planes[3];
                    m.b1 = p.bias; m.b2 = q.bias; m.stats_out = q.stats_out; m.eps_out = q.ln_eps;
                    issue([&] { return launch_mlp32(m, s); });
                    break;
                }
                case L_ATTN32: {     // LayerNorm + window gather + qkv, attention core, proj + scatter + residual
                    const GemmParams p = gp(L.first), q = gp(L.last);
                    const AttnOp& a = plan.ops[L.first + 1].at;
                    SwinAttn32Params m;
                    m.x = (const float*)p.a.p; m.y = (float*)q.out.p; m.res = (const float*)q.res.p; m.B = live; m.nwin = a.nwin; m.C = p.K; m.pix_per_item = p.Mrows;
                    m.table_in = p.win_table; m.table_out = q.win_table; m.stats_in = p.stats_in;
                    m.wqkv_h = planes[0]; m.wqkv_l = planes[1]; m.wproj_h = planes[2]; m.wproj_l = planes[3];
                    m.bqkv = p.bias; m.bproj = q.bias; m.scale = a.scale; m.bias = (const float*)blobs[a.bias]; m.maskid = (const int*)blobs[a.maskid];
                    m.stats_out = q.stats_out; m.eps_out = q.ln_eps;
                    issue([&] { return launch_swinattn32(m, s); });
                    break;
                }
                case L_OP: switch (op.kind) {
                    case OP_GEMM: {
                        const GemmParams p = gp(L.first);
                        if (op.g.pool_out >= 0) pool_blocks[op.g.pool_out] = plan.elt == 2 && conv3_supported(p) ? conv3_tiles(p) : 0;   // partial sums per image written by this launch (0: plan default)
                        issue([&] { return plan.elt == 4 ? launch_gemm_f32(p, s, cfg.precision == Precision::FP32) : pixgemm_supported(p) ? launch_pixgemm(p, s) : conv3_supported(p) ? launch_conv3(p, s) : conv3h_supported(p) ? launch_conv3h(p, s) : conv48_supported(p) ? launch_conv48(p, s) : stem_supported(p) ? launch_stem(p, s) : launch_gemm(p, s); });
                        if (check_general && plan.elt == 2 && (pixgemm_supported(p) || conv3_supported(p) || conv3h_supported(p) || conv48_supported(p) || stem_supported(p))) check_against_general(p, L.first, live);
                        break;
                    }
                    case OP_ATTN: {
                        const AttnOp& a = op.at;
                        AttnParams p;
                        p.qkv = tp(a.qkv); p.out = tp(a.out); p.B = live; p.nwin = a.nwin; p.heads = a.heads; p.hd = a.hd;
                        p.ntok = a.ws * a.ws; p.scale = a.scale; p.bias = blobs[a.bias]; p.maskid = (const int*)blobs[a.maskid];
                        issue([&] { return plan.elt == 4 ? launch_attn_f32(p, s) : launch_attn(p, s); });
                        break;
                    }
                    case OP_SWINATTN: {
                        const SwinAttnOp& a = op.sa;
                        const TensorDesc& d = plan.tensors[a.x];
                        SwinAttnParams p;
                        p.x = tp(a.x); p.y = tp(a.y); p.table = (const int*)blobs[a.table]; p.H = a.H; p.W = a.W; p.ry = a.ry; p.rx = a.rx; p.B = live; p.nwin = a.nwin; p.C = a.C; p.hd = a.hd;
                        p.wqkv = blobs[a.wqkv]; p.bqkv = (const float*)blobs[a.bqkv]; p.scale = a.scale; p.bias32 = (const float*)blobs[a.bias]; p.maskid = (const int*)blobs[a.maskid];
                        p.wproj = blobs[a.wproj]; p.bproj = (const float*)blobs[a.bproj]; p.eps = a.eps;
                        p.wqkv_frag = frag_blobs[a.wqkv]; p.wproj_frag = frag_blobs[a.wproj];
                        p.stats_out = (float*)tp(a.stats_out); p.eps_out = a.eps_out;
                        p.live = lv(L.first);
                        if (d.C != a.C || plan.tensors[a.y].C != a.C || d.H * d.W != a.nwin * a.ws * a.ws) throw std::runtime_error("plan: attention geometry mismatch");
                        issue([&] { return launch_swin_attn(p, s); });
                        break;
                    }
                    case OP_MLP: {
                        MlpParams p = mlp_params(op, live, tp);
                        p.live = lv(L.first);
                        issue([&] { return launch_mlp(p, s); });
                        break;
                    }
                    case OP_SE: {
                        const SeOp& se = op.se;
                        SeParams p;
                        p.pool = (const float*)tp(se.pool); p.scale = (float*)tp(se.scale); p.B = live; p.C = se.C;
                        p.Cs = plan.tensors[se.pool].C; p.Cmid = se.Cmid; p.inv_count = se.inv_count; p.nblocks = pool_blocks[se.pool] > 0 ? pool_blocks[se.pool] : se.nblocks; p.Mrows = se.Mrows;
                        p.w1 = (const float*)blobs[se.w1]; p.b1 = (const float*)blobs[se.b1]; p.w2 = (const float*)blobs[se.w2]; p.b2 = (const float*)blobs[se.b2];
                        issue([&] { return launch_se(p, s); });
                        break;
                    }
                    case OP_SCALE_ADD: {
                        const TensorDesc& d = plan.tensors[op.se.pool];
                        issue([&] { return launch_scale(tp(op.se.pool), (const float*)tp(op.se.scale), live, d.H * d.W, d.C, plan.elt == 4, s); });
                        break;
                    }
                    default: throw std::runtime_error("plan: unknown op kind");
                }
            }
        } catch (const std::exception& e) {     // name the op: "invalid argument" alone says nothing about a 60-op plan
            throw std::runtime_error("op " + launch_label(plan, L) + ": " + e.what());
        }
    }
    template <class TP> MlpParams mlp_params(const Op& op, int live, const TP& tp) const {
        const MlpOp& m = op.m;
        const TensorDesc& d = plan.tensors[m.x];
        MlpParams p;
        p.x = tp(m.x); p.y = tp(m.y); p.M = (long)live * d.H * d.W; p.C = m.C;
        p.w1 = blobs[m.w1]; p.b1 = (const float*)blobs[m.b1]; p.w2 = blobs[m.w2]; p.b2 = (const float*)blobs[m.b2];
        p.w1_frag = frag_blobs[m.w1]; p.w2_frag = frag_blobs[m.w2]; p.frag32 = mlp_frag32(m.C);
        p.eps = m.eps; p.stats_out = (float*)tp(m.stats_out); p.eps_out = m.eps_out;
        p.live_W = d.W; p.live_H = d.H;
        if (d.C != m.C || plan.tensors[m.y].C != m.C) throw std::runtime_error("plan: MLP width mismatch");
        return p;
    }
    // W2X_CHECK_GENERAL (diagnostic): the general kernel must agree with the shape-specialised launch of op i that just wrote p.out
    void check_against_general(const GemmParams& p, int i, int live) {
        const Op& op = plan.ops[i];
        const TensorDesc& od = plan.tensors[op.g.out.t];
        const size_t n = (size_t)live * od.H * od.W * od.C;
        std::vector<uint16_t> a(n), b(n);
        void* tmp = nullptr;
        hipAssert(hipMalloc(&tmp, n * 2));
        hipAssert(hipStreamSynchronize(stream));
        hipAssert(hipMemcpy(a.data(), p.out.p, n * 2, hipMemcpyDeviceToHost));
        hipAssert(hipMemcpy(tmp, p.out.p, n * 2, hipMemcpyDeviceToDevice));   // pixels neither kernel writes compare equal
        GemmParams q = p; q.out.p = tmp; q.pool_out = nullptr;   // the pooling partials of the real launch stay
        hipAssert(launch_gemm(q, stream));
        hipAssert(hipStreamSynchronize(stream));
        hipAssert(hipMemcpy(b.data(), tmp, n * 2, hipMemcpyDeviceToHost));
        hipAssert(hipFree(tmp));
        double md = 0; size_t at = 0, bad = 0;
        for (size_t k = 0; k < n; ++k) { const double d = std::fabs(f16_to_f32(a[k]) - f16_to_f32(b[k])); if (d > 0.01) ++bad; if (d > md) { md = d; at = k; } }
        log(Severity::warn, "pixgemm check op " + std::to_string(i) + " [" + op.name + "]: max|d|=" + std::to_string(md) + " at pixel " + std::to_string(at / od.C) +
            " ch " + std::to_string(at % od.C) + " (x=" + std::to_string(at / od.C % od.W) + ", y=" + std::to_string(at / od.C / od.W % od.H) + "), " + std::to_string(bad) + " of " + std::to_string(n) + " off by > 0.01");
    }

    template <class T> void ensure(T*& p, size_t& cap, size_t bytes) {
        if (bytes <= cap) return;
        drop_graphs();                        // captured passes hold the old addresses
        if (p) hipAssert(hipFree(p));
        p = nullptr; cap = 0;
        hipAssert(hipMalloc((void**)&p, bytes));
        cap = bytes;
    }

    // device part of one frame: gather -> network per batch -> the format's end of a frame (finish_frame).  Frame must already be in d_frame.
    // `started` (a single-frame call's ev0): recorded in front of the passes - of an RGBA frame behind its bleed, whose two-phase schedule is rgba_frame()
    void run_frame(int rows, int cols, const TileGrid& grid, bool report, const StripPlan& sp, hipEvent_t started = nullptr) {
        if (two_tile_sets()) { rgba_frame(rows, cols, grid, sp, report, started); return; }
        if (started) hipAssert(hipEventRecord(started, stream));
        run_passes(rows, cols, sp.tile_count, 0, report, 0, true);
        finish_frame(rows, cols, grid, sp, stream, nullptr, nullptr);
    }

    // One frame of a ROLLING sequence (benchResident, renderSequence): frames of one size, one after the other, whose passes all run as two tile groups.
    // A lone frame ends with a join (the first stream waits for the second group), then the compose launch runs alone, then the next frame forks again:
    // a tenth of a millisecond of compose plus the last tiles of the longer group with half the device idle, per frame.  Here nothing joins: the first
    // stream carries its group from pass to pass and from frame to frame; the second stream carries the other group and, behind it, the frame's compose
    // launch (which waits for the first stream's last pass of the frame by event) - so frame f is composed while frame f + 1's first group is already
    // running.  What that takes: a second tile slab (frame f + 1's tiles must not land on the tiles compose(f) is reading; `which` alternates), and
    // events instead of stream order where a buffer comes round again (ev_cmp).  Same launches on the same data: the frames are the bytes of render().
    // Returns false when the frame cannot roll (a pass that does not split, profiling, one group): the caller then runs run_frame().
    bool can_roll(int tile_count) const {
        return rolling_ok && groups == 2 && use_graphs && !profiling && !check_general && !poison && gstream[0] && last_pass_live(tile_count, cfg.tta ? 8 : 1, plan.B) >= 8 && plan.B % 2 == 0;
    }
    void run_rolling_frame(int rows, int cols, const TileGrid& grid, const StripPlan& sp, int which, hipEvent_t out_free) {
        for (int k = 0; k < 2; ++k) {
            if (!ev_g0[k]) hipAssert(hipEventCreateWithFlags(&ev_g0[k], hipEventDisableTiming));
            if (!ev_cmp[k]) hipAssert(hipEventCreateWithFlags(&ev_cmp[k], hipEventDisableTiming));
        }
        struct Swap { Impl* e; void* slab; size_t cap; bool on; ~Swap() { if (on) { std::swap(e->d_slab, e->d_slab2); std::swap(e->slab_cap, e->slab2_cap); } e->rolling = false; } } sw{this, d_slab, slab_cap, which == 1};
        if (which == 1) { std::swap(d_slab, d_slab2); std::swap(slab_cap, slab2_cap); }
        rolling = true;
        hipAssert(hipStreamWaitEvent(stream, ev_cmp[which], 0));          // the compose launch that last read this slab (two frames ago) is done (a never-recorded event does not wait)
        run_passes(rows, cols, sp.tile_count, 0, false, 0, true);
        hipAssert(hipEventRecord(ev_g0[which], stream));
        hipStream_t s2 = gstream[0];
        hipAssert(hipStreamWaitEvent(s2, ev_g0[which], 0));
        finish_frame(rows, cols, grid, sp, s2, ev_cmp[which], out_free);
    }
    // after the last frame of a rolling sequence: the first stream waits for the second, so that whatever follows on it sees the sequence done
    void end_rolling() { hipAssert(hipEventRecord(ev_join[0], gstream[0])); hipAssert(hipStreamWaitEvent(stream, ev_join[0], 0)); }
    // The error exit of the frame entry points: every stream that may still touch the caller's buffers, the slabs or d_out drains before the function returns
    // false - a frame in parts and a sequence copy to and from the caller's buffers on the side streams, and a rolling sequence composes on the second group's
    // stream (end_rolling() has not run when an exception fires).  Errors here are ignored, the first one is what gets reported; the next call starts outside a
    // rolling sequence.
    void drain_after_error() {
        rolling = false;
        for (hipStream_t st : {s_up, s_dn, gstream[0], stream}) if (st && hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError();
    }
    // What every frame entry point does around its own work `body` (which returns the call's result): refused with `not_ready` before a successful load (shardFinish: or before a shardCompute); the
    // engine's device current and the job back at its default on every exit; an exception drains the streams and is logged behind `failed`.
    template <class Body> bool entry(const char* who, const char* not_ready, const char* failed, const Body& body) try {
        if (!loaded) { log(Severity::error, not_ready, who, __LINE__); return false; }
        DeviceGuard guard(device);
        JobScope job_scope{this};
        return body();
    } catch (const std::exception& e) {
        drain_after_error();
        log(Severity::error, failed + std::string(e.what()) + ".", who, __LINE__);
        return false;
    }

    // The graphs of one pass into `pg`: run_pass() captured on the compute stream, or (per_group) run_group(c) on the stream of each of the `ngroups` tile groups,
    // each instantiated.  Returns "" or the step that failed and the runtime's text; then `pg` holds the graphs made before it, for the caller to destroy.
    template <class RunGroup, class RunPass>
    std::string capture_pass(bool per_group, int ngroups, const RunGroup& run_group, const RunPass& run_pass, PassGraphs& pg) {
        std::string why;
        const int ncap = per_group ? ngroups : 1;
        for (int c = 0; c < ncap && why.empty(); ++c) {
            hipStream_t cs = per_group && c ? gstream[c - 1] : stream;
            hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
            hipError_t ge = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
            if (ge != hipSuccess) { why = std::string("begin capture: ") + hipGetErrorString(ge); break; }
            try { if (per_group) run_group(c); else run_pass(); } catch (const std::exception& e) { why = std::string("capture: ") + e.what(); }
            ge = hipStreamEndCapture(cs, &graph);
            if (why.empty() && ge != hipSuccess) why = std::string("end capture: ") + hipGetErrorString(ge);
            if (why.empty()) { ge = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0); if (ge != hipSuccess) why = std::string("instantiation: ") + hipGetErrorString(ge); }
            if (graph) (void)hipGraphDestroy(graph);
            if (why.empty()) pg.g[pg.n++] = exec;
        }
        return why;
    }

    // the network passes of `tile_count` tiles (slots d_slots[slots_off ..]); their outputs go to slab slots slab_slot0, slab_slot0 + 1, ...
    // fresh: the first passes of a frame (W2X_POISON wipes the arena and the slab here, not between the parts of a pipelined frame)
    // pass0 / pass1: only the passes [pass0, pass1) of that schedule (pass1 < 0: to its end)
    void run_passes(int rows, int cols, int tile_count, size_t slab_slot0, bool report, size_t slots_off, bool fresh, int batch0 = 0, int batch_total = 0, int pass0 = 0, int pass1 = -1) {
        const int B = plan.B, T = plan.T, To = plan.Tout;
        const int steps = cfg.tta ? 8 : 1;
        const int userB = plan.userB, S = B / userB;
        const int batchCount = batch_count(tile_count);
        const int passCount = (int)(pass_slots(tile_count) / B);
        const size_t slot_bytes = (size_t)To * To * 4 * plan.elt;
        if (poison && fresh) {
            hipAssert(hipMemsetAsync(arena_base, 0x7E, arena_bytes, stream));
            hipAssert(hipMemsetAsync(d_slab, 0x7E, slab_cap, stream));
        }
        // (W2X_POISON fills the whole arena before the frame and so runs the default path: tile groups in their arena parts, replayed graphs)
        const bool graphable = use_graphs && !profiling && !check_general;
        for (int bi = pass0; bi < (pass1 < 0 ? passCount : std::min(pass1, passCount)); ++bi) {
            const auto t0 = std::chrono::steady_clock::now();
            const int live = std::max(0, std::min(B, tile_count * steps - bi * B));
            void* const slab_out = (uint8_t*)d_slab + (slab_slot0 + (size_t)bi * B) * slot_bytes;
            GatherParams gp0;
            gp0.frame = d_frame; gp0.rows = rows; gp0.cols = cols; gp0.step = bgr_step(cols, deep); gp0.deep = deep ? 1 : 0;
            gp0.out = tensors[plan.in_tensor]; gp0.slots = d_slots + slots_off + (size_t)bi * B; gp0.B = B; gp0.T = T; gp0.fp32 = plan.elt == 4;
            const int NG = groups;
            struct NgReset { int& r; ~NgReset() { r = 1; } } ng_reset{ng_now};   // also when a launch throws mid-pass
            ng_now = NG;                                                          // (arena_part() is the part of an NG-group pass)
            const bool split = NG > 1 && !profiling && !check_general && live >= 4 * NG && B % NG == 0 && (size_t)NG * arena_part() <= arena_bytes + 1024;
            ng_now = 1;
            // NG tile groups side by side: tiles never exchange data, so the groups run the same launches on their own streams in
            // their own parts of the arena.  Each kernel then has 1/NG of the workgroups, but a kernel's ramp and tail (and the
            // gaps between launches) fill with the other groups' work.  Bit-identical by construction.
            int first[5] = {0, 0, 0, 0, 0};
            for (int grp = 0; grp < NG; ++grp) first[grp + 1] = first[grp] + live / NG + (grp < live % NG ? 1 : 0);
            if (split) {
                if (!ev_fork) hipAssert(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
                for (int k = 0; k + 1 < NG; ++k) if (!gstream[k]) {
                    hipAssert(hipStreamCreateWithFlags(&gstream[k], hipStreamNonBlocking));
                    hipAssert(hipEventCreateWithFlags(&ev_join[k], hipEventDisableTiming));
                }
            }
            auto group_stream = [&](int grp) { return grp ? gstream[grp - 1] : stream; };
            auto gather_group = [&](int grp, hipStream_t gs) {       // the group's tiles at the start of its part of the arena
                GatherParams gp = gp0;
                gp.out = group_ptr(tensors[plan.in_tensor], grp); gp.slots = gp0.slots + (size_t)first[grp]; gp.B = first[grp + 1] - first[grp];
                gather_tiles(gp, gs);
            };
            const LiveExt* const ext0 = d_live && slots_off + (size_t)(bi + 1) * B <= live_stride ? d_live + slots_off + (size_t)bi * B : nullptr;   // this pass's slots in op 0's table
            auto network_group = [&](int grp, hipStream_t gs) { run_network((uint8_t*)slab_out + (size_t)first[grp] * slot_bytes, first[grp + 1] - first[grp], grp, gs, ext0 ? ext0 + first[grp] : nullptr); };
            auto fork = [&] { hipAssert(hipEventRecord(ev_fork, stream)); for (int grp = 1; grp < NG; ++grp) hipAssert(hipStreamWaitEvent(gstream[grp - 1], ev_fork, 0)); };
            auto join = [&] { for (int grp = 1; grp < NG; ++grp) { hipAssert(hipEventRecord(ev_join[grp - 1], gstream[grp - 1])); hipAssert(hipStreamWaitEvent(stream, ev_join[grp - 1], 0)); } };
            // the whole pass as launches issued from `stream` (the groups forked off it by events: capturable as ONE graph with NG branches)
            auto run_pass = [&] {
                if (!split) {
                    stamp_begin(3, 0);
                    gather_tiles(gp0, stream);
                    stamp_end();
                    run_network(slab_out, live, -1, nullptr, ext0);
                    return;
                }
                ng_now = NG;
                for (int grp = 0; grp < NG; ++grp) gather_group(grp, stream);
                fork();
                for (int grp = 0; grp < NG; ++grp) network_group(grp, group_stream(grp));
                join();
                ng_now = 1;
            };
            // one group of a split pass, gather included, as launches on ONE stream (capturable as a straight-line graph)
            auto run_group = [&](int grp) { ng_now = NG; gather_group(grp, group_stream(grp)); network_group(grp, group_stream(grp)); ng_now = 1; };
            const bool per_group = split;
            // (a rolling sequence leaves the groups un-joined: each stream carries its group from pass to pass and from frame to frame, run_rolling_frame)
            const bool no_join = rolling && split;
            auto run_eager = [&] { if (per_group) { fork(); for (int grp = 0; grp < NG; ++grp) run_group(grp); if (!no_join) join(); } else { if (rolling && gstream[0]) { join(); } run_pass(); } };
            if (!graphable) run_eager();
            else {
                const GraphKey key{pass_source(), d_slots + slots_off + (size_t)bi * B, slab_out, arena_base, rows, cols, live, sample_format()};
                auto replay = [&](const PassGraphs& pg) {
                    if (pg.n == 1) { if (rolling && gstream[0]) join(); hipAssert(hipGraphLaunch(pg.g[0], stream)); return; }   // (a whole-arena pass inside a rolling sequence: the other stream's group first)
                    fork();
                    for (int grp = 0; grp < pg.n; ++grp) hipAssert(hipGraphLaunch(pg.g[grp], group_stream(grp)));
                    if (!no_join) join();
                };
                auto it = graphs.find(key);
                if (it != graphs.end()) { replay(it->second); ++graph_replays; }
                else if (graph_seen.size() >= 4096 && !graph_seen.count(key)) { graph_seen.clear(); run_eager(); ++eager_passes; }   // sizes that keep changing: bounded bookkeeping
                else if (graph_seen[key]++ == 0 && !(rolling && !graphs.empty())) { run_eager(); ++eager_passes; }   // (a rolling frame on the second slab repeats launches that have run: captured at first sight)
                else {
                    if (graphs.size() >= 1024) drop_graphs();      // frames of ever-changing sizes: start over rather than grow without bound
                    // Capture -> instantiate -> launch.  Nothing runs while a stream captures, so whatever fails on the way (begin,
                    // a capture invalidated by a runtime call inside a launcher, end, instantiate) the pass is still to be done:
                    // graphs are switched off for good (otherwise every later frame would retry and fail again) and it runs on plain launches.
                    PassGraphs pg;
                    if (const std::string why = capture_pass(per_group, NG, run_group, run_pass, pg); !why.empty()) {
                        (void)hipGetLastError();
                        for (int c = 0; c < pg.n; ++c) (void)hipGraphExecDestroy(pg.g[c]);
                        use_graphs = false;
                        log(Severity::warn, "hipGraph " + why + " - passes stay on plain launches");
                        run_eager(); ++eager_passes;          // a real launch error surfaces here, outside the capture
                    } else {
                        graphs[key] = pg;
                        replay(pg); ++graph_replays;
                    }
                }
            }
            if (report) {
                const auto t1 = std::chrono::steady_clock::now();
                const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
                for (int k = bi * S; k < std::min((bi + 1) * S, batchCount); ++k)
                    log(batch0 + k + 1, batch_total > 0 ? batch_total : batchCount, 1000.0 * S / std::max(ms, 1e-6));                     // :336-338
            }
        }
        last_batches = batch0 + batchCount;
    }

    // compose: output columns [x0, x1) (x1 = 0: to the right edge) and rows [y0, y1) (y1 = 0: to the bottom) from the slab, whose slot 0 holds
    // global tile `first_tile`
    void compose_rect(int rows, int cols, const TileGrid& grid, int x0, int x1, int y0, int y1, long first_tile, hipStream_t on = nullptr) {
        ComposeParams cp = compose_base(rows, cols, grid);
        cp.dst = d_out; cp.dst_step = bgr_step(cp.outW, deep); cp.deep = deep ? 1 : 0;
        cp.x0 = x0; cp.x1 = x1; cp.y0 = y0; cp.y1 = y1; cp.first_tile = first_tile;
        stamp_begin(4, 0);
        hipAssert(launch_compose(cp, on ? on : stream, dither_now()));
        stamp_end();
    }
    // what every compose launch shares: the slab, the canvas size, the tile grid and its strides, the blend ramps, the TTA flags
    ComposeParams compose_base(int rows, int cols, const TileGrid& grid) const {
        const int To = plan.Tout;
        ComposeParams cp;
        cp.tiles = d_slab; cp.fp32 = plan.elt == 4;
        cp.outW = cols * cfg.scaling; cp.outH = rows * cfg.scaling; cp.To = To;
        cp.nx = grid.nx; cp.ny = grid.ny; cp.stride_x = To - grid.outOvX; cp.stride_y = To - grid.outOvY;
        const bool overlapping = cfg.overlapX != 0 || cfg.overlapY != 0;                      // :244
        cp.ovx = overlapping ? ovx : 0; cp.ovy = overlapping ? ovy : 0;
        cp.ramp_x = d_rampx; cp.ramp_y = d_rampy; cp.tta = cfg.tta ? 1 : 0; cp.tta_bug_compat = cfg.ttaBugCompat ? 1 : 0;
        return cp;
    }
    // what the four resample launches share: the canvas, its size and the target's, and the tap tables of job.rs
    template <class Params> void resample_base(Params& rp) const {
        const ResizeTables* const rs = job.rs;
        rp.canvas = d_canvas; rp.inW = rs->inW; rp.inH = rs->inH;
        rp.outW = rs->outW; rp.outH = rs->outH;
        rp.fx = rs->fx; rp.wx = rs->wx; rp.kx = rs->kx; rp.fy = rs->fy; rp.wy = rs->wy; rp.ky = rs->ky; rp.rows_max = rs->rows_max;
    }
    // The device layouts the formats are made of.  BGR: packed rows.  YUV: Y, U, V
    // (NV12: Y, UV) one after the other, rows padded to 16 bytes (the stores of the compose kernels).
    static size_t bgr_step(int cols, bool deep16) { return (size_t)cols * 3 * (deep16 ? 2 : 1); }
    static YuvPlanes yuv_layout(uint8_t* base, int rows, int cols, int bits, int layout) {
        const size_t bps = bits > 8 ? 2 : 1;
        const int cw = yuv_chroma_samples(cols, layout), ch = yuv_chroma_rows(rows, layout);
        YuvPlanes f;
        f.rows = rows; f.cols = cols; f.bits = bits; f.layout = layout;
        f.step[0] = ((size_t)cols * bps + 15) / 16 * 16; f.step[1] = f.step[2] = ((size_t)cw * bps + 15) / 16 * 16;
        f.p[0] = base; f.p[1] = base + f.step[0] * rows; f.p[2] = layout == kYuvNV12 ? nullptr : f.p[1] + f.step[1] * ch;
        return f;
    }
    // Planar RGB: R, G, B one after the other, every plane's rows padded to 16 bytes like the planes of yuv_layout, at 1, 2 or 4 bytes per sample.  Gray: the
    // same with one plane.
    static size_t planar_step(int cols, int bits) { return ((size_t)cols * planar_sample_bytes(bits) + 15) / 16 * 16; }
    static PlanarPlanes planar_layout(uint8_t* base, int rows, int cols, int bits, int n = 3) {
        PlanarPlanes f;
        f.rows = rows; f.cols = cols; f.bits = bits; f.n = n;
        for (int k = 0; k < n; ++k) { f.step[k] = planar_step(cols, bits); f.p[k] = base + (size_t)k * f.step[k] * rows; }
        return f;
    }
    static int planar_key(int bits) { return kPlanarKey + (bits == 8 ? 0 : bits == 10 ? 1 : bits == 12 ? 2 : bits == 16 ? 3 : 4); }
    static int yuv_planes(int layout) { return layout == kYuvNV12 ? 2 : 3; }
    static size_t yuv_bytes(int rows, int cols, int bits, int layout) {
        const YuvPlanes f = yuv_layout(nullptr, rows, cols, bits, layout);
        return f.step[0] * rows + (yuv_planes(layout) - 1) * f.step[1] * yuv_chroma_rows(rows, layout);
    }

    // ---- The frame formats: what a Job::Kind does at each device step, each step written once with one switch over job.kind.  Outside this block
    // only the places that set a job's kind name one (run_frame() hands a frame of two tile sets to rgba_frame() through two_tile_sets()).  A new format is a case in each function here, a
    // checker and an entry point that sets its job ("Adding a frame format").
    //
    // The key of a captured pass: the sample format - 0 / 1 BGR of 8 / 16 bits, 2 .. 49 YuvJob::key, kRgbaKey, kGrayKey / kGrayKey + 1 gray of 8 / 16 bits, kPlanarKey .. + 4 planar by
    // input depth, kPlanarRgbaKey .. + 4 planar RGBA likewise - and the buffer the pass's gather reads (an RGBA or planar RGBA pass reads d_bgr / d_alpha, never d_frame: its graphs do not depend on which frame buffer of a sequence is current)
    // The edge mode is part of it too (kEdgeKey per mode, above every format's key): the gather kernel a captured pass bakes in is an instantiation per mode, and
    // a call after setEdge() must not replay the old one.
    static constexpr int kEdgeKey = 1024;
    int sample_format() const { return frame_format() + kEdgeKey * edge; }
    int frame_format() const {
        if (job.chain.src) return kChainKey;
        switch (job.kind) {
            case Job::YUV: return job.yuv.key;
            case Job::RGBA: return kRgbaKey;
            case Job::GRAY: return kGrayKey + (job.gray.deep ? 1 : 0);
            case Job::PLANAR: return planar_key(job.planar.in_bits);
            case Job::PLANAR_RGBA: return planar_key(job.planar.in_bits) - kPlanarKey + kPlanarRgbaKey;
            default: return deep ? 1 : 0;
        }
    }
    // gray and planar frames: the sample depth of the frame (`out`: of the output) and its planes in d_frame / d_out
    int plane_bits(bool out) const { return job.kind == Job::GRAY ? (job.gray.deep ? 16 : 8) : out ? job.planar.out_bits : job.planar.in_bits; }
    PlanarPlanes frame_planes(uint8_t* base, int rows, int cols, bool out) const { return planar_layout(base, rows, cols, plane_bits(out), job.kind == Job::GRAY ? 1 : 3); }
    const void* pass_source() const { return job.chain.src ? job.chain.src : two_tile_sets() ? (const void*)d_bgr : (const void*)d_frame; }
    // RGBA and planar RGBA frames: colour tiles and alpha tiles in one schedule (rgba_setup, rgba_frame), gathered from d_bgr / d_alpha
    bool two_tile_sets() const { return job.kind == Job::RGBA || job.kind == Job::PLANAR_RGBA; }
    RgbaPlanes rgba_planes(uint8_t* base, int rows, int cols, bool out) const {
        const int bits = plane_bits(out);
        RgbaPlanes f;
        f.rows = rows; f.cols = cols; f.bits = bits;
        for (int k = 0; k < 4; ++k) { f.step[k] = planar_step(cols, bits); f.p[k] = base + (size_t)k * f.step[k] * rows; }
        return f;
    }
    // What the bleed of such a frame works with: the bytes of one of the four planes it writes (RGBA: a byte per pixel, three of them per BGR pixel), the top of
    // the alpha key range its two words are reduced over, and its launch - from d_frame into d_bgr / d_alpha / d_minmax on `stream`
    size_t bleed_plane_bytes(int rows, int cols) const { return job.kind == Job::PLANAR_RGBA ? planar_step(cols, job.planar.in_bits) * rows : (size_t)rows * cols; }
    unsigned alpha_top() const { return job.kind == Job::PLANAR_RGBA ? alpha_key_top(job.planar.in_bits) : 255u; }
    void launch_bleed(int rows, int cols, int radius) {
        if (job.kind == Job::PLANAR_RGBA) {
            AlphaBleedPlanesParams bp;
            bp.src = rgba_planes(d_frame, rows, cols, false); bp.radius = radius;
            bp.colour_step = bp.alpha_step = planar_step(cols, job.planar.in_bits);
            for (int k = 0; k < 3; ++k) bp.colour[k] = d_bgr + (size_t)k * bp.colour_step * rows;
            bp.alpha = d_alpha; bp.minmax = d_minmax;
            hipAssert(launch_alpha_bleed_planes(bp, stream, edge == kEdgeWrap));
            return;
        }
        AlphaBleedParams bp;
        bp.bgra = d_frame; bp.step = (size_t)cols * 4; bp.rows = rows; bp.cols = cols; bp.radius = radius;
        bp.bgr = d_bgr; bp.bgr_step = (size_t)cols * 3; bp.alpha = d_alpha; bp.alpha_step = (size_t)cols; bp.minmax = d_minmax;
        hipAssert(launch_alpha_bleed(bp, stream, edge == kEdgeWrap));
    }
    // the value of a uniform alpha plane as the gather would read it, from its key (job.rgba.value)
    float uniform_alpha() const {
        const int bits = job.planar.in_bits;
        if (bits == 32) { float v; memcpy(&v, &job.rgba.value, sizeof v); return v; }
        return (float)job.rgba.value * (float)(1.0 / (double)((1 << bits) - 1));
    }
    // The device layout of a frame: bytes per row and bytes of a rows x cols frame in d_frame, or (`out`) in d_out.  A YUV frame has a step per plane
    // (yuv_layout); frame_step() gives its Y plane's.
    size_t frame_step(int cols, bool out) const {
        switch (job.kind) {
            case Job::YUV: return yuv_layout(nullptr, 0, cols, out ? job.yuv.out_bits : job.yuv.in_bits, out ? job.yuv.out_layout : job.yuv.in_layout).step[0];
            case Job::RGBA: return (size_t)cols * 4;
            case Job::GRAY: case Job::PLANAR: case Job::PLANAR_RGBA: return planar_step(cols, plane_bits(out));
            default: return bgr_step(cols, deep);
        }
    }
    size_t frame_bytes(int rows, int cols, bool out) const {
        if (job.kind == Job::YUV) return yuv_bytes(rows, cols, out ? job.yuv.out_bits : job.yuv.in_bits, out ? job.yuv.out_layout : job.yuv.in_layout);
        return frame_step(cols, out) * rows * (job.kind == Job::PLANAR ? 3 : job.kind == Job::PLANAR_RGBA ? 4 : 1);
    }
    // the fp32 planes of a resized frame's canvas
    int canvas_planes() const { return two_tile_sets() ? 4 : job.kind == Job::GRAY ? 1 : 3; }
    // RGBA and planar RGBA frames do not roll: d_bgr, d_alpha and d_minmax are single buffers the bleed writes on the compute stream, and in a rolling sequence the second
    // tile group of frame f would still gather from them while frame f + 1 bleeds into them.  Through run_frame() every pass joins its groups before the
    // next launch on `stream`, so stream order alone keeps the single buffers (and the one slab and canvas) safe.
    bool rolls() const { return !two_tile_sets(); }
    // only BGR frames are what benchResident / residentOutput / profileFrame replay out of d_frame / d_out
    bool replayable() const { return job.kind == Job::BGR; }
    // the slot table, the liveness table and the slab the frames of a call share: every tile of the frame in one part, RGBA and planar RGBA the 2N schedule (rgba_setup)
    void call_slots(int rows, int cols, const TileGrid& grid, const StripPlan& sp) {
        if (two_tile_sets()) { rgba_setup(rows, cols, grid, job.rgba.skip); return; }
        const size_t stepCount = pass_slots(sp.tile_count);
        fill_slots(grid, 0, sp.tile_count, 1, 0, stepCount);
        upload_slots(grid, stepCount, stepCount);
        hipAssert(hipStreamSynchronize(stream));
    }
    // The gather of a pass (or of one tile group of it): the tiles of gp.slots out of the frame.  `gp` carries the BGR frame; the other formats take its tile side.
    template <class P> static P tile_side(const GatherParams& gp) { P p; p.out = gp.out; p.fp32 = gp.fp32; p.slots = gp.slots; p.B = gp.B; p.T = gp.T; return p; }
    void gather_tiles(const GatherParams& gp, hipStream_t gs) {
        if (job.chain.src) {                                          // a later stage of a chained render: the tiles copied out of the frame of tile pixels
            GatherPxParams p = tile_side<GatherPxParams>(gp);
            p.frame = job.chain.src; p.rows = gp.rows; p.cols = gp.cols;
            hipAssert(launch_gather_px(p, gs, edge));
            return;
        }
        switch (job.kind) {
            case Job::BGR: hipAssert(launch_gather(gp, gs, edge)); break;
            case Job::YUV: {                                          // the same tiles from the frame's planes
                GatherYuvParams p = tile_side<GatherYuvParams>(gp);
                p.src = yuv_layout(d_frame, gp.rows, gp.cols, job.yuv.in_bits, job.yuv.in_layout); p.src.siting = job.yuv.in_siting; p.k = job.yuv.in;
                hipAssert(launch_gather_yuv(p, gs));
                break;
            }
            case Job::RGBA: {                                         // from the bled BGR frame or the alpha plane
                GatherRgbaParams p = tile_side<GatherRgbaParams>(gp);
                p.bgr = d_bgr; p.bgr_step = (size_t)gp.cols * 3; p.alpha = d_alpha; p.alpha_step = (size_t)gp.cols; p.rows = gp.rows; p.cols = gp.cols;
                hipAssert(launch_gather_rgba(p, gs, edge));
                break;
            }
            case Job::GRAY: case Job::PLANAR: {                       // from the frame's one plane or three
                GatherPlanarParams p = tile_side<GatherPlanarParams>(gp);
                p.src = frame_planes(d_frame, gp.rows, gp.cols, false);
                hipAssert(launch_gather_planar(p, gs, edge));
                break;
            }
            case Job::PLANAR_RGBA: {                                  // from the bled colour planes or the alpha plane
                GatherPlanarRgbaParams p = tile_side<GatherPlanarRgbaParams>(gp);
                p.rows = gp.rows; p.cols = gp.cols; p.bits = job.planar.in_bits;
                p.colour_step = p.alpha_step = planar_step(gp.cols, p.bits);
                for (int k = 0; k < 3; ++k) p.colour[k] = d_bgr + (size_t)k * p.colour_step * gp.rows;
                p.alpha = d_alpha;
                hipAssert(launch_gather_planar_rgba(p, gs, edge));
                break;
            }
        }
    }
    // The three launches that can end a frame, all over the whole canvas of the frame's tiles (one part, slot 0 = tile 0; BGR: the strip's columns): the canvas
    // as fp32 planes into d_canvas (RGBA: R, G, B, A - uniform: three; gray: one), the resize of d_canvas into d_out (rs->outW x rs->outH), or the canvas
    // quantised straight into d_out.  RGBA: colour tiles from slab slot 0, alpha tiles from slot job.rgba.alpha_slot0 (uniform: none, A = value).
    const void* alpha_tiles() const { return job.rgba.uniform ? nullptr : (const uint8_t*)d_slab + job.rgba.alpha_slot0 * (size_t)plan.Tout * plan.Tout * 4 * plan.elt; }
    void compose_canvas(int rows, int cols, const TileGrid& grid, hipStream_t on) {
        const ComposeParams cp = compose_base(rows, cols, grid);
        switch (job.kind) {
            case Job::RGBA: case Job::PLANAR_RGBA: {                  // (the same four fp32 planes)
                ComposeCanvasRgbaParams p;
                p.c = cp; p.alpha_tiles = alpha_tiles(); p.canvas = d_canvas;
                hipAssert(launch_compose_canvas_rgba(p, on, light_now()));
                break;
            }
            case Job::GRAY: hipAssert(launch_compose_canvas_gray(cp, d_canvas, on, light_now())); break;
            default: hipAssert(launch_compose_canvas(cp, d_canvas, on, light_now()));
        }
    }
    // (the edge mode of a resize launch is the one its tables were made under: job.rs->edge)
    EdgeArgs resize_edge() const { EdgeArgs e; e.mode = job.rs->edge; return e; }
    template <class P> void resample_into(P& p, hipStream_t on, hipError_t (*launch)(const P&, hipStream_t, const DitherArgs&, const LightArgs&, const EdgeArgs&)) {
        resample_base(p);
        p.dst = d_out; p.dst_step = frame_step(p.outW, true);
        hipAssert(launch(p, on, dither_now(), light_now(), resize_edge()));
    }
    void resample(hipStream_t on) {
        switch (job.kind) {
            case Job::BGR: { ResampleParams p; p.deep = deep ? 1 : 0; resample_into(p, on, launch_resample); break; }
            case Job::RGBA: { ResampleRgbaParams p; p.uniform = job.rgba.uniform ? 1 : 0; p.alpha_value = job.rgba.value; resample_into(p, on, launch_resample_rgba); break; }
            case Job::GRAY: case Job::PLANAR: {                       // the one plane or three of the target size
                ResamplePlanarParams p;
                resample_base(p);
                p.dst = frame_planes(d_out, p.outH, p.outW, true);
                hipAssert(launch_resample_planar(p, on, dither_now(), light_now(), resize_edge()));
                break;
            }
            case Job::PLANAR_RGBA: {                                  // the four planes of the target size
                ResamplePlanarRgbaParams p;
                resample_base(p);
                p.dst = rgba_planes(d_out, p.outH, p.outW, true);
                p.uniform = job.rgba.uniform ? 1 : 0; p.alpha_value = uniform_alpha();
                hipAssert(launch_resample_planar_rgba(p, on, dither_now(), light_now(), resize_edge()));
                break;
            }
            case Job::YUV: {                                          // the planes of job.yuv.out_layout at the target size
                ResampleYuvParams p;
                resample_base(p);
                p.dst = yuv_layout(d_out, p.outH, p.outW, job.yuv.out_bits, job.yuv.out_layout); p.dst.siting = job.yuv.out_siting; p.k = job.yuv.out;
                hipAssert(launch_resample_yuv(p, job.rs->rows_max_above, on, dither_now(), light_now()));
                break;
            }
        }
    }
    void compose(int rows, int cols, const TileGrid& grid, const StripPlan& sp, hipStream_t on) {
        switch (job.kind) {
            case Job::BGR: compose_rect(rows, cols, grid, sp.x0, sp.x1, 0, 0, sp.first_tile, on); break;
            case Job::YUV: {                                          // the planes of job.yuv.out_layout
                ComposeYuvParams p;
                p.c = compose_base(rows, cols, grid);
                p.dst = yuv_layout(d_out, p.c.outH, p.c.outW, job.yuv.out_bits, job.yuv.out_layout); p.dst.siting = job.yuv.out_siting; p.k = job.yuv.out;
                stamp_begin(4, 0);
                hipAssert(launch_compose_yuv(p, on, dither_now()));
                stamp_end();
                break;
            }
            case Job::RGBA: {                                         // BGRA dwords
                ComposeRgbaParams p;
                p.c = compose_base(rows, cols, grid);
                p.c.dst = d_out; p.c.dst_step = frame_step(p.c.outW, true);
                p.alpha_tiles = alpha_tiles(); p.alpha_value = job.rgba.value;
                hipAssert(launch_compose_rgba(p, on, dither_now()));
                break;
            }
            case Job::PLANAR_RGBA: {                                  // four planes of job.planar.out_bits
                ComposePlanarRgbaParams p;
                p.c = compose_base(rows, cols, grid);
                p.dst = rgba_planes(d_out, p.c.outH, p.c.outW, true);
                p.alpha_tiles = alpha_tiles(); p.alpha_value = uniform_alpha();
                hipAssert(launch_compose_planar_rgba(p, on, dither_now()));
                break;
            }
            case Job::GRAY: case Job::PLANAR: {                       // one sample per pixel, or three planes of job.planar.out_bits
                ComposePlanarParams p;
                p.c = compose_base(rows, cols, grid);
                p.dst = frame_planes(d_out, p.c.outH, p.c.outW, true);
                stamp_begin(4, 0);
                hipAssert(launch_compose_planar(p, on, dither_now()));
                stamp_end();
                break;
            }
        }
    }
    // The end of a frame on stream `on`, behind its passes.  Resized (job.rs): the canvas compose is the slab's last reader, the resample the writer of d_out; in
    // order on `on`, they share one canvas.  `slab_read`: recorded behind the slab's last reader; `out_free`: the frame that last left through this output buffer
    // has been downloaded (a rolling sequence gives both, run_frame() and rgba_frame() neither: stream order serves).
    void finish_frame(int rows, int cols, const TileGrid& grid, const StripPlan& sp, hipStream_t on, hipEvent_t slab_read, hipEvent_t out_free) {
        if (job.chain.dst) {                                          // an earlier stage of a chained render: the canvas as the next stage's frame of tile pixels
            ComposePxParams p;
            p.c = compose_base(rows, cols, grid); p.frame = job.chain.dst; p.frame_fp32 = job.chain.dst_fp32 ? 1 : 0;
            hipAssert(launch_compose_px(p, on));
            if (slab_read) hipAssert(hipEventRecord(slab_read, on));
            return;
        }
        if (job.rs) {
            compose_canvas(rows, cols, grid, on);
            if (slab_read) hipAssert(hipEventRecord(slab_read, on));
            if (out_free) hipAssert(hipStreamWaitEvent(on, out_free, 0));
            resample(on);
            return;
        }
        if (out_free) hipAssert(hipStreamWaitEvent(on, out_free, 0));
        compose(rows, cols, grid, sp, on);
        if (slab_read) hipAssert(hipEventRecord(slab_read, on));
    }
    // ---- (end of the frame formats)

    // RGBA frames (renderRgba / alphaBleed): the BGRA frame into d_frame, the two words zeroed, alpha_bleed_kernel -> d_bgr, d_alpha, d_minmax; all on `stream`
    void upload_and_bleed(const Image& src, int radius) {
        const int rows = src.rows, cols = src.cols;
        ensure(d_frame, frame_cap, (size_t)rows * cols * 4);
        ensure_bleed_planes(rows, cols);
        hipAssert(hipMemcpy2DAsync(d_frame, (size_t)cols * 4, src.data, src.step, (size_t)cols * 4, rows, hipMemcpyHostToDevice, stream));
        bleed_frame(rows, cols, radius);
    }
    void ensure_bleed_planes(int rows, int cols) {
        const size_t plane = bleed_plane_bytes(rows, cols);
        ensure(d_bgr, bgr_cap, plane * 3);
        ensure(d_alpha, alpha_cap, plane);
        if (!d_minmax) hipAssert(hipMalloc((void**)&d_minmax, 2 * sizeof(unsigned)));
    }
    // the frame in d_frame (BGRA, packed; planar RGBA: its four planes) -> d_bgr, d_alpha, d_minmax, on `stream`
    void bleed_frame(int rows, int cols, int radius) {
        hipAssert(hipMemsetAsync(d_minmax, 0, 2 * sizeof(unsigned), stream));
        launch_bleed(rows, cols, radius);
    }

    // ---- The frame calls: one record, one checker per format, one runner.  An entry point checks (X_check fills the record or returns the first refusal's
    // text), sets the job of its format, and hands the record and its two copy lambdas to run_call() - render() / renderStrip() (renderPart) hand theirs to
    // run_frame() or, for a frame in pipelined parts, run_frame_in_parts().
    struct FrameCall { int rows = 0, cols = 0, out_rows = 0, out_cols = 0; bool resized = false; TileGrid grid; StripPlan sp; };
    // The pieces the checkers share, where text and position agree.  call_target(): the sizes of the call into `c` - with a resize filter the target is the size of
    // the first output image, else the scaled size; at the scaled size a resized call is the plain one - and why a call with a filter (`any_filter` false: only a
    // resized one) cannot have that target, or "".  out_size_text(): the refusal of an output of another size.  call_grid(): the last check, the tile grid (and its one strip).
    template <class Img> std::string call_target(int resizeFilter, const Img& dst0, int rows, int cols, bool any_filter, FrameCall& c) const {
        const int s = cfg.scaling;
        c.rows = rows; c.cols = cols; c.out_rows = resizeFilter >= 0 ? dst0.rows : rows * s; c.out_cols = resizeFilter >= 0 ? dst0.cols : cols * s;
        c.resized = resizeFilter >= 0 && !(c.out_rows == rows * s && c.out_cols == cols * s);
        return (any_filter ? resizeFilter >= 0 : c.resized) ? resize_problem(rows, cols, c.out_rows, c.out_cols, resizeFilter) : "";
    }
    static std::string out_size_text(const FrameCall& c) { return "Output image has invalid size: expected " + std::to_string(c.out_cols) + "x" + std::to_string(c.out_rows) + "."; }
    std::string call_grid(FrameCall& c) const {
        const std::string why = frame_grid(c.rows, c.cols, c.grid);
        if (why.empty()) c.sp = strip_plan(c.grid, c.cols * cfg.scaling, plan.Tout, 0, 1);
        return why;
    }
    // renderSequence / renderSequenceResized.  At the scaled size a resized sequence is the plain one: no filter is looked at.  (Not const: `deep` is written
    // between the target and the per-frame checks, where it always was.)
    std::string bgr_sequence_check(const Image* srcs, const Image* dsts, int count, int resizeFilter, const char* who, FrameCall& c) {
        for (int i = 0; i < count; ++i) if (srcs[i].depth != 8 || dsts[i].depth != 8) return std::string(who) + " takes 8-bit frames (16-bit images go through render()).";
        if (const std::string why = call_target(resizeFilter, dsts[0], srcs[0].rows, srcs[0].cols, false, c); !why.empty()) return why;
        deep = false;
        for (int i = 0; i < count; ++i) {
            if (!srcs[i].data || srcs[i].rows != c.rows || srcs[i].cols != c.cols || srcs[i].step < (size_t)c.cols * 3 || c.rows <= 0 || c.cols <= 0) return "Input images must be non-empty and of one size.";
            if (!dsts[i].data || dsts[i].rows != c.out_rows || dsts[i].cols != c.out_cols || dsts[i].step < (size_t)c.out_cols * 3) return out_size_text(c);
        }
        return call_grid(c);
    }
    // render / renderResized / renderStrip: one frame of 8 or 16 bits, or strip `part` of `parts` of it (c.sp is that strip; it has no tiles when there are more
    // strips than tile columns).  At the scaled size a resized frame is the plain one.
    std::string bgr_frame_check(const Image& src, const Image& dst, int part, int parts, int resizeFilter, FrameCall& c) const {
        if (parts <= 0 || part < 0 || part >= parts) return "Invalid strip index.";
        if ((src.depth != 8 && src.depth != 16) || dst.depth != src.depth) return "Input and output images must both be 8-bit or both 16-bit.";
        const size_t px = (size_t)3 * (src.depth / 8);                 // bytes per pixel
        if (!src.data || src.rows <= 0 || src.cols <= 0 || src.step < src.cols * px) return "Input image is empty or has an invalid step.";
        if (const std::string why = call_target(resizeFilter, dst, src.rows, src.cols, false, c); !why.empty()) return why;
        if (!dst.data || dst.rows != c.out_rows || dst.cols != c.out_cols || dst.step < dst.cols * px) return c.resized ? "Output image is empty or has an invalid step." : out_size_text(c);
        if (const std::string why = call_grid(c); !why.empty()) return why;
        if (parts > 1) c.sp = strip_plan(c.grid, c.cols * cfg.scaling, plan.Tout, part, parts);
        return "";
    }
    // The YUV calls: one size, one pair of depths and one pair of layouts (srcs[0]'s, dsts[0]'s) for the sequence, resized or not.
    std::string yuv_check(const YuvImage* srcs, const YuvImage* dsts, int count, YuvFormat format, int resizeFilter, FrameCall& c) const {
        const int matrix = (int)format.matrix, range = (int)format.range;
        if (matrix < 0 || matrix > 2) return "Unknown YUV matrix " + std::to_string(matrix) + ".";
        if (range < 0 || range > 1) return "Unknown YUV range " + std::to_string(range) + ".";
        const int rows = srcs[0].rows, cols = srcs[0].cols, in_bits = srcs[0].bits, out_bits = dsts[0].bits;
        if ((in_bits != 8 && in_bits != 10) || (out_bits != 8 && out_bits != 10)) return "YUV frames must have 8 or 10 bits.";
        if (rows <= 0 || cols <= 0) return "Input image is empty.";
        const int in_layout = (int)srcs[0].layout, out_layout = (int)dsts[0].layout;
        if (in_layout < kYuvI420 || in_layout > kYuvNV12 || out_layout < kYuvI420 || out_layout > kYuvNV12)
            return "Unknown YUV layout " + std::to_string(in_layout < kYuvI420 || in_layout > kYuvNV12 ? in_layout : out_layout) + ".";
        const int in_siting = (int)srcs[0].siting, out_siting = (int)dsts[0].siting;
        if (in_siting < kYuvLeft || in_siting > kYuvTopLeft || out_siting < kYuvLeft || out_siting > kYuvTopLeft)
            return "Unknown YUV chroma siting " + std::to_string(in_siting < kYuvLeft || in_siting > kYuvTopLeft ? in_siting : out_siting) + ".";
        if (const std::string why = call_target(resizeFilter, dsts[0], rows, cols, true, c); !why.empty()) return why;
        // every plane of the layout present (NV12: Y and UV), with a step that holds its row
        auto planes_ok = [](const YuvImage& f) {
            const size_t bps = f.bits > 8 ? 2 : 1;
            for (int k = 0; k < yuv_planes((int)f.layout); ++k) if (!f.planes[k] || f.steps[k] < (size_t)(k ? yuv_chroma_samples(f.cols, (int)f.layout) : f.cols) * bps) return false;
            return true;
        };
        for (int i = 0; i < count; ++i) {
            if ((int)srcs[i].layout != in_layout || (int)dsts[i].layout != out_layout) return "The frames of a sequence must be of one layout (one for the inputs, one for the outputs).";
            if ((int)srcs[i].siting != in_siting || (int)dsts[i].siting != out_siting) return "The frames of a sequence must be of one chroma siting (one for the inputs, one for the outputs).";
            if (srcs[i].rows != rows || srcs[i].cols != cols || srcs[i].bits != in_bits) return "Input images must be of one size and depth.";
            if (!planes_ok(srcs[i])) return "Input image has a missing plane or an invalid step.";
            if (dsts[i].rows != c.out_rows || dsts[i].cols != c.out_cols) return out_size_text(c);
            if (dsts[i].bits != out_bits) return "Output images must be of one depth.";
            if (!planes_ok(dsts[i])) return "Output image has a missing plane or an invalid step.";
        }
        return call_grid(c);
    }
    // The RGBA and the gray calls: `count` frames of one size, one target and (RGBA) one set of options.  The order is deliberate and the same for one frame and
    // for a sequence: depth, the first frame's size, the target (resize_problem), then per frame its size, its pointers and steps, then (RGBA) the bleed radius,
    // then the grid - so a null dst with an out-of-range target reports the target.  packed_check(): all of it behind the depth, for `bpp` bytes per pixel.
    std::string packed_check(const Image* srcs, const Image* dsts, int count, int resizeFilter, size_t bpp, FrameCall& c) const {
        const int rows = srcs[0].rows, cols = srcs[0].cols;
        if (rows <= 0 || cols <= 0) return "Input image is empty or has an invalid step.";
        if (const std::string why = call_target(resizeFilter, dsts[0], rows, cols, true, c); !why.empty()) return why;
        for (int i = 0; i < count; ++i) {
            if (srcs[i].rows != rows || srcs[i].cols != cols) return "Input images must be of one size.";
            if (!srcs[i].data || srcs[i].step < (size_t)cols * bpp) return "Input image is empty or has an invalid step.";
            if (!dsts[i].data || dsts[i].rows != c.out_rows || dsts[i].cols != c.out_cols || dsts[i].step < (size_t)c.out_cols * bpp) return out_size_text(c);
        }
        return "";
    }
    std::string rgba_check(const Image* srcs, const Image* dsts, int count, const RgbaOptions& opt, int resizeFilter, FrameCall& c) const {
        for (int i = 0; i < count; ++i) if (srcs[i].depth != 8 || dsts[i].depth != 8) return "RGBA input and output images must be 8-bit.";
        if (const std::string why = packed_check(srcs, dsts, count, resizeFilter, 4, c); !why.empty()) return why;
        if (opt.bleed < 0 || opt.bleed > kBleedMaxRadius) return "Alpha bleed radius " + std::to_string(opt.bleed) + " is not in [0, " + std::to_string(kBleedMaxRadius) + "].";
        return call_grid(c);
    }
    // single: one frame of 8 or 16 bits (renderGray / renderGrayResized); else a sequence of 8-bit frames
    std::string gray_check(const Image* srcs, const Image* dsts, int count, int resizeFilter, const char* who, bool single, FrameCall& c) const {
        const int depth = srcs[0].depth;
        if (single) {
            if ((depth != 8 && depth != 16) || dsts[0].depth != depth) return "Input and output images must both be 8-bit or both 16-bit.";
        } else {
            for (int i = 0; i < count; ++i) if (srcs[i].depth != 8 || dsts[i].depth != 8) return std::string(who) + " takes 8-bit frames (16-bit images go through renderGray()).";
        }
        if (const std::string why = packed_check(srcs, dsts, count, resizeFilter, depth == 16 ? 2 : 1, c); !why.empty()) return why;
        return call_grid(c);
    }
    // The planar calls: one size and one pair of depths (srcs[0]'s, dsts[0]'s) for the call.  The order: the depths, the first frame's size, the target
    // (resize_problem: the filter, then the range), then per frame its size and depth, its planes, the output's size, its depth, its planes, then the grid.
    std::string planar_check(const PlanarImage* srcs, const PlanarImage* dsts, int count, int resizeFilter, FrameCall& c) const {
        const int rows = srcs[0].rows, cols = srcs[0].cols, in_bits = srcs[0].bits, out_bits = dsts[0].bits;
        if (!planar_bits_ok(in_bits) || !planar_bits_ok(out_bits)) return "Planar frames must have 8, 10, 12, 16 or 32 (float) bits.";
        if (rows <= 0 || cols <= 0) return "Input image is empty.";
        if (const std::string why = call_target(resizeFilter, dsts[0], rows, cols, true, c); !why.empty()) return why;
        // every plane present, with a step that holds its row, u16 / f32 samples aligned to their size
        auto planes_ok = [](const PlanarImage& f) {
            const size_t bps = planar_sample_bytes(f.bits);
            for (int k = 0; k < 3; ++k) if (!f.planes[k] || f.steps[k] < (size_t)f.cols * bps || ((((size_t)f.planes[k]) | f.steps[k]) & (bps - 1)) != 0) return false;
            return true;
        };
        for (int i = 0; i < count; ++i) {
            if (srcs[i].rows != rows || srcs[i].cols != cols || srcs[i].bits != in_bits) return "Input images must be of one size and depth.";
            if (!planes_ok(srcs[i])) return "Input image has a missing plane or an invalid step.";
            if (dsts[i].rows != c.out_rows || dsts[i].cols != c.out_cols) return out_size_text(c);
            if (dsts[i].bits != out_bits) return "Output images must be of one depth.";
            if (!planes_ok(dsts[i])) return "Output image has a missing plane or an invalid step.";
        }
        return call_grid(c);
    }
    // The planar RGBA calls: planar_check's order over four planes, then the bleed radius (and that a bleed has integer samples to work on), then the grid
    std::string planar_rgba_check(const PlanarRgbaImage* srcs, const PlanarRgbaImage* dsts, int count, const RgbaOptions& opt, int resizeFilter, FrameCall& c) const {
        const int rows = srcs[0].rows, cols = srcs[0].cols, in_bits = srcs[0].bits, out_bits = dsts[0].bits;
        if (!planar_bits_ok(in_bits) || !planar_bits_ok(out_bits)) return "Planar frames must have 8, 10, 12, 16 or 32 (float) bits.";
        if (rows <= 0 || cols <= 0) return "Input image is empty.";
        if (const std::string why = call_target(resizeFilter, dsts[0], rows, cols, true, c); !why.empty()) return why;
        for (int i = 0; i < count; ++i) {
            if (srcs[i].rows != rows || srcs[i].cols != cols || srcs[i].bits != in_bits) return "Input images must be of one size and depth.";
            if (!rgba_planes_ok(srcs[i])) return "Input image has a missing plane or an invalid step.";
            if (dsts[i].rows != c.out_rows || dsts[i].cols != c.out_cols) return out_size_text(c);
            if (dsts[i].bits != out_bits) return "Output images must be of one depth.";
            if (!rgba_planes_ok(dsts[i])) return "Output image has a missing plane or an invalid step.";
        }
        if (const std::string why = bleed_problem(opt.bleed, in_bits); !why.empty()) return why;
        return call_grid(c);
    }
    // every plane present, with a step that holds its row, u16 / f32 samples aligned to their size
    static bool rgba_planes_ok(const PlanarRgbaImage& f) {
        const size_t bps = planar_sample_bytes(f.bits);
        for (int k = 0; k < 4; ++k) if (!f.planes[k] || f.steps[k] < (size_t)f.cols * bps || ((((size_t)f.planes[k]) | f.steps[k]) & (bps - 1)) != 0) return false;
        return true;
    }
    static std::string bleed_problem(int radius, int bits) {
        if (radius < 0 || radius > kBleedMaxRadius) return "Alpha bleed radius " + std::to_string(radius) + " is not in [0, " + std::to_string(kBleedMaxRadius) + "].";
        if (radius > 0 && bits == 32) return "Colour bleed takes integer samples.";
        return "";
    }
    // The tile grid of a rows x cols frame into `grid`; returns "" or why the engine cannot render it (img2img_render.cpp:232-240)
    std::string frame_grid(int rows, int cols, TileGrid& grid) const {
        const int s = cfg.scaling;
        grid = calculate_tiles(cols, rows, cols * s, rows * s, plan.T, plan.T, plan.Tout, plan.Tout, s, cfg.overlapX, cfg.overlapY);
        if (grid.count <= 0) return "Tile grid is empty.";
        for (const Rect& r : grid.out) if (r.w <= 0 || r.h <= 0) return "Tile grid does not fit the output (scaling does not match the model).";
        return "";
    }
    // the two frame and the two output buffers of a sequence, and the copy streams that fill and empty them
    void sequence_buffers(size_t in_bytes, size_t out_bytes) {
        ensure_copy_streams();
        ensure(d_frame, frame_cap, in_bytes);   ensure(d_frame2, frame2_cap, in_bytes);
        ensure(d_out, out_cap, out_bytes);      ensure(d_out2, out2_cap, out_bytes);
    }
    // a resized frame: the tap tables of its target into the job and a canvas of the format's fp32 planes of the scaled size
    void job_resize(int rows, int cols, int out_rows, int out_cols, int resizeFilter) {
        const int s = cfg.scaling;
        job.rs = resize_tables(cols * s, rows * s, out_cols, out_rows, resizeFilter);
        ensure_canvas((size_t)rows * s * cols * s * canvas_planes() * sizeof(float));
    }
    // What every frame call does behind its checks, with the job of its format set: the buffers (single: one frame on the compute stream, else the two pairs of
    // a sequence), the slot tables, a resized call's tables and canvas, then the frames - up(i, device buffer, stream) and down(i, device buffer, stream) copy
    // frame i between the caller's memory and the device layout - and last_ms, the compute stream's milliseconds per frame.  A format that is not replayable
    // marks the engine so once its buffers are sized (d_frame / d_out hold its samples from here on).
    template <class Up, class Down>
    void run_call(const FrameCall& c, int count, bool single, int resizeFilter, const Up& up, const Down& down) {
        const size_t in_bytes = frame_bytes(c.rows, c.cols, false), out_bytes = frame_bytes(c.out_rows, c.out_cols, true);
        if (single) { ensure(d_frame, frame_cap, in_bytes); ensure(d_out, out_cap, out_bytes); }
        else sequence_buffers(in_bytes, out_bytes);
        if (!replayable()) { deep = false; last_rows = last_cols = 0; }
        call_slots(c.rows, c.cols, c.grid, c.sp);
        if (!replayable()) one_part_stale = false;
        if (c.resized) job_resize(c.rows, c.cols, c.out_rows, c.out_cols, resizeFilter);
        if (!single) { last_ms = run_sequence(count, c.rows, c.cols, c.grid, c.sp, up, down) / count; return; }
        up(0, d_frame, stream);
        run_frame(c.rows, c.cols, c.grid, true, c.sp, ev0);
        hipAssert(hipEventRecord(ev1, stream));
        down(0, d_out, stream);
        hipAssert(hipStreamSynchronize(stream));
        hipAssert(hipEventElapsedTime(&last_ms, ev0, ev1));
    }
    // run_call() for packed frames (every format but YUV): frame i travels as one 2-D copy of `bpp` bytes per pixel between the caller's Image and the device layout
    void run_packed_call(const FrameCall& c, const Image* srcs, Image* dsts, int count, bool single, int resizeFilter, size_t bpp) {
        const size_t in_step = frame_step(c.cols, false), out_step = frame_step(c.out_cols, true);
        run_call(c, count, single, resizeFilter,
            [&](int i, uint8_t* dev, hipStream_t on) { hipAssert(hipMemcpy2DAsync(dev, in_step, srcs[i].data, srcs[i].step, (size_t)c.cols * bpp, c.rows, hipMemcpyHostToDevice, on)); },
            [&](int i, uint8_t* dev, hipStream_t on) { hipAssert(hipMemcpy2DAsync(dsts[i].data, dsts[i].step, dev, out_step, (size_t)c.out_cols * bpp, c.out_rows, hipMemcpyDeviceToHost, on)); });
    }
    // A render() frame in the pipelined parts of render_parts() (tiles.h), behind the upload of the columns [0, rp.x_split) and the slot tables: per part its
    // passes, its cells composed and an event; the rest of the upload behind the first part's launches; the downloads of the parts' cells, in order, on a copy
    // stream; ev1 behind the last part.  Returns with dst complete.
    void run_frame_in_parts(const FrameCall& c, const RenderParts& rp, const Image& src, Image& dst) {
        const int rows = c.rows, cols = c.cols, steps = cfg.tta ? 8 : 1;
        const size_t px = deep ? 6 : 3;                                   // bytes per pixel
        ensure_copy_streams();
        for (int k = 0; k < rp.n; ++k) if (!ev_part[k]) hipAssert(hipEventCreateWithFlags(&ev_part[k], hipEventDisableTiming));
        // the parts ROLL like the frames of a sequence (run_rolling_frame) when all their passes split: no join at the end of a part - the second group's stream
        // composes the part's cells behind its own tiles while the first stream starts the next part's (one slab: the parts' tiles lie side by side in it)
        bool roll = true;
        for (int k = 0; k < rp.n; ++k) roll = roll && can_roll(rp.part[k].tiles);
        struct Unroll { Impl* e; ~Unroll() { e->rolling = false; } } unroll{this};
        if (roll) for (int k = 0; k < 2; ++k) if (!ev_g0[k]) hipAssert(hipEventCreateWithFlags(&ev_g0[k], hipEventDisableTiming));
        for (int k = 0; k < rp.n; ++k) {
            const RenderParts::Part& p = rp.part[k];
            if (k == 1 && rp.x_split < cols) hipAssert(hipStreamWaitEvent(stream, ev_up[0], 0));      // the rest of the frame has arrived
            rolling = roll;
            run_passes(rows, cols, p.tiles, (size_t)p.first * steps, true, p.slots_off, k == 0, p.batches_before, rp.batch_total);
            rolling = false;
            if (k == 0 && rp.x_split < cols) {      // issued behind the first part's launches: from pageable memory the call returns when the copy is done
                hipAssert(hipMemcpy2DAsync(d_frame + (size_t)rp.x_split * px, (size_t)cols * px, src.data + (size_t)rp.x_split * px, src.step, (size_t)(cols - rp.x_split) * px, rows,
                                           hipMemcpyHostToDevice, s_dn));
                hipAssert(hipEventRecord(ev_up[0], s_dn));
            }
            hipStream_t cs = stream;
            if (roll) {
                cs = gstream[0];
                hipAssert(hipEventRecord(ev_g0[k & 1], stream));
                hipAssert(hipStreamWaitEvent(cs, ev_g0[k & 1], 0));
            }
            for (int r = 0; r < p.nrect; ++r) compose_rect(rows, cols, c.grid, p.rect[r].x, p.rect[r].x + p.rect[r].w, p.rect[r].y, p.rect[r].y + p.rect[r].h, 0, cs);
            hipAssert(hipEventRecord(ev_part[k], cs));
            if (k + 1 == rp.n) { if (roll) end_rolling(); hipAssert(hipEventRecord(ev1, stream)); }
        }
        // the downloads, in order, on a copy stream: a part's cells travel while the next part computes.  Which of the two copy streams: the one created
        // FIRST (renderSequence()'s upload stream, idle here) - the runtime spreads streams over its hardware queues in creation order, and from
        // pageable memory the download only ran beside the kernels on that one (9.1 against 9.9 ms per call, profiles/r4_kernels/render_parts_ab*.txt)
        for (int k = 0; k < rp.n; ++k) {
            hipAssert(hipStreamWaitEvent(s_up, ev_part[k], 0));
            for (int r = 0; r < rp.part[k].nrect; ++r) {
                const Rect& rc = rp.part[k].rect[r];
                hipAssert(hipMemcpy2DAsync(dst.data + (size_t)rc.y * dst.step + (size_t)rc.x * px, dst.step, d_out + ((size_t)rc.y * dst.cols + rc.x) * px, (size_t)dst.cols * px,
                                           (size_t)rc.w * px, rc.h, hipMemcpyDeviceToHost, s_up));
            }
        }
        hipAssert(hipStreamSynchronize(s_up));
        hipAssert(hipStreamSynchronize(stream));
    }
    // the RGBA calls behind entry(): one frame on the compute stream with progress (renderRgbaFrame), or a sequence (runSequenceRgba)
    bool rgba_call(const Image* srcs, Image* dsts, int count, const RgbaOptions& opt, int resizeFilter, const char* who, bool single) {
        FrameCall c;
        if (const std::string why = rgba_check(srcs, dsts, count, opt, resizeFilter, c); !why.empty()) { log(Severity::error, why, who, __LINE__); return false; }
        job.kind = Job::RGBA; job.rgba = RgbaJob{opt.bleed, opt.skipUniformAlpha};
        run_packed_call(c, srcs, dsts, count, single, resizeFilter, 4);
        return true;
    }
    // What the frames of an RGBA call share, made once per call (the RGBA side of call_slots): the planes the bleed writes, the two words' host side,
    // and the slot table, liveness table and slab of the 2N schedule - slot = step index, tile = step / stepsPerTile over the 2N tiles (colour 0 .. N - 1,
    // alpha N .. 2N - 1), zero pad slots at the end.  A frame whose alpha tiles are skipped runs a prefix of the same table.
    void rgba_setup(int rows, int cols, const TileGrid& grid, bool skip) {
        const int steps = cfg.tta ? 8 : 1, N = grid.count;
        const size_t stepTotal = pass_slots(2 * N), colour = (size_t)N * steps;
        ensure_bleed_planes(rows, cols);
        if (skip) {
            if (!h_minmax) hipAssert(hipHostMalloc((void**)&h_minmax, 2 * sizeof(unsigned), hipHostMallocDefault));
            if (!ev_minmax) hipAssert(hipEventCreateWithFlags(&ev_minmax, hipEventDisableTiming));
        }
        fill_slots(grid, 0, N, kSlotColour, 0, colour);
        fill_slots(grid, 0, N, kSlotAlpha, colour, stepTotal - colour);
        upload_slots(grid, stepTotal, stepTotal);
    }
    // The device part of one RGBA frame, on `stream`, with the BGRA frame in d_frame and rgba_setup() done: alpha_bleed_kernel, ONE schedule of the frame's N
    // colour tiles followed by its N alpha tiles, then the end of an RGBA frame (finish_frame: compose_rgba_kernel - or, with job.rs set, compose_canvas_rgba_kernel
    // and resample_rgba_kernel - into d_out).
    // skip (skipUniformAlpha): the two words come back behind the bleed kernel while the passes that hold colour tiles only - the same in the 2N and the N
    // schedule - are issued; the host waits for them, then issues the rest of whichever schedule the frame takes.  `started`: recorded behind the bleed.
    void rgba_frame(int rows, int cols, const TileGrid& grid, const StripPlan& sp, bool report, hipEvent_t started) {
        RgbaJob& opt = job.rgba;
        const int steps = cfg.tta ? 8 : 1, B = plan.B, S = plan.B / plan.userB, N = grid.count;
        bleed_frame(rows, cols, opt.bleed);
        if (opt.skip) {
            hipAssert(hipMemcpyAsync(h_minmax, d_minmax, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
            hipAssert(hipEventRecord(ev_minmax, stream));
        }
        if (started) hipAssert(hipEventRecord(started, stream));
        opt.alpha_slot0 = (size_t)N * steps; opt.uniform = false; opt.value = 255;
        if (!opt.skip) run_passes(rows, cols, 2 * N, 0, report, 0, true);
        else {
            const int F = N * steps / B;                 // passes of colour tiles only: the same launches whether the alpha tiles follow or not
            const auto t0 = std::chrono::steady_clock::now();
            run_passes(rows, cols, 2 * N, 0, false, 0, true, 0, 0, 0, F);
            hipAssert(hipEventSynchronize(ev_minmax));
            opt.uniform = h_minmax[0] + h_minmax[1] == alpha_top();       // max(A) + max(top - A) == top  <=>  min(A) == max(A)
            opt.value = h_minmax[0];
            const int tiles = opt.uniform ? N : 2 * N, batchCount = batch_count(tiles);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (report) for (int k = 0; k < std::min(F * S, batchCount); ++k) log(k + 1, batchCount, 1000.0 * F * S / std::max(ms, 1e-6));
            run_passes(rows, cols, tiles, 0, report, 0, false, 0, 0, F, -1);
        }
        finish_frame(rows, cols, grid, sp, stream, nullptr, nullptr);
    }
    // The frame loop of a sequence call (run_call): frame i is uploaded by up(i, device buffer, s_up) into one of two frame buffers, rendered
    // (rolling when every pass of a frame splits: run_rolling_frame) into one of two output buffers, and downloaded by down(i, device buffer, s_dn); events
    // order the three streams where a buffer comes round again.  Returns the compute stream's milliseconds for the whole sequence.
    template <class Up, class Down>
    float run_sequence(int count, int rows, int cols, const TileGrid& grid, const StripPlan& sp, const Up& up, const Down& down) {
        uint8_t* const frames[2] = {d_frame, d_frame2};
        uint8_t* const outs[2] = {d_out, d_out2};
        struct Restore { Impl* im; uint8_t* f; uint8_t* o; ~Restore() { im->d_frame = f; im->d_out = o; im->seq_frame = 0; } } restore{this, frames[0], outs[0]};   // also on exceptions
        // frame f is composed on the second group's stream while frame f + 1's first group already runs (run_rolling_frame) when every pass of a frame splits
        const bool roll = count > 1 && rolls() && can_roll(sp.tile_count);
        if (roll) ensure(d_slab2, slab2_cap, slab_cap);
        hipAssert(hipStreamSynchronize(stream));
        hipAssert(hipEventRecord(ev0, stream));
        for (int i = 0; i < count; ++i) {
            const int b = i & 1;
            if (i >= 2) hipAssert(hipStreamWaitEvent(s_up, ev_comp[b], 0));       // frame i-2 has been gathered out of this buffer
            up(i, frames[b], s_up);
            hipAssert(hipEventRecord(ev_up[b], s_up));
            hipAssert(hipStreamWaitEvent(stream, ev_up[b], 0));
            d_frame = frames[b]; d_out = outs[b];
            seq_frame = (unsigned)i;                                     // (the frame's dither phase: dither_now())
            if (roll) {
                run_rolling_frame(rows, cols, grid, sp, b, i >= 2 ? ev_dn[b] : nullptr);
                hipAssert(hipEventRecord(ev_comp[b], gstream[0]));              // (behind the compose launch: both groups have gathered, the output is whole)
            } else {
                if (i >= 2) hipAssert(hipStreamWaitEvent(stream, ev_dn[b], 0));         // frame i-2 has left this output buffer
                run_frame(rows, cols, grid, false, sp);
                hipAssert(hipEventRecord(ev_comp[b], stream));
            }
            hipAssert(hipStreamWaitEvent(s_dn, ev_comp[b], 0));
            down(i, outs[b], s_dn);
            hipAssert(hipEventRecord(ev_dn[b], s_dn));
        }
        if (roll) end_rolling();
        hipAssert(hipEventRecord(ev1, stream));
        hipAssert(hipStreamSynchronize(s_dn));
        hipAssert(hipStreamSynchronize(stream));
        hipAssert(hipStreamSynchronize(s_up));
        float total_ms = 0.f;
        hipAssert(hipEventElapsedTime(&total_ms, ev0, ev1));
        return total_ms;
    }
    // the device tap tables of one (canvas, target, filter): what job_resize() puts into the job for the frame
    const ResizeTables* resize_tables(int inW, int inH, int outW, int outH, int filter) {
        for (const ResizeTables& t : rs_tables) if (t.inW == inW && t.inH == inH && t.outW == outW && t.outH == outH && t.filter == filter && t.edge == edge) return &t;
        if (rs_tables.size() >= 16) {                                        // sizes that keep changing: start over rather than grow without bound
            for (ResizeTables& t : rs_tables) for (void* q : {(void*)t.fx, (void*)t.fy, (void*)t.wx, (void*)t.wy}) if (q) hipAssert(hipFree(q));
            rs_tables.clear();
        }
        // (under Wrap and Mirror the tables keep every tap - resize_taps_edge - and a tile's rows are not cut at the canvas: rows_max from those tables; no YUV
        // frame is resized under such a mode, so rows_max_above stays 0 there)
        const ResizeTaps tx = resize_taps_edge(inW, outW, filter, edge), ty = resize_taps_edge(inH, outH, filter, edge);
        if (tx.taps <= 0 || ty.taps <= 0) throw std::runtime_error("invalid resize");
        ResizeTables t;
        t.inW = inW; t.inH = inH; t.outW = outW; t.outH = outH; t.filter = filter; t.edge = edge; t.kx = tx.taps; t.ky = ty.taps;
        if (edge == kEdgeReplicate) {
            t.rows_max = resample_rows_max(ty.first.data(), outH, inH, ty.taps);
            t.rows_max_above = resample_rows_max(ty.first.data(), outH, inH, ty.taps, 1);
        } else t.rows_max = resample_rows_max_edge(ty.first.data(), outH, ty.taps);
        auto upload = [&](auto*& d, const auto& v) {
            hipAssert(hipMalloc((void**)&d, v.size() * sizeof(v[0])));
            hipAssert(hipMemcpy(d, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice));
        };
        try { upload(t.fx, tx.first); upload(t.wx, tx.w); upload(t.fy, ty.first); upload(t.wy, ty.w); }
        catch (...) { for (void* q : {(void*)t.fx, (void*)t.fy, (void*)t.wx, (void*)t.wy}) if (q) (void)hipFree(q); throw; }   // (no half-made entry is cached)
        rs_tables.push_back(t);
        return &rs_tables.back();
    }
    void ensure_canvas(size_t bytes) {
        if (bytes <= canvas_cap) return;
        if (d_canvas) hipAssert(hipFree(d_canvas));
        d_canvas = nullptr; canvas_cap = 0;
        hipAssert(hipMalloc((void**)&d_canvas, bytes));
        canvas_cap = bytes;
    }
    // renderResized() / renderSequenceResized(): the target size of a frame must be a downsample of the network output by a factor of 1 to s per axis
    std::string resize_problem(int rows, int cols, int out_rows, int out_cols, int filter) const {
        const int s = cfg.scaling;
        if (filter != 0 && filter != 1) return "Unknown resize filter.";
        if (out_rows < rows || out_rows > rows * s || out_cols < cols || out_cols > cols * s || out_rows <= 0 || out_cols <= 0)
            return "Output image has invalid size for a resize: " + std::to_string(out_cols) + "x" + std::to_string(out_rows) + " is not between " + std::to_string(cols) + "x" +
                   std::to_string(rows) + " and " + std::to_string(cols * s) + "x" + std::to_string(rows * s) + ".";
        return "";
    }
};

Img2Img::Img2Img() : impl(new Impl) {}
Img2Img::~Img2Img() = default;

void Img2Img::setMessageCallback(MessageCallback callback) { impl->messageCallback = std::move(callback); }
void Img2Img::setProgressCallback(ProgressCallback callback) { impl->progressCallback = std::move(callback); }

bool Img2Img::build(const std::string& onnxModelPath, const BuildConfig& config) try {
    // img2img_build.cpp:56-64
    const int dev = physical_device(config.deviceId);
    if (const std::string why = device_ordinal_problem(config.deviceId, dev); !why.empty()) {
        W2X_LOG(error, "Failed to set hip device: " + why + ".");
        return false;
    }
    std::unique_ptr<DeviceGuard> guard;
    try {
        guard.reset(new DeviceGuard(dev));
    } catch (const std::exception& e) {
        W2X_LOG(error, "Failed to set hip device to device id " + std::to_string(config.deviceId) + ": " + std::string(e.what()) + ".");
        return false;
    }
    // :123-135 - precision: FP16 = the fused fp16 kernels; gfx950 has no TF32 matrix instruction, a TF32 request gets the fp32-storage
    // engine (k_f32.hip: fp32 maps and accumulation, un-fused operator set) with split-bf16 products, FP32 the same engine with exact
    // fp32 products (include/w2x/config.h)
    switches_from_env();                                   // (W2X_SUPERBATCH is read by the lowering: switches.h)
    const bool fp32 = config.precision != Precision::FP16;
    if (config.precision == Precision::TF32) W2X_LOG(info, "Precision TF32: this platform has no TF32 matrix instructions, the engine keeps fp32 maps and multiplies split-bf16 operands (16 significant bits each).");
    // :81-88 parse ; :102-116 one profile: the plan on disk is specialised for the opt shape (channels come from the model);
    // any other shape inside [min, max] is specialised by load() from the same ONNX file
    if (config.minBatchSize > config.optBatchSize || config.optBatchSize > config.maxBatchSize || config.minWidth > config.optWidth || config.optWidth > config.maxWidth ||
        config.minHeight > config.optHeight || config.optHeight > config.maxHeight || config.minChannels > config.optChannels || config.optChannels > config.maxChannels) {
        W2X_LOG(error, "Failed to build engine: optimization profile is not min <= opt <= max.");
        return false;
    }
    Plan plan;
    try {
        W2X_LOG(info, "ONNX graph \"" + onnxModelPath + "\": " + onnx_op_histogram(onnxModelPath) + ".");
        plan = lower_for_shape(onnxModelPath, config.optBatchSize, config.optChannels, config.optHeight, config.optWidth, fp32);
    } catch (const std::exception& e) {
        W2X_LOG(error, "Failed to parse ONNX model: " + std::string(e.what()) + ".");
        return false;
    }
    W2X_LOG(info, "Lowered \"" + onnxModelPath + "\": " + std::to_string(plan.ops.size()) + " fused ops, " +
                      std::to_string((long long)plan.flops) + " algorithmic FLOP per batch, output tile " + std::to_string(plan.Tout) + ".");
    // :151-161
    const std::string deviceName = hipGetDeviceName(dev);
    const auto basePath = std::filesystem::path(onnxModelPath).replace_extension("").string() + "_" + getConfigHash(config, deviceName).substr(0, 16);
    serializeConfig(basePath + ".json", config, deviceName);
    try {
        const auto bytes = plan.serialize();
        std::ofstream engineFile(basePath + kEngineExt, std::ios::binary);
        if (!engineFile.is_open()) throw std::runtime_error("could not open \"" + basePath + kEngineExt + "\"");
        engineFile.write((const char*)bytes.data(), (std::streamsize)bytes.size());
    } catch (const std::exception& e) {
        W2X_LOG(error, "Failed to serialize network to disk: " + std::string(e.what()) + ".");
        return false;
    }
    return true;
} catch (const std::exception& e) {
    W2X_LOG(error, "Engine build failed unexpectedly: " + std::string(e.what()) + ".");
    return false;
}

bool Img2Img::load(const std::string& modelPath, const RenderConfig& config) try {
    namespace fs = std::filesystem;
    // img2img_load.cpp:127-135
    const int dev = physical_device(config.deviceId);
    if (const std::string why = device_ordinal_problem(config.deviceId, dev); !why.empty()) {
        W2X_LOG(error, "Failed to set hip device: " + why + ".");
        return false;
    }
    std::unique_ptr<DeviceGuard> guard;
    try {
        guard.reset(new DeviceGuard(dev));
    } catch (const std::exception& e) {
        W2X_LOG(error, "Failed to set hip device to device id " + std::to_string(config.deviceId) + ": " + std::string(e.what()) + ".");
        return false;
    }
    // :79-114 getEnginePath
    std::string enginePath;
    bool optimized = false;
    try {
        if (!fs::exists(modelPath)) throw std::runtime_error("model file does not exist");
        const std::string runningOn = hipGetDeviceName(dev);
        const std::string engineName = fs::path(modelPath).stem().string();
        fs::path dir = fs::path(modelPath).parent_path();
        if (dir.empty()) dir = ".";
        std::vector<fs::path> entries;
        for (const auto& entry : fs::directory_iterator(dir)) if (entry.is_regular_file()) entries.push_back(entry.path());
        std::sort(entries.begin(), entries.end());
        for (const auto& path : entries) {
            if (path.filename().string().rfind(engineName, 0) != 0 || path.extension().string() != kEngineExt) continue;
            const std::string configPath = fs::path(path).replace_extension("").string() + ".json";
            if (!fs::exists(configPath)) continue;
            BuildConfig bc; std::string builtOn;
            deserializeConfig(configPath, bc, builtOn);
            // img2img_load.cpp:100-107: the first optimized engine, else the first compatible one
            if (!isCompatible(config, bc, builtOn, runningOn)) continue;
            if (isOptimized(config, bc)) { enginePath = path.string(); optimized = true; break; }
            if (enginePath.empty()) enginePath = path.string();
        }
        if (enginePath.empty()) throw std::runtime_error("could not satisfy render configuration");
    } catch (const std::exception& e) {
        W2X_LOG(error, "Failed to find engine file for model \"" + modelPath + "\": " + std::string(e.what()) + ".");
        return false;
    }
    // :137-147
    std::ifstream file(enginePath, std::ios::binary | std::ios::ate);
    if (!file.is_open()) { W2X_LOG(error, "Failed to open engine file \"" + enginePath + "\"."); return false; }
    std::streamsize fileSize = file.tellg();
    std::vector<char> engineBuffer((size_t)fileSize);
    file.seekg(0, std::ios::beg);
    file.read(engineBuffer.data(), fileSize);

    impl->release();   // :149-154, :209-222
    impl->device = dev;
    switches_from_env();                                   // every switch of the library: switches.h
    const Switches& sw = switches();
    impl->poison = sw.poison;
    impl->check_general = sw.check_general;
    impl->use_graphs = !sw.no_graph;
    impl->rolling_ok = !sw.no_rolling;
    impl->pipeline_parts = std::min(kMaxRenderParts, std::max(1, sw.render_parts));
    if (const std::string nd = switches_nondefault(); !nd.empty()) W2X_LOG(warn, "Switches off their defaults: " + nd + ".");
    if (sw.roctx && !impl->roctx_push) {
        if (void* h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL)) {
            impl->roctx_push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
            impl->roctx_pop = (int (*)())dlsym(h, "roctxRangePop");
            if (!impl->roctx_push || !impl->roctx_pop) impl->roctx_push = nullptr;
        }
        if (!impl->roctx_push) W2X_LOG(warn, "W2X_ROCTX is set but libroctx64.so could not be loaded: no marker ranges.");
    }
    try {
        impl->plan = Plan::deserialize((const uint8_t*)engineBuffer.data(), engineBuffer.size());
    } catch (const std::exception& e) {
        W2X_LOG(error, "Failed to deserialize engine from buffer: " + std::string(e.what()) + ".");
        return false;
    }
    if (!optimized) {
        // A TensorRT engine runs any shape of its optimization profile (img2img_build.cpp:102-116); a plan is specialised for one
        // shape, so for a compatible-but-not-optimized engine the same ONNX file is lowered again for the requested shape (the
        // engine file only vouches for the device, the precision and the range).
        W2X_LOG(warn, "Engine \"" + enginePath + "\" is compatible with but not optimized for the render configuration; specialising the plan for batch " +
                          std::to_string(config.batchSize) + ", tile " + std::to_string(config.width) + "x" + std::to_string(config.height) + ".");
        try {
            impl->plan = lower_for_shape(modelPath, config.batchSize, config.channels, config.height, config.width, config.precision != Precision::FP16);
        } catch (const std::exception& e) {
            W2X_LOG(error, "Failed to set input tensor shape: " + std::string(e.what()) + ".");
            return false;
        }
    }
    const Plan& plan = impl->plan;
    if ((plan.elt == 4) != (config.precision != Precision::FP16)) {   // the JSON sidecar and the engine file disagree
        W2X_LOG(error, "Failed to deserialize engine from buffer: precision of the plan differs from the engine's configuration.");
        return false;
    }
    // :197-203 - the input shape must be the one the plan was specialised for; T' is read from the plan
    if (plan.userB != config.batchSize || plan.B % std::max(plan.userB, 1) || plan.Cin != config.channels || plan.T != config.height || plan.T != config.width) {
        W2X_LOG(error, "Failed to set input tensor shape.");
        return false;
    }
    hipAssert(hipStreamCreateWithFlags(&impl->stream, hipStreamNonBlocking));   // :206
    hipAssert(hipEventCreate(&impl->ev0));
    hipAssert(hipEventCreate(&impl->ev1));
    impl->groups = sw.groups;
    // Every stream the engine will use is created HERE, before anything touches the null stream (upload_plan()'s synchronous copies do): the runtime hands its
    // hardware queues (four by default) to streams in creation order and lets later streams share, so created now the compute stream, the two copy streams and the
    // second tile group's stream have a queue each and the null stream shares one.  Created lazily, in whatever order the first calls needed them, the second
    // group's kernels shared a queue with a copy stream on some orders: renderSequence() 7.69 (this order) / 7.85 (lazy) / 10.0 ms per frame (group stream
    // first), profiles/r4_kernels/stream_order.txt.  Further group streams (W2X_GROUPS > 2) are created by the first pass that splits.
    impl->ensure_copy_streams();
    if (impl->groups > 1) { hipAssert(hipStreamCreateWithFlags(&impl->gstream[0], hipStreamNonBlocking)); hipAssert(hipEventCreateWithFlags(&impl->ev_join[0], hipEventDisableTiming)); }
    try {
        impl->upload_plan(config.precision);                                      // :225-248
    } catch (const std::exception& e) {
        W2X_LOG(error, "Failed to allocate resources: " + std::string(e.what()) + ".");
        impl->release();
        return false;
    }
    impl->cfg = config;
    int folds[L_ATTN32 + 1] = {};
    for (const Launch& L : impl->launches) ++folds[L.kind];
    W2X_LOG(info, "Loaded \"" + enginePath + "\": " + std::to_string(plan.ops.size()) + " ops, " + std::to_string(plan.B) + " tiles per pass, activation arena " +
                      std::to_string(impl->arena_bytes >> 20) + " MiB" +
                      (folds[L_STEM] ? ", " + std::to_string(folds[L_STEM]) + " stem folded into the launch of the convolution behind it" : "") +
                      (folds[L_UP] ? ", " + std::to_string(folds[L_UP]) + " transposed convolution folded into the launch of the convolution behind it" : "") +
                      (folds[L_HEAD] ? ", image head folded into the last MLP launch" : "") +
                      (folds[L_ATTN32] + folds[L_MLP32] ? ", " + std::to_string(folds[L_ATTN32]) + " attention and " + std::to_string(folds[L_MLP32]) + " MLP branches as fused fp32-row launches." : "."));
    // :262-269 blend ramps
    impl->ovx = (int)std::lround(plan.T * config.scaling * config.overlapX);
    impl->ovy = (int)std::lround(plan.T * config.scaling * config.overlapY);
    if (config.overlapX != 0 || config.overlapY != 0) {
        auto rx = blend_ramp(impl->ovx), ry = blend_ramp(impl->ovy);
        hipAssert(hipMalloc((void**)&impl->d_rampx, std::max<size_t>(rx.size(), 1) * sizeof(float)));
        hipAssert(hipMalloc((void**)&impl->d_rampy, std::max<size_t>(ry.size(), 1) * sizeof(float)));
        hipAssert(hipMemcpy(impl->d_rampx, rx.data(), rx.size() * sizeof(float), hipMemcpyHostToDevice));
        hipAssert(hipMemcpy(impl->d_rampy, ry.data(), ry.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    impl->loaded = true;
    return true;
} catch (const std::exception& e) {
    W2X_LOG(error, "Engine load failed unexpectedly: " + std::string(e.what()) + ".");
    impl->release();
    return false;
}

bool Img2Img::render(const Image& src, Image& dst) { return renderPart(src, dst, 0, 1, "render"); }

// render() followed by an antialiased resize of the canvas to dst.rows x dst.cols (between the input size and s times it), on the device: the frame's
// tiles, compose_canvas_kernel (fp32 canvas), resample_kernel (k_resample.hip), the download of the target size.  At the scaled size it is render().
bool Img2Img::renderResized(const Image& src, Image& dst, ResizeFilter filter) {
    return renderPart(src, dst, 0, 1, "renderResized", filter_id(filter));
}

// One GPU's share of a frame when a single image is spread over several devices: renders and writes only the
// output columns strip_plan() assigns to `part`; the other columns of dst are left untouched.  part 0 of 1 = render().
bool Img2Img::renderStrip(const Image& src, Image& dst, int part, int parts) {
    if (impl->edge_refuses("renderStrip", "Strips of a frame are")) return false;
    return renderPart(src, dst, part, parts, "renderStrip");
}

bool Img2Img::renderPart(const Image& src, Image& dst, int part, int parts, const char* who, int resizeFilter) {
    return impl->entry(who, kNotLoaded, kRenderFailed, [&] {   // (the call's own work, to the closing `});` - deliberately left at function indentation)
    Impl::FrameCall c;
    if (const std::string why = impl->bgr_frame_check(src, dst, part, parts, resizeFilter, c); !why.empty()) { W2X_LOG_AS(who, error, why); return false; }
    const Plan& plan = impl->plan;
    const int rows = c.rows, cols = c.cols, s = impl->cfg.scaling;
    const size_t bps = src.depth / 8;                          // bytes per sample
    hipStream_t stream = impl->stream;
    impl->ensure(impl->d_frame, impl->frame_cap, Impl::bgr_step(cols, bps == 2) * rows);
    impl->ensure(impl->d_out, impl->out_cap, Impl::bgr_step(dst.cols, bps == 2) * dst.rows);
    if (c.resized) impl->job_resize(rows, cols, dst.rows, dst.cols, resizeFilter);
    impl->deep = bps == 2;
    const StripPlan& sp = c.sp;
    if (sp.tile_count == 0) return true;                       // more devices than tile columns: this one has no share
    // the frame's parts (tiles.h): several for a whole frame at the scaled size when the pipeline is switched on and the frame is large enough
    const RenderParts rp = render_parts(c.grid, sp, cols, cols * s, rows * s, plan.T, plan.Tout, impl->cfg.tta ? 8 : 1, plan.userB, plan.B,
                                        parts == 1 && !c.resized ? impl->pipeline_parts : 1);
    // img2img_render.cpp:226 upload.  In parts: the frame columns the first part's tiles read go first, on the compute stream; the rest follows on the upload
    // stream while that part computes (run_frame_in_parts)
    hipAssert(hipMemcpy2DAsync(impl->d_frame, (size_t)cols * 3 * bps, src.data, src.step, (size_t)rp.x_split * 3 * bps, rows, hipMemcpyHostToDevice, stream));
    for (int k = 0; k < rp.n; ++k) impl->fill_slots(c.grid, sp.first_tile + rp.part[k].first, rp.part[k].tiles, 1, rp.part[k].slots_off, rp.part[k].slots);
    impl->upload_slots(c.grid, rp.slot_total, rp.slab_slots);   // (the slab sized for the parts and for the frame as one part now: an allocation later would drop the captured passes)

    hipAssert(hipEventRecord(impl->ev0, stream));
    if (rp.n == 1) {
        impl->run_frame(rows, cols, c.grid, true, sp);
        hipAssert(hipEventRecord(impl->ev1, stream));
        // :344 download ; the reference leaves the sync commented out (:345, quirk Q10) - we wait before handing dst back
        const int dx0 = c.resized ? 0 : sp.x0, dx1 = c.resized ? dst.cols : sp.x1;
        hipAssert(hipMemcpy2DAsync(dst.data + (size_t)dx0 * 3 * bps, dst.step, impl->d_out + (size_t)dx0 * 3 * bps, (size_t)dst.cols * 3 * bps, (size_t)(dx1 - dx0) * 3 * bps, dst.rows, hipMemcpyDeviceToHost, stream));
        hipAssert(hipStreamSynchronize(stream));
    } else impl->run_frame_in_parts(c, rp, src, dst);
    hipAssert(hipEventElapsedTime(&impl->last_ms, impl->ev0, impl->ev1));
    impl->last_rows = rows; impl->last_cols = cols; impl->last_grid = c.grid; impl->last_strip = sp;
    impl->one_part_stale = rp.n > 1;      // (benchResident / profileFrame replay the frame as ONE part and rebuild the slot table when they are called: one_part_slots)
    if (c.resized) impl->last_rows = impl->last_cols = 0;   // (a resized frame is not replayed: benchResident / residentOutput / profileFrame serve render() frames)
    // the second slab of a rolling sequence now (an allocation drops the captured passes: better here, on the frame size's first sight, than inside benchResident / renderSequence)
    if (parts == 1 && impl->slab2_cap < impl->slab_cap && impl->can_roll(sp.tile_count)) impl->ensure(impl->d_slab2, impl->slab2_cap, impl->slab_cap);
    return true;
    });
}

// ONE frame over several engines, every tile computed once (img2img.h; SURVEY 8e second option; the reference is single-device,
// main.cpp:70-74).  Engine k takes part k of tiles.cpp shard_plan(): a contiguous range of the reference's column-major tile order
// (img2img_render.cpp:43-44) and the canvas cells of those tiles.  Phase 1, every engine on its own stream: upload, gather + network
// passes of its own tiles into its slab, an event.  Phase 2, per engine: behind the events of the engines that computed the ny + 1
// tiles in front of its range, copy their blend bands into the slab slots in front of its own (the seam exchange: two bands per tile,
// all four per augmented tile under TTA - a dihedral map sends the right / bottom band to any of the four), compose its cells (the
// same kernel and the same ascending-tile order as a whole-frame render, img2img_render.cpp:329-330: identical bytes), download them.
// The calling thread drives all engines; nothing here is a collective.
// what a part needs to know about the part(s) in front of it: where their slab is and how it is laid out
struct ShardPeer { const void* slab = nullptr; size_t halo_slots = 0; int device = -1; hipEvent_t ev = nullptr; int first_tile = 0, tile_count = 0; };

// phase 1 of a sharded frame on this engine: upload, slots of its own tiles, their network passes into the slab behind the slots reserved for the
// preceding parts' bands; records ev0 and ev_shard on the compute stream (no host synchronisation)
static void shard_phase1(Img2Img::Impl& e, const Image& src, const TileGrid& grid, const ShardPlan& sp, bool report) {
    const int rows = src.rows, cols = src.cols, s = e.cfg.scaling, steps = e.cfg.tta ? 8 : 1;
    e.deep = false;
    e.ensure(e.d_frame, e.frame_cap, (size_t)rows * cols * 3);
    e.ensure(e.d_out, e.out_cap, (size_t)rows * s * cols * s * 3);
    hipAssert(hipMemcpy2DAsync(e.d_frame, (size_t)cols * 3, src.data, src.step, (size_t)cols * 3, rows, hipMemcpyHostToDevice, e.stream));
    const size_t stepCount = e.pass_slots(sp.tile_count);
    e.fill_slots(grid, sp.first_tile, sp.tile_count, 1, 0, stepCount);
    e.shard_halo_slots = halo_slots(sp, steps);
    e.upload_slots(grid, stepCount, e.shard_halo_slots + stepCount);
    hipAssert(hipEventRecord(e.ev0, e.stream));
    e.run_passes(rows, cols, sp.tile_count, e.shard_halo_slots, report, 0, true);
    if (!e.ev_shard) hipAssert(hipEventCreateWithFlags(&e.ev_shard, hipEventDisableTiming));
    hipAssert(hipEventRecord(e.ev_shard, e.stream));
}

// phase 2 on this engine (part k): the seam exchange - behind the owners' events (where there are events: engines of this process; slabs of other
// processes are complete when their handles arrive) copy the blend bands of the tiles [halo_first, first_tile) out of the owners' slabs - then compose and
// download this part's rectangles (asynchronously: the caller synchronises the stream)
static void shard_phase2(Img2Img::Impl& e, int k, const std::vector<ShardPlan>& sp, const std::vector<ShardPeer>& peers, const TileGrid& grid, int rows, int cols, Image& dst) {
    const int steps = e.cfg.tta ? 8 : 1, To = e.plan.Tout;
    const size_t px = (size_t)4 * e.plan.elt, slot_bytes = (size_t)To * To * px;
    const bool overlapping = e.cfg.overlapX != 0 || e.cfg.overlapY != 0;
    int waited = -1;
    bool peer2d = true;                                                    // (of the owner last waited for)
    for (int g = sp[k].halo_first; g < sp[k].first_tile && overlapping; ++g) {
        int q = k - 1;
        while (q >= 0 && !(sp[q].tile_count > 0 && g >= sp[q].first_tile && g < sp[q].first_tile + sp[q].tile_count)) --q;
        if (q < 0 || !peers[q].slab) throw std::runtime_error("shard plan: tile " + std::to_string(g) + " has no owner");
        const ShardPeer& o = peers[q];
        if (q != waited) {                                                 // once per owner: its event, and how its bands can travel
            if (o.ev) hipAssert(hipStreamWaitEvent(e.stream, o.ev, 0));
            waited = q;
            peer2d = o.device == e.device;
            if (!peer2d) {      // strided band copies between devices need peer access; without it whole slots travel by hipMemcpyPeerAsync
                int can = 0;
                if (o.device >= 0 && hipDeviceCanAccessPeer(&can, e.device, o.device) == hipSuccess && can) {
                    const hipError_t pe = hipDeviceEnablePeerAccess(o.device, 0);
                    peer2d = pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled;
                }
                (void)hipGetLastError();
            }
        }
        for (int a = 0; a < steps; ++a) {
            const uint8_t* from = (const uint8_t*)o.slab + (o.halo_slots + (size_t)(g - sp[q].first_tile) * steps + a) * slot_bytes;
            uint8_t* to = (uint8_t*)e.d_slab + ((size_t)(g - sp[k].halo_first) * steps + a) * slot_bytes;
            if (!peer2d) {
                if (o.device >= 0) hipAssert(hipMemcpyPeerAsync(to, e.device, from, o.device, slot_bytes, e.stream));
                else hipAssert(hipMemcpyAsync(to, from, slot_bytes, hipMemcpyDefault, e.stream));
                continue;
            }
            int bx = std::min(To, grid.outOvX), by = std::min(To, grid.outOvY);
            if (steps > 1) bx = by = std::max(bx, by);                     // a rotation turns a column band into a row band of the same width
            const size_t pitch = (size_t)To * px;
            auto cols_band = [&](int x0) { if (bx > 0) hipAssert(hipMemcpy2DAsync(to + (size_t)x0 * px, pitch, from + (size_t)x0 * px, pitch, (size_t)bx * px, To, hipMemcpyDeviceToDevice, e.stream)); };
            auto rows_band = [&](int y0) { if (by > 0) hipAssert(hipMemcpyAsync(to + (size_t)y0 * pitch, from + (size_t)y0 * pitch, (size_t)by * pitch, hipMemcpyDeviceToDevice, e.stream)); };
            cols_band(To - bx); rows_band(To - by);                        // what the cells to the right of / below the tile read
            if (steps > 1) { cols_band(0); rows_band(0); }                // an augmented tile is read through its inverse dihedral map
        }
    }
    for (int r = 0; r < sp[k].nrect; ++r) {
        const Rect& rc = sp[k].rect[r];
        e.compose_rect(rows, cols, grid, rc.x, rc.x + rc.w, rc.y, rc.y + rc.h, sp[k].halo_first);
    }
    hipAssert(hipEventRecord(e.ev1, e.stream));
    for (int r = 0; r < sp[k].nrect; ++r) {
        const Rect& rc = sp[k].rect[r];
        hipAssert(hipMemcpy2DAsync(dst.data + (size_t)rc.y * dst.step + (size_t)rc.x * 3, dst.step, e.d_out + ((size_t)rc.y * dst.cols + rc.x) * 3, (size_t)dst.cols * 3,
                                   (size_t)rc.w * 3, rc.h, hipMemcpyDeviceToHost, e.stream));
    }
}

// the total factor of a chain
static int cp_total(const int* scalings, int count) { int S = 1; for (int k = 0; k < count; ++k) S *= scalings[k]; return S; }

// frame / output checks shared by the sharded entries; "" when fine
static std::string shard_frame_problem(const Img2Img::Impl& e, const Image& src, const Image* dst) {
    const int s = e.cfg.scaling;
    if (src.depth != 8 || (dst && dst->depth != 8)) return "sharded rendering takes 8-bit frames.";
    if (!src.data || src.rows <= 0 || src.cols <= 0 || src.step < (size_t)src.cols * 3) return "Input image is empty or has an invalid step.";
    if (dst && (!dst->data || dst->rows != src.rows * s || dst->cols != src.cols * s || dst->step < (size_t)dst->cols * 3))
        return "Output image has invalid size: expected " + std::to_string(src.cols * s) + "x" + std::to_string(src.rows * s) + ".";
    return "";
}

bool Img2Img::renderSharded(Img2Img* const* engines, int count, const Image& src, Image& dst) {
    if (!engines || count <= 0 || !engines[0]) return false;
    Img2Img* const first = engines[0];
    Impl* const impl = first->impl.get();                      // (the log macros name `impl`)
    for (int k = 0; k < count; ++k)                            // (any engine under Wrap or Mirror: refused through engines[0]'s callback)
        if (engines[k] && engines[k]->impl->edge != kEdgeReplicate) {
            W2X_LOG(error, "Shards of a frame are not built under setEdge(" + std::string(edge_mode_name(engines[k]->impl->edge)) + ") (engine " + std::to_string(k) + "): only setEdge(replicate) serves this call.");
            return false;
        }
    try {
        for (int k = 0; k < count; ++k) {
            if (!engines[k] || !engines[k]->impl->loaded) { W2X_LOG(error, "Render called before a successful load (engine " + std::to_string(k) + ")."); return false; }
            const Impl& a = *engines[k]->impl;
            const RenderConfig &c = a.cfg, &c0 = impl->cfg;
            if (a.plan.T != impl->plan.T || a.plan.Tout != impl->plan.Tout || a.plan.elt != impl->plan.elt || c.scaling != c0.scaling || c.overlapX != c0.overlapX ||
                c.overlapY != c0.overlapY || c.tta != c0.tta || c.ttaBugCompat != c0.ttaBugCompat || c.batchSize != c0.batchSize) {
                W2X_LOG(error, "renderSharded: engine " + std::to_string(k) + " was loaded with another model or configuration."); return false;
            }
            if (a.light != impl->light) { W2X_LOG(error, "renderSharded: engine " + std::to_string(k) + " has another resize-light setting."); return false; }
            if (a.dither.mode != impl->dither.mode || a.dither.phase != impl->dither.phase || a.dither.advance != impl->dither.advance) {
                W2X_LOG(error, "renderSharded: engine " + std::to_string(k) + " has another dither setting."); return false;
            }
            for (int j = 0; j < k; ++j) if (engines[j] == engines[k]) { W2X_LOG(error, "renderSharded: the same engine twice."); return false; }
        }
        const RenderConfig& cfg = impl->cfg;
        const Plan& plan = impl->plan;
        const int rows = src.rows, cols = src.cols, s = cfg.scaling;
        if (const std::string why = shard_frame_problem(*impl, src, &dst); !why.empty()) { W2X_LOG(error, why); return false; }
        TileGrid grid;
        if (const std::string why = impl->frame_grid(rows, cols, grid); !why.empty()) { W2X_LOG(error, why); return false; }
        std::vector<ShardPlan> sp;
        if (!shard_plans(grid, cols * s, rows * s, plan.Tout, count, sp)) { W2X_LOG(error, "renderSharded: the blend bands are wider than the tile stride; use render or renderStrip."); return false; }
        // ---- phase 1: every engine computes its own tiles
        for (int k = 0; k < count; ++k) {
            Impl& e = *engines[k]->impl;
            if (sp[k].tile_count == 0) continue;
            DeviceGuard guard(e.device);
            shard_phase1(e, src, grid, sp[k], k == 0);
        }
        // ---- phase 2: seam exchange, compose, download
        std::vector<ShardPeer> peers(count);
        for (int k = 0; k < count; ++k) {
            const Impl& e = *engines[k]->impl;
            if (sp[k].tile_count) peers[k] = ShardPeer{e.d_slab, e.shard_halo_slots, e.device, e.ev_shard, sp[k].first_tile, sp[k].tile_count};
        }
        for (int k = 0; k < count; ++k) {
            Impl& e = *engines[k]->impl;
            if (sp[k].tile_count == 0) continue;
            DeviceGuard guard(e.device);
            shard_phase2(e, k, sp, peers, grid, rows, cols, dst);
        }
        for (int k = 0; k < count; ++k) {
            Impl& e = *engines[k]->impl;
            if (sp[k].tile_count == 0) continue;
            DeviceGuard guard(e.device);
            hipAssert(hipStreamSynchronize(e.stream));
            hipAssert(hipEventElapsedTime(&e.last_ms, e.ev0, e.ev1));
        }
        return true;
    } catch (const std::exception& ex) {
        for (int k = 0; k < count; ++k) if (engines[k] && engines[k]->impl->stream) { try { DeviceGuard guard(engines[k]->impl->device); (void)hipStreamSynchronize(engines[k]->impl->stream); } catch (...) {} }
        W2X_LOG(error, "Render failed unexpectedly: " + std::string(ex.what()) + ".");
        return false;
    }
}

// The same two phases for ONE PROCESS PER GPU (the launch contract of bench.py / torch.distributed.run): rank r calls shardCompute(src, r, N), publishes
// its slab (shardSlab: a device pointer the caller exports with w2x_ipc_export and its peers open with w2x_ipc_open), and after every rank has done so
// (a host-side barrier - the handle exchange itself) shardFinish(dst, r, N, slabs) with the opened pointers of the parts in front of it.  No collective on
// the data path: the seam bands are device-to-device copies out of the neighbours' slabs.
bool Img2Img::shardCompute(const Image& src, int part, int parts) {
    const char* who = "shardCompute";
    if (impl->edge_refuses(who, "Shards of a frame are")) return false;
    return impl->entry(who, kNotLoaded, kRenderFailed, [&] {   // (the call's own work, to the closing `});` - deliberately left at function indentation)
    if (parts <= 0 || part < 0 || part >= parts) { W2X_LOG_AS(who, error, "Invalid part index."); return false; }
    if (const std::string why = shard_frame_problem(*impl, src, nullptr); !why.empty()) { W2X_LOG_AS(who, error, why); return false; }
    const Plan& plan = impl->plan;
    const int rows = src.rows, cols = src.cols, s = impl->cfg.scaling;
    TileGrid grid;
    if (const std::string why = impl->frame_grid(rows, cols, grid); !why.empty()) { W2X_LOG_AS(who, error, why); return false; }
    impl->shard_rows = rows; impl->shard_cols = cols;
    std::vector<ShardPlan> sp;
    if (!shard_plans(grid, cols * s, rows * s, plan.Tout, parts, sp)) { W2X_LOG_AS(who, error, "the blend bands are wider than the tile stride; use render or renderStrip."); return false; }
    if (sp[part].tile_count == 0) return true;                 // more parts than tiles: this one has no share
    shard_phase1(*impl, src, grid, sp[part], true);
    hipAssert(hipStreamSynchronize(impl->stream));           // the slab is complete when this returns: what the peers copy from after the barrier
    return true;
    });
}

const void* Img2Img::shardSlab(size_t* bytes) const { if (bytes) *bytes = impl->slab_cap; return impl->d_slab; }

bool Img2Img::shardFinish(Image& dst, int part, int parts, const void* const* slabs, const int* devices) {
    const char* who = "shardFinish";
    const char* no_compute = "shardFinish without a shardCompute.";
    if (impl->edge_refuses(who, "Shards of a frame are")) return false;
    return impl->entry(who, no_compute, kRenderFailed, [&] {   // (the call's own work, to the closing `});` - deliberately left at function indentation)
    if (impl->shard_rows <= 0) { W2X_LOG_AS(who, error, no_compute); return false; }
    if (parts <= 0 || part < 0 || part >= parts || !slabs) { W2X_LOG_AS(who, error, "Invalid part index."); return false; }
    const Plan& plan = impl->plan;
    const int rows = impl->shard_rows, cols = impl->shard_cols, s = impl->cfg.scaling, steps = impl->cfg.tta ? 8 : 1;
    Image probe; probe.data = (uint8_t*)1; probe.rows = rows; probe.cols = cols; probe.step = (size_t)cols * 3;
    if (const std::string why = shard_frame_problem(*impl, probe, &dst); !why.empty()) { W2X_LOG_AS(who, error, why); return false; }
    TileGrid grid;                                             // (the grid shardCompute() accepted)
    if (const std::string why = impl->frame_grid(rows, cols, grid); !why.empty()) { W2X_LOG_AS(who, error, why); return false; }
    std::vector<ShardPlan> sp;
    std::vector<ShardPeer> peers(parts);
    shard_plans(grid, cols * s, rows * s, plan.Tout, parts, sp);   // (shardCompute() has checked that every tile has an owner)
    for (int k = 0; k < parts; ++k)
        if (sp[k].tile_count) peers[k] = ShardPeer{k == part ? impl->d_slab : slabs[k], halo_slots(sp[k], steps), k == part ? impl->device : devices ? physical_device(devices[k]) : -1,
                                                   nullptr, sp[k].first_tile, sp[k].tile_count};
    if (sp[part].tile_count == 0) return true;
    shard_phase2(*impl, part, sp, peers, grid, rows, cols, dst);
    hipAssert(hipStreamSynchronize(impl->stream));
    hipAssert(hipEventElapsedTime(&impl->last_ms, impl->ev0, impl->ev1));
    return true;
    });
}

// device memory of another process: export / open / close (hipIpc*); the opened pointer is valid in this process on the current device
bool ipc_export(const void* device_ptr, uint8_t out[64]) {
    static_assert(sizeof(hipIpcMemHandle_t) <= 64, "handle size");
    hipIpcMemHandle_t h;
    if (!device_ptr || hipIpcGetMemHandle(&h, const_cast<void*>(device_ptr)) != hipSuccess) { (void)hipGetLastError(); return false; }
    memset(out, 0, 64); memcpy(out, &h, sizeof(h));
    return true;
}
void* ipc_open(const uint8_t handle[64], int deviceId) {
    const int dev = physical_device(deviceId);
    if (!device_ordinal_problem(deviceId, dev).empty()) return nullptr;
    DeviceGuard guard(dev);
    hipIpcMemHandle_t h; memcpy(&h, handle, sizeof(h));
    void* p = nullptr;
    if (hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void ipc_close(void* p) { if (p && hipIpcCloseMemHandle(p) != hipSuccess) (void)hipGetLastError(); }

// A sequence of equally sized frames (a video, main.cpp:263-269) with the PCIe copies taken off the critical path: frame i+1 is
// uploaded and frame i-1 downloaded on two copy streams while frame i runs on the compute stream (two device frame / output
// buffers, events between the three streams).  Each frame is the same gather -> network -> compose as render(), so outputs are
// bit-identical; the progress callback is not raised per batch here.  Copies only overlap when the host buffers are page-locked
// (pinHost); with pageable memory the call is still correct, the runtime just serialises the copies.
bool Img2Img::renderSequence(const Image* srcs, Image* dsts, int count) { return runSequence(srcs, dsts, count, -1, "renderSequence"); }

// renderResized() over a sequence: every frame resized to dsts[i].rows x dsts[i].cols (one target size), the canvas compose and the resample on the
// compute side of the rolling pipeline (run_rolling_frame), the copy streams overlapped as in renderSequence().  At the scaled size it is renderSequence().
bool Img2Img::renderSequenceResized(const Image* srcs, Image* dsts, int count, ResizeFilter filter) {
    return runSequence(srcs, dsts, count, filter_id(filter), "renderSequenceResized");
}

bool Img2Img::runSequence(const Image* srcs, Image* dsts, int count, int resizeFilter, const char* who) {
    return impl->entry(who, kNotLoaded, kRenderFailed, [&] {   // (the call's own work, to the closing `});` - deliberately left at function indentation)
    if (count <= 0) return true;
    Impl::FrameCall c;
    if (const std::string why = impl->bgr_sequence_check(srcs, dsts, count, resizeFilter, who, c); !why.empty()) { W2X_LOG_AS(who, error, why); return false; }
    impl->run_packed_call(c, srcs, dsts, count, false, resizeFilter, 3);      // (lastRenderMs(): compute-stream time per frame of the sequence)
    impl->last_rows = c.rows; impl->last_cols = c.cols; impl->last_grid = c.grid; impl->last_strip = c.sp;
    if (c.resized) impl->last_rows = impl->last_cols = 0;   // (not replayed by benchResident: renderPart)
    return true;
    });
}

// renderYuv(): the sequence of one frame (run_frame: no rolling)
bool Img2Img::renderYuv(const YuvImage& src, YuvImage& dst, YuvFormat format) { return runSequenceYuv(&src, &dst, 1, format, -1, "renderYuv"); }

bool Img2Img::renderSequenceYuv(const YuvImage* srcs, YuvImage* dsts, int count, YuvFormat format) {
    return runSequenceYuv(srcs, dsts, count, format, -1, "renderSequenceYuv");
}

// renderYuv() with the canvas resized to dst.rows x dst.cols before it is encoded: the frame's tiles from its planes (gather_yuv_kernel),
// compose_canvas_kernel (fp32 canvas, not clamped), resample_yuv_kernel (k_resample.hip: the resize of renderResized, then clamp, Y per pixel, chroma of
// the filtered RGB; dst.layout I422, I444, NV12: the kernels of k_resample_yuv.hip), the download of the target's planes.  At the scaled size it is
// renderYuv().
bool Img2Img::renderYuvResized(const YuvImage& src, YuvImage& dst, YuvFormat format, ResizeFilter filter) {
    return runSequenceYuv(&src, &dst, 1, format, filter_id(filter), "renderYuvResized");
}

bool Img2Img::renderSequenceYuvResized(const YuvImage* srcs, YuvImage* dsts, int count, YuvFormat format, ResizeFilter filter) {
    return runSequenceYuv(srcs, dsts, count, format, filter_id(filter), "renderSequenceYuvResized");
}

// YUV frames through renderSequence()'s pipeline: per frame one copy per plane up on s_up (three, NV12 two), the passes with gather_yuv_kernel, the compose
// kernel of the output layout (on the second group's stream when the sequence rolls), one copy per plane down on s_dn.  One size, one pair of depths and one
// pair of layouts (srcs[0].layout, dsts[0].layout: DESIGN 9f) for the sequence; nothing is repacked or converted on the host.
// resizeFilter >= 0 (renderYuvResized / renderSequenceYuvResized): every dst is the target size of dsts[0], the frame step ends with the canvas compose
// and resample_yuv_kernel; at the scaled size it is the plain sequence.
bool Img2Img::runSequenceYuv(const YuvImage* srcs, YuvImage* dsts, int count, YuvFormat format, int resizeFilter, const char* who) {
    if (impl->edge_refuses(who, "YUV frames are")) return false;
    return impl->entry(who, kNotLoaded, kRenderFailed, [&] {   // (the call's own work, to the closing `});` - deliberately left at function indentation)
    if (count <= 0) return true;
    if (!srcs || !dsts) { W2X_LOG_AS(who, error, "No frames given."); return false; }
    Impl::FrameCall call;
    if (const std::string why = impl->yuv_check(srcs, dsts, count, format, resizeFilter, call); !why.empty()) { W2X_LOG_AS(who, error, why); return false; }
    const int matrix = (int)format.matrix, range = (int)format.range, in_bits = srcs[0].bits, out_bits = dsts[0].bits, in_layout = (int)srcs[0].layout;
    Impl::YuvJob& job = impl->job.yuv;
    impl->job.kind = Impl::Job::YUV;
    job.in = yuv_coefs(matrix, range, in_bits); job.out = yuv_coefs(matrix, range, out_bits);
    job.in_bits = in_bits; job.out_bits = out_bits; job.in_layout = in_layout; job.out_layout = (int)dsts[0].layout;
    job.in_siting = (int)srcs[0].siting; job.out_siting = (int)dsts[0].siting;
    job.key = 2 + (in_bits == 10 ? 1 : 0) + 2 * range + 4 * matrix + 12 * in_layout;   // 2 .. 13 per layout: 2 .. 49, below kRgbaKey
    // the siting the gather launch dispatches on (launch_gather_yuv: I444 none, I422 the column rule alone): centre 102 .. 149, top-left 202 .. 249, above every other format's key
    job.key += 100 * (in_layout == kYuvI444 || (in_layout == kYuvI422 && job.in_siting == kYuvTopLeft) ? kYuvLeft : job.in_siting);
    // the planes of a frame (NV12 two, else three) between the caller's layout and the device's (yuv_layout), on copy stream `on`
    auto copy_planes = [&](const YuvImage& host, uint8_t* dev, int r, int c, bool up, hipStream_t on) {
        const int layout = (int)host.layout;
        const YuvPlanes d = Impl::yuv_layout(dev, r, c, host.bits, layout);
        const size_t bps = host.bits > 8 ? 2 : 1;
        for (int k = 0; k < Impl::yuv_planes(layout); ++k) {
            const size_t width = (size_t)(k ? yuv_chroma_samples(c, layout) : c) * bps; const int h = k ? yuv_chroma_rows(r, layout) : r;
            if (up) hipAssert(hipMemcpy2DAsync(d.p[k], d.step[k], host.planes[k], host.steps[k], width, h, hipMemcpyHostToDevice, on));
            else hipAssert(hipMemcpy2DAsync(host.planes[k], host.steps[k], d.p[k], d.step[k], width, h, hipMemcpyDeviceToHost, on));
        }
    };
    impl->run_call(call, count, false, resizeFilter,
        [&](int i, uint8_t* dev, hipStream_t on) { copy_planes(srcs[i], dev, call.rows, call.cols, true, on); },
        [&](int i, uint8_t* dev, hipStream_t on) { copy_planes(dsts[i], dev, call.out_rows, call.out_cols, false, on); });
    return true;
    });
}

// RGBA frames.  One upload (4 bytes per pixel), alpha_bleed_kernel (the BGR frame with the visible colours spread under alpha == 0, the alpha plane, the
// plane's range), ONE schedule of the frame's N colour tiles followed by its N alpha tiles - cut into reference batches and network passes as run_passes() cuts any
// tile count, so a pass at the boundary holds tiles of both kinds -, compose_rgba_kernel, one download (4 bytes per output pixel).  A single part on the compute
// stream: the multi-part overlap of render() is not used here.  skipUniformAlpha: the two words come back behind the bleed kernel while the passes that hold colour
// tiles only - the same in the 2N and the N schedule - are issued; their progress is reported once the total is known.  (The frame step is Impl::rgba_frame.)
bool Img2Img::renderRgba(const Image& src, Image& dst, const RgbaOptions& opt) { return renderRgbaFrame(src, dst, opt, -1, "renderRgba"); }

// renderRgba() with the canvas resized to dst.rows x dst.cols: the same upload, bleed and schedule, then compose_canvas_rgba_kernel (four fp32 planes,
// not quantised) and resample_rgba_kernel (the resize of renderResized over the four planes, BGRA dwords), the download of the target.  Colour and alpha are resized
// separately and straight.  At the scaled size it is renderRgba().
bool Img2Img::renderRgbaResized(const Image& src, Image& dst, const RgbaOptions& opt, ResizeFilter filter) {
    return renderRgbaFrame(src, dst, opt, filter_id(filter), "renderRgbaResized");
}

bool Img2Img::renderRgbaFrame(const Image& src, Image& dst, const RgbaOptions& opt, int resizeFilter, const char* who) {
    return impl->entry(who, kNotLoaded, kRenderFailed, [&] { return impl->rgba_call(&src, &dst, 1, opt, resizeFilter, who, true); });
}

// RGBA frames through renderSequence()'s pipeline: frame i is uploaded at 4 bytes per pixel on s_up into one of two frame buffers, its frame step
// (Impl::rgba_frame) runs on the compute stream into one of two output buffers, and the output leaves at 4 bytes per pixel on s_dn while frame i + 1 runs.
// One size, one target and one set of options for the sequence; output i is the bytes of the single-frame call on frame i.  No progress is reported.
bool Img2Img::renderSequenceRgba(const Image* srcs, Image* dsts, int count, const RgbaOptions& opt) { return runSequenceRgba(srcs, dsts, count, opt, -1, "renderSequenceRgba"); }

bool Img2Img::renderSequenceRgbaResized(const Image* srcs, Image* dsts, int count, const RgbaOptions& opt, ResizeFilter filter) {
    return runSequenceRgba(srcs, dsts, count, opt, filter_id(filter), "renderSequenceRgbaResized");
}

bool Img2Img::runSequenceRgba(const Image* srcs, Image* dsts, int count, const RgbaOptions& opt, int resizeFilter, const char* who) {
    return impl->entry(who, kNotLoaded, kRenderFailed, [&] {   // (the call's own work, to the closing `});` - deliberately left at function indentation)
    if (count <= 0) return true;
    if (!srcs || !dsts) { W2X_LOG_AS(who, error, "No frames given."); return false; }
    return impl->rgba_call(srcs, dsts, count, opt, resizeFilter, who, false);
    });
}

// Gray frames: Image read as ONE channel.  renderGray(g) is the green channel of render() of the frame B = G = R = g, byte for byte, at 8 and 16 bits:
// one 2-D upload of a sample per pixel, the frame's tiles through gather_planes_kernel, compose_planes_kernel at one plane, one 2-D download of a sample per output pixel; nothing is
// replicated or picked apart on the host.  A single part on the compute stream; progress as render() reports it, ceil(N * steps / batchSize) batches.
bool Img2Img::renderGray(const Image& src, Image& dst) { return runGray(&src, &dst, 1, -1, "renderGray", true); }

// renderGray() with the canvas resized to dst.rows x dst.cols: compose_canvas_gray_kernel (one fp32 plane) and resample_planes_kernel; the green channel of
// renderResized() of the replicated frame.  At the scaled size it is renderGray().
bool Img2Img::renderGrayResized(const Image& src, Image& dst, ResizeFilter filter) { return runGray(&src, &dst, 1, filter_id(filter), "renderGrayResized", true); }

// Gray frames through renderSequence()'s pipeline (rolling when a BGR sequence of the size rolls): 8-bit frames of one size, output i the bytes of the single call
bool Img2Img::renderSequenceGray(const Image* srcs, Image* dsts, int count) { return runGray(srcs, dsts, count, -1, "renderSequenceGray", false); }

bool Img2Img::renderSequenceGrayResized(const Image* srcs, Image* dsts, int count, ResizeFilter filter) {
    return runGray(srcs, dsts, count, filter_id(filter), "renderSequenceGrayResized", false);
}

// single: one frame on the compute stream with progress (8 or 16 bits); else the sequence pipeline (8 bits, no progress)
bool Img2Img::runGray(const Image* srcs, Image* dsts, int count, int resizeFilter, const char* who, bool single) {
    return impl->entry(who, kNotLoaded, kRenderFailed, [&] {   // (the call's own work, to the closing `});` - deliberately left at function indentation)
    if (count <= 0) return true;
    if (!srcs || !dsts) { W2X_LOG_AS(who, error, "No frames given."); return false; }
    Impl::FrameCall c;
    if (const std::string why = impl->gray_check(srcs, dsts, count, resizeFilter, who, single, c); !why.empty()) { W2X_LOG_AS(who, error, why); return false; }
    impl->job.kind = Impl::Job::GRAY; impl->job.gray.deep = srcs[0].depth == 16;
    impl->run_packed_call(c, srcs, dsts, count, single, resizeFilter, srcs[0].depth / 8);
    return true;
    });
}

// Planar RGB frames: three planes R, G, B of 8, 10, 12, 16 bits or float32 on either side.  At 8 / 8 and 16 / 16 bits renderPlanar() gives the planes
// of render() of the interleaved frame, byte for byte; the other depths widen the same expressions (img2img.h).  Per frame three 2-D copies up, the frame's tiles
// through gather_planes_kernel, compose_planes_kernel, three 2-D copies down; nothing is interleaved or narrowed on the host.  The single calls run as one part on
// the compute stream and report progress as render() does, ceil(N * steps / batchSize) batches.
bool Img2Img::renderPlanar(const PlanarImage& src, PlanarImage& dst) { return runPlanar(&src, &dst, 1, -1, "renderPlanar", true); }

// renderPlanar() with the canvas resized to dst.rows x dst.cols: compose_canvas_kernel (the canvas of renderResized()) and resample_planes_kernel.  At the
// scaled size it is renderPlanar().
bool Img2Img::renderPlanarResized(const PlanarImage& src, PlanarImage& dst, ResizeFilter filter) {
    return runPlanar(&src, &dst, 1, filter_id(filter), "renderPlanarResized", true);
}

// Planar frames through renderSequence()'s pipeline (rolling when a BGR sequence of the size rolls): every depth, one pair of depths and one size per sequence,
// output i the bytes of the single call on frame i.  No progress is reported.
bool Img2Img::renderSequencePlanar(const PlanarImage* srcs, PlanarImage* dsts, int count) { return runPlanar(srcs, dsts, count, -1, "renderSequencePlanar", false); }

bool Img2Img::renderSequencePlanarResized(const PlanarImage* srcs, PlanarImage* dsts, int count, ResizeFilter filter) {
    return runPlanar(srcs, dsts, count, filter_id(filter), "renderSequencePlanarResized", false);
}

bool Img2Img::runPlanar(const PlanarImage* srcs, PlanarImage* dsts, int count, int resizeFilter, const char* who, bool single) {
    return impl->entry(who, kNotLoaded, kRenderFailed, [&] {   // (the call's own work, to the closing `});` - deliberately left at function indentation)
    if (count <= 0) return true;
    if (!srcs || !dsts) { W2X_LOG_AS(who, error, "No frames given."); return false; }
    Impl::FrameCall call;
    if (const std::string why = impl->planar_check(srcs, dsts, count, resizeFilter, call); !why.empty()) { W2X_LOG_AS(who, error, why); return false; }
    impl->job.kind = Impl::Job::PLANAR; impl->job.planar.in_bits = srcs[0].bits; impl->job.planar.out_bits = dsts[0].bits;
    // the three planes of a frame between the caller's pointers and the device layout (planar_layout), on stream `on`
    auto copy_planes = [&](const PlanarImage& host, uint8_t* dev, int r, int c, bool up, hipStream_t on) {
        const PlanarPlanes d = Impl::planar_layout(dev, r, c, host.bits);
        const size_t width = (size_t)c * planar_sample_bytes(host.bits);
        for (int k = 0; k < 3; ++k) {
            if (up) hipAssert(hipMemcpy2DAsync(d.p[k], d.step[k], host.planes[k], host.steps[k], width, r, hipMemcpyHostToDevice, on));
            else hipAssert(hipMemcpy2DAsync(host.planes[k], host.steps[k], d.p[k], d.step[k], width, r, hipMemcpyDeviceToHost, on));
        }
    };
    impl->run_call(call, count, single, resizeFilter,
        [&](int i, uint8_t* dev, hipStream_t on) { copy_planes(srcs[i], dev, call.rows, call.cols, true, on); },
        [&](int i, uint8_t* dev, hipStream_t on) { copy_planes(dsts[i], dev, call.out_rows, call.out_cols, false, on); });
    return true;
    });
}

// Chained renders: ONE frame through `count` engines, the frame staying in HBM between them.  The six entries are runChained() over n frames,
// interleaved or planar.  Per stage k on engine e_k, all on e_k's compute stream: wait for stage k - 1's event, the stage's passes (gather_px_kernel out of
// engines[0]'s d_chain[k - 1] - stage 0: the format's gather out of d_frame), then compose_px_kernel into d_chain[k] - the last stage: the format's end of a frame
// into d_out -, an event.  Quantised, the stages run the format's own gather and compose with d_frame / d_out pointed at the chain's buffers.  Every stage has slot
// and liveness tables of its own (Impl::chain_tables), uploaded before the first frame without waiting for them.  The host synchronises once, behind the download.
bool Img2Img::renderChained(Img2Img* const* engines, int count, const Image& src, Image& dst, const ChainOptions& opt) {
    return runChained(engines, count, &src, &dst, nullptr, nullptr, 1, opt, -1, "renderChained", true);
}
bool Img2Img::renderChainedResized(Img2Img* const* engines, int count, const Image& src, Image& dst, const ChainOptions& opt, ResizeFilter filter) {
    return runChained(engines, count, &src, &dst, nullptr, nullptr, 1, opt, filter_id(filter), "renderChainedResized", true);
}
bool Img2Img::renderSequenceChained(Img2Img* const* engines, int count, const Image* srcs, Image* dsts, int n, const ChainOptions& opt) {
    return runChained(engines, count, srcs, dsts, nullptr, nullptr, n, opt, -1, "renderSequenceChained", false);
}
bool Img2Img::renderSequenceChainedResized(Img2Img* const* engines, int count, const Image* srcs, Image* dsts, int n, const ChainOptions& opt, ResizeFilter filter) {
    return runChained(engines, count, srcs, dsts, nullptr, nullptr, n, opt, filter_id(filter), "renderSequenceChainedResized", false);
}
bool Img2Img::renderChainedPlanar(Img2Img* const* engines, int count, const PlanarImage& src, PlanarImage& dst, const ChainOptions& opt) {
    return runChained(engines, count, nullptr, nullptr, &src, &dst, 1, opt, -1, "renderChainedPlanar", true);
}
bool Img2Img::renderChainedPlanarResized(Img2Img* const* engines, int count, const PlanarImage& src, PlanarImage& dst, const ChainOptions& opt, ResizeFilter filter) {
    return runChained(engines, count, nullptr, nullptr, &src, &dst, 1, opt, filter_id(filter), "renderChainedPlanarResized", true);
}

bool Img2Img::runChained(Img2Img* const* engines, int count, const Image* srcs, Image* dsts, const PlanarImage* psrcs, PlanarImage* pdsts, int n, const ChainOptions& opt,
                         int resizeFilter, const char* who, bool single) {
    if (!engines || !engines[0]) return false;                 // (nobody to tell)
    Impl* const impl = engines[0]->impl.get();                 // (the log macros name `impl`)
    auto refuse = [&](const std::string& why) { W2X_LOG_AS(who, error, why); return false; };
    // ---- the checks: the chain, the source as the single calls check it, the target (chain_plan), the destination, every stage's tile grid
    if (count < kChainMinStages || count > kChainMaxStages) return refuse(chain_refusal_text(kChainCount));
    for (int k = 0; k < count; ++k) if (!engines[k] || !engines[k]->impl->loaded) return refuse("Render called before a successful load (engine " + std::to_string(k) + ").");
    for (int k = 1; k < count; ++k) if (engines[k]->impl->device != impl->device) return refuse("The engines of a chain must live on one device (engine " + std::to_string(k) + " is on another).");
    if (n <= 0) return n == 0 ? true : refuse("No frames given.");
    const bool planar = psrcs != nullptr || pdsts != nullptr;
    if (planar ? !psrcs || !pdsts : !srcs || !dsts) return refuse("No frames given.");
    const bool quantize = opt.quantize;
    const int last = count - 1;
    const int rows = planar ? psrcs[0].rows : srcs[0].rows, cols = planar ? psrcs[0].cols : srcs[0].cols;
    const int in_bits = planar ? psrcs[0].bits : srcs[0].depth, out_bits = planar ? pdsts[0].bits : dsts[0].depth;
    auto planes_ok = [](const PlanarImage& f) {
        const size_t bps = planar_sample_bytes(f.bits);
        for (int k = 0; k < 3; ++k) if (!f.planes[k] || f.steps[k] < (size_t)f.cols * bps || ((((size_t)f.planes[k]) | f.steps[k]) & (bps - 1)) != 0) return false;
        return true;
    };
    if (planar) {
        if (!planar_bits_ok(in_bits) || !planar_bits_ok(out_bits)) return refuse("Planar frames must have 8, 10, 12, 16 or 32 (float) bits.");
        if (quantize && in_bits == 32) return refuse("A quantised chain takes integer samples: the frame between two stages has the source's depth.");
        if (rows <= 0 || cols <= 0) return refuse("Input image is empty.");
    } else {
        if (single) { if ((in_bits != 8 && in_bits != 16) || out_bits != in_bits) return refuse("Input and output images must both be 8-bit or both 16-bit."); }
        else for (int i = 0; i < n; ++i) if (srcs[i].depth != 8 || dsts[i].depth != 8) return refuse(std::string(who) + " takes 8-bit frames (16-bit images go through renderChained()).");
        if (!srcs[0].data || rows <= 0 || cols <= 0 || srcs[0].step < (size_t)cols * 3 * (in_bits / 8)) return refuse("Input image is empty or has an invalid step.");
    }
    if (resizeFilter >= 0 && resizeFilter != 0 && resizeFilter != 1) return refuse("Unknown resize filter.");
    int scalings[kChainMaxStages];
    for (int k = 0; k < count; ++k) scalings[k] = engines[k]->impl->cfg.scaling;
    ChainPlan cp;
    const int want_rows = planar ? pdsts[0].rows : dsts[0].rows, want_cols = planar ? pdsts[0].cols : dsts[0].cols;
    if (const ChainRefusal why = chain_plan(rows, cols, scalings, count, resizeFilter >= 0 ? want_rows : 0, resizeFilter >= 0 ? want_cols : 0, cp); why != kChainOk) {
        if (why == kChainTarget) return refuse("Output image has invalid size for a resize: " + std::to_string(want_cols) + "x" + std::to_string(want_rows) + " is not between " + std::to_string(cols) + "x" +
                                               std::to_string(rows) + " and " + std::to_string(cols * cp_total(scalings, count)) + "x" + std::to_string(rows * cp_total(scalings, count)) + ".");
        return refuse(chain_refusal_text(why));
    }
    const std::string out_size = "Output image has invalid size: expected " + std::to_string(cp.out_cols) + "x" + std::to_string(cp.out_rows) + ".";
    for (int i = 0; i < n; ++i) {
        if (planar) {
            if (psrcs[i].rows != rows || psrcs[i].cols != cols || psrcs[i].bits != in_bits) return refuse("Input images must be of one size and depth.");
            if (!planes_ok(psrcs[i])) return refuse("Input image has a missing plane or an invalid step.");
            if (pdsts[i].rows != cp.out_rows || pdsts[i].cols != cp.out_cols) return refuse(out_size);
            if (pdsts[i].bits != out_bits) return refuse("Output images must be of one depth.");
            if (!planes_ok(pdsts[i])) return refuse("Output image has a missing plane or an invalid step.");
        } else {
            const size_t px = (size_t)3 * (in_bits / 8);
            if (!srcs[i].data || srcs[i].rows != rows || srcs[i].cols != cols || srcs[i].step < cols * px) return refuse("Input images must be non-empty and of one size.");
            if (!dsts[i].data || dsts[i].rows != cp.out_rows || dsts[i].cols != cp.out_cols || dsts[i].step < cp.out_cols * px) return refuse(out_size);
        }
    }
    struct Stage { Impl* e = nullptr; Impl::FrameCall c; Impl::Job job; };
    Stage st[kChainMaxStages];
    for (int k = 0; k < count; ++k) {
        Stage& g = st[k];
        g.e = engines[k]->impl.get();
        g.c.rows = cp.rows[k]; g.c.cols = cp.cols[k];
        g.c.out_rows = k == last ? cp.out_rows : cp.rows[k + 1]; g.c.out_cols = k == last ? cp.out_cols : cp.cols[k + 1];
        g.c.resized = k == last && cp.resized;
        if (const std::string why = g.e->call_grid(g.c); !why.empty()) return refuse(why + " (stage " + std::to_string(k) + ")");
    }
    const bool deep = !planar && in_bits == 16;
    // the bytes of the frame behind stage k: tile pixels of the consuming engine, or (quantised) the format's device frame at the source's depth
    auto between_bytes = [&](int k) {
        const size_t r = (size_t)cp.rows[k + 1], c = (size_t)cp.cols[k + 1];
        if (!quantize) return r * c * 4 * (size_t)st[k + 1].e->plan.elt;
        return planar ? Impl::planar_step((int)c, in_bits) * r * 3 : Impl::bgr_step((int)c, deep) * r;
    };
    // Everything a stage changes on its engine for its own duration, put back on every exit: the job, the slot tables, the frame buffers, the sample depth, the
    // sequence's frame index, where progress goes, and the dither - the frame between two stages is never dithered, whatever the setting of the engine that
    // writes it; the last stage keeps its engine's.  (An engine may run several stages: each one enters and leaves.)
    struct StageScope {
        Impl& e; int k; Impl::Job job; uint8_t* frame; uint8_t* out; bool deep; unsigned seq; Impl* report; DitherOptions dither;
        StageScope(Impl& e_, int k_, bool is_last) : e(e_), k(k_), job(e_.job), frame(e_.d_frame), out(e_.d_out), deep(e_.deep), seq(e_.seq_frame), report(e_.report_to), dither(e_.dither) {
            e.swap_tables(k);
            if (!is_last) e.dither = DitherOptions{};
        }
        ~StageScope() { e.swap_tables(k); e.job = job; e.d_frame = frame; e.d_out = out; e.deep = deep; e.seq_frame = seq; e.report_to = report; e.dither = dither; }
    };
    try {
        DeviceGuard guard(impl->device);
        Impl& e0 = *st[0].e; Impl& eL = *st[last].e;
        // ---- set-up, once per call: the frames between the stages, the events, every stage's job, tables and slab, the two ends' frame buffers
        for (int k = 0; k < last; ++k) impl->ensure_chain(k, between_bytes(k));
        for (int k = 0; k < count; ++k) if (!impl->ev_chain_done[k]) hipAssert(hipEventCreateWithFlags(&impl->ev_chain_done[k], hipEventDisableTiming));
        for (int k = 0; k < last; ++k) if (!impl->ev_chain_read[k]) hipAssert(hipEventCreateWithFlags(&impl->ev_chain_read[k], hipEventDisableTiming));
        int batch0[kChainMaxStages + 1] = {0};
        for (int k = 0; k < count; ++k) batch0[k + 1] = batch0[k] + st[k].e->batch_count(st[k].c.sp.tile_count);
        for (int k = 0; k < count; ++k) {
            Stage& g = st[k];
            g.job.kind = planar ? Impl::Job::PLANAR : Impl::Job::BGR;
            g.job.planar.in_bits = k == 0 || quantize ? in_bits : 32; g.job.planar.out_bits = k == last ? out_bits : in_bits;
            if (!quantize) {
                if (k > 0) g.job.chain.src = impl->d_chain[k - 1];
                if (k < last) { g.job.chain.dst = impl->d_chain[k]; g.job.chain.dst_fp32 = st[k + 1].e->plan.elt == 4; }
            }
        }
        const size_t in_bytes = planar ? Impl::planar_step(cols, in_bits) * rows * 3 : Impl::bgr_step(cols, deep) * rows;
        const size_t out_bytes = planar ? Impl::planar_step(cp.out_cols, out_bits) * cp.out_rows * 3 : Impl::bgr_step(cp.out_cols, deep) * cp.out_rows;
        e0.ensure(e0.d_frame, e0.frame_cap, in_bytes);
        eL.ensure(eL.d_out, eL.out_cap, out_bytes);
        if (!single) {
            e0.ensure_copy_streams(); eL.ensure_copy_streams();
            e0.ensure(e0.d_frame2, e0.frame2_cap, in_bytes);
            eL.ensure(eL.d_out2, eL.out2_cap, out_bytes);
        }
        // render()'s pipelined parts for the last stage of a plain interleaved single call (tiles.h render_parts; one part for a small frame)
        RenderParts rp;
        {
            const Stage& g = st[last];
            const Plan& pl = g.e->plan;
            rp = render_parts(g.c.grid, g.c.sp, g.c.cols, g.c.cols * g.e->cfg.scaling, g.c.rows * g.e->cfg.scaling, pl.T, pl.Tout, g.e->cfg.tta ? 8 : 1, pl.userB, pl.B,
                              single && !planar && !cp.resized ? g.e->pipeline_parts : 1);
            rp.x_split = g.c.cols;                                 // (nothing of the stage's frame is uploaded: run_frame_in_parts copies no columns)
            rp.batch_total = batch0[count];
            for (int q = 0; q < rp.n; ++q) rp.part[q].batches_before += batch0[last];
        }
        for (int k = 0; k < count; ++k) {
            Stage& g = st[k];
            Impl& e = *g.e;
            StageScope scope(e, k, k == last);
            e.job = g.job;
            if (k == last && rp.n > 1) {
                for (int q = 0; q < rp.n; ++q) e.fill_slots(g.c.grid, g.c.sp.first_tile + rp.part[q].first, rp.part[q].tiles, 1, rp.part[q].slots_off, rp.part[q].slots);
                e.upload_slots(g.c.grid, rp.slot_total, rp.slab_slots);
            } else {
                const size_t stepCount = e.pass_slots(g.c.sp.tile_count);
                e.fill_slots(g.c.grid, 0, g.c.sp.tile_count, 1, 0, stepCount);
                e.upload_slots(g.c.grid, stepCount, stepCount);
            }
            if (g.c.resized) { e.job_resize(g.c.rows, g.c.cols, g.c.out_rows, g.c.out_cols, resizeFilter); g.job.rs = e.job.rs; }
        }
        for (int k = 0; k < count; ++k) { Impl& e = *st[k].e; e.last_rows = e.last_cols = 0; e.one_part_stale = false; e.deep = false; }   // (nothing of a chained call is replayable)
        // ---- one frame through the stages: its source in `frame` (stage 0's device buffer), its output in `out` (the last stage's); i: its index in the sequence
        auto run_stages = [&](uint8_t* frame, uint8_t* out, int i, hipEvent_t in_read, hipEvent_t out_free) {
            for (int k = 0; k < count; ++k) {
                Stage& g = st[k];
                Impl& e = *g.e;
                StageScope scope(e, k, k == last);
                e.job = g.job; e.deep = deep; e.report_to = impl;
                if (k == 0) e.d_frame = frame; else if (quantize) e.d_frame = (uint8_t*)impl->d_chain[k - 1];
                if (k == last) { e.d_out = out; e.seq_frame = (unsigned)i; } else if (quantize) e.d_out = (uint8_t*)impl->d_chain[k];
                if (k > 0) hipAssert(hipStreamWaitEvent(e.stream, impl->ev_chain_done[k - 1], 0));
                if (k == last && rp.n > 1) {                           // (a single call: nothing else is in flight)
                    e.run_frame_in_parts(g.c, rp, srcs[0], dsts[0]);
                    continue;
                }
                e.run_passes(g.c.rows, g.c.cols, g.c.sp.tile_count, 0, single, 0, true, batch0[k], batch0[count]);
                if (k > 0) hipAssert(hipEventRecord(impl->ev_chain_read[k - 1], e.stream));      // (every pass has joined its tile groups: the gathers are done)
                if (k == 0 && in_read) hipAssert(hipEventRecord(in_read, e.stream));
                if (k < last) hipAssert(hipStreamWaitEvent(e.stream, impl->ev_chain_read[k], 0));   // (a never-recorded event does not wait)
                if (k == last && out_free) hipAssert(hipStreamWaitEvent(e.stream, out_free, 0));
                e.finish_frame(g.c.rows, g.c.cols, g.c.grid, g.c.sp, e.stream, nullptr, nullptr);
                hipAssert(hipEventRecord(impl->ev_chain_done[k], e.stream));
            }
        };
        // frame i between the caller's memory and the device layout of the format, on stream `on`
        auto copy_planes = [&](const PlanarImage& host, uint8_t* dev, int r, int c, bool up, hipStream_t on) {
            const PlanarPlanes d = Impl::planar_layout(dev, r, c, host.bits);
            const size_t width = (size_t)c * planar_sample_bytes(host.bits);
            for (int k = 0; k < 3; ++k) {
                if (up) hipAssert(hipMemcpy2DAsync(d.p[k], d.step[k], host.planes[k], host.steps[k], width, r, hipMemcpyHostToDevice, on));
                else hipAssert(hipMemcpy2DAsync(host.planes[k], host.steps[k], d.p[k], d.step[k], width, r, hipMemcpyDeviceToHost, on));
            }
        };
        const size_t px = (size_t)3 * (deep ? 2 : 1);
        auto up = [&](int i, uint8_t* dev, hipStream_t on) {
            if (planar) copy_planes(psrcs[i], dev, rows, cols, true, on);
            else hipAssert(hipMemcpy2DAsync(dev, (size_t)cols * px, srcs[i].data, srcs[i].step, (size_t)cols * px, rows, hipMemcpyHostToDevice, on));
        };
        auto down = [&](int i, uint8_t* dev, hipStream_t on) {
            if (planar) copy_planes(pdsts[i], dev, cp.out_rows, cp.out_cols, false, on);
            else hipAssert(hipMemcpy2DAsync(dsts[i].data, dsts[i].step, dev, (size_t)cp.out_cols * px, (size_t)cp.out_cols * px, cp.out_rows, hipMemcpyDeviceToHost, on));
        };
        auto sync_all = [&] { for (int k = 0; k < count; ++k) hipAssert(hipStreamSynchronize(st[k].e->stream)); };
        if (single) {
            up(0, e0.d_frame, e0.stream);
            hipAssert(hipEventRecord(e0.ev0, e0.stream));
            run_stages(e0.d_frame, eL.d_out, 0, nullptr, nullptr);
            if (rp.n == 1) {
                hipAssert(hipEventRecord(eL.ev1, eL.stream));
                down(0, eL.d_out, eL.stream);
            }
            sync_all();
            hipAssert(hipEventElapsedTime(&impl->last_ms, e0.ev0, eL.ev1));
            return true;
        }
        // a sequence: run_sequence()'s three streams - frame i + 1 travels up on e0's upload stream and frame i - 1 down on the last engine's download stream while
        // frame i runs through the stages; two frame buffers on e0, two output buffers on the last engine, one frame between each pair of stages
        uint8_t* const frames[2] = {e0.d_frame, e0.d_frame2};
        uint8_t* const outs[2] = {eL.d_out, eL.d_out2};
        sync_all();
        hipAssert(hipEventRecord(e0.ev0, e0.stream));
        for (int i = 0; i < n; ++i) {
            const int b = i & 1;
            if (i >= 2) hipAssert(hipStreamWaitEvent(e0.s_up, e0.ev_comp[b], 0));                 // frame i - 2 has been gathered out of this buffer
            up(i, frames[b], e0.s_up);
            hipAssert(hipEventRecord(e0.ev_up[b], e0.s_up));
            hipAssert(hipStreamWaitEvent(e0.stream, e0.ev_up[b], 0));
            run_stages(frames[b], outs[b], i, e0.ev_comp[b], i >= 2 ? eL.ev_dn[b] : nullptr);
            hipAssert(hipStreamWaitEvent(eL.s_dn, impl->ev_chain_done[last], 0));
            down(i, outs[b], eL.s_dn);
            hipAssert(hipEventRecord(eL.ev_dn[b], eL.s_dn));
        }
        hipAssert(hipEventRecord(eL.ev1, eL.stream));
        hipAssert(hipStreamSynchronize(eL.s_dn));
        sync_all();
        hipAssert(hipStreamSynchronize(e0.s_up));
        float total_ms = 0.f;
        hipAssert(hipEventElapsedTime(&total_ms, e0.ev0, eL.ev1));
        impl->last_ms = total_ms / n;
        return true;
    } catch (const std::exception& ex) {
        for (int k = 0; k < count; ++k) { try { DeviceGuard guard(st[k].e->device); st[k].e->drain_after_error(); } catch (...) {} }
        W2X_LOG_AS(who, error, kRenderFailed + std::string(ex.what()) + ".");
        return false;
    }
}

// Planar RGBA frames: renderRgba()'s frame on renderPlanar()'s samples.  Four 2-D copies up, alpha_bleed_planes_kernel (three colour planes with the
// visible colours spread under alpha == 0, the alpha plane, the plane's range), ONE schedule of the frame's N colour tiles followed by its N alpha tiles through
// gather_planes_rgba_kernel, compose_planes_rgba_kernel - resized: compose_canvas_rgba_kernel and resample_planes_rgba_kernel -, four 2-D copies down.  A single
// part on the compute stream; progress and skipUniformAlpha as renderRgba() (the frame step is Impl::rgba_frame).
bool Img2Img::renderPlanarRgba(const PlanarRgbaImage& src, PlanarRgbaImage& dst, const RgbaOptions& opt) { return runPlanarRgba(&src, &dst, 1, opt, -1, "renderPlanarRgba", true); }

bool Img2Img::renderPlanarRgbaResized(const PlanarRgbaImage& src, PlanarRgbaImage& dst, const RgbaOptions& opt, ResizeFilter filter) {
    return runPlanarRgba(&src, &dst, 1, opt, filter_id(filter), "renderPlanarRgbaResized", true);
}

// Planar RGBA frames through renderSequence()'s pipeline (never rolling: the bleed's planes are single buffers): output i is the bytes of the single call
bool Img2Img::renderSequencePlanarRgba(const PlanarRgbaImage* srcs, PlanarRgbaImage* dsts, int count, const RgbaOptions& opt) {
    return runPlanarRgba(srcs, dsts, count, opt, -1, "renderSequencePlanarRgba", false);
}

bool Img2Img::renderSequencePlanarRgbaResized(const PlanarRgbaImage* srcs, PlanarRgbaImage* dsts, int count, const RgbaOptions& opt, ResizeFilter filter) {
    return runPlanarRgba(srcs, dsts, count, opt, filter_id(filter), "renderSequencePlanarRgbaResized", false);
}

bool Img2Img::runPlanarRgba(const PlanarRgbaImage* srcs, PlanarRgbaImage* dsts, int count, const RgbaOptions& opt, int resizeFilter, const char* who, bool single) {
    return impl->entry(who, kNotLoaded, kRenderFailed, [&] {   // (the call's own work, to the closing `});` - deliberately left at function indentation)
    if (count <= 0) return true;
    if (!srcs || !dsts) { W2X_LOG_AS(who, error, "No frames given."); return false; }
    Impl::FrameCall call;
    if (const std::string why = impl->planar_rgba_check(srcs, dsts, count, opt, resizeFilter, call); !why.empty()) { W2X_LOG_AS(who, error, why); return false; }
    impl->job.kind = Impl::Job::PLANAR_RGBA; impl->job.planar.in_bits = srcs[0].bits; impl->job.planar.out_bits = dsts[0].bits;
    impl->job.rgba = Impl::RgbaJob{opt.bleed, opt.skipUniformAlpha};
    // the four planes of a frame between the caller's pointers and the device layout (rgba_planes), on stream `on`
    auto copy_planes = [&](const PlanarRgbaImage& host, uint8_t* dev, int r, int c, bool up, hipStream_t on) {
        const RgbaPlanes d = impl->rgba_planes(dev, r, c, !up);
        const size_t width = (size_t)c * planar_sample_bytes(host.bits);
        for (int k = 0; k < 4; ++k) {
            if (up) hipAssert(hipMemcpy2DAsync(d.p[k], d.step[k], host.planes[k], host.steps[k], width, r, hipMemcpyHostToDevice, on));
            else hipAssert(hipMemcpy2DAsync(host.planes[k], host.steps[k], d.p[k], d.step[k], width, r, hipMemcpyDeviceToHost, on));
        }
    };
    impl->run_call(call, count, single, resizeFilter,
        [&](int i, uint8_t* dev, hipStream_t on) { copy_planes(srcs[i], dev, call.rows, call.cols, true, on); },
        [&](int i, uint8_t* dev, hipStream_t on) { copy_planes(dsts[i], dev, call.out_rows, call.out_cols, false, on); });
    return true;
    });
}

bool Img2Img::alphaBleedPlanes(const PlanarRgbaImage& src, PlanarImage& colour, int radius, unsigned* words) {
    const char* who = "alphaBleedPlanes";
    return impl->entry(who, "Alpha bleed called before a successful load.", "Alpha bleed failed unexpectedly: ",
                       [&] {   // (the call's own work, to the closing `});` - deliberately left at function indentation)
    const int rows = src.rows, cols = src.cols, bits = src.bits;
    if (!planar_bits_ok(bits) || colour.bits != bits) { W2X_LOG_AS(who, error, "Planar frames must have 8, 10, 12, 16 or 32 (float) bits, the same on both sides."); return false; }
    if (rows <= 0 || cols <= 0) { W2X_LOG_AS(who, error, "Input image is empty."); return false; }
    if (!Impl::rgba_planes_ok(src)) { W2X_LOG_AS(who, error, "Input image has a missing plane or an invalid step."); return false; }
    if (colour.rows != rows || colour.cols != cols) { W2X_LOG_AS(who, error, "Output image has invalid size: expected " + std::to_string(cols) + "x" + std::to_string(rows) + "."); return false; }
    const size_t bps = planar_sample_bytes(bits), width = (size_t)cols * bps;
    for (int k = 0; k < 3; ++k)
        if (!colour.planes[k] || colour.steps[k] < width || ((((size_t)colour.planes[k]) | colour.steps[k]) & (bps - 1)) != 0) { W2X_LOG_AS(who, error, "Output image has a missing plane or an invalid step."); return false; }
    if (const std::string why = Impl::bleed_problem(radius, bits); !why.empty()) { W2X_LOG_AS(who, error, why); return false; }
    impl->last_rows = impl->last_cols = 0;   // (d_frame is overwritten: the last render() frame is no longer there to replay)
    impl->job.kind = Impl::Job::PLANAR_RGBA; impl->job.planar.in_bits = impl->job.planar.out_bits = bits;
    impl->ensure(impl->d_frame, impl->frame_cap, impl->frame_bytes(rows, cols, false));
    impl->ensure_bleed_planes(rows, cols);
    const RgbaPlanes d = impl->rgba_planes(impl->d_frame, rows, cols, false);
    for (int k = 0; k < 4; ++k) hipAssert(hipMemcpy2DAsync(d.p[k], d.step[k], src.planes[k], src.steps[k], width, rows, hipMemcpyHostToDevice, impl->stream));
    impl->bleed_frame(rows, cols, radius);
    for (int k = 0; k < 3; ++k)
        hipAssert(hipMemcpy2DAsync(colour.planes[k], colour.steps[k], impl->d_bgr + (size_t)k * d.step[0] * rows, d.step[0], width, rows, hipMemcpyDeviceToHost, impl->stream));
    if (words) hipAssert(hipMemcpyAsync(words, impl->d_minmax, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, impl->stream));
    hipAssert(hipStreamSynchronize(impl->stream));
    return true;
    });
}

bool Img2Img::setDither(const DitherOptions& options) {
    if (!dither_mode_ok((int)options.mode)) { W2X_LOG(error, "Unknown dither mode " + std::to_string((int)options.mode) + ": expected none, ordered or bluenoise."); return false; }
    impl->dither = options;
    return true;
}
DitherOptions Img2Img::dither() const { return impl->dither; }

bool Img2Img::ditherPlanes(const PlanarImage& src, PlanarImage& dst) {
    const char* who = "ditherPlanes";
    return impl->entry(who, "Dither planes called before a successful load.", "Dither planes failed unexpectedly: ",
                       [&] {   // (the call's own work, to the closing `});` - deliberately left at function indentation)
    const int rows = src.rows, cols = src.cols, bits = dst.bits;
    if (src.bits != 32 || (bits != 8 && bits != 10 && bits != 12 && bits != 16)) { W2X_LOG_AS(who, error, "Dither planes take float (32-bit) planes and give planes of 8, 10, 12 or 16 bits."); return false; }
    if (rows <= 0 || cols <= 0) { W2X_LOG_AS(who, error, "Input image is empty."); return false; }
    if (dst.rows != rows || dst.cols != cols) { W2X_LOG_AS(who, error, "Output image has invalid size: expected " + std::to_string(cols) + "x" + std::to_string(rows) + "."); return false; }
    const size_t bps = planar_sample_bytes(bits), in_width = (size_t)cols * 4, out_width = (size_t)cols * bps;
    for (int k = 0; k < 3; ++k) {
        if (!src.planes[k] || src.steps[k] < in_width || ((((size_t)src.planes[k]) | src.steps[k]) & 3) != 0) { W2X_LOG_AS(who, error, "Input image has a missing plane or an invalid step."); return false; }
        if (!dst.planes[k] || dst.steps[k] < out_width || ((((size_t)dst.planes[k]) | dst.steps[k]) & (bps - 1)) != 0) { W2X_LOG_AS(who, error, "Output image has a missing plane or an invalid step."); return false; }
    }
    impl->last_rows = impl->last_cols = 0;   // (d_frame and d_out are overwritten: the last render() frame is no longer there to replay)
    const size_t in_step = Impl::planar_step(cols, 32), out_step = Impl::planar_step(cols, bits);
    impl->ensure(impl->d_frame, impl->frame_cap, 3 * in_step * rows);
    impl->ensure(impl->d_out, impl->out_cap, 3 * out_step * rows);
    PlanarPlanes a, b;
    a.rows = b.rows = rows; a.cols = b.cols = cols; a.n = b.n = 3; a.bits = 32; b.bits = bits;
    for (int k = 0; k < 3; ++k) {
        a.p[k] = impl->d_frame + (size_t)k * in_step * rows; a.step[k] = in_step;
        b.p[k] = impl->d_out + (size_t)k * out_step * rows; b.step[k] = out_step;
        hipAssert(hipMemcpy2DAsync(a.p[k], in_step, src.planes[k], src.steps[k], in_width, rows, hipMemcpyHostToDevice, impl->stream));
    }
    hipAssert(launch_dither_planes(a, b, impl->dither_now(), impl->stream));
    for (int k = 0; k < 3; ++k) hipAssert(hipMemcpy2DAsync(dst.planes[k], dst.steps[k], b.p[k], out_step, out_width, rows, hipMemcpyDeviceToHost, impl->stream));
    hipAssert(hipStreamSynchronize(impl->stream));
    return true;
    });
}

bool Img2Img::setEdge(EdgeMode mode) {
    if (!edge_mode_ok((int)mode)) { W2X_LOG(error, "Unknown edge mode " + std::to_string((int)mode) + ": expected replicate, wrap or mirror."); return false; }
    impl->edge = (int)mode;
    return true;
}
EdgeMode Img2Img::edge() const { return (EdgeMode)impl->edge; }

bool Img2Img::setResizeLight(ResizeLight mode) {
    if (!light_mode_ok((int)mode)) { W2X_LOG(error, "Unknown resize light " + std::to_string((int)mode) + ": expected gamma, srgb or bt709."); return false; }
    impl->light = mode;
    return true;
}
ResizeLight Img2Img::resizeLight() const { return impl->light; }

bool Img2Img::resizePlanes(const PlanarImage& src, PlanarImage& dst, ResizeFilter filter) {
    const char* who = "resizePlanes";
    return impl->entry(who, "Resize planes called before a successful load.", "Resize planes failed unexpectedly: ",
                       [&] {   // (the call's own work, to the closing `});` - deliberately left at function indentation)
    const int rows = src.rows, cols = src.cols, out_rows = dst.rows, out_cols = dst.cols, bits = dst.bits;
    if (src.bits != 32 || !planar_bits_ok(bits)) { W2X_LOG_AS(who, error, "Resize planes take float (32-bit) planes and give planes of 8, 10, 12, 16 or 32 bits."); return false; }
    if (rows <= 0 || cols <= 0) { W2X_LOG_AS(who, error, "Input image is empty."); return false; }
    if (filter != ResizeFilter::Bicubic && filter != ResizeFilter::Bilinear) { W2X_LOG_AS(who, error, "Unknown resize filter."); return false; }
    // a downscale by 1 to 4 per axis, the range the resize kernels' LDS is sized for (kResampleRows rows of a tile reach at most 4 x as many input rows plus the taps)
    if (out_rows <= 0 || out_cols <= 0 || out_rows > rows || out_cols > cols || (long)out_rows * 4 < rows || (long)out_cols * 4 < cols) {
        W2X_LOG_AS(who, error, "Output image has invalid size for a resize: " + std::to_string(out_cols) + "x" + std::to_string(out_rows) + " is not between a quarter of " +
                   std::to_string(cols) + "x" + std::to_string(rows) + " and it."); return false;
    }
    const size_t bps = planar_sample_bytes(bits), in_width = (size_t)cols * 4, out_width = (size_t)out_cols * bps;
    for (int k = 0; k < 3; ++k) {
        if (!src.planes[k] || src.steps[k] < in_width || ((((size_t)src.planes[k]) | src.steps[k]) & 3) != 0) { W2X_LOG_AS(who, error, "Input image has a missing plane or an invalid step."); return false; }
        if (!dst.planes[k] || dst.steps[k] < out_width || ((((size_t)dst.planes[k]) | dst.steps[k]) & (bps - 1)) != 0) { W2X_LOG_AS(who, error, "Output image has a missing plane or an invalid step."); return false; }
    }
    impl->last_rows = impl->last_cols = 0;   // (d_out is overwritten: the last render() frame is no longer there to replay)
    const Impl::ResizeTables* const rs = impl->resize_tables(cols, rows, out_cols, out_rows, (int)filter);
    const size_t plane = (size_t)rows * cols, out_step = Impl::planar_step(out_cols, bits);
    impl->ensure_canvas(3 * plane * sizeof(float));
    impl->ensure(impl->d_out, impl->out_cap, 3 * out_step * out_rows);
    for (int k = 0; k < 3; ++k)
        hipAssert(hipMemcpy2DAsync(impl->d_canvas + (size_t)k * plane, in_width, src.planes[k], src.steps[k], in_width, rows, hipMemcpyHostToDevice, impl->stream));
    const LightArgs light = impl->light_now();
    hipAssert(launch_light_decode_planes(impl->d_canvas, 3 * plane, light, impl->stream));
    ResamplePlanarParams p;
    p.canvas = impl->d_canvas; p.inW = cols; p.inH = rows; p.outW = out_cols; p.outH = out_rows;
    p.fx = rs->fx; p.wx = rs->wx; p.kx = rs->kx; p.fy = rs->fy; p.wy = rs->wy; p.ky = rs->ky; p.rows_max = rs->rows_max;
    p.dst.rows = out_rows; p.dst.cols = out_cols; p.dst.n = 3; p.dst.bits = bits;
    for (int k = 0; k < 3; ++k) { p.dst.p[k] = impl->d_out + (size_t)k * out_step * out_rows; p.dst.step[k] = out_step; }
    EdgeArgs edge; edge.mode = rs->edge;
    hipAssert(launch_resample_planar(p, impl->stream, impl->dither_now(), light, edge));
    for (int k = 0; k < 3; ++k) hipAssert(hipMemcpy2DAsync(dst.planes[k], dst.steps[k], p.dst.p[k], out_step, out_width, out_rows, hipMemcpyDeviceToHost, impl->stream));
    hipAssert(hipStreamSynchronize(impl->stream));
    return true;
    });
}

bool Img2Img::alphaBleed(const Image& bgra, Image& bgr, int radius) {
    const char* who = "alphaBleed";
    return impl->entry(who, "Alpha bleed called before a successful load.", "Alpha bleed failed unexpectedly: ",
                       [&] {   // (the call's own work, to the closing `});` - deliberately left at function indentation)
    const int rows = bgra.rows, cols = bgra.cols;
    if (bgra.depth != 8 || bgr.depth != 8) { W2X_LOG_AS(who, error, "RGBA input and output images must be 8-bit."); return false; }
    if (!bgra.data || rows <= 0 || cols <= 0 || bgra.step < (size_t)cols * 4) { W2X_LOG_AS(who, error, "Input image is empty or has an invalid step."); return false; }
    if (!bgr.data || bgr.rows != rows || bgr.cols != cols || bgr.step < (size_t)cols * 3) { W2X_LOG_AS(who, error, "Output image has invalid size: expected " + std::to_string(cols) + "x" + std::to_string(rows) + "."); return false; }
    if (radius < 0 || radius > kBleedMaxRadius) { W2X_LOG_AS(who, error, "Alpha bleed radius " + std::to_string(radius) + " is not in [0, " + std::to_string(kBleedMaxRadius) + "]."); return false; }
    impl->last_rows = impl->last_cols = 0;   // (d_frame is overwritten: the last render() frame is no longer there to replay)
    impl->upload_and_bleed(bgra, radius);
    hipAssert(hipMemcpy2DAsync(bgr.data, bgr.step, impl->d_bgr, (size_t)cols * 3, (size_t)cols * 3, rows, hipMemcpyDeviceToHost, impl->stream));
    hipAssert(hipStreamSynchronize(impl->stream));
    return true;
    });
}

// Page-locked frame buffers for renderSequence(): owned by the engine, freed by freeHost() or with the engine.
void* Img2Img::allocHost(size_t bytes) try {
    if (!bytes) return nullptr;
    std::unique_ptr<DeviceGuard> guard;
    if (impl->device >= 0) guard.reset(new DeviceGuard(impl->device));
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    impl->host_allocs.push_back(p);
    return p;
} catch (const std::exception&) {
    return nullptr;
}
void Img2Img::freeHost(void* data) try {
    auto it = std::find(impl->host_allocs.begin(), impl->host_allocs.end(), data);
    if (it == impl->host_allocs.end()) return;
    std::unique_ptr<DeviceGuard> guard;
    if (impl->device >= 0) guard.reset(new DeviceGuard(impl->device));
    if (hipHostFree(data) != hipSuccess) (void)hipGetLastError();
    impl->host_allocs.erase(it);
} catch (const std::exception&) {
}

// Page-lock a caller-owned frame buffer in place so that renderSequence() can copy it by DMA while kernels run (whole pages only).
bool Img2Img::pinHost(void* data, size_t bytes) try {
    if (!data || !bytes) return false;
    if (((size_t)data | bytes) & 4095) { W2X_LOG(warn, "pinHost: only whole pages can be page-locked in place (use allocHost)."); return false; }
    DeviceGuard guard(impl->device);
    if (hipHostRegister(data, bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return false; }
    impl->pinned.push_back(data);
    return true;
} catch (const std::exception&) {
    return false;
}
void Img2Img::unpinHost(void* data) try {
    DeviceGuard guard(impl->device);
    auto it = std::find(impl->pinned.begin(), impl->pinned.end(), data);
    if (it == impl->pinned.end()) return;
    if (hipHostUnregister(data) != hipSuccess) (void)hipGetLastError();
    impl->pinned.erase(it);
} catch (const std::exception&) {
}

bool Img2Img::infer(const float* input, float* output) try {
    if (!impl->loaded) { W2X_LOG(error, "Infer called before a successful load."); return false; }
    DeviceGuard guard(impl->device);
    const Plan& plan = impl->plan;
    const size_t in_elems = (size_t)plan.B * 3 * plan.T * plan.T, out_elems = (size_t)plan.B * 3 * plan.Tout * plan.Tout;
    const size_t user_in = (size_t)plan.userB * 3 * plan.T * plan.T, user_out = (size_t)plan.userB * 3 * plan.Tout * plan.Tout;
    hipStream_t stream = impl->stream;
    if (!impl->d_blob_in) {
        hipAssert(hipMalloc((void**)&impl->d_blob_in, in_elems * sizeof(float)));      // img2img_load.cpp:228-232: f32 IO buffers
        hipAssert(hipMalloc((void**)&impl->d_blob_out, out_elems * sizeof(float)));
        hipAssert(hipMemsetAsync(impl->d_blob_in, 0, in_elems * sizeof(float), stream));   // slots beyond the caller's batch stay zero
    }
    hipAssert(hipMemcpyAsync(impl->d_blob_in, input, user_in * sizeof(float), hipMemcpyHostToDevice, stream));
    hipAssert(launch_blob_to_nhwc(impl->d_blob_in, impl->tensors[plan.in_tensor], plan.B, plan.T, plan.elt == 4, stream));
    impl->run_network(nullptr, plan.userB);                                            // img2img_infer.cpp:80 (the slots beyond the caller's batch are not computed)
    hipAssert(launch_nhwc_to_blob(impl->tensors[plan.out_tensor], impl->d_blob_out, plan.B, plan.Tout, plan.elt == 4, stream));
    hipAssert(hipMemcpyAsync(output, impl->d_blob_out, user_out * sizeof(float), hipMemcpyDeviceToHost, stream));
    hipAssert(hipStreamSynchronize(stream));
    return true;
} catch (const std::exception& e) {
    W2X_LOG(error, "Engine inference failed unexpectedly: " + std::string(e.what()) + ".");
    return false;
}

int Img2Img::outputTileSize() const { return impl->loaded ? impl->plan.Tout : 0; }
int Img2Img::opTimes(double* out, int cap) const { int n = (int)impl->op_ms.size(); for (int i = 0; i < n && i < cap; ++i) out[i] = impl->op_ms[i]; return n; }
int Img2Img::scaling() const { return impl->loaded ? impl->cfg.scaling : 0; }
int Img2Img::passTiles() const { return impl->loaded ? impl->plan.B : 0; }
double Img2Img::planFlops() const { return impl->loaded ? impl->plan.flops : 0.0; }
float Img2Img::lastRenderMs() const { return impl->last_ms; }

float Img2Img::benchResident(int iters) try {
    if (!impl->loaded || impl->last_rows == 0 || iters <= 0) return -1.f;
    DeviceGuard guard(impl->device);
    hipStream_t stream = impl->stream;
    impl->one_part_slots();
    // frames of one size back to back: a rolling sequence where every pass splits (run_rolling_frame), else frame after frame
    const bool roll = iters > 1 && impl->can_roll(impl->last_strip.tile_count);
    if (roll) impl->ensure(impl->d_slab2, impl->slab2_cap, impl->slab_cap);
    hipAssert(hipEventRecord(impl->ev0, stream));
    for (int i = 0; i < iters; ++i) {
        if (roll) impl->run_rolling_frame(impl->last_rows, impl->last_cols, impl->last_grid, impl->last_strip, i & 1, nullptr);
        else impl->run_frame(impl->last_rows, impl->last_cols, impl->last_grid, false, impl->last_strip);
    }
    if (roll) impl->end_rolling();
    hipAssert(hipEventRecord(impl->ev1, stream));
    hipAssert(hipStreamSynchronize(stream));
    float ms = 0.f;
    hipAssert(hipEventElapsedTime(&ms, impl->ev0, impl->ev1));
    return ms / iters;
} catch (const std::exception& e) {
    W2X_LOG(error, "Bench failed unexpectedly: " + std::string(e.what()) + ".");
    return -1.f;
}

// The output frame the last benchResident() step (or render()) left in device memory: rows * s x cols * s x 3 samples, packed; `bytes` must be that size.
bool Img2Img::residentOutput(void* dst, size_t bytes) try {
    if (!impl->loaded || impl->last_rows == 0 || !dst) return false;
    const size_t s = (size_t)impl->cfg.scaling, bps = impl->deep ? 2 : 1;
    if (bytes != (size_t)impl->last_rows * s * impl->last_cols * s * 3 * bps) return false;
    DeviceGuard guard(impl->device);
    hipAssert(hipMemcpyAsync(dst, impl->d_out, bytes, hipMemcpyDeviceToHost, impl->stream));
    hipAssert(hipStreamSynchronize(impl->stream));
    return true;
} catch (const std::exception& e) {
    W2X_LOG(error, "Reading the resident output failed unexpectedly: " + std::string(e.what()) + ".");
    return false;
}

// Per-kernel-family device time of one resident frame, measured with HIP events on the compute stream.
// out[5*k + {0,1,2}] = {milliseconds, launches, algorithmic FLOP} for k = 0 gemm, 1 attention, 2 se/scale, 3 gather,
// 4 compose, 5 fused mlp; out[30] = wall ms of the whole frame (first launch start to last launch end).
bool Img2Img::profileFrame(double* out, int cap) try {
    if (!impl->loaded || impl->last_rows == 0 || cap < 31) return false;
    DeviceGuard guard(impl->device);
    for (int i = 0; i < 31; ++i) out[i] = 0;
    impl->one_part_slots();
    impl->profiling = true; impl->stamps.clear();
    impl->run_frame(impl->last_rows, impl->last_cols, impl->last_grid, false, impl->last_strip);
    impl->profiling = false;
    hipAssert(hipStreamSynchronize(impl->stream));
    impl->op_ms.assign(impl->plan.ops.size(), 0.0);
    for (auto& st : impl->stamps) {
        float ms = 0.f;
        hipAssert(hipEventElapsedTime(&ms, st.a, st.b));
        if (st.op >= 0) impl->op_ms[st.op] += ms;
        out[5 * st.kind] += ms; out[5 * st.kind + 1] += 1; out[5 * st.kind + 2] += st.flops;
    }
    if (!impl->stamps.empty()) { float ms = 0.f; hipAssert(hipEventElapsedTime(&ms, impl->stamps.front().a, impl->stamps.back().b)); out[30] = ms; }
    for (auto& st : impl->stamps) { (void)hipEventDestroy(st.a); (void)hipEventDestroy(st.b); }
    impl->stamps.clear();
    return true;
} catch (const std::exception& e) {
    impl->profiling = false;
    W2X_LOG(error, "Profile failed unexpectedly: " + std::string(e.what()) + ".");
    return false;
}

}  // namespace w2x
