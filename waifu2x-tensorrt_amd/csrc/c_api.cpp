// Flat C ABI over w2x::Img2Img (declared in include/w2x/c_api.h, which cites the reference interfaces).
#include "../../include/w2x/c_api.h"
#include "../../include/w2x/c_api_chain.h"
#include "../../include/w2x/c_api_dither.h"
#include "../../include/w2x/c_api_edge.h"
#include "../../include/w2x/c_api_gray.h"
#include "../../include/w2x/c_api_planar.h"
#include "../../include/w2x/c_api_resize_light.h"
#include "../../include/w2x/c_api_rgbap.h"
#include "../../include/w2x/c_api_yuv_resized.h"
#include "../../include/w2x/c_api_yuv_siting.h"
#include <mutex>

#include <cstring>
#include <fstream>
#include <vector>
#include <string>

#include "../../include/w2x/img2img.h"
#include "liveness.h"
#include "lower.h"
#include "sha256.h"
#include "tiles.h"
#include "kernels.h"

struct w2x_engine {
    w2x::Img2Img engine;
    w2x_message_fn msg = nullptr; void* msg_user = nullptr;
    w2x_progress_fn prog = nullptr; void* prog_user = nullptr;
};

extern "C" {

w2x_engine* w2x_create(void) { try { return new w2x_engine; } catch (...) { return nullptr; } }
void w2x_destroy(w2x_engine* e) { delete e; }

void w2x_set_message_callback(w2x_engine* e, w2x_message_fn fn, void* user) {
    if (!e) return;
    e->msg = fn; e->msg_user = user;
    if (fn) e->engine.setMessageCallback([e](w2x::Severity s, const std::string& m) { if (e->msg) e->msg((int)s, m.c_str(), e->msg_user); });
    else e->engine.setMessageCallback(nullptr);
}
void w2x_set_progress_callback(w2x_engine* e, w2x_progress_fn fn, void* user) {
    if (!e) return;
    e->prog = fn; e->prog_user = user;
    if (fn) e->engine.setProgressCallback([e](int c, int t, double s) { if (e->prog) e->prog(c, t, s, e->prog_user); });
    else e->engine.setProgressCallback(nullptr);
}

// ---- the frame arguments of every render entry, built in one place
// an interleaved BGR / BGRA frame of the ABI (steps in bytes)
static w2x::Image image(const void* data, int rows, int cols, size_t step, int depth = 8) {
    w2x::Image m; m.data = static_cast<uint8_t*>(const_cast<void*>(data)); m.rows = rows; m.cols = cols; m.step = step; m.depth = depth;
    return m;
}
// the destination the caller pre-sized to size * scale (main.cpp:234-235); the scale is the engine's
static w2x::Image scaled_image(w2x::Img2Img& engine, void* data, int rows, int cols, size_t step, int depth = 8) {
    const int sc = engine.scaling();
    return image(data, rows * sc, cols * sc, step, depth);
}
struct ImageSequence { std::vector<w2x::Image> src, dst; };
// the frames of an Image sequence entry: srcs[i] / dsts[i] with the size, step and depth of the two model frames
static ImageSequence image_sequence(const uint8_t* const* srcs, const w2x::Image& src, uint8_t* const* dsts, const w2x::Image& dst, int count) {
    ImageSequence q; q.src.assign(count, src); q.dst.assign(count, dst);
    for (int i = 0; i < count; ++i) { q.src[i].data = const_cast<uint8_t*>(srcs[i]); q.dst[i].data = dsts[i]; }
    return q;
}
static bool sequence_ok(const w2x_engine* e, int count, const void* srcs, const void* dsts) { return e && count >= 0 && (count == 0 || (srcs && dsts)); }
static w2x::RgbaOptions rgba_options(int bleed, int skip_uniform_alpha) { w2x::RgbaOptions o; o.bleed = bleed; o.skipUniformAlpha = skip_uniform_alpha != 0; return o; }
static w2x::Precision precision_of(int p) { return p == W2X_PRECISION_FP16 ? w2x::Precision::FP16 : p == W2X_PRECISION_FP32 ? w2x::Precision::FP32 : w2x::Precision::TF32; }
// s into the caller's buffer of cap bytes, cut to fit, always terminated
static void copy_out(const std::string& s, char* buf, size_t cap) {
    if (!buf || !cap) return;
    const size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
    memcpy(buf, s.data(), n); buf[n] = 0;
}
// the resized renders: the target size is explicit; an unknown filter is refused here, through the engine's message callback
static bool resize_filter(w2x_engine* e, int filter, const char* who, w2x::ResizeFilter& f) {
    if (filter == W2X_RESIZE_BICUBIC || filter == W2X_RESIZE_BILINEAR) { f = filter == W2X_RESIZE_BILINEAR ? w2x::ResizeFilter::Bilinear : w2x::ResizeFilter::Bicubic; return true; }
    if (e->msg) e->msg((int)w2x::Severity::error, (std::string("[") + who + "@0] Unknown resize filter " + std::to_string(filter) + ".").c_str(), e->msg_user);
    return false;
}
// the YUV renders: matrix and range go to the engine as given (it refuses unknown values through the message callback)
static w2x::YuvImage yuv_image(const void* const* planes, const size_t* steps, int rows, int cols, int bits, int layout, int siting = W2X_YUV_SITING_LEFT) {
    w2x::YuvImage f;
    for (int k = 0; k < 3; ++k) { f.planes[k] = planes ? (uint8_t*)const_cast<void*>(planes[k]) : nullptr; f.steps[k] = steps ? steps[k] : 0; }
    f.rows = rows; f.cols = cols; f.bits = bits; f.layout = (w2x::YuvLayout)layout;   // (the engine refuses unknown layouts like unknown matrices)
    f.siting = (w2x::YuvSiting)siting;
    return f;
}
static w2x::YuvFormat yuv_format(int matrix, int range) { w2x::YuvFormat f; f.matrix = (w2x::YuvMatrix)matrix; f.range = (w2x::YuvRange)range; return f; }
// the planar RGB renders (include/w2x/c_api_planar.h): three planes R, G, B with their steps; the engine refuses unknown depths
static w2x::PlanarImage planar_image(const void* const* planes, const size_t* steps, int rows, int cols, int bits) {
    w2x::PlanarImage f;
    for (int k = 0; k < 3; ++k) { f.planes[k] = planes ? (uint8_t*)const_cast<void*>(planes[k]) : nullptr; f.steps[k] = steps ? steps[k] : 0; }
    f.rows = rows; f.cols = cols; f.bits = bits;
    return f;
}
struct PlanarSequence { std::vector<w2x::PlanarImage> src, dst; };
// the frames of a planar sequence entry: frame i's planes at [3i .. 3i + 2], one set of steps for the sequence
static PlanarSequence planar_sequence(const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                                      void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int count) {
    PlanarSequence q; q.src.reserve(count); q.dst.reserve(count);
    for (int i = 0; i < count; ++i) {
        q.src.push_back(planar_image(src_planes + 3 * i, src_steps, rows, cols, src_bits));
        q.dst.push_back(planar_image(dst_planes + 3 * i, dst_steps, dst_rows, dst_cols, dst_bits));
    }
    return q;
}
// the planar RGBA renders (include/w2x/c_api_rgbap.h): four planes R, G, B, A; a sequence holds frame i's planes at [4i .. 4i + 3]
static w2x::PlanarRgbaImage rgbap_image(const void* const* planes, const size_t* steps, int rows, int cols, int bits) {
    w2x::PlanarRgbaImage f;
    for (int k = 0; k < 4; ++k) { f.planes[k] = planes ? (uint8_t*)const_cast<void*>(planes[k]) : nullptr; f.steps[k] = steps ? steps[k] : 0; }
    f.rows = rows; f.cols = cols; f.bits = bits;
    return f;
}
struct RgbapSequence { std::vector<w2x::PlanarRgbaImage> src, dst; };
static RgbapSequence rgbap_sequence(const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                                    void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int count) {
    RgbapSequence q; q.src.reserve(count); q.dst.reserve(count);
    for (int i = 0; i < count; ++i) {
        q.src.push_back(rgbap_image(src_planes + 4 * i, src_steps, rows, cols, src_bits));
        q.dst.push_back(rgbap_image(dst_planes + 4 * i, dst_steps, dst_rows, dst_cols, dst_bits));
    }
    return q;
}
struct YuvSequence { std::vector<w2x::YuvImage> src, dst; };
// the frames of a YUV sequence entry: frame i's planes at [3i .. 3i + 2], one set of steps for the sequence
static YuvSequence yuv_sequence(const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits, int src_layout,
                                void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int dst_layout, int count,
                                int src_siting = W2X_YUV_SITING_LEFT, int dst_siting = W2X_YUV_SITING_LEFT) {
    YuvSequence q; q.src.reserve(count); q.dst.reserve(count);
    for (int i = 0; i < count; ++i) {
        q.src.push_back(yuv_image(src_planes + 3 * i, src_steps, rows, cols, src_bits, src_layout, src_siting));
        q.dst.push_back(yuv_image(dst_planes + 3 * i, dst_steps, dst_rows, dst_cols, dst_bits, dst_layout, dst_siting));
    }
    return q;
}

int w2x_build(w2x_engine* e, const char* onnx_path, const w2x_build_config* c) {
    if (!e || !onnx_path || !c) return 0;
    w2x::BuildConfig b;
    b.deviceId = c->deviceId; b.precision = precision_of(c->precision);
    b.minBatchSize = c->minBatchSize; b.optBatchSize = c->optBatchSize; b.maxBatchSize = c->maxBatchSize;
    b.minChannels = c->minChannels; b.optChannels = c->optChannels; b.maxChannels = c->maxChannels;
    b.minWidth = c->minWidth; b.optWidth = c->optWidth; b.maxWidth = c->maxWidth;
    b.minHeight = c->minHeight; b.optHeight = c->optHeight; b.maxHeight = c->maxHeight;
    return e->engine.build(onnx_path, b) ? 1 : 0;
}

int w2x_load(w2x_engine* e, const char* onnx_path, const w2x_render_config* c) {
    if (!e || !onnx_path || !c) return 0;
    w2x::RenderConfig r;
    r.deviceId = c->deviceId; r.precision = precision_of(c->precision);
    r.batchSize = c->batchSize; r.channels = c->channels; r.height = c->height; r.width = c->width; r.scaling = c->scaling;
    r.overlapX = c->overlapX; r.overlapY = c->overlapY; r.tta = c->tta != 0; r.ttaBugCompat = c->ttaBugCompat != 0;
    return e->engine.load(onnx_path, r) ? 1 : 0;
}

int w2x_render(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, size_t dst_step) {
    if (!e) return 0;
    w2x::Image d = scaled_image(e->engine, dst, rows, cols, dst_step);
    return e->engine.render(image(src, rows, cols, src_step), d) ? 1 : 0;
}

int w2x_render16(w2x_engine* e, const uint16_t* src, int rows, int cols, size_t src_step, uint16_t* dst, size_t dst_step) {
    if (!e) return 0;
    w2x::Image d = scaled_image(e->engine, dst, rows, cols, dst_step, 16);
    return e->engine.render(image(src, rows, cols, src_step, 16), d) ? 1 : 0;
}

int w2x_render_resized(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, int dst_rows, int dst_cols, size_t dst_step, int filter) {
    w2x::ResizeFilter f;
    if (!e || !resize_filter(e, filter, "w2x_render_resized", f)) return 0;
    w2x::Image d = image(dst, dst_rows, dst_cols, dst_step);
    return e->engine.renderResized(image(src, rows, cols, src_step), d, f) ? 1 : 0;
}

int w2x_render16_resized(w2x_engine* e, const uint16_t* src, int rows, int cols, size_t src_step, uint16_t* dst, int dst_rows, int dst_cols, size_t dst_step, int filter) {
    w2x::ResizeFilter f;
    if (!e || !resize_filter(e, filter, "w2x_render16_resized", f)) return 0;
    w2x::Image d = image(dst, dst_rows, dst_cols, dst_step, 16);
    return e->engine.renderResized(image(src, rows, cols, src_step, 16), d, f) ? 1 : 0;
}

int w2x_render_strip(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, size_t dst_step, int part, int parts) {
    if (!e) return 0;
    w2x::Image d = scaled_image(e->engine, dst, rows, cols, dst_step);
    return e->engine.renderStrip(image(src, rows, cols, src_step), d, part, parts) ? 1 : 0;
}

int w2x_render_sharded(w2x_engine* const* engines, int count, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, size_t dst_step) {
    if (!engines || count <= 0) return 0;
    std::vector<w2x::Img2Img*> es(count);
    for (int k = 0; k < count; ++k) { if (!engines[k]) return 0; es[k] = &engines[k]->engine; }
    w2x::Image d = scaled_image(*es[0], dst, rows, cols, dst_step);
    return w2x::Img2Img::renderSharded(es.data(), count, image(src, rows, cols, src_step), d) ? 1 : 0;
}

int w2x_shard_compute(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, int part, int parts) {
    return e && e->engine.shardCompute(image(src, rows, cols, src_step), part, parts) ? 1 : 0;
}
const void* w2x_shard_slab(w2x_engine* e, size_t* bytes) { return e ? e->engine.shardSlab(bytes) : nullptr; }
int w2x_shard_finish(w2x_engine* e, uint8_t* dst, int rows, int cols, size_t dst_step, int part, int parts, const void* const* slabs, const int* devices) {
    if (!e) return 0;
    w2x::Image d = image(dst, rows, cols, dst_step);
    return e->engine.shardFinish(d, part, parts, slabs, devices) ? 1 : 0;
}
int w2x_ipc_export(const void* device_ptr, uint8_t* out64) { return out64 && w2x::ipc_export(device_ptr, out64) ? 1 : 0; }
void* w2x_ipc_open(const uint8_t* handle64, int device) { return handle64 ? w2x::ipc_open(handle64, device) : nullptr; }
void w2x_ipc_close(void* p) { w2x::ipc_close(p); }

int w2x_render_sequence(w2x_engine* e, const uint8_t* const* srcs, int rows, int cols, size_t src_step, uint8_t* const* dsts, size_t dst_step, int count) {
    if (!sequence_ok(e, count, srcs, dsts)) return 0;
    ImageSequence q = image_sequence(srcs, image(nullptr, rows, cols, src_step), dsts, scaled_image(e->engine, nullptr, rows, cols, dst_step), count);
    return e->engine.renderSequence(q.src.data(), q.dst.data(), count) ? 1 : 0;
}
int w2x_render_sequence_resized(w2x_engine* e, const uint8_t* const* srcs, int rows, int cols, size_t src_step, uint8_t* const* dsts, int dst_rows, int dst_cols, size_t dst_step,
                                int count, int filter) {
    w2x::ResizeFilter f;
    if (!sequence_ok(e, count, srcs, dsts) || !resize_filter(e, filter, "w2x_render_sequence_resized", f)) return 0;
    ImageSequence q = image_sequence(srcs, image(nullptr, rows, cols, src_step), dsts, image(nullptr, dst_rows, dst_cols, dst_step), count);
    return e->engine.renderSequenceResized(q.src.data(), q.dst.data(), count, f) ? 1 : 0;
}

int w2x_render_yuv(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                   void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int matrix, int range) {
    return w2x_render_yuv_layout(e, src_planes, src_steps, rows, cols, src_bits, W2X_YUV_I420, dst_planes, dst_steps, dst_rows, dst_cols, dst_bits, W2X_YUV_I420, matrix, range);
}
int w2x_render_sequence_yuv(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                            void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int count, int matrix, int range) {
    return w2x_render_sequence_yuv_layout(e, src_planes, src_steps, rows, cols, src_bits, W2X_YUV_I420, dst_planes, dst_steps, dst_rows, dst_cols, dst_bits, W2X_YUV_I420, count,
                                          matrix, range);
}
int w2x_render_yuv_layout(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits, int src_layout,
                          void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int dst_layout, int matrix, int range) {
    if (!e) return 0;
    w2x::YuvImage d = yuv_image(dst_planes, dst_steps, dst_rows, dst_cols, dst_bits, dst_layout);
    return e->engine.renderYuv(yuv_image(src_planes, src_steps, rows, cols, src_bits, src_layout), d, yuv_format(matrix, range)) ? 1 : 0;
}
int w2x_render_sequence_yuv_layout(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits, int src_layout,
                                   void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int dst_layout, int count, int matrix, int range) {
    if (!sequence_ok(e, count, src_planes, dst_planes)) return 0;
    YuvSequence q = yuv_sequence(src_planes, src_steps, rows, cols, src_bits, src_layout, dst_planes, dst_steps, dst_rows, dst_cols, dst_bits, dst_layout, count);
    return e->engine.renderSequenceYuv(q.src.data(), q.dst.data(), count, yuv_format(matrix, range)) ? 1 : 0;
}
int w2x_render_yuv_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                           void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int matrix, int range, int filter) {
    w2x::ResizeFilter f;
    if (!e || !resize_filter(e, filter, "w2x_render_yuv_resized", f)) return 0;
    w2x::YuvImage d = yuv_image(dst_planes, dst_steps, dst_rows, dst_cols, dst_bits, W2X_YUV_I420);
    return e->engine.renderYuvResized(yuv_image(src_planes, src_steps, rows, cols, src_bits, W2X_YUV_I420), d, yuv_format(matrix, range), f) ? 1 : 0;
}
int w2x_render_sequence_yuv_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                                    void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int count, int matrix, int range, int filter) {
    w2x::ResizeFilter f;
    if (!sequence_ok(e, count, src_planes, dst_planes) || !resize_filter(e, filter, "w2x_render_sequence_yuv_resized", f)) return 0;
    YuvSequence q = yuv_sequence(src_planes, src_steps, rows, cols, src_bits, W2X_YUV_I420, dst_planes, dst_steps, dst_rows, dst_cols, dst_bits, W2X_YUV_I420, count);
    return e->engine.renderSequenceYuvResized(q.src.data(), q.dst.data(), count, yuv_format(matrix, range), f) ? 1 : 0;
}
// resized YUV frames of any layout (include/w2x/c_api_yuv_resized.h).  An unknown layout is refused here like an unknown filter, in the engine's words: both can
// be told without a loaded engine
static bool yuv_layouts(w2x_engine* e, int src_layout, int dst_layout, const char* who) {
    const bool src_ok = src_layout >= W2X_YUV_I420 && src_layout <= W2X_YUV_NV12;
    if (src_ok && dst_layout >= W2X_YUV_I420 && dst_layout <= W2X_YUV_NV12) return true;
    if (e->msg) e->msg((int)w2x::Severity::error, (std::string("[") + who + "@0] Unknown YUV layout " + std::to_string(src_ok ? dst_layout : src_layout) + ".").c_str(), e->msg_user);
    return false;
}
int w2x_render_yuv_layout_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits, int src_layout,
                                  void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int dst_layout, int matrix, int range,
                                  int filter) {
    w2x::ResizeFilter f;
    if (!e || !resize_filter(e, filter, "w2x_render_yuv_layout_resized", f) || !yuv_layouts(e, src_layout, dst_layout, "w2x_render_yuv_layout_resized")) return 0;
    w2x::YuvImage d = yuv_image(dst_planes, dst_steps, dst_rows, dst_cols, dst_bits, dst_layout);
    return e->engine.renderYuvResized(yuv_image(src_planes, src_steps, rows, cols, src_bits, src_layout), d, yuv_format(matrix, range), f) ? 1 : 0;
}
int w2x_render_sequence_yuv_layout_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits, int src_layout,
                                           void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int dst_layout, int count,
                                           int matrix, int range, int filter) {
    w2x::ResizeFilter f;
    if (!sequence_ok(e, count, src_planes, dst_planes) || !resize_filter(e, filter, "w2x_render_sequence_yuv_layout_resized", f) ||
        !yuv_layouts(e, src_layout, dst_layout, "w2x_render_sequence_yuv_layout_resized")) return 0;
    YuvSequence q = yuv_sequence(src_planes, src_steps, rows, cols, src_bits, src_layout, dst_planes, dst_steps, dst_rows, dst_cols, dst_bits, dst_layout, count);
    return e->engine.renderSequenceYuvResized(q.src.data(), q.dst.data(), count, yuv_format(matrix, range), f) ? 1 : 0;
}
// YUV frames with a chroma siting per side (include/w2x/c_api_yuv_siting.h): the two entries above with the sitings, which go to the engine as given (it refuses
// unknown values through the message callback, like unknown matrices)
int w2x_render_yuv_sited(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits, int src_layout, int src_siting,
                         void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int dst_layout, int dst_siting, int matrix, int range,
                         int filter) {
    w2x::ResizeFilter f;
    if (!e || !resize_filter(e, filter, "w2x_render_yuv_sited", f) || !yuv_layouts(e, src_layout, dst_layout, "w2x_render_yuv_sited")) return 0;
    w2x::YuvImage d = yuv_image(dst_planes, dst_steps, dst_rows, dst_cols, dst_bits, dst_layout, dst_siting);
    return e->engine.renderYuvResized(yuv_image(src_planes, src_steps, rows, cols, src_bits, src_layout, src_siting), d, yuv_format(matrix, range), f) ? 1 : 0;
}
int w2x_render_sequence_yuv_sited(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits, int src_layout, int src_siting,
                                  void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int dst_layout, int dst_siting, int count,
                                  int matrix, int range, int filter) {
    w2x::ResizeFilter f;
    if (!sequence_ok(e, count, src_planes, dst_planes) || !resize_filter(e, filter, "w2x_render_sequence_yuv_sited", f) ||
        !yuv_layouts(e, src_layout, dst_layout, "w2x_render_sequence_yuv_sited")) return 0;
    YuvSequence q = yuv_sequence(src_planes, src_steps, rows, cols, src_bits, src_layout, dst_planes, dst_steps, dst_rows, dst_cols, dst_bits, dst_layout, count, src_siting, dst_siting);
    return e->engine.renderSequenceYuvResized(q.src.data(), q.dst.data(), count, yuv_format(matrix, range), f) ? 1 : 0;
}
int w2x_render_rgba(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, size_t dst_step, int bleed, int skip_uniform_alpha) {
    if (!e) return 0;
    w2x::Image d = scaled_image(e->engine, dst, rows, cols, dst_step);
    return e->engine.renderRgba(image(src, rows, cols, src_step), d, rgba_options(bleed, skip_uniform_alpha)) ? 1 : 0;
}
int w2x_render_rgba_resized(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, int dst_rows, int dst_cols, size_t dst_step, int bleed,
                            int skip_uniform_alpha, int filter) {
    w2x::ResizeFilter f;
    if (!e || !resize_filter(e, filter, "w2x_render_rgba_resized", f)) return 0;
    w2x::Image d = image(dst, dst_rows, dst_cols, dst_step);
    return e->engine.renderRgbaResized(image(src, rows, cols, src_step), d, rgba_options(bleed, skip_uniform_alpha), f) ? 1 : 0;
}
int w2x_render_sequence_rgba(w2x_engine* e, const uint8_t* const* srcs, int rows, int cols, size_t src_step, uint8_t* const* dsts, size_t dst_step, int count, int bleed,
                             int skip_uniform_alpha) {
    if (!sequence_ok(e, count, srcs, dsts)) return 0;
    ImageSequence q = image_sequence(srcs, image(nullptr, rows, cols, src_step), dsts, scaled_image(e->engine, nullptr, rows, cols, dst_step), count);
    return e->engine.renderSequenceRgba(q.src.data(), q.dst.data(), count, rgba_options(bleed, skip_uniform_alpha)) ? 1 : 0;
}
int w2x_render_sequence_rgba_resized(w2x_engine* e, const uint8_t* const* srcs, int rows, int cols, size_t src_step, uint8_t* const* dsts, int dst_rows, int dst_cols,
                                     size_t dst_step, int count, int bleed, int skip_uniform_alpha, int filter) {
    w2x::ResizeFilter f;
    if (!sequence_ok(e, count, srcs, dsts) || !resize_filter(e, filter, "w2x_render_sequence_rgba_resized", f)) return 0;
    ImageSequence q = image_sequence(srcs, image(nullptr, rows, cols, src_step), dsts, image(nullptr, dst_rows, dst_cols, dst_step), count);
    return e->engine.renderSequenceRgbaResized(q.src.data(), q.dst.data(), count, rgba_options(bleed, skip_uniform_alpha), f) ? 1 : 0;
}
// gray frames (include/w2x/c_api_gray.h): the Image of one channel goes through image() like a BGR one - the method says how many channels the buffer holds
int w2x_render_gray(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, size_t dst_step) {
    if (!e) return 0;
    w2x::Image d = scaled_image(e->engine, dst, rows, cols, dst_step);
    return e->engine.renderGray(image(src, rows, cols, src_step), d) ? 1 : 0;
}
int w2x_render_gray16(w2x_engine* e, const uint16_t* src, int rows, int cols, size_t src_step, uint16_t* dst, size_t dst_step) {
    if (!e) return 0;
    w2x::Image d = scaled_image(e->engine, dst, rows, cols, dst_step, 16);
    return e->engine.renderGray(image(src, rows, cols, src_step, 16), d) ? 1 : 0;
}
int w2x_render_gray_resized(w2x_engine* e, const uint8_t* src, int rows, int cols, size_t src_step, uint8_t* dst, int dst_rows, int dst_cols, size_t dst_step, int filter) {
    w2x::ResizeFilter f;
    if (!e || !resize_filter(e, filter, "w2x_render_gray_resized", f)) return 0;
    w2x::Image d = image(dst, dst_rows, dst_cols, dst_step);
    return e->engine.renderGrayResized(image(src, rows, cols, src_step), d, f) ? 1 : 0;
}
int w2x_render_gray16_resized(w2x_engine* e, const uint16_t* src, int rows, int cols, size_t src_step, uint16_t* dst, int dst_rows, int dst_cols, size_t dst_step, int filter) {
    w2x::ResizeFilter f;
    if (!e || !resize_filter(e, filter, "w2x_render_gray16_resized", f)) return 0;
    w2x::Image d = image(dst, dst_rows, dst_cols, dst_step, 16);
    return e->engine.renderGrayResized(image(src, rows, cols, src_step, 16), d, f) ? 1 : 0;
}
int w2x_render_sequence_gray(w2x_engine* e, const uint8_t* const* srcs, int rows, int cols, size_t src_step, uint8_t* const* dsts, size_t dst_step, int count) {
    if (!sequence_ok(e, count, srcs, dsts)) return 0;
    ImageSequence q = image_sequence(srcs, image(nullptr, rows, cols, src_step), dsts, scaled_image(e->engine, nullptr, rows, cols, dst_step), count);
    return e->engine.renderSequenceGray(q.src.data(), q.dst.data(), count) ? 1 : 0;
}
int w2x_render_sequence_gray_resized(w2x_engine* e, const uint8_t* const* srcs, int rows, int cols, size_t src_step, uint8_t* const* dsts, int dst_rows, int dst_cols,
                                     size_t dst_step, int count, int filter) {
    w2x::ResizeFilter f;
    if (!sequence_ok(e, count, srcs, dsts) || !resize_filter(e, filter, "w2x_render_sequence_gray_resized", f)) return 0;
    ImageSequence q = image_sequence(srcs, image(nullptr, rows, cols, src_step), dsts, image(nullptr, dst_rows, dst_cols, dst_step), count);
    return e->engine.renderSequenceGrayResized(q.src.data(), q.dst.data(), count, f) ? 1 : 0;
}
// planar RGB frames (include/w2x/c_api_planar.h): the sizes of both sides are explicit, as in the YUV entries
int w2x_render_planar(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                      void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits) {
    if (!e) return 0;
    w2x::PlanarImage d = planar_image(dst_planes, dst_steps, dst_rows, dst_cols, dst_bits);
    return e->engine.renderPlanar(planar_image(src_planes, src_steps, rows, cols, src_bits), d) ? 1 : 0;
}
int w2x_render_planar_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                              void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int filter) {
    w2x::ResizeFilter f;
    if (!e || !resize_filter(e, filter, "w2x_render_planar_resized", f)) return 0;
    w2x::PlanarImage d = planar_image(dst_planes, dst_steps, dst_rows, dst_cols, dst_bits);
    return e->engine.renderPlanarResized(planar_image(src_planes, src_steps, rows, cols, src_bits), d, f) ? 1 : 0;
}
int w2x_render_sequence_planar(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                               void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int count) {
    if (!sequence_ok(e, count, src_planes, dst_planes)) return 0;
    PlanarSequence q = planar_sequence(src_planes, src_steps, rows, cols, src_bits, dst_planes, dst_steps, dst_rows, dst_cols, dst_bits, count);
    return e->engine.renderSequencePlanar(q.src.data(), q.dst.data(), count) ? 1 : 0;
}
int w2x_render_sequence_planar_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                                       void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int count, int filter) {
    w2x::ResizeFilter f;
    if (!sequence_ok(e, count, src_planes, dst_planes) || !resize_filter(e, filter, "w2x_render_sequence_planar_resized", f)) return 0;
    PlanarSequence q = planar_sequence(src_planes, src_steps, rows, cols, src_bits, dst_planes, dst_steps, dst_rows, dst_cols, dst_bits, count);
    return e->engine.renderSequencePlanarResized(q.src.data(), q.dst.data(), count, f) ? 1 : 0;
}
size_t w2x_planar_plane_bytes(int rows, int cols, int bits) {
    if (rows <= 0 || cols <= 0 || !(bits == 8 || bits == 10 || bits == 12 || bits == 16 || bits == 32)) return 0;
    return (size_t)rows * cols * (bits == 32 ? 4 : bits > 8 ? 2 : 1);
}
// chained renders (include/w2x/c_api_chain.h): the engines of the handles, or nothing where one is missing
static std::vector<w2x::Img2Img*> chain_engines(w2x_engine* const* engines, int count) {
    std::vector<w2x::Img2Img*> es;
    if (!engines || count <= 0 || count > 64) return es;
    for (int k = 0; k < count; ++k) { if (!engines[k]) return {}; es.push_back(&engines[k]->engine); }
    return es;
}
static w2x::ChainOptions chain_options(int quantize) { w2x::ChainOptions o; o.quantize = quantize != 0; return o; }
static int chain_total(const std::vector<w2x::Img2Img*>& es) { int S = 1; for (w2x::Img2Img* e : es) S *= e->scaling() > 0 && e->scaling() <= 4 ? e->scaling() : 1; return S; }
int w2x_chain_plan(int rows, int cols, const int* scalings, int count, int dst_rows, int dst_cols, int* out) {
    w2x::ChainPlan cp;
    const w2x::ChainRefusal why = w2x::chain_plan(rows, cols, scalings, count, dst_rows, dst_cols, cp);
    if (why != w2x::kChainOk || !out) return why != w2x::kChainOk ? (int)why : W2X_CHAIN_COUNT;
    for (int k = 0; k <= count; ++k) { out[2 * k] = cp.rows[k]; out[2 * k + 1] = cp.cols[k]; }
    out[2 * count + 2] = cp.out_rows; out[2 * count + 3] = cp.out_cols; out[2 * count + 4] = cp.S;
    return W2X_CHAIN_OK;
}
int w2x_render_chained(w2x_engine* const* engines, int count, const void* src, int rows, int cols, size_t src_step, void* dst, size_t dst_step, int depth, int quantize) {
    const std::vector<w2x::Img2Img*> es = chain_engines(engines, count);
    if (es.empty()) return 0;
    const int S = chain_total(es);
    w2x::Image d = image(dst, rows * S, cols * S, dst_step, depth);
    return w2x::Img2Img::renderChained(es.data(), count, image(src, rows, cols, src_step, depth), d, chain_options(quantize)) ? 1 : 0;
}
int w2x_render_chained_resized(w2x_engine* const* engines, int count, const void* src, int rows, int cols, size_t src_step, void* dst, int dst_rows, int dst_cols,
                               size_t dst_step, int depth, int quantize, int filter) {
    const std::vector<w2x::Img2Img*> es = chain_engines(engines, count);
    w2x::ResizeFilter f;
    if (es.empty() || !resize_filter(engines[0], filter, "w2x_render_chained_resized", f)) return 0;
    w2x::Image d = image(dst, dst_rows, dst_cols, dst_step, depth);
    return w2x::Img2Img::renderChainedResized(es.data(), count, image(src, rows, cols, src_step, depth), d, chain_options(quantize), f) ? 1 : 0;
}
int w2x_render_sequence_chained(w2x_engine* const* engines, int count, const void* const* srcs, int rows, int cols, size_t src_step, void* const* dsts, size_t dst_step,
                                int frames, int quantize) {
    const std::vector<w2x::Img2Img*> es = chain_engines(engines, count);
    if (es.empty() || !sequence_ok(engines[0], frames, srcs, dsts)) return 0;
    const int S = chain_total(es);
    ImageSequence q = image_sequence((const uint8_t* const*)srcs, image(nullptr, rows, cols, src_step), (uint8_t* const*)dsts, image(nullptr, rows * S, cols * S, dst_step), frames);
    return w2x::Img2Img::renderSequenceChained(es.data(), count, q.src.data(), q.dst.data(), frames, chain_options(quantize)) ? 1 : 0;
}
int w2x_render_sequence_chained_resized(w2x_engine* const* engines, int count, const void* const* srcs, int rows, int cols, size_t src_step, void* const* dsts,
                                        int dst_rows, int dst_cols, size_t dst_step, int frames, int quantize, int filter) {
    const std::vector<w2x::Img2Img*> es = chain_engines(engines, count);
    w2x::ResizeFilter f;
    if (es.empty() || !sequence_ok(engines[0], frames, srcs, dsts) || !resize_filter(engines[0], filter, "w2x_render_sequence_chained_resized", f)) return 0;
    ImageSequence q = image_sequence((const uint8_t* const*)srcs, image(nullptr, rows, cols, src_step), (uint8_t* const*)dsts, image(nullptr, dst_rows, dst_cols, dst_step), frames);
    return w2x::Img2Img::renderSequenceChainedResized(es.data(), count, q.src.data(), q.dst.data(), frames, chain_options(quantize), f) ? 1 : 0;
}
int w2x_render_chained_planes(w2x_engine* const* engines, int count, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                              void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int quantize) {
    const std::vector<w2x::Img2Img*> es = chain_engines(engines, count);
    if (es.empty()) return 0;
    w2x::PlanarImage d = planar_image(dst_planes, dst_steps, dst_rows, dst_cols, dst_bits);
    return w2x::Img2Img::renderChainedPlanar(es.data(), count, planar_image(src_planes, src_steps, rows, cols, src_bits), d, chain_options(quantize)) ? 1 : 0;
}
int w2x_render_chained_planes_resized(w2x_engine* const* engines, int count, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                                      void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int quantize, int filter) {
    const std::vector<w2x::Img2Img*> es = chain_engines(engines, count);
    w2x::ResizeFilter f;
    if (es.empty() || !resize_filter(engines[0], filter, "w2x_render_chained_planes_resized", f)) return 0;
    w2x::PlanarImage d = planar_image(dst_planes, dst_steps, dst_rows, dst_cols, dst_bits);
    return w2x::Img2Img::renderChainedPlanarResized(es.data(), count, planar_image(src_planes, src_steps, rows, cols, src_bits), d, chain_options(quantize), f) ? 1 : 0;
}

// planar RGBA frames (include/w2x/c_api_rgbap.h)
int w2x_render_rgbap(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                     void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int bleed, int skip_uniform_alpha) {
    if (!e) return 0;
    w2x::PlanarRgbaImage d = rgbap_image(dst_planes, dst_steps, dst_rows, dst_cols, dst_bits);
    return e->engine.renderPlanarRgba(rgbap_image(src_planes, src_steps, rows, cols, src_bits), d, rgba_options(bleed, skip_uniform_alpha)) ? 1 : 0;
}
int w2x_render_rgbap_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                             void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int bleed, int skip_uniform_alpha, int filter) {
    w2x::ResizeFilter f;
    if (!e || !resize_filter(e, filter, "w2x_render_rgbap_resized", f)) return 0;
    w2x::PlanarRgbaImage d = rgbap_image(dst_planes, dst_steps, dst_rows, dst_cols, dst_bits);
    return e->engine.renderPlanarRgbaResized(rgbap_image(src_planes, src_steps, rows, cols, src_bits), d, rgba_options(bleed, skip_uniform_alpha), f) ? 1 : 0;
}
int w2x_render_sequence_rgbap(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                              void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int count, int bleed, int skip_uniform_alpha) {
    if (!sequence_ok(e, count, src_planes, dst_planes)) return 0;
    RgbapSequence q = rgbap_sequence(src_planes, src_steps, rows, cols, src_bits, dst_planes, dst_steps, dst_rows, dst_cols, dst_bits, count);
    return e->engine.renderSequencePlanarRgba(q.src.data(), q.dst.data(), count, rgba_options(bleed, skip_uniform_alpha)) ? 1 : 0;
}
int w2x_render_sequence_rgbap_resized(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, int src_bits,
                                      void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int dst_bits, int count, int bleed,
                                      int skip_uniform_alpha, int filter) {
    w2x::ResizeFilter f;
    if (!sequence_ok(e, count, src_planes, dst_planes) || !resize_filter(e, filter, "w2x_render_sequence_rgbap_resized", f)) return 0;
    RgbapSequence q = rgbap_sequence(src_planes, src_steps, rows, cols, src_bits, dst_planes, dst_steps, dst_rows, dst_cols, dst_bits, count);
    return e->engine.renderSequencePlanarRgbaResized(q.src.data(), q.dst.data(), count, rgba_options(bleed, skip_uniform_alpha), f) ? 1 : 0;
}
int w2x_alpha_bleed_rgbap_device(w2x_engine* e, const void* const* planes, const size_t* steps, int rows, int cols, int bits, int radius,
                                 void* const* out_planes, const size_t* out_steps, unsigned* words) {
    if (!e) return 0;
    w2x::PlanarImage d = planar_image(out_planes, out_steps, rows, cols, bits);
    return e->engine.alphaBleedPlanes(rgbap_image(planes, steps, rows, cols, bits), d, radius, words) ? 1 : 0;
}
int w2x_alpha_bleed_device(w2x_engine* e, const uint8_t* bgra, int rows, int cols, size_t bgra_step, uint8_t* bgr, size_t bgr_step, int radius) {
    if (!e) return 0;
    w2x::Image d = image(bgr, rows, cols, bgr_step);
    return e->engine.alphaBleed(image(bgra, rows, cols, bgra_step), d, radius) ? 1 : 0;
}
// dithered output (include/w2x/c_api_dither.h)
int w2x_set_dither(w2x_engine* e, int mode, unsigned phase, unsigned advance) {
    if (!e) return 0;
    w2x::DitherOptions o; o.mode = (w2x::Dither)mode; o.phase = phase; o.advance = advance;   // (the engine refuses unknown modes through the message callback)
    return e->engine.setDither(o) ? 1 : 0;
}
int w2x_get_dither(const w2x_engine* e, int* mode, unsigned* phase, unsigned* advance) {
    if (!e) return 0;
    const w2x::DitherOptions o = e->engine.dither();
    if (mode) *mode = (int)o.mode;
    if (phase) *phase = o.phase;
    if (advance) *advance = o.advance;
    return 1;
}
int w2x_dither_table(int mode, uint16_t* out, int* side) {
    if (mode != W2X_DITHER_ORDERED && mode != W2X_DITHER_BLUENOISE) return 0;
    const int n = mode == W2X_DITHER_ORDERED ? 8 : w2x::kDitherSide;
    if (side) *side = n;
    if (out) for (int y = 0; y < n; ++y) for (int x = 0; x < n; ++x) out[y * n + x] = (uint16_t)w2x::dither_rank(mode, 0, 0, x, y);
    return 1;
}
int w2x_dither_rank(int mode, unsigned phase, int c, int x, int y) { return w2x::dither_rank(mode, phase, c, x, y); }
int w2x_dither_planes(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols, void* const* dst_planes, const size_t* dst_steps, int bits) {
    if (!e) return 0;
    w2x::PlanarImage d = planar_image(dst_planes, dst_steps, rows, cols, bits);
    return e->engine.ditherPlanes(planar_image(src_planes, src_steps, rows, cols, 32), d) ? 1 : 0;
}
// resize in linear light (include/w2x/c_api_resize_light.h)
int w2x_set_resize_light(w2x_engine* e, int mode) { return e && e->engine.setResizeLight((w2x::ResizeLight)mode) ? 1 : 0; }   // (the engine refuses unknown modes)
int w2x_get_resize_light(const w2x_engine* e) { return e ? (int)e->engine.resizeLight() : -1; }
static float light_clamped(float v) { return !(v >= 0.f) ? 0.f : (v > 1.f ? 1.f : v); }
float w2x_light_decode(int mode, float v) { return w2x::light_mode_ok(mode) ? w2x::light_decode(w2x::light_args(mode), light_clamped(v)) : NAN; }
float w2x_light_encode(int mode, float v) { return w2x::light_mode_ok(mode) ? w2x::light_encode(w2x::light_args(mode), light_clamped(v)) : NAN; }
int w2x_resize_planes(w2x_engine* e, const void* const* src_planes, const size_t* src_steps, int rows, int cols,
                      void* const* dst_planes, const size_t* dst_steps, int dst_rows, int dst_cols, int bits, int filter) {
    if (!e) return 0;
    w2x::ResizeFilter f;
    if (!resize_filter(e, filter, "resizePlanes", f)) return 0;
    w2x::PlanarImage d = planar_image(dst_planes, dst_steps, dst_rows, dst_cols, bits);
    return e->engine.resizePlanes(planar_image(src_planes, src_steps, rows, cols, 32), d, f) ? 1 : 0;
}
void* w2x_alloc_host(w2x_engine* e, size_t bytes) { return e ? e->engine.allocHost(bytes) : nullptr; }
void w2x_free_host(w2x_engine* e, void* data) { if (e) e->engine.freeHost(data); }
int w2x_pin_host(w2x_engine* e, void* data, size_t bytes) { return e && e->engine.pinHost(data, bytes) ? 1 : 0; }
void w2x_unpin_host(w2x_engine* e, void* data) { if (e) e->engine.unpinHost(data); }

int w2x_strip_plan(int in_w, int in_h, int out_w, int out_h, int tile_in, int tile_out, int scaling, double overlap_x, double overlap_y,
                   int part, int parts, int* out4) {
    if (!out4) return 0;
    w2x::TileGrid g = w2x::calculate_tiles(in_w, in_h, out_w, out_h, tile_in, tile_in, tile_out, tile_out, scaling, overlap_x, overlap_y);
    w2x::StripPlan sp = w2x::strip_plan(g, out_w, tile_out, part, parts);
    out4[0] = sp.first_tile; out4[1] = sp.tile_count; out4[2] = sp.x0; out4[3] = sp.x1;
    return 1;
}

int w2x_shard_plan(int in_w, int in_h, int out_w, int out_h, int tile_in, int tile_out, int scaling, double overlap_x, double overlap_y,
                   int part, int parts, int* out16) {
    if (!out16) return 0;
    w2x::TileGrid g = w2x::calculate_tiles(in_w, in_h, out_w, out_h, tile_in, tile_in, tile_out, tile_out, scaling, overlap_x, overlap_y);
    w2x::ShardPlan sp = w2x::shard_plan(g, out_w, out_h, tile_out, tile_out, part, parts);
    out16[0] = sp.first_tile; out16[1] = sp.tile_count; out16[2] = sp.halo_first; out16[3] = sp.nrect;
    for (int r = 0; r < 3; ++r) { out16[4 + 4 * r] = sp.rect[r].x; out16[5 + 4 * r] = sp.rect[r].y; out16[6 + 4 * r] = sp.rect[r].w; out16[7 + 4 * r] = sp.rect[r].h; }
    return 1;
}

int w2x_infer(w2x_engine* e, const float* in, float* out) { return e && e->engine.infer(in, out) ? 1 : 0; }
int w2x_output_tile_size(w2x_engine* e) { return e ? e->engine.outputTileSize() : 0; }
int w2x_pass_tiles(w2x_engine* e) { return e ? e->engine.passTiles() : 0; }
double w2x_plan_flops(w2x_engine* e) { return e ? e->engine.planFlops() : 0.0; }
float w2x_last_render_ms(w2x_engine* e) { return e ? e->engine.lastRenderMs() : -1.f; }
int w2x_profile_frame(w2x_engine* e, double* out, int cap) { return e && e->engine.profileFrame(out, cap) ? 1 : 0; }
int w2x_op_times(w2x_engine* e, double* out, int cap) { return e ? e->engine.opTimes(out, cap) : 0; }
float w2x_bench_resident(w2x_engine* e, int iters) { return e ? e->engine.benchResident(iters) : -1.f; }
int w2x_resident_output(w2x_engine* e, void* dst, size_t bytes) { return e && e->engine.residentOutput(dst, bytes) ? 1 : 0; }

int w2x_calculate_tiles(int in_w, int in_h, int out_w, int out_h, int tile_in, int tile_out, int scaling,
                        double overlap_x, double overlap_y, int* in_rects, int* out_rects, int cap) {
    w2x::TileGrid g = w2x::calculate_tiles(in_w, in_h, out_w, out_h, tile_in, tile_in, tile_out, tile_out, scaling, overlap_x, overlap_y);
    if (g.count > cap) return -1;
    for (int i = 0; i < g.count; ++i) {
        if (in_rects) { in_rects[4 * i] = g.in[i].x; in_rects[4 * i + 1] = g.in[i].y; in_rects[4 * i + 2] = g.in[i].w; in_rects[4 * i + 3] = g.in[i].h; }
        if (out_rects) { out_rects[4 * i] = g.out[i].x; out_rects[4 * i + 1] = g.out[i].y; out_rects[4 * i + 2] = g.out[i].w; out_rects[4 * i + 3] = g.out[i].h; }
    }
    return g.count;
}

int w2x_yuv_plane_sizes(int rows, int cols, int bits, int* plane_rows, int* plane_cols, size_t* plane_bytes) {
    return w2x_yuv_layout_plane_sizes(rows, cols, bits, W2X_YUV_I420, nullptr, plane_rows, plane_cols, plane_bytes);
}

int w2x_yuv_layout_plane_sizes(int rows, int cols, int bits, int layout, int* nplanes, int* plane_rows, int* plane_cols, size_t* plane_bytes) {
    if (rows <= 0 || cols <= 0 || (bits != 8 && bits != 10) || layout < W2X_YUV_I420 || layout > W2X_YUV_NV12) return 0;
    const int n = layout == W2X_YUV_NV12 ? 2 : 3;
    const int cr = layout == W2X_YUV_I420 || layout == W2X_YUV_NV12 ? (rows + 1) / 2 : rows;
    const int cc = layout == W2X_YUV_I444 ? cols : layout == W2X_YUV_NV12 ? 2 * ((cols + 1) / 2) : (cols + 1) / 2;
    if (nplanes) *nplanes = n;
    for (int k = 0; k < 3; ++k) {
        const int r = k >= n ? 0 : k ? cr : rows, c = k >= n ? 0 : k ? cc : cols;
        if (plane_rows) plane_rows[k] = r;
        if (plane_cols) plane_cols[k] = c;
        if (plane_bytes) plane_bytes[k] = (size_t)r * c * (bits > 8 ? 2 : 1);
    }
    return 1;
}

int w2x_alpha_bleed(const uint8_t* bgr, size_t bgr_step, const uint8_t* alpha, size_t alpha_step, int rows, int cols, int radius, uint8_t* out, size_t out_step) {
    try { return w2x::alpha_bleed(bgr, bgr_step, alpha, alpha_step, rows, cols, radius, out, out_step) ? 1 : 0; } catch (...) { return 0; }
}

int w2x_alpha_bleed_rgbap(const void* const* planes, const size_t* steps, int rows, int cols, int bits, int radius, void* const* out_planes, const size_t* out_steps) {
    if (!planes || !steps || !out_planes || !out_steps || !(bits == 8 || bits == 10 || bits == 12 || bits == 16)) return 0;
    try { return w2x::alpha_bleed_planes(planes, steps, planes[3], steps[3], rows, cols, bits > 8 ? 2 : 1, (1u << bits) - 1u, radius, out_planes, out_steps) ? 1 : 0; } catch (...) { return 0; }
}

int w2x_resize_weights(int in, int out, int filter, int* first, float* weights, int cap) {
    if (in <= 0 || out <= 0 || (filter != W2X_RESIZE_BICUBIC && filter != W2X_RESIZE_BILINEAR)) return 0;
    const w2x::ResizeTaps t = w2x::resize_taps(in, out, filter);
    if (!first || !weights) return t.taps;
    if ((long)cap < (long)out * t.taps) return -t.taps;
    memcpy(first, t.first.data(), t.first.size() * sizeof(int));
    memcpy(weights, t.w.data(), t.w.size() * sizeof(float));
    return t.taps;
}

// edge modes (include/w2x/c_api_edge.h)
int w2x_set_edge(w2x_engine* e, int mode) { return e && e->engine.setEdge((w2x::EdgeMode)mode) ? 1 : 0; }   // (the engine refuses unknown modes)
int w2x_get_edge(const w2x_engine* e) { return e ? (int)e->engine.edge() : -1; }
int w2x_edge_index(int mode, long long i, int n) { return w2x::edge_mode_ok(mode) && n > 0 ? w2x::edge_index(mode, i, n) : -1; }
int w2x_resize_weights_edge(int in, int out, int filter, int mode, int* first, float* weights, int cap) {
    if (in <= 0 || out <= 0 || (filter != W2X_RESIZE_BICUBIC && filter != W2X_RESIZE_BILINEAR) || !w2x::edge_mode_ok(mode)) return 0;
    const w2x::ResizeTaps t = w2x::resize_taps_edge(in, out, filter, mode);
    if (!first || !weights) return t.taps;
    if ((long)cap < (long)out * t.taps) return -t.taps;
    memcpy(first, t.first.data(), t.first.size() * sizeof(int));
    memcpy(weights, t.w.data(), t.w.size() * sizeof(float));
    return t.taps;
}
int w2x_alpha_bleed_edge(const uint8_t* bgr, size_t bgr_step, const uint8_t* alpha, size_t alpha_step, int rows, int cols, int radius, uint8_t* out, size_t out_step, int mode) {
    try { return w2x::alpha_bleed(bgr, bgr_step, alpha, alpha_step, rows, cols, radius, out, out_step, mode) ? 1 : 0; } catch (...) { return 0; }
}
int w2x_alpha_bleed_planes_edge(const void* const* planes, const size_t* steps, int rows, int cols, int bits, int radius, void* const* out_planes, const size_t* out_steps, int mode) {
    if (!planes || !steps || !out_planes || !out_steps || !(bits == 8 || bits == 10 || bits == 12 || bits == 16)) return 0;
    try { return w2x::alpha_bleed_planes(planes, steps, planes[3], steps[3], rows, cols, bits > 8 ? 2 : 1, (1u << bits) - 1u, radius, out_planes, out_steps, mode) ? 1 : 0; } catch (...) { return 0; }
}

int w2x_tile_weights(int which, int overlap_x, int overlap_y, int size, float* out) {
    if (which < 0 || which > 3 || size <= 0 || !out) return 0;
    auto m = w2x::tile_weight_mask(which, overlap_x, overlap_y, size);
    memcpy(out, m.data(), m.size() * sizeof(float));
    return 1;
}

int w2x_describe_plan(const char* onnx_path, int batch, int tile, char* buf, size_t cap) { return w2x_describe_plan_precision(onnx_path, batch, tile, W2X_PRECISION_FP16, buf, cap); }

int w2x_describe_plan_precision(const char* onnx_path, int batch, int tile, int precision, char* buf, size_t cap) {
    std::string s; int ok = 1;
    try {
        w2x::Plan plan = w2x::build_plan(onnx_path, batch, 3, tile, tile, precision != W2X_PRECISION_FP16);
        plan.userB = batch;
        const auto bytes = plan.serialize();                          // what build() writes must be what load() accepts
        s = w2x::Plan::deserialize(bytes.data(), bytes.size()).describe();
    }
    catch (const std::exception& e) { s = std::string("ERROR: ") + e.what(); ok = 0; }
    copy_out(s, buf, cap);
    return ok;
}

int w2x_validate_engine_file(const char* path, char* buf, size_t cap) {
    std::string s = "ok"; int ok = 1;
    try {
        std::ifstream f(path, std::ios::binary | std::ios::ate);
        if (!f.is_open()) throw std::runtime_error("could not open engine file");
        std::vector<char> bytes((size_t)f.tellg());
        f.seekg(0); f.read(bytes.data(), (std::streamsize)bytes.size());
        (void)w2x::Plan::deserialize((const uint8_t*)bytes.data(), bytes.size());
    } catch (const std::exception& e) { s = e.what(); ok = 0; }
    copy_out(s, buf, cap);
    return ok;
}

int w2x_write_engine_file(const char* onnx_path, int batch, int tile, const char* out_path) {
    try {
        w2x::Plan plan = w2x::build_plan(onnx_path, batch, 3, tile, tile);
        plan.userB = batch;
        const auto bytes = plan.serialize();
        std::ofstream f(out_path, std::ios::binary);
        if (!f.is_open()) return 0;
        f.write((const char*)bytes.data(), (std::streamsize)bytes.size());
        return f.good() ? 1 : 0;
    } catch (const std::exception&) { return 0; }
}

int w2x_device_pci_bus_id(int device, char* buf, size_t cap) { return buf && cap >= 16 && w2x::device_pci_bus_id(device, buf, cap) ? 1 : 0; }

void w2x_sha256_hex(const void* data, size_t len, char* out) {
    std::string h = w2x::sha256_hex(data, len);
    memcpy(out, h.c_str(), 65);
}

const char* w2x_version(void) { return "w2x-hip 0.1 (gfx950)"; }

int w2x_dead_skip_extents(const char* onnx_path, int batch, int tile, int in_w, int in_h, int scaling, double overlap_x, double overlap_y, int tile_index, int tta,
                          int* out, int cap) {
    try {
        // (the lowered plan of the last (file, batch, tile) is kept: a test asks for many frames and tiles of one plan)
        static std::mutex mu;
        static std::string key;
        static w2x::Plan plan;
        std::lock_guard<std::mutex> lock(mu);
        const std::string k = std::string(onnx_path ? onnx_path : "") + "|" + std::to_string(batch) + "|" + std::to_string(tile);
        if (k != key) { plan = w2x::build_plan(onnx_path, batch, 3, tile, tile, false); plan.userB = batch; key = k; }
        const int nops = (int)plan.ops.size();
        if (!out || cap < nops * W2X_EXTENT_INTS) return -nops;
        int kept_w = plan.Tout, kept_h = plan.Tout;
        bool all = tta != 0 || tile_index < 0 || w2x::switches().no_dead_skip;
        if (tile_index >= 0) {
            const w2x::TileGrid g = w2x::calculate_tiles(in_w, in_h, in_w * scaling, in_h * scaling, tile, tile, plan.Tout, plan.Tout, scaling, overlap_x, overlap_y);
            if (tile_index >= g.count) return 0;
            kept_w = g.out[tile_index].w; kept_h = g.out[tile_index].h;
        }
        const std::vector<w2x::OpExtent> ext = w2x::dead_skip_extents(plan, kept_w, kept_h, all);
        for (int i = 0; i < nops; ++i) {
            const w2x::Op& op = plan.ops[i]; const w2x::OpExtent& e = ext[i];
            int* o = out + (size_t)i * W2X_EXTENT_INTS;
            int in_t = -1, out_t = -1, res_t = -1, kh = 1, kw = 1, stride = 1, x0 = 0, y0 = 0, r = 1;
            if (op.kind == w2x::OP_GEMM) {
                in_t = op.g.a.t; out_t = op.g.out.t; res_t = op.g.res.t; x0 = op.g.a.x0; y0 = op.g.a.y0;
                if (op.g.amode == w2x::A_CONV) { kh = op.g.kh; kw = op.g.kw; stride = op.g.stride; }
                if (op.g.omode == w2x::O_PIXSHUF) r = op.g.r;
            } else if (op.kind == w2x::OP_MLP) { in_t = op.m.x; out_t = op.m.y; }
            else if (op.kind == w2x::OP_SWINATTN) { in_t = op.sa.x; out_t = op.sa.y; }
            auto dim = [&](int t, bool w) { return t >= 0 && t < (int)plan.tensors.size() ? (w ? plan.tensors[t].W : plan.tensors[t].H) : 0; };
            const int v[W2X_EXTENT_INTS] = {op.kind, e.x.n, e.y.n, e.x.c, e.x.w, e.y.c, e.y.w, e.rx, e.ry, e.ws, in_t, out_t, res_t, kh, kw, stride, x0, y0, r,
                                            dim(in_t, true), dim(in_t, false), dim(out_t, true), dim(out_t, false), (int)e.live_units(), (int)e.total_units()};
            for (int k = 0; k < W2X_EXTENT_INTS; ++k) o[k] = v[k];
        }
        return nops;
    } catch (const std::exception&) { return 0; }
}

int w2x_debug_set(const char* name, int value) { return w2x::set_switch(name, value) ? 1 : 0; }

}  // extern "C"
