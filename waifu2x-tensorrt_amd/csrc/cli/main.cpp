// w2x: the reference's command line (src/main.cpp) on top of w2x::Img2Img.
//   w2x --model swin_unet/art --scale 4 --noise 3 --batchSize 4 --tileSize 256 build
//   w2x --model swin_unet/art --scale 4 --noise 3 --batchSize 4 --tileSize 256 render -i in.png -o outdir [--tta] [--blend 1/16]
// Stills (.png / .ppm / .bmp) and uncompressed .avi files are read and written by the built-in codecs (imageio.h); other formats and
// videos are piped through ffmpeg as raw bgr24 when ffmpeg/ffprobe are on PATH (videoio/capture.cpp:96-99, writer.cpp:24-33 do the same).
// A PNG / BMP with an alpha channel keeps it (upstream TODO, README.md:88): an 8-bit still on one device goes through Img2Img::renderRgba, or with --outscale /
// --outsize through Img2Img::renderRgbaResized (colour and alpha in one call, --alpha-bleed / --alpha-skip-uniform on the GPU); on the other routes
// (--devices > 1, --deep) the alpha plane goes through the same engine as a gray image.
// Extension: --gray keeps gray PNGs (colour type 0) and ffmpeg videos one channel wide: Img2Img::renderGray / renderGrayResized for stills, raw `gray` frames
// through renderSequenceGray[Resized] for videos; colour files, single frames read through ffmpeg, gray + alpha PNGs and the built-in AVI route are rendered
// as without it.
// Extension: --rgb-in / --rgb-out FMT carry ffmpeg videos as raw planar RGB frames (gbrp, gbrp10le, gbrp12le, gbrp16le, gbrpf32le: planes G, B, R, contiguous)
// through Img2Img::renderSequencePlanar[Resized], the two depths independent (--rgba-in / --rgba-out: gbrap*, a fourth plane A, through
// Img2Img::renderSequencePlanarRgba[Resized] with --alpha-bleed / --alpha-skip-uniform); stills, single frames read through ffmpeg and the built-in AVI route are
// rendered as without them.  Over --devices N the chunks go to the engines like bgr24 chunks.
// Extension: --devices N drives N engines - a single image is split into tile-column strips (Img2Img::renderStrip), every engine
// writing its own columns of the shared output buffer; a video is cut into chunks of frames that go round-robin to one persistent
// worker thread per engine (renderSequence over that engine's page-locked buffers), with one reader and one in-order writer thread.
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <iostream>
#include <atomic>
#include <condition_variable>
#include <csignal>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>

#include "../../../include/w2x/img2img.h"
#include "../tiles.h"
#include "args.h"
#include "imageio.h"

using namespace w2x;
namespace fs = std::filesystem;

namespace {

bool on_path(const char* tool) { return std::system((std::string("command -v ") + tool + " >/dev/null 2>&1").c_str()) == 0; }

std::string shell_quote(const std::string& s) { std::string r = "'"; for (char c : s) { if (c == '\'') r += "'\\''"; else r += c; } return r + "'"; }

struct Probe { int width = 0, height = 0, frames = 0; double fps = 0; };

Probe ffprobe(const std::string& file) {
    const std::string cmd = "ffprobe -v error -select_streams v:0 -count_packets -show_entries stream=width,height,r_frame_rate,nb_read_packets -of csv=p=0 " + shell_quote(file);
    Probe p;
    if (FILE* f = popen(cmd.c_str(), "r")) {
        int num = 0, den = 1;
        if (fscanf(f, "%d,%d,%d/%d,%d", &p.width, &p.height, &num, &den, &p.frames) >= 4 && den) p.fps = (double)num / den;
        pclose(f);
    }
    if (p.width <= 0 || p.height <= 0) throw std::runtime_error("ffprobe could not read " + file);
    if (p.frames <= 0) p.frames = 1;
    return p;
}

std::vector<std::string> find_inputs(const cli::Options& o) {
    static const char* exts[] = {".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".ppm", ".mp4", ".avi", ".mkv"};   // main.cpp:156-159 (+ .ppm)
    auto wanted = [&](const fs::path& p) { std::string e = p.extension().string(); for (auto& c : e) c = (char)tolower(c); for (const char* x : exts) if (e == x) return true; return false; };
    std::vector<std::string> files;
    for (const std::string& in : o.inputs) {
        if (fs::is_directory(in)) {
            if (o.recursive) { for (const auto& e : fs::recursive_directory_iterator(in)) if (e.is_regular_file() && wanted(e.path())) files.push_back(e.path().string()); }
            else for (const auto& e : fs::directory_iterator(in)) if (e.is_regular_file() && wanted(e.path())) files.push_back(e.path().string());
        } else if (wanted(in)) files.push_back(in);
    }
    std::sort(files.begin(), files.end());
    return files;
}

// ---- YUV frames as ffmpeg's rawvideo carries them (cli::kYuvFormats): the planes back to back - Y, U, V, or Y, UV for nv12 / p010le -, rows unpadded
struct RawYuv { YuvLayout layout; int bits; };
RawYuv raw_yuv(const std::string& fmt) {
    const bool ten = fmt.size() > 4 && fmt.compare(fmt.size() - 4, 4, "10le") == 0;
    if (fmt == "nv12" || fmt == "p010le") return {YuvLayout::NV12, ten ? 10 : 8};
    return {fmt.rfind("yuv422p", 0) == 0 ? YuvLayout::I422 : fmt.rfind("yuv444p", 0) == 0 ? YuvLayout::I444 : YuvLayout::I420, ten ? 10 : 8};
}
// a packed frame over p: chroma of ch rows x cw samples (nv12: both components in one plane)
YuvImage packed_yuv(uint8_t* p, int rows, int cols, const RawYuv& fmt) {
    const bool sub_y = fmt.layout == YuvLayout::I420 || fmt.layout == YuvLayout::NV12;
    const size_t bps = fmt.bits > 8 ? 2 : 1, ch = sub_y ? (size_t)(rows + 1) / 2 : (size_t)rows;
    const size_t cw = fmt.layout == YuvLayout::I444 ? (size_t)cols : (size_t)((cols + 1) / 2) * (fmt.layout == YuvLayout::NV12 ? 2 : 1);
    YuvImage f;
    f.planes[0] = p; f.planes[1] = p + (size_t)rows * cols * bps; f.planes[2] = fmt.layout == YuvLayout::NV12 ? nullptr : f.planes[1] + ch * cw * bps;
    f.steps[0] = (size_t)cols * bps; f.steps[1] = cw * bps; f.steps[2] = fmt.layout == YuvLayout::NV12 ? 0 : cw * bps;
    f.rows = rows; f.cols = cols; f.bits = fmt.bits; f.layout = fmt.layout;
    return f;
}
size_t yuv_frame_bytes(int rows, int cols, const RawYuv& fmt) {
    const YuvImage f = packed_yuv(nullptr, rows, cols, fmt);
    const size_t ch = fmt.layout == YuvLayout::I420 || fmt.layout == YuvLayout::NV12 ? (size_t)(rows + 1) / 2 : (size_t)rows;
    return f.steps[0] * rows + (f.steps[1] + f.steps[2]) * ch;
}
// the writer's colour tags for --colorspace / --color_range
std::string colour_tags(const cli::Options& o) {
    const char* m = o.colorspace == "bt601" ? "smpte170m" : o.colorspace == "bt2020" ? "bt2020nc" : "bt709";
    const char* pr = o.colorspace == "bt601" ? "smpte170m" : o.colorspace == "bt2020" ? "bt2020" : "bt709";
    const char* trc = o.colorspace == "bt601" ? "smpte170m" : o.colorspace == "bt2020" ? "bt2020-10" : "bt709";
    const std::string loc = o.chromaLoc.empty() ? "" : "-chroma_sample_location " + o.chromaLoc + " ";   // --chroma-loc
    return std::string("-colorspace ") + m + " -color_primaries " + pr + " -color_trc " + trc + " -color_range " + o.colorRange + " " + loc;
}

// ---- frame streams: raw bgr24 (or --colorspace: YUV 4:2:0) frames from / to an ffmpeg pipe or a built-in uncompressed AVI
struct FrameSource { virtual ~FrameSource() {} virtual bool read(uint8_t* bgr) = 0; };
struct FrameSink { virtual ~FrameSink() {} virtual bool write(const uint8_t* bgr) = 0; virtual bool close() = 0; };

struct PipeSource : FrameSource {
    FILE* f; size_t bytes;
    PipeSource(const std::string& cmd, size_t b) : f(popen(cmd.c_str(), "r")), bytes(b) { if (!f) throw std::runtime_error("cannot start ffmpeg"); }
    ~PipeSource() override { if (f) pclose(f); }
    bool read(uint8_t* bgr) override { return fread(bgr, 1, bytes, f) == bytes; }
};
struct PipeSink : FrameSink {
    FILE* f; size_t bytes;
    PipeSink(const std::string& cmd, size_t b) : f(popen(cmd.c_str(), "w")), bytes(b) { if (!f) throw std::runtime_error("cannot start ffmpeg"); }
    ~PipeSink() override { if (f) pclose(f); }
    bool write(const uint8_t* bgr) override { return fwrite(bgr, 1, bytes, f) == bytes; }
    bool close() override { FILE* g = f; f = nullptr; return g && pclose(g) == 0; }
};
struct AviSource : FrameSource {
    cli::AviReader rd;
    bool read(uint8_t* bgr) override { return rd.read(bgr); }
};
struct AviSink : FrameSink {
    cli::AviWriter wr;
    bool write(const uint8_t* bgr) override { try { wr.write(bgr); return true; } catch (const std::exception& e) { std::cerr << e.what() << "\n"; return false; } }
    bool close() override { try { wr.close(); return true; } catch (const std::exception& e) { std::cerr << e.what() << "\n"; return false; } }
};

// The frame loop of main.cpp:263-269 over N engines.  Chunk c (CH consecutive frames) belongs to engine c % N; every engine owns SLOTS
// chunk slots of page-locked frame buffers (allocHost: the copies of renderSequence run by DMA beside the kernels).  One reader thread
// fills slots in stream order, one persistent worker per engine renders its chunks with renderSequence (upload / compute / download of
// consecutive frames overlapped), one writer thread drains the slots in stream order - decoding, N renders and encoding all overlap,
// and frames leave in the order they came (the reference serialises read -> render -> write per frame).
// A frame is inBytes in and outBytes out; `render` turns `count` of them into outputs on one engine (renderSequence, renderSequenceResized for
// --outscale / --outsize, renderSequenceYuv for --colorspace, renderSequenceYuvResized for --colorspace with --outsize).
using RenderFrames = std::function<bool(Img2Img&, uint8_t* const* in, uint8_t* const* out, int count)>;
bool run_frame_pipeline(std::vector<std::unique_ptr<Img2Img>>& engines, FrameSource& src, FrameSink& dst, size_t inBytes, size_t outBytes,
                        const RenderFrames& render, const std::function<void(int)>& on_frames) {
    const int N = (int)engines.size(), CH = 4, SLOTS = 2;
    struct Slot { std::vector<uint8_t*> in, out; int frames = 0; int state = 0; };   // 0 free, 1 read, 2 rendered
    std::vector<std::vector<Slot>> slots(N, std::vector<Slot>(SLOTS));
    auto release = [&] { for (int e = 0; e < N; ++e) for (Slot& sl : slots[e]) { for (uint8_t* p : sl.in) engines[e]->freeHost(p); for (uint8_t* p : sl.out) engines[e]->freeHost(p); sl.in.clear(); sl.out.clear(); } };
    for (int e = 0; e < N; ++e)
        for (Slot& sl : slots[e])
            for (int k = 0; k < CH; ++k) {
                sl.in.push_back((uint8_t*)engines[e]->allocHost(inBytes)); sl.out.push_back((uint8_t*)engines[e]->allocHost(outBytes));
                if (!sl.in.back() || !sl.out.back()) { release(); throw std::runtime_error("cannot allocate page-locked frame buffers"); }
            }
    std::mutex mu; std::condition_variable cv;
    bool failed = false;
    long total_chunks = -1;                         // known once the reader has hit the end of the stream
    auto slot_of = [&](long c) -> Slot& { return slots[c % N][(c / N) % SLOTS]; };
    std::thread reader([&] {
        for (long c = 0;; ++c) {
            Slot& sl = slot_of(c);
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return sl.state == 0 || failed; }); if (failed) return; }
            int got = 0;
            for (; got < CH; ++got) if (!src.read(sl.in[got])) break;
            { std::lock_guard<std::mutex> lk(mu); sl.frames = got; if (got) sl.state = 1; if (got < CH) total_chunks = c + (got ? 1 : 0); }
            cv.notify_all();
            if (got < CH) return;
        }
    });
    std::vector<std::thread> workers;
    for (int e = 0; e < N; ++e) workers.emplace_back([&, e] {
        for (long c = e;; c += N) {
            Slot& sl = slot_of(c);
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return sl.state == 1 || failed || (total_chunks >= 0 && c >= total_chunks); }); if (failed || sl.state != 1) return; }
            const bool ok = render(*engines[e], sl.in.data(), sl.out.data(), sl.frames);
            { std::lock_guard<std::mutex> lk(mu); if (!ok) failed = true; sl.state = 2; }
            cv.notify_all();
            if (!ok) return;
        }
    });
    std::thread writer([&] {
        for (long c = 0;; ++c) {
            Slot& sl = slot_of(c);
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return sl.state == 2 || failed || (total_chunks >= 0 && c >= total_chunks); }); if (failed || sl.state != 2) return; }
            const int n = sl.frames;
            for (int k = 0; k < n; ++k) if (!dst.write(sl.out[k])) { std::lock_guard<std::mutex> lk(mu); failed = true; }
            { std::lock_guard<std::mutex> lk(mu); sl.state = 0; }
            cv.notify_all();
            on_frames(n);
        }
    });
    reader.join();
    for (auto& t : workers) t.join();
    writer.join();
    release();
    return !failed;
}

}  // namespace

int main(int argc, char** argv) {
    cli::Options o;
    try { o = cli::parse(argc, argv); }
    catch (const std::exception& e) { std::cerr << e.what() << "\nRun with --help for more information.\n"; return -1; }
    if (o.help) { std::cout << cli::usage(); return 0; }
    if (o.printConfig) { std::cout << cli::to_json(o) << "\n"; return 0; }
    try {
        if (o.command == "convert") { cli::write_image(o.output, cli::read_image(o.inputs[0])); return 0; }

        const std::string modelPath = cli::model_path(o);
        // the progress callback runs on the engines' worker threads while the writer thread advances the frame counter
        std::atomic<size_t> fileIndex{0}, fileCount{0}, frameIndex{0}, frameCount{0};
        auto on_message = [](Severity s, const std::string& m) {
            static const char* names[] = {"critical", "error", "warning", "info", "debug", "trace"};
            std::cerr << "[" << names[(int)s < 6 ? (int)s : 5] << "] " << m << "\n";
        };
        auto on_progress = [&](int current, int total, double speed) {
            fprintf(stderr, "[info] Rendered file %zu/%zu, frame %zu/%zu, batch %d/%d @ %.2f it/s\n", fileIndex.load(), fileCount.load(), frameIndex.load(), frameCount.load(), current, total, speed);
        };
        const Precision prec = o.precision == "tf32" ? Precision::TF32 : o.precision == "fp32" ? Precision::FP32 : Precision::FP16;

        if (o.command == "build") {
            Img2Img engine;
            engine.setMessageCallback(on_message);
            BuildConfig c;
            c.deviceId = o.device; c.precision = prec;
            c.minBatchSize = c.optBatchSize = c.maxBatchSize = o.batchSize;
            c.minChannels = c.optChannels = c.maxChannels = 3;                       // main.cpp:280-282
            c.minWidth = c.optWidth = c.maxWidth = c.minHeight = c.optHeight = c.maxHeight = o.tileSize;
            if (!engine.build(modelPath, c)) return -1;
            // --chain: the engine file of the stages behind the first, where they take another model file
            if (o.chain > 1 && cli::chain_model_path(o) != modelPath && !engine.build(cli::chain_model_path(o), c)) return -1;
            return 0;
        }

        // render: one engine per device
        std::vector<std::unique_ptr<Img2Img>> engines;
        // external tools are probed (fork + exec of a shell) before the first engine brings the HIP runtime up; a dying encoder must
        // surface as a failed write, not as SIGPIPE
        const bool have_ffmpeg = on_path("ffmpeg") && on_path("ffprobe");
        signal(SIGPIPE, SIG_IGN);
        for (int d = 0; d < o.devices; ++d) {
            engines.emplace_back(new Img2Img);
            engines.back()->setMessageCallback(on_message);
            if (d == 0) engines.back()->setProgressCallback(on_progress);
            RenderConfig c;
            c.deviceId = o.device + d; c.precision = prec; c.batchSize = o.batchSize; c.channels = 3; c.height = c.width = o.tileSize; c.scaling = o.scale;
            c.overlapX = c.overlapY = o.blend; c.tta = o.tta; c.ttaBugCompat = o.ttaMode == "reference";
            if (!engines.back()->load(modelPath, c)) return -1;
        }
        // --chain: the stages of a chained frame - engines[0], then the engine of the stages behind it (one engine, run chain - 1 times; engines[0] again
        // where --chain-noise is --noise).  Img2Img::renderChained* drive them; the frame stays on the device in between.
        std::unique_ptr<Img2Img> chainEngine;
        std::vector<Img2Img*> stages;
        if (o.chain > 1) {
            Img2Img* later = engines[0].get();
            if (cli::chain_model_path(o) != modelPath) {
                chainEngine.reset(new Img2Img);
                chainEngine->setMessageCallback(on_message);
                RenderConfig c;
                c.deviceId = o.device; c.precision = prec; c.batchSize = o.batchSize; c.channels = 3; c.height = c.width = o.tileSize; c.scaling = o.scale;
                c.overlapX = c.overlapY = o.blend; c.tta = o.tta; c.ttaBugCompat = o.ttaMode == "reference";
                if (!chainEngine->load(cli::chain_model_path(o), c)) return -1;
                later = chainEngine.get();
            }
            stages.push_back(engines[0].get());
            for (int k = 1; k < o.chain; ++k) stages.push_back(later);
        }
        ChainOptions chainOptions;
        chainOptions.quantize = o.chainQuantize;
        // --dither: a setting of the engines, so every route below - stills, --deep, --gray, the colour of alpha PNGs, every raw video format, --outscale /
        // --outsize - writes dithered samples without knowing about it; a video moves the pattern per frame with --dither-temporal.  dither_on(false) switches it
        // off around the one thing that must not be dithered and is rendered as a frame of its own: the alpha plane of the two-call routes.
        DitherOptions ditherOptions;
        ditherOptions.mode = o.dither == "ordered" ? Dither::Ordered : o.dither == "bluenoise" ? Dither::BlueNoise : Dither::None;
        ditherOptions.advance = o.ditherTemporal ? 1u : 0u;
        // --resize-light: a setting of the engines likewise - every route below that resizes (--outscale / --outsize) averages in that light.  Alpha is coverage
        // and is neither dithered nor decoded: dither_on(false) puts both settings back to their defaults around the alpha plane's own frame.
        const ResizeLight light = o.resizeLight == "srgb" ? ResizeLight::LinearSrgb : o.resizeLight == "bt709" ? ResizeLight::LinearBt709 : ResizeLight::Gamma;
        auto dither_on = [&](bool on) {
            for (auto& e : engines) if (!e->setDither(on ? ditherOptions : DitherOptions()) || !e->setResizeLight(on ? light : ResizeLight::Gamma)) return false;
            if (chainEngine && (!chainEngine->setDither(on ? ditherOptions : DitherOptions()) || !chainEngine->setResizeLight(on ? light : ResizeLight::Gamma))) return false;   // (the last stage's settings count)
            return true;
        };
        if (!dither_on(true)) return -1;
        // --edge: a setting of the engines likewise, and one that stays on for the alpha plane's own frame - every route below reads beyond the frame edge by it
        const EdgeMode edge = o.edge == "wrap" ? EdgeMode::Wrap : o.edge == "mirror" ? EdgeMode::Mirror : EdgeMode::Replicate;
        for (auto& e : engines) if (!e->setEdge(edge)) return -1;
        if (chainEngine && !chainEngine->setEdge(edge)) return -1;
        // --outscale (extension): every output lround(W * F) x lround(H * F), the network's output resized on the device; --outsize: every output W x H
        const ResizeFilter filter = o.resizeFilter == "bilinear" ? ResizeFilter::Bilinear : ResizeFilter::Bicubic;
        const bool resize = o.outscale > 0 || o.outsizeW > 0;
        // --outsize: an input the size cannot be reached from stops the run
        auto check_outsize = [&](const std::string& file, int w, int h) {
            const int total = cli::total_scale(o);
            const bool shrink_ok = o.chain <= 1 || ((long)o.outsizeW * 4 >= (long)w * total && (long)o.outsizeH * 4 >= (long)h * total);   // (the last stage of a chain shrinks by 4 at most)
            if (o.outsizeW <= 0 || (o.outsizeW >= w && o.outsizeW <= w * total && o.outsizeH >= h && o.outsizeH <= h * total && shrink_ok)) return;
            throw std::runtime_error(file + ": --outsize " + std::to_string(o.outsizeW) + "x" + std::to_string(o.outsizeH) + " cannot be reached from this " + std::to_string(w) + "x" +
                                     std::to_string(h) + " input: the output must lie between " + std::to_string(w) + "x" + std::to_string(h) + " and " + std::to_string(w * total) + "x" +
                                     std::to_string(h * total) + " (--scale " + std::to_string(o.scale) + (o.chain > 1 ? ", --chain " + std::to_string(o.chain) + ": and no less than a quarter of the latter" : "") + ")");
        };
        const std::vector<std::string> files = find_inputs(o);
        fileCount = files.size();
        for (const std::string& file : files) {
            if (cli::is_builtin_still(file)) {
                frameIndex = 0; frameCount = 1;
                cli::Bitmap in = cli::read_image(file, o.deep), out;
                check_outsize(file, in.cols, in.rows);
                out.rows = cli::out_dim(o, in.rows, false); out.cols = cli::out_dim(o, in.cols, true);
                if (resize && o.devices > 1) throw std::runtime_error(file + ": --outscale / --outsize render a still on one device (--devices 1)");
                const bool deep = !in.bgr16.empty();                   // --deep on a 16-bit PNG: CV_16UC3 through the engine (extension)
                // --gray on a gray PNG: one plane through renderGray / renderGrayResized and a gray PNG out; without the flag the file is the colour image it always was
                const bool gray_still = o.gray && in.gray && in.alpha.empty();
                Image src, dst;
                if (gray_still) {
                    // (no colour planes: the result is one plane, out.luma / out.luma16)
                } else if (deep) {
                    out.bgr16.resize((size_t)out.rows * out.cols * 3);
                    src = Image{(uint8_t*)in.bgr16.data(), in.rows, in.cols, (size_t)in.cols * 6, 16}; dst = Image{(uint8_t*)out.bgr16.data(), out.rows, out.cols, (size_t)out.cols * 6, 16};
                } else {
                    out.bgr.resize((size_t)out.rows * out.cols * 3);
                    src = Image{in.bgr.data(), in.rows, in.cols, (size_t)in.cols * 3}; dst = Image{out.bgr.data(), out.rows, out.cols, (size_t)out.cols * 3};
                }
                if (o.chain > 1 && !in.alpha.empty()) throw std::runtime_error(file + ": --chain renders no alpha channel (an RGBA chain is not built)");
                auto render_still = [&](const Image& s0, Image& d0) {
                    if (o.chain > 1) return resize ? Img2Img::renderChainedResized(stages.data(), o.chain, s0, d0, chainOptions, filter) : Img2Img::renderChained(stages.data(), o.chain, s0, d0, chainOptions);
                    if (resize) return engines[0]->renderResized(s0, d0, filter);
                    if (o.devices == 1) return engines[0]->render(s0, d0);
                    // every tile once: engine k takes the k-th contiguous range of the tile order, the seam bands travel device to device, each
                    // engine composes and downloads its own cells of the output (Img2Img::renderSharded).  16-bit frames and --split strips keep the
                    // tile-column strips (each engine on its own host thread, the seam column recomputed instead of exchanged).
                    if (s0.depth == 8 && o.split == "shards") {
                        std::vector<Img2Img*> es;
                        for (auto& e : engines) es.push_back(e.get());
                        return Img2Img::renderSharded(es.data(), (int)es.size(), s0, d0);
                    }
                    std::vector<std::thread> th; std::vector<char> oks(o.devices, 1);
                    for (int d = 0; d < o.devices; ++d) th.emplace_back([&, d] { Image s2 = s0, d2 = d0; oks[d] = engines[d]->renderStrip(s2, d2, d, o.devices); });
                    for (auto& t : th) t.join();
                    bool all = true;
                    for (char k : oks) all = all && k;
                    return all;
                };
                // an 8-bit still with alpha on one device: colour and alpha in one renderRgba() call, or one renderRgbaResized() call with --outscale / --outsize
                const bool one_call = !in.alpha.empty() && !deep && o.devices == 1;
                // one plane of `bps`-byte samples through the engine as a gray frame
                auto render_plane = [&](const void* plane, void* result, size_t bps) {
                    Image s1{(uint8_t*)const_cast<void*>(plane), in.rows, in.cols, (size_t)in.cols * bps, (int)(8 * bps)}, d1{(uint8_t*)result, out.rows, out.cols, (size_t)out.cols * bps, (int)(8 * bps)};
                    return resize ? engines[0]->renderGrayResized(s1, d1, filter) : engines[0]->renderGray(s1, d1);
                };
                if (gray_still) {      // the green samples of the (input-sized) frame as the plane; the result is the one-plane image write_image takes
                    const size_t n = (size_t)in.rows * in.cols, m = (size_t)out.rows * out.cols;
                    if (deep) {
                        std::vector<uint16_t> g(n);
                        for (size_t i = 0; i < n; ++i) g[i] = in.bgr16[3 * i + 1];
                        out.luma16.resize(m);
                        if (!render_plane(g.data(), out.luma16.data(), 2)) return -1;
                    } else {
                        std::vector<uint8_t> g(n);
                        for (size_t i = 0; i < n; ++i) g[i] = in.bgr[3 * i + 1];
                        out.luma.resize(m);
                        if (!render_plane(g.data(), out.luma.data(), 1)) return -1;
                    }
                } else if (one_call) {
                    std::vector<uint8_t> bgra((size_t)in.rows * in.cols * 4), obgra((size_t)out.rows * out.cols * 4);
                    for (size_t i = 0; i < in.alpha.size(); ++i) { bgra[4 * i] = in.bgr[3 * i]; bgra[4 * i + 1] = in.bgr[3 * i + 1]; bgra[4 * i + 2] = in.bgr[3 * i + 2]; bgra[4 * i + 3] = in.alpha[i]; }
                    Image s4{bgra.data(), in.rows, in.cols, (size_t)in.cols * 4}, d4{obgra.data(), out.rows, out.cols, (size_t)out.cols * 4};
                    RgbaOptions ro; ro.bleed = o.alphaBleed; ro.skipUniformAlpha = o.alphaSkipUniform;
                    if (!(resize ? engines[0]->renderRgbaResized(s4, d4, ro, filter) : engines[0]->renderRgba(s4, d4, ro))) return -1;
                    out.alpha.resize((size_t)out.rows * out.cols);
                    for (size_t i = 0; i < out.alpha.size(); ++i) { out.bgr[3 * i] = obgra[4 * i]; out.bgr[3 * i + 1] = obgra[4 * i + 1]; out.bgr[3 * i + 2] = obgra[4 * i + 2]; out.alpha[i] = obgra[4 * i + 3]; }
                } else {
                    // the two-call routes: --alpha-bleed spreads the visible colours on the host first (8-bit colour; the parser refuses it with --deep)
                    std::vector<uint8_t> bled;
                    if (!in.alpha.empty() && !deep && o.alphaBleed > 0) {
                        bled.resize(in.bgr.size());
                        if (!alpha_bleed(in.bgr.data(), (size_t)in.cols * 3, in.alpha.data(), (size_t)in.cols, in.rows, in.cols, o.alphaBleed, bled.data(), (size_t)in.cols * 3))
                            throw std::runtime_error(file + ": --alpha-bleed " + std::to_string(o.alphaBleed) + " could not be applied");
                        src.data = bled.data();
                    }
                    if (!render_still(src, dst)) return -1;
                }
                if (!in.alpha.empty() && !one_call && !dither_on(false)) return -1;   // alpha is never dithered: an opaque cut-out stays opaque
                if (!in.alpha.empty() && !one_call && o.devices == 1) {   // the alpha plane as a gray frame (renderGray: the green channel of render() of B = G = R = A)
                    out.alpha.resize((size_t)out.rows * out.cols);
                    if (!render_plane(in.alpha.data(), out.alpha.data(), 1)) return -1;
                } else if (!in.alpha.empty() && !one_call) {   // over several devices: the alpha plane as a gray image through the same engines; its green channel is the new alpha
                    cli::Bitmap ga, go;
                    // sized from the geometry: with --deep the colour planes live in bgr16 and in.bgr / out.bgr are empty
                    ga.rows = in.rows; ga.cols = in.cols; ga.bgr.resize((size_t)in.rows * in.cols * 3);
                    for (size_t i = 0; i < in.alpha.size(); ++i) ga.bgr[3 * i] = ga.bgr[3 * i + 1] = ga.bgr[3 * i + 2] = in.alpha[i];
                    go.bgr.resize((size_t)out.rows * out.cols * 3);
                    Image as{ga.bgr.data(), in.rows, in.cols, (size_t)in.cols * 3}, ad{go.bgr.data(), out.rows, out.cols, (size_t)out.cols * 3};
                    if (!render_still(as, ad)) return -1;
                    out.alpha.resize((size_t)out.rows * out.cols);
                    for (size_t i = 0; i < out.alpha.size(); ++i) out.alpha[i] = go.bgr[3 * i + 1];
                }
                if (!in.alpha.empty() && !one_call && !dither_on(true)) return -1;
                std::string outFile = cli::output_path(o, file, true);
                if (fs::path(file).extension() == ".bmp" || fs::path(file).extension() == ".BMP") outFile = fs::path(outFile).replace_extension(".bmp").string();   // built-in formats stay what they were, except ...
                if (fs::path(outFile).extension() == ".ppm") outFile = fs::path(outFile).replace_extension(".png").string();
                cli::write_image(outFile, out);
                ++frameIndex;
            } else {
                // a video (or a still in a format only ffmpeg reads): uncompressed AVI files through the built-in reader, the rest through ffmpeg
                std::unique_ptr<FrameSource> source; std::unique_ptr<FrameSink> sink;
                int width = 0, height = 0, frames = 1; double fps = 30.0;
                std::string why;
                auto avi = std::make_unique<AviSource>();
                const bool is_avi = fs::path(file).extension() == ".avi" || fs::path(file).extension() == ".AVI";
                bool yuv = false;                                      // --colorspace on a multi-frame input read through ffmpeg: YUV frames
                bool gray = false;                                     // --gray on an input read through ffmpeg: raw gray frames, one byte per pixel
                bool planar = false;                                   // --rgb-in / --rgb-out on a multi-frame input read through ffmpeg: raw planar RGB frames
                const bool alphaFrames = !o.rgbaIn.empty() || !o.rgbaOut.empty();   // --rgba-in / --rgba-out: the same with a fourth plane, A (gbrap*; one given: the other side is gbrap)
                const std::string rgbIn = alphaFrames ? (o.rgbaIn.empty() ? "gbrap" : o.rgbaIn) : o.rgbIn.empty() ? "gbrp" : o.rgbIn;
                const std::string rgbOut = alphaFrames ? (o.rgbaOut.empty() ? "gbrap" : o.rgbaOut) : o.rgbOut.empty() ? "gbrp" : o.rgbOut;
                const int rgbInBits = alphaFrames ? cli::rgba_format_bits(rgbIn) : cli::rgb_format_bits(rgbIn), rgbOutBits = alphaFrames ? cli::rgba_format_bits(rgbOut) : cli::rgb_format_bits(rgbOut);
                const int rgbPlanes = alphaFrames ? 4 : 3;
                auto plane_bytes = [](int rows, int cols, int bits) { return (size_t)rows * cols * (bits == 32 ? 4 : bits > 8 ? 2 : 1); };
                const std::string& rawIn = o.yuvIn.empty() ? o.pixFmt : o.yuvIn, & rawOut = o.yuvOut.empty() ? o.pixFmt : o.yuvOut;   // --yuv-in / --yuv-out
                const RawYuv fmtIn = raw_yuv(rawIn), fmtOut = raw_yuv(rawOut);
                if (is_avi && avi->rd.open(file, &why)) {
                    width = avi->rd.info().width; height = avi->rd.info().height; frames = avi->rd.info().frames; fps = avi->rd.info().fps;
                    source = std::move(avi);
                    if (o.gray) on_message(Severity::warn, file + ": the built-in AVI route is 24-bit only: --gray is ignored");
                    if (!o.rgbIn.empty() || !o.rgbOut.empty()) on_message(Severity::warn, file + ": the built-in AVI route is 24-bit only: --rgb-in / --rgb-out are ignored");
                    if (alphaFrames) on_message(Severity::warn, file + ": the built-in AVI route is 24-bit only: --rgba-in / --rgba-out are ignored");
                } else {
                    if (!have_ffmpeg) throw std::runtime_error(file + ": needs ffmpeg and ffprobe on PATH (built in: .png, .ppm, .bmp, uncompressed 24-bit .avi" + (why.empty() ? "" : "; " + why) +
                                                               (o.colorspace.empty() ? "" : "; --colorspace reads and writes YUV frames through ffmpeg only") + ")");
                    const Probe pr = ffprobe(file);
                    width = pr.width; height = pr.height; frames = pr.frames; fps = pr.fps;
                    yuv = !o.colorspace.empty() && frames != 1;
                    gray = o.gray && frames != 1;                      // (a single frame is a still in a format only ffmpeg reads: rendered in colour, as without the flag)
                    planar = (!o.rgbIn.empty() || !o.rgbOut.empty() || alphaFrames) && frames != 1;   // (a single frame: a still, rendered as bgr24 like any other)
                    const size_t inBytes = yuv ? yuv_frame_bytes(height, width, fmtIn) : planar ? rgbPlanes * plane_bytes(height, width, rgbInBits) : (size_t)width * height * (gray ? 1 : 3);
                    source.reset(new PipeSource("ffmpeg -v error -i " + shell_quote(file) + " -f rawvideo -pix_fmt " + (yuv ? rawIn : planar ? rgbIn : std::string(gray ? "gray" : "bgr24")) + " -", inBytes));
                }
                frameIndex = 0; frameCount = frames;
                const bool single = frames == 1;
                std::string outFile = cli::output_path(o, file, single);
                check_outsize(file, width, height);
                const int outW = cli::out_dim(o, width, true), outH = cli::out_dim(o, height, false);
                const size_t inBytes = yuv ? yuv_frame_bytes(height, width, fmtIn) : planar ? rgbPlanes * plane_bytes(height, width, rgbInBits) : (size_t)width * height * (gray ? 1 : 3);
                const size_t outBytes = yuv ? yuv_frame_bytes(outH, outW, fmtOut) : planar ? rgbPlanes * plane_bytes(outH, outW, rgbOutBits) : (size_t)outW * outH * (gray ? 1 : 3);
                if (have_ffmpeg) {
                    std::string wcmd = "ffmpeg -v error -y -f rawvideo -pix_fmt " + (yuv ? rawOut : planar ? rgbOut : std::string(gray ? "gray" : "bgr24")) + " -s " + std::to_string(outW) + "x" + std::to_string(outH) +
                                       " -r " + std::to_string(single ? 1.0 : fps) + " -i - ";
                    if (!single) wcmd += "-c:v " + o.codec + " -pix_fmt " + o.pixFmt + " -crf " + std::to_string(o.crf) + " ";
                    if (yuv) wcmd += colour_tags(o);
                    sink.reset(new PipeSink(wcmd + shell_quote(outFile), outBytes));
                } else {   // no encoder here: the upscaled stream as an uncompressed AVI
                    outFile = fs::path(outFile).replace_extension(".avi").string();
                    on_message(Severity::info, "ffmpeg is not on PATH: writing uncompressed video to " + outFile);
                    auto as = std::make_unique<AviSink>();
                    as->wr.open(outFile, outW, outH, fps);
                    sink = std::move(as);
                }
                RenderFrames render = [&](Img2Img& e, uint8_t* const* in, uint8_t* const* out, int n) {
                    std::vector<Image> si(n), di(n);
                    for (int k = 0; k < n; ++k) { si[k] = Image{in[k], height, width, (size_t)width * 3}; di[k] = Image{out[k], outH, outW, (size_t)outW * 3}; }
                    if (o.chain > 1) return resize ? Img2Img::renderSequenceChainedResized(stages.data(), o.chain, si.data(), di.data(), n, chainOptions, filter)
                                                   : Img2Img::renderSequenceChained(stages.data(), o.chain, si.data(), di.data(), n, chainOptions);
                    return resize ? e.renderSequenceResized(si.data(), di.data(), n, filter) : e.renderSequence(si.data(), di.data(), n);
                };
                if (gray) render = [&](Img2Img& e, uint8_t* const* in, uint8_t* const* out, int n) {
                    std::vector<Image> si(n), di(n);
                    for (int k = 0; k < n; ++k) { si[k] = Image{in[k], height, width, (size_t)width}; di[k] = Image{out[k], outH, outW, (size_t)outW}; }
                    return resize ? e.renderSequenceGrayResized(si.data(), di.data(), n, filter) : e.renderSequenceGray(si.data(), di.data(), n);
                };
                // a raw gbrp* frame is its planes G, B, R back to back, rows unpadded: PlanarImage wants R, G, B
                if (planar) render = [&](Img2Img& e, uint8_t* const* in, uint8_t* const* out, int n) {
                    std::vector<PlanarImage> si(n), di(n);
                    auto frame = [&](uint8_t* base, int rows, int cols, int bits) {
                        const size_t plane = plane_bytes(rows, cols, bits), step = plane / rows;
                        PlanarImage f;
                        f.rows = rows; f.cols = cols; f.bits = bits;
                        f.planes[0] = base + 2 * plane; f.planes[1] = base; f.planes[2] = base + plane;
                        f.steps[0] = f.steps[1] = f.steps[2] = step;
                        return f;
                    };
                    for (int k = 0; k < n; ++k) { si[k] = frame(in[k], height, width, rgbInBits); di[k] = frame(out[k], outH, outW, rgbOutBits); }
                    if (o.chain > 1) {      // (a chained planar sequence is not built: frame by frame)
                        for (int k = 0; k < n; ++k)
                            if (!(resize ? Img2Img::renderChainedPlanarResized(stages.data(), o.chain, si[k], di[k], chainOptions, filter) : Img2Img::renderChainedPlanar(stages.data(), o.chain, si[k], di[k], chainOptions))) return false;
                        return true;
                    }
                    return resize ? e.renderSequencePlanarResized(si.data(), di.data(), n, filter) : e.renderSequencePlanar(si.data(), di.data(), n);
                };
                // a raw gbrap* frame: G, B, R, A; PlanarRgbaImage wants R, G, B, A
                if (planar && alphaFrames) render = [&](Img2Img& e, uint8_t* const* in, uint8_t* const* out, int n) {
                    std::vector<PlanarRgbaImage> si(n), di(n);
                    auto frame = [&](uint8_t* base, int rows, int cols, int bits) {
                        const size_t plane = plane_bytes(rows, cols, bits), step = plane / rows;
                        PlanarRgbaImage f;
                        f.rows = rows; f.cols = cols; f.bits = bits;
                        f.planes[0] = base + 2 * plane; f.planes[1] = base; f.planes[2] = base + plane; f.planes[3] = base + 3 * plane;
                        f.steps[0] = f.steps[1] = f.steps[2] = f.steps[3] = step;
                        return f;
                    };
                    for (int k = 0; k < n; ++k) { si[k] = frame(in[k], height, width, rgbInBits); di[k] = frame(out[k], outH, outW, rgbOutBits); }
                    RgbaOptions ro; ro.bleed = o.alphaBleed; ro.skipUniformAlpha = o.alphaSkipUniform;
                    return resize ? e.renderSequencePlanarRgbaResized(si.data(), di.data(), n, ro, filter) : e.renderSequencePlanarRgba(si.data(), di.data(), n, ro);
                };
                if (yuv) {
                    YuvFormat f;
                    f.matrix = o.colorspace == "bt601" ? YuvMatrix::BT601 : o.colorspace == "bt2020" ? YuvMatrix::BT2020 : YuvMatrix::BT709;
                    f.range = o.colorRange == "pc" ? YuvRange::Full : YuvRange::Limited;
                    const YuvSiting siting = o.chromaLoc == "center" ? YuvSiting::Center : o.chromaLoc == "topleft" ? YuvSiting::TopLeft : YuvSiting::Left;   // --chroma-loc: both sides
                    render = [=](Img2Img& e, uint8_t* const* in, uint8_t* const* out, int n) {
                        std::vector<YuvImage> si(n), di(n);
                        for (int k = 0; k < n; ++k) { si[k] = packed_yuv(in[k], height, width, fmtIn); di[k] = packed_yuv(out[k], outH, outW, fmtOut); si[k].siting = di[k].siting = siting; }
                        return resize ? e.renderSequenceYuvResized(si.data(), di.data(), n, f, filter) : e.renderSequenceYuv(si.data(), di.data(), n, f);
                    };
                }
                const bool ok = run_frame_pipeline(engines, *source, *sink, inBytes, outBytes, render, [&](int n) { frameIndex += n; if (n) on_progress(1, 1, 0.0); });
                const bool closed = sink->close();
                if (!ok || !closed) return -1;
            }
            ++fileIndex;
        }
        return 0;
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return -1;
    }
}
