// The engine interface: drop-in for trt::Img2Img (/root/reference/src/tensorrt/img2img.h:14-50) with the same five
// public methods, the same bool + callback error convention (function-try-blocks that log "[func@line] msg" at
// severity `error` and return false: logger.h:8, logger.cpp:19-22), one instance = one GPU = one compute stream.
// cv::Mat is replaced by a (pointer, rows, cols, step) view of interleaved 8-bit BGR pixels.
#ifndef W2X_IMG2IMG_H
#define W2X_IMG2IMG_H

#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <string>

#include "config.h"

namespace w2x {

enum Severity { critical, error, warn, info, debug, trace };             // logger.h:11-18
using MessageCallback = std::function<void(Severity, const std::string&)>;  // logger.h:20
using ProgressCallback = std::function<void(int, int, double)>;             // logger.h:21  (current, total, it/s)

struct Image {          // stand-in for cv::Mat of type CV_8UC3
    uint8_t* data = nullptr;
    int rows = 0, cols = 0;
    size_t step = 0;    // bytes per row
    // Extension (alpha / 16-bit images are a TODO upstream, README.md:88): depth 16 = CV_16UC3, data points at uint16_t samples (BGR), step stays
    // in bytes.  render() / renderStrip() take 16-bit frames when src and dst agree: u16 -> x * float(1/65535) in, sat(rint(x * 65535)) out.
    int depth = 8;
};

// Extension: planar YUV 4:2:0 frames as ffmpeg's yuv420p / yuv420p10le lay them out (an AVFrame's data[0..2] / linesize[0..2]): a Y plane of
// rows x cols samples, U (Cb) and V (Cr) planes of ceil(rows/2) x ceil(cols/2); bits 8 (uint8 samples) or 10 (little-endian uint16 holding the low
// 10 bits); each plane has its own pointer and step in bytes.
// `siting` says where the chroma samples sit, per frame like layout and depth and independent for source and destination: Left (the default;
// MPEG-2, H.264: chroma (i, j) at luma x = 2j, y = 2i + 1/2), Center (JPEG, MJPEG, MPEG-1: x = 2j + 1/2, y = 2i + 1/2; AVCHROMA_LOC_CENTER) or TopLeft
// (BT.2020 / UHD: x = 2j, y = 2i; AVCHROMA_LOC_TOPLEFT).  Chroma is upsampled from and filtered onto that grid.  I422 has a column rule only (TopLeft is Left
// there), I444 none: both are accepted and give Left's bytes.
// `layout` picks one of four arrangements of the same samples: I420 is the above; I422 (yuv422p / yuv422p10le) has U and V of
// rows x ceil(cols/2), chroma row y co-sited with luma row y; I444 (yuv444p / yuv444p10le) has U and V of rows x cols; NV12 (nv12 / p010le) is I420
// with the chroma in ONE plane, planes[1], of ceil(rows/2) rows of 2 * ceil(cols/2) samples U, V, U, V, ... (planes[2] is ignored and may be null) - and
// at 10 bits it is P010: the code sits in the HIGH 10 bits of each uint16 (read v >> 6, written code << 6), in Y and in UV.
enum class YuvLayout { I420 = 0, I422 = 1, I444 = 2, NV12 = 3 };
enum class YuvSiting { Left = 0, Center = 1, TopLeft = 2 };
struct YuvImage {
    uint8_t* planes[3] = {nullptr, nullptr, nullptr};
    size_t steps[3] = {0, 0, 0};
    int rows = 0, cols = 0;
    int bits = 8;
    YuvLayout layout = YuvLayout::I420;
    YuvSiting siting = YuvSiting::Left;
};
// Extension: a planar RGB frame - three planes of rows x cols samples, each with its own pointer and step (bytes).  planes[0] = R, planes[1] = G,
// planes[2] = B (a gbrp AVFrame: data[2], data[0], data[1]); the order carries no meaning of its own, the caller orders the pointers.
// bits: 8 (uint8), 10 / 12 / 16 (little-endian uint16, the code in the LOW bits), 32 (IEEE float32, nominal [0, 1]); u16 / f32 samples aligned to their size.
struct PlanarImage {
    uint8_t* planes[3] = {nullptr, nullptr, nullptr};
    size_t steps[3] = {0, 0, 0};
    int rows = 0, cols = 0;
    int bits = 8;
};
// Extension: a planar RGBA frame - PlanarImage with a fourth plane: planes[0..3] = R, G, B, A (a gbrap AVFrame: data[2], data[0], data[1], data[3]),
// all of one sample type and size; alpha is straight (not premultiplied) and read like a colour sample.
struct PlanarRgbaImage {
    uint8_t* planes[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t steps[4] = {0, 0, 0, 0};
    int rows = 0, cols = 0;
    int bits = 8;
};
enum class YuvMatrix { BT601 = 0, BT709 = 1, BT2020 = 2 };   // (Kr, Kb) = (0.299, 0.114), (0.2126, 0.0722), (0.2627, 0.0593); BT.2020 non-constant luminance
enum class YuvRange { Limited = 0, Full = 1 };               // "tv": Y 16..235, C 16..240 (times 2^(bits-8)); "pc": 0 .. 2^bits - 1
struct YuvFormat {
    YuvMatrix matrix = YuvMatrix::BT709;
    YuvRange range = YuvRange::Limited;
};

// Extension: RGBA frames (renderRgba).  bleed: radius (0..16 pixels) over which the colours of the visible pixels (alpha > 0) are spread under
// the transparent ones before the network sees the frame; skipUniformAlpha: a frame whose alpha plane is one value keeps it and runs no alpha tiles.
struct RgbaOptions { int bleed = 0; bool skipUniformAlpha = false; };

// Extension: dithered output (setDither).  Without it every integer sample the engine writes is sat(rint(V)) of an fp32 value V; with it the sample
// (x, y) of plane c is min(max(floor(fl32(V + t)), 0), maxcode) with the threshold t = (rank + 0.5) / N of its position:
//   Ordered:   N = 64, rank from the recursive 8 x 8 Bayer matrix at ((x + dx) & 7, (y + dy) & 7);
//   BlueNoise: N = 4096, rank from a 64 x 64 void-and-cluster table at ((x + dx) & 63, (y + dy) & 63);
//   dx = 17 c + 23 phase, dy = 29 c + 41 phase; c: R, G, B = 0, 1, 2 whatever the memory order, a gray frame is plane 1, Y, U, V = 0, 1, 2; (x, y) absolute in the destination.
// Alpha is never dithered, float destinations are not touched, and a V that is an integer gives that integer.  Frame i of a sequence call is dithered as a
// single call at phase + i * advance would be: advance 0 keeps the pattern still (what encoders prefer), 1 is temporal dither.
enum class Dither { None = 0, Ordered = 1, BlueNoise = 2 };
struct DitherOptions { Dither mode = Dither::None; unsigned phase = 0; unsigned advance = 0; };

// Extension: chained renders (renderChained*).  quantize: the frame between two stages is rounded to the samples of the source's depth, which is what
// running the single calls one after the other gives; the default keeps it unrounded.
struct ChainOptions { bool quantize = false; };

class Img2Img {
public:
    Img2Img();
    virtual ~Img2Img();
    // img2img.h:18 - ONNX path in; writes <stem>_<sha256(cfg)[:16]>.{w2x,json} next to it (img2img_build.cpp:151-161)
    bool build(const std::string& path, const BuildConfig& config);
    // img2img.h:19 - the ONNX path again; the engine is found by scanning its directory (img2img_load.cpp:79-114)
    bool load(const std::string& path, const RenderConfig& config);
    // img2img.h:20 - dst must be rows*scaling x cols*scaling (caller pre-sizes it, main.cpp:234-235)
    bool render(const Image& src, Image& dst);
    // Extension: render() to any output size between the input and the scaled frame - dst.rows x dst.cols, each in [src dim, src dim * scaling] - through
    // an antialiased resize on the device (PIL's convolution resampler, as torch.nn.functional.interpolate(antialias=True) computes it) of the fp32 canvas
    // render() would quantise; 8- or 16-bit frames.  At dst = rows*scaling x cols*scaling the bytes are render()'s.  Other sizes: false (message callback).
    bool renderResized(const Image& src, Image& dst, ResizeFilter filter = ResizeFilter::Bicubic);
    // One device's share of a single frame spread over `parts` devices (tile-column strips): composes and writes only
    // the output columns of strip `part` (w2x_strip_plan); identical bytes to render() there.  render() == renderStrip(.., 0, 1).
    bool renderStrip(const Image& src, Image& dst, int part, int parts);
    // ONE frame over `count` engines with every tile computed exactly once (seam exchange): engine k runs the k-th of `count`
    // contiguous ranges of the reference's tile order (w2x_shard_plan), the blend bands of the ny + 1 tiles in front of a range are copied
    // from the engine(s) that computed them (device-to-device on one GPU, hipMemcpyPeerAsync / peer 2-D copies across GPUs, no collective),
    // and every engine composes and downloads the canvas cells of its own tiles.  All engines must be loaded with the same model and
    // RenderConfig, live in this process, and are driven from the calling thread; the bytes are render()'s.  engines[0] reports progress.
    static bool renderSharded(Img2Img* const* engines, int count, const Image& src, Image& dst);
    // The same with ONE PROCESS PER GPU (bench.py / torch.distributed.run ranks): rank r runs shardCompute(src, r, N) - its own tiles into its slab,
    // complete on return -, exports shardSlab() with ipc_export(), and once every rank has published its handle (the caller's barrier: the exchange
    // itself) shardFinish(dst, r, N, slabs, devices) with the ipc_open()ed slabs of the parts in front of it (entries of later / own parts are ignored):
    // seam bands copied device to device, its canvas cells composed and written to dst.
    bool shardCompute(const Image& src, int part, int parts);
    const void* shardSlab(size_t* bytes = nullptr) const;
    bool shardFinish(Image& dst, int part, int parts, const void* const* slabs, const int* devices);
    // A sequence of equally sized frames (the per-frame loop of main.cpp:263-269) with upload, compute and download overlapped on
    // three HIP streams; outputs are the bytes render() gives.  The copies only overlap for page-locked host memory: take the frame
    // buffers from allocHost() (owned by the engine, released by freeHost(), release at destruction at the latest).
    bool renderSequence(const Image* srcs, Image* dsts, int count);
    // renderSequence() with every frame resized like renderResized() to dsts[i].rows x dsts[i].cols (one size for the sequence; 8-bit frames)
    bool renderSequenceResized(const Image* srcs, Image* dsts, int count, ResizeFilter filter = ResizeFilter::Bicubic);
    // Extension: render() on YUV 4:2:0 frames.  The frame is converted to RGB on the device as it is read into tiles (chroma upsampled
    // to the luma grid, the matrix inverted, R, G, B clamped to [0, 1]: these values take the place of u8 * float(1/255)) and the canvas render()
    // would quantise is written back as YUV 4:2:0 at dst.bits (clamped to [0, 1], Y per pixel, chroma of the RGB filtered onto each chroma site).
    // src.bits and dst.bits are chosen independently (8 or 10); dst must be rows*scaling x cols*scaling.  Other arguments: false (message callback).
    // src.layout and dst.layout are independent too (nv12 in, yuv444p10le out): I444 chroma is read at the pixel and written per pixel without a
    // filter, I422 filters columns only (1/4, 1/2, 1/4), NV12 is I420's arithmetic on interleaved samples.  One layout per side for a sequence.
    bool renderYuv(const YuvImage& src, YuvImage& dst, YuvFormat format);
    // renderYuv() over a sequence of equally sized frames through the pipeline of renderSequence() (three plane copies per frame each way)
    bool renderSequenceYuv(const YuvImage* srcs, YuvImage* dsts, int count, YuvFormat format);
    // Extension: renderYuv() to any output size between the input and the scaled frame - dst.rows x dst.cols, each in [src dim, src dim * scaling],
    // the two independent, odd sizes allowed.  The frame is read as renderYuv() reads it, the fp32 canvas is formed and resized as renderResized() does it
    // (not clamped before the resize: the filter's overshoot is part of the result), and the resized RGB is encoded as renderYuv() encodes the canvas, at
    // dst.bits.  At dst = rows*scaling x cols*scaling the bytes are renderYuv()'s.  Other sizes and whatever renderYuv() refuses: false (message callback).
    // Every layout on either side, source and destination independent like the depths: the resized RGB is encoded as renderYuv() encodes the canvas for
    // dst.layout - I444 each pixel's own chroma, I422 the chroma filter along the row, NV12 / P010 I420's samples interleaved -, and the Y plane is the same
    // bytes whatever dst.layout is.
    bool renderYuvResized(const YuvImage& src, YuvImage& dst, YuvFormat format, ResizeFilter filter = ResizeFilter::Bicubic);
    // renderSequenceYuv() with every frame resized like renderYuvResized() to dsts[i].rows x dsts[i].cols (one size, one pair of depths and one pair of layouts
    // for the sequence)
    bool renderSequenceYuvResized(const YuvImage* srcs, YuvImage* dsts, int count, YuvFormat format, ResizeFilter filter = ResizeFilter::Bicubic);
    // Extension: render() on 8-bit interleaved BGRA frames (CV_8UC4, what cv::imread(IMREAD_UNCHANGED) hands out; step >= cols * 4; dst rows*scaling x
    // cols*scaling) in one call: one upload of 4 bytes per pixel, the colour bleed on the device, the frame's N colour tiles and N alpha tiles (the alpha plane
    // as the gray image B = G = R = A) as ONE schedule of 2N tiles - colour first, cut into batches and passes like render()'s N, so the progress callback
    // counts ceil(2N * steps / batchSize) batches -, one compose, one download of 4 bytes per output pixel.  Colour bytes: render() of alpha_bleed(BGR, A, bleed);
    // alpha bytes: the green channel of render() of the gray image.  skipUniformAlpha and min(A) == max(A) == v: no alpha tiles, every output alpha is v, the
    // progress total is the colour tiles' alone.  Other depths, empty images, short steps, other sizes, bleed outside [0, 16]: false (message callback).
    bool renderRgba(const Image& src, Image& dst, const RgbaOptions& opt = {});
    // renderRgba() with the output resized on the device to dst.rows x dst.cols, the targets and filters of renderResized() for 8-bit frames: each
    // dimension in [src dim, src dim * scaling], independently.  Colour bytes: renderResized() of alpha_bleed(BGR, A, bleed); alpha bytes: the green channel of
    // renderResized() of the gray image - resized separately and straight, not premultiplied.  At the scaled size it is renderRgba().
    bool renderRgbaResized(const Image& src, Image& dst, const RgbaOptions& opt = {}, ResizeFilter filter = ResizeFilter::Bicubic);
    // A sequence of equally sized BGRA frames with one set of options, upload / compute / download overlapped as in renderSequence() (page-locked buffers:
    // allocHost()); output i is the bytes of renderRgba() / renderRgbaResized() on frame i.  skipUniformAlpha is decided per frame.  No progress is reported.
    bool renderSequenceRgba(const Image* srcs, Image* dsts, int count, const RgbaOptions& opt = {});
    bool renderSequenceRgbaResized(const Image* srcs, Image* dsts, int count, const RgbaOptions& opt = {}, ResizeFilter filter = ResizeFilter::Bicubic);
    // Extension: gray frames.  The Image is read as ONE channel: step >= cols * (depth / 8), depth 8 or 16, dst rows*scaling x cols*scaling of the
    // same depth.  For rep(g) the BGR frame with B = G = R = g, renderGray(g) is the green channel of render(rep(g)), byte for byte, at 8 and at 16 bits - the rule
    // renderRgba() states for its alpha plane - with one upload and one download of a sample per pixel and nothing replicated on the host.  Progress counts
    // ceil(N * steps / batchSize) batches, as render().  Empty images, other or differing depths, short steps, other sizes: false (message callback).
    bool renderGray(const Image& src, Image& dst);
    // renderGray() resized on the device to dst.rows x dst.cols, the targets and filters of renderResized(): the green channel of renderResized(rep(g)), byte for
    // byte.  At the scaled size it is renderGray().
    bool renderGrayResized(const Image& src, Image& dst, ResizeFilter filter = ResizeFilter::Bicubic);
    // A sequence of equally sized 8-bit gray frames through renderSequence()'s pipeline (page-locked buffers: allocHost()); output i is the bytes of renderGray() /
    // renderGrayResized() on frame i.  16-bit frames and frames of differing sizes: false.  No progress is reported.
    bool renderSequenceGray(const Image* srcs, Image* dsts, int count);
    bool renderSequenceGrayResized(const Image* srcs, Image* dsts, int count, ResizeFilter filter = ResizeFilter::Bicubic);
    // Extension: planar RGB frames.  src.bits and dst.bits are independent (8 in and 10, 16 or float out is allowed).  The arithmetic is render()'s,
    // widened to the depths:
    //   in, integer:  the tile pixel is (r, g, b), each sample min(code, 2^bits - 1) * fl32(1 / (2^bits - 1)) - at 8 and 16 bits render()'s fl32(1/255) / fl32(1/65535);
    //   in, float:    min(max(x, 0), 1), NaN -> 0;
    //   out:          render()'s three sums per pixel (resized: renderResized()'s tap tables and tap order on the three canvas planes), then
    //                 integer sat(rint(x * (2^bits - 1))), float min(max(x, 0), 1) stored as fp32, never rounded to a code.
    // So at 8 / 8 bits renderPlanar() gives the planes of render() of the interleaved frame, byte for byte, at 16 / 16 bits those of the 16-bit render(); the same
    // holds for renderPlanarResized() against renderResized(); at the scaled size the resized call is the plain one; a sequence gives the bytes of the single calls.
    // The single calls report progress as render(): ceil(N * steps / batchSize) batches.  Other depths, empty frames, missing planes, short steps, misaligned
    // u16 / f32 samples, other sizes: false (message callback).
    bool renderPlanar(const PlanarImage& src, PlanarImage& dst);
    bool renderPlanarResized(const PlanarImage& src, PlanarImage& dst, ResizeFilter filter = ResizeFilter::Bicubic);
    // Planar frames through renderSequence()'s pipeline (page-locked buffers: allocHost()): every depth, one pair of depths and one size per sequence; three 2-D
    // copies per frame each way.  No progress is reported.
    bool renderSequencePlanar(const PlanarImage* srcs, PlanarImage* dsts, int count);
    bool renderSequencePlanarResized(const PlanarImage* srcs, PlanarImage* dsts, int count, ResizeFilter filter = ResizeFilter::Bicubic);
    // Extension: planar RGBA frames - renderRgba() on renderPlanar()'s samples: four planes R, G, B, A at 8, 10, 12, 16 bits or float on either side,
    // src.bits and dst.bits independent, one upload of four planes, the bleed on the device at every integer depth, ONE schedule of the frame's N colour tiles
    // and N alpha tiles (progress: ceil(2N * steps / batchSize) batches), one download of four planes.  Every sample, alpha included, is read as renderPlanar()
    // reads it; a pixel is visible iff its alpha sample read that way is > 0.  No tolerance anywhere:
    //   colour planes: renderPlanar() / renderPlanarResized() of alpha_bleed_planes((R, G, B), A, bleed) at the same depths, byte for byte (float: bit for bit);
    //   alpha plane:   the G plane of renderPlanar() / renderPlanarResized() of the frame (A, A, A) at the same depths (8 / 8 and 16 / 16 bits: renderGray(A));
    //   8 / 8 bits:    the four planes interleaved as B, G, R, A are the bytes of renderRgba() / renderRgbaResized() with the same options.
    // skipUniformAlpha and every alpha sample, read as above, one value v: no alpha tiles, every output alpha is sat(rint(v * (2^dst.bits - 1))) - float: v -, the
    // progress total is the colour tiles' alone.  At the scaled size a resized call is the plain one.  An integer frame and its float frame give the same
    // bytes wherever renderPlanar() gives them the same: not where the B or the A plane holds code 2047 or 4094 of 12 bits, 65455 or 65519 of 16.  Other depths, empty frames, missing planes, short steps,
    // misaligned u16 / f32 samples, other sizes, bleed outside [0, 16], bleed > 0 on float samples (a float bleed is not built): false (message callback).
    bool renderPlanarRgba(const PlanarRgbaImage& src, PlanarRgbaImage& dst, const RgbaOptions& opt = {});
    bool renderPlanarRgbaResized(const PlanarRgbaImage& src, PlanarRgbaImage& dst, const RgbaOptions& opt = {}, ResizeFilter filter = ResizeFilter::Bicubic);
    // Planar RGBA frames through renderSequence()'s pipeline (page-locked buffers: allocHost()): one size, one pair of depths and one set of options per sequence;
    // output i is the bytes of the single call on frame i, skipUniformAlpha decided per frame.  No progress is reported.
    bool renderSequencePlanarRgba(const PlanarRgbaImage* srcs, PlanarRgbaImage* dsts, int count, const RgbaOptions& opt = {});
    bool renderSequencePlanarRgbaResized(const PlanarRgbaImage* srcs, PlanarRgbaImage* dsts, int count, const RgbaOptions& opt = {}, ResizeFilter filter = ResizeFilter::Bicubic);
    // Extension: ONE frame through `count` engines one after the other - x4 from two x2 models, x8, x16 - with the frame staying on the device between
    // them.  count is 2, 3 or 4; the total factor is S, the product of the engines' scaling(); all engines are loaded, live in this process and share one device;
    // model, noise level, tile size, batch size, TTA, blend and precision may differ from stage to stage, and the same engine may appear more than once.  The
    // calling convention is renderSharded()'s: driven from the calling thread, engines[0] owns the message and progress callbacks and the chain's device buffers.
    // Stage 0 reads src as render() / renderPlanar() read it, stage k reads stage k - 1's output, the last stage writes dst as render() / renderResized() / the
    // planar calls write it: the LAST engine's setDither() and setResizeLight() apply, to the last stage only.  The frame between two stages:
    //   quantize = false: stage k's canvas clamped to [0, 1], unrounded, in the element type of the CONSUMING engine's tiles (fp16; TF32 / FP32 engines: fp32), the
    //                     consuming stage's tiles taken from it with gather's replicate padding and TTA maps.  This is the value chain of renderPlanar(dst.bits = 32)
    //                     followed by renderPlanar(src.bits = 32) - clamp, fp32, clamp, rounded to the tile type - so the bytes are that route's, bit for bit.
    //   quantize = true:  render()'s bytes at src.depth (planar: renderPlanar()'s at src.bits, an integer depth), read as render() reads a frame: the bytes of
    //                     calling the single calls one after the other.
    // renderChained: dst is rows * S x cols * S.  The resized calls: each dimension of dst in [src dim, src dim * S], the two independent, and at least a quarter
    // of the last stage's canvas (w2x_chain_plan holds the rules); the last stage's canvas is resized as renderResized() does it - so its own ratio may be below 1
    // (480 rows to 1080 through x2 x2 shrinks a canvas of 1920) -, and at the full size a resized call is the plain one.  No host synchronisation between the
    // stages: stage k's stream records an event stage k + 1's waits on.  A single call reports progress to engines[0]'s callback: total = the sum over the stages
    // of ceil(N * steps / batchSize), current = 1 .. total in stage order; the last stage of renderChained() runs in render()'s pipelined parts.  Sequences
    // (8-bit interleaved frames of one size, page-locked buffers: allocHost()) overlap upload, stages and download like renderSequence(), report nothing, and
    // output i is the bytes of the single call on frame i.  Refused (false through engines[0]'s message callback, nothing written): a count outside 2 .. 4, a null
    // or unloaded engine, engines on differing devices, a dst of another size, quantize on float planes, whatever the single calls refuse of src and dst.
    // Not built: YUV, RGBA and gray chains; strips, shards and several devices for a chained frame; planar sequences.
    static bool renderChained(Img2Img* const* engines, int count, const Image& src, Image& dst, const ChainOptions& opt = {});
    static bool renderChainedResized(Img2Img* const* engines, int count, const Image& src, Image& dst, const ChainOptions& opt = {}, ResizeFilter filter = ResizeFilter::Bicubic);
    static bool renderSequenceChained(Img2Img* const* engines, int count, const Image* srcs, Image* dsts, int n, const ChainOptions& opt = {});
    static bool renderSequenceChainedResized(Img2Img* const* engines, int count, const Image* srcs, Image* dsts, int n, const ChainOptions& opt = {}, ResizeFilter filter = ResizeFilter::Bicubic);
    static bool renderChainedPlanar(Img2Img* const* engines, int count, const PlanarImage& src, PlanarImage& dst, const ChainOptions& opt = {});
    static bool renderChainedPlanarResized(Img2Img* const* engines, int count, const PlanarImage& src, PlanarImage& dst, const ChainOptions& opt = {}, ResizeFilter filter = ResizeFilter::Bicubic);
    void* allocHost(size_t bytes);
    void freeHost(void* data);
    // Page-locks caller-owned memory in place.  Only whole pages are accepted (data and bytes multiples of 4096): a registration
    // covers whole pages, and buffers that share a page with other live data (heap blocks, neighbouring registrations) left stale
    // registrations behind on this runtime - a later copy from recycled addresses then aborted the process.
    bool pinHost(void* data, size_t bytes);
    void unpinHost(void* data);
    // Extension: the dither of every integer sample the following frame calls write (DitherOptions above).  A setting of the engine like the callbacks: allowed
    // before load(), kept across calls and loads, read by the very next frame.  An unknown mode: false (message callback), the previous setting stays.  The
    // default, Dither::None, is the undithered engine: the same kernels, the same bytes.  renderStrip / renderSharded / shardFinish keep their bytes equal to
    // render()'s (the threshold depends on absolute coordinates only; renderSharded refuses engines whose settings differ).  YUV frames: Y, U, V are
    // the plane indices 0, 1, 2, a chroma sample takes the coordinates of its own plane, NV12 / P010 those of the I420 samples they are.
    bool setDither(const DitherOptions& options);
    DitherOptions dither() const;
    // Extension: resize in linear light (config.h ResizeLight).  With LinearSrgb / LinearBt709 every following resized frame - render*Resized, the
    // resized sequences, every frame format - is L = decode(sat01(canvas)) per colour sample, the same resize of L, and V = encode(sat01(L')) where the kernels
    // otherwise clamp; quantisation, dither, packing, the Y'CbCr matrix and the chroma-site filters follow on V.  Alpha is coverage: never decoded, never encoded,
    // its bytes do not depend on the setting.  Float destinations hold V.  A resized call at the scaled size stays the plain call (no round trip).  A setting
    // of the engine like setDither: allowed before load(), kept across calls and loads, read by the very next frame; an unknown mode: false (message
    // callback), the previous setting stays.  Gamma, the default, is the engine that never heard of the setting: the same kernels, the same bytes.
    bool setResizeLight(ResizeLight mode);
    ResizeLight resizeLight() const;
    // Extension: edge modes (config.h EdgeMode).  With Wrap / Mirror every following frame call of the RGB family - render, gray, planar, RGBA, planar
    // RGBA, their resized calls and sequences, chains - takes what a tile, the colour bleed and the resize read beyond the frame edge through the mode's rule:
    //   tiles:   the gather's source index (the tile border may fold round a small frame more than once);
    //   bleed:   under Wrap a pixel's eight neighbours are taken through the rule - all eight exist, colour spreads across the joint; Mirror keeps Replicate's
    //            rule (a neighbour outside the frame does not exist: its reflection carries no new information);
    //   resize:  the taps are not cut off and renormalised at the border; every output sample has its full support, read through the rule.
    // Dither and linear light are per sample and do not know about it.  A chained render's stage gathers under its own engine's mode; the resize at its end is
    // the last engine's.  A setting of the engine like setDither: allowed before load(), kept across calls and loads, read by the very next frame (it is part
    // of the key of the captured passes); an unknown mode: false (message callback), the previous setting stays.  Replicate, the default, is the engine that never
    // heard of the setting: the same kernels, the same bytes.  Not built under Wrap / Mirror and refused by name (false, message callback, nothing written):
    // every YUV call, renderStrip, renderSharded, shardCompute and shardFinish.
    bool setEdge(EdgeMode mode);
    EdgeMode edge() const;
    void setMessageCallback(MessageCallback callback);   // img2img.h:21
    void setProgressCallback(ProgressCallback callback); // img2img.h:22

    // Test hook mirroring the private trt::Img2Img::infer (img2img.h:25, img2img_infer.cpp:41-93):
    // host NCHW f32 blob [B,3,T,T] in [0,1] -> [B,3,T',T'] f32.
    bool infer(const float* input, float* output);
    // Test hook: alpha_bleed_kernel alone - the BGRA frame up, the bleed at `radius`, the BGR frame gather would read down (bgr: rows x cols, step >= cols * 3)
    bool alphaBleed(const Image& bgra, Image& bgr, int radius);
    // Test hook: alpha_bleed_planes_kernel alone - the four planes up, the bleed at `radius`, the three colour planes gather would read down (colour: the size and
    // depth of src).  words (two, or null): the reduced alpha range, max(key) and max(top - key) (kernels.h AlphaBleedPlanesParams).
    bool alphaBleedPlanes(const PlanarRgbaImage& src, PlanarImage& colour, int radius, unsigned* words = nullptr);
    // Test hook: the dithered store alone - the planes of src (bits 32: fp32 values v, any number) up, every sample quantised from V = v * (2^bits - 1)
    // by the device function the compose and resample kernels store through, with the current setDither() options (None: sat(rint(V))), the planes of dst (8, 10,
    // 12 or 16 bits, the size of src) down.  Plane k has plane index k.  No network, no tiles.
    bool ditherPlanes(const PlanarImage& src, PlanarImage& dst);
    // Test hook: the resize of a resized frame alone - the three fp32 planes of src are taken as the canvas and go the production way: the decode of
    // the canvas kernels (their device function in a kernel of its own; Gamma: nothing), resample_planes_kernel, the store, under the current setResizeLight()
    // and setDither() settings, into the planes of dst (8 .. 16 bits or float; its size the target: between a quarter of src's and src's per axis).  No network,
    // no tiles.
    bool resizePlanes(const PlanarImage& src, PlanarImage& dst, ResizeFilter filter = ResizeFilter::Bicubic);
    int outputTileSize() const;
    int scaling() const;   // RenderConfig::scaling of the loaded configuration (0 before load)
    double planFlops() const;
    int passTiles() const;   // tiles carried by one network pass (batchSize x super-batch factor)
    // Steady-state device timing of the last render() (ms), HIP events on the compute stream.
    float lastRenderMs() const;
    // Re-run the device part of the last render() (gather, network, compose; no H2D/D2H) `iters` times and return the
    // average milliseconds per frame - inputs already resident in HBM (bench.py's timed region).
    float benchResident(int iters);
    // Copy the output frame the last benchResident() step left in HBM to dst (`bytes` = the scaled frame's size).
    bool residentOutput(void* dst, size_t bytes);
    // Per-kernel-family HIP-event timing of one resident frame (layout documented at the definition).
    bool profileFrame(double* out, int cap);
    int opTimes(double* out, int cap) const;   // ms per plan op of the last profileFrame(); returns the op count

    struct Impl;
private:
    bool renderPart(const Image& src, Image& dst, int part, int parts, const char* who, int resizeFilter = -1);   // resizeFilter >= 0: renderResized
    bool runSequence(const Image* srcs, Image* dsts, int count, int resizeFilter, const char* who);
    bool renderRgbaFrame(const Image& src, Image& dst, const RgbaOptions& opt, int resizeFilter, const char* who);   // resizeFilter >= 0: renderRgbaResized
    bool runSequenceRgba(const Image* srcs, Image* dsts, int count, const RgbaOptions& opt, int resizeFilter, const char* who);
    bool runGray(const Image* srcs, Image* dsts, int count, int resizeFilter, const char* who, bool single);   // single: renderGray / renderGrayResized (8 or 16 bits, progress)
    bool runPlanar(const PlanarImage* srcs, PlanarImage* dsts, int count, int resizeFilter, const char* who, bool single);   // single: renderPlanar / renderPlanarResized (progress)
    bool runPlanarRgba(const PlanarRgbaImage* srcs, PlanarRgbaImage* dsts, int count, const RgbaOptions& opt, int resizeFilter, const char* who, bool single);
    bool runSequenceYuv(const YuvImage* srcs, YuvImage* dsts, int count, YuvFormat format, int resizeFilter, const char* who);   // resizeFilter >= 0: renderYuvResized
    // the six chained calls: n frames, interleaved (srcs / dsts) or planar (psrcs / pdsts; the other pair null); single: one frame with progress
    static bool runChained(Img2Img* const* engines, int count, const Image* srcs, Image* dsts, const PlanarImage* psrcs, PlanarImage* pdsts, int n, const ChainOptions& opt,
                           int resizeFilter, const char* who, bool single);
    std::unique_ptr<Impl> impl;
};

// Device memory across processes (hipIpc*): export a device pointer of this process as a 64-byte handle; open another process's handle on logical device
// `deviceId` (nullptr on failure); close it again.
bool ipc_export(const void* device_ptr, uint8_t out[64]);
void* ipc_open(const uint8_t handle[64], int deviceId);
void ipc_close(void* p);
// PCI bus id of HIP device `deviceId` (the logical id RenderConfig::deviceId takes, W2X_DEVICE_MAP applied); false if there is no such device
bool device_pci_bus_id(int deviceId, char* buf, size_t cap);

}  // namespace w2x

#endif
