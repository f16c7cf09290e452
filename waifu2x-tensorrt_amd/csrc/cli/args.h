// Command line of the reference (src/main.cpp:18-153): global model options, exactly one of the subcommands
// `render` / `build`, options may appear before or after the subcommand (CLI11 "fallthrough").  Hand-written parser:
// no CLI11 in this tree.  Extensions are marked below.
#pragma once
#include <string>
#include <vector>

namespace w2x::cli {

struct Options {
    // global (main.cpp:25-84)
    std::string model;                    // cunet/art | swin_unet/art | swin_unet/art_scan | swin_unet/photo
    int scale = 0, noise = -2, batchSize = 0, tileSize = 0;
    int device = 0;
    std::string precision = "fp16";       // fp16 | tf32 (tf32 is rejected by build/load on gfx950, like platformHasTf32()==false)
    // subcommand
    std::string command;                  // "render" | "build" | "convert" (extension: image format conversion, no GPU)
    // render (main.cpp:86-139)
    std::vector<std::string> inputs;
    bool recursive = false;
    std::string output;                   // directory
    bool nosuffix = false;
    double blend = 1.0 / 16.0;
    bool tta = false;
    std::string codec = "libx264", pixFmt = "yuv420p";
    int crf = 23;
    // extensions
    int devices = 1;                      // --devices N: frames of a video round-robin, a single image as N tile ranges (--split)
    std::string split = "shards";         // --split {shards,strips}: how ONE image is spread over --devices N: shards = every tile once, seam bands exchanged
                                          // (Img2Img::renderSharded); strips = whole tile columns per device, the seam column recomputed (Img2Img::renderStrip)
    std::string models = "models";        // --models DIR: root of models/<model>/... (reference: fixed relative "models/")
    std::string ttaMode = "mean";         // --tta-mode {mean,reference}: mean = the true average of the 8 augmentations; reference = the bytes the
                                          // reference's accumulation produces (img2img_render.cpp:313-316) -> RenderConfig::ttaBugCompat
    bool deep = false;                    // --deep: 16-bit PNGs keep 16 bits per sample (read, rendered and written as CV_16UC3; default: cut to 8 like cv::imread)
    double outscale = 0;                  // --outscale F: output lround(W * F) x lround(H * F), F in [1, --scale]: the network's output resized on the device
                                          // (Img2Img::renderResized / renderSequenceResized); 0 = the network's own size, the reference's behaviour
    int outsizeW = 0, outsizeH = 0;       // --outsize WxH: every output exactly W x H, each input w x h with w <= W <= w * scale, h <= H <= h * scale (the two factors
                                          // independent): resized on the device like --outscale; with --colorspace through Img2Img::renderSequenceYuvResized; 0 = not given
    std::string resizeFilter = "bicubic"; // --resize-filter {bicubic,bilinear}: the antialiasing filter of --outscale / --outsize
    std::string edge = "replicate";       // --edge {replicate,wrap,mirror}: what tiles, the colour bleed and the resize read beyond the frame edge (Img2Img::setEdge)
    std::string resizeLight = "gamma";    // --resize-light {gamma,srgb,bt709}: the light --outscale / --outsize average in (Img2Img::setResizeLight)
    std::string colorspace;               // --colorspace {bt601,bt709,bt2020}: videos read through ffmpeg travel as raw --pix_fmt (yuv420p / yuv420p10le)
                                          // frames, converted on the GPU (Img2Img::renderSequenceYuv); "" = bgr24 frames, the reference's path
    std::string chromaLoc;                // --chroma-loc {left,center,topleft} (with --colorspace only): where the chroma samples of those frames sit, both for the frames read and
                                          // the frames written (YuvImage::siting); empty = not given (left)
    std::string colorRange = "tv";        // --color_range {tv,pc}: the range of those frames (with --colorspace only)
    std::string yuvIn, yuvOut;            // --yuv-in / --yuv-out FMT (with --colorspace only; kYuvFormats): the raw format asked of the ffmpeg reader / handed to the
                                          // writer, converted on the GPU in either direction (YuvImage::layout); "" = --pix_fmt, which with --yuv-out given is the
                                          // encoder's format alone (unrestricted, default the --yuv-out format)
    int alphaBleed = 0;                   // --alpha-bleed N (0..16): stills with an alpha channel: the colours of the visible pixels are spread N pixels under the
                                          // transparent ones before the network sees them (Img2Img::renderRgba, with --outscale / --outsize Img2Img::renderRgbaResized; on
                                          // the routes that render colour and alpha in two calls - --devices > 1 - the host alpha_bleed); 0 = the colours as stored
    bool alphaSkipUniform = false;        // --alpha-skip-uniform: a still whose alpha plane is one value keeps it without running the plane through the network
    bool gray = false;                    // --gray (extension, render only): gray PNGs and ffmpeg videos stay one channel (Img2Img::renderGray*)
    std::string rgbIn, rgbOut;            // --rgb-in / --rgb-out FMT (extension, render only; kRgbFormats): videos read through ffmpeg travel as raw planar RGB frames
                                          // of these formats (Img2Img::renderSequencePlanar*); with --rgb-out and no --pix_fmt the encoder's format is the --rgb-out one
    std::string dither = "none";          // --dither {none,ordered,bluenoise} (extension, render only): every integer sample the engine writes is dithered
                                          // (Img2Img::setDither) - stills, --deep, --gray, colour of alpha PNGs, every raw video format; alpha never
    bool ditherTemporal = false;          // --dither-temporal: videos move the pattern from frame to frame (DitherOptions::advance = 1); default: a still pattern
    std::string rgbaIn, rgbaOut;          // --rgba-in / --rgba-out FMT (extension, render only; kRgbaFormats): videos read through ffmpeg travel as raw planar RGBA frames
                                          // of these formats (Img2Img::renderSequencePlanarRgba*, with --alpha-bleed / --alpha-skip-uniform); the encoder's format as with --rgb-out
    int chain = 1;                        // --chain N (extension; 2..4): the frame goes through N engines one after the other on the GPU (Img2Img::renderChained*):
                                          // stage 1 is --model at --scale and --noise, the stages behind it --model at --scale and --chain-noise; 1 = not given
    int chainNoise = -1;                  // --chain-noise L [-1]: the noise level of the stages behind the first (-1: they only scale - the rule of waifu2x-caffe)
    bool chainQuantize = false;           // --chain-quantize: the frame between two stages is rounded to the samples of the input's depth (ChainOptions::quantize)
    bool printConfig = false;             // --print-config: dump the parsed options and derived names as JSON and exit (tests)
    bool help = false;
};

// the raw frame formats of --yuv-in / --yuv-out (ffmpeg's names): planar 4:2:0, 4:2:2, 4:4:4 at 8 / 10 bits, semi-planar 4:2:0 (nv12, 10 bits: p010le)
extern const char* const kYuvFormats[8];
// the raw formats of --rgb-in / --rgb-out (ffmpeg's planar RGB: planes G, B, R) and the bits of a sample of each (32: float); 0 for another name
extern const char* const kRgbFormats[5];
int rgb_format_bits(const std::string& name);
// the raw formats of --rgba-in / --rgba-out (ffmpeg's planar RGB with alpha: planes G, B, R, A) and the bits of a sample of each (32: float); 0 for another name
extern const char* const kRgbaFormats[5];
int rgba_format_bits(const std::string& name);
// throws std::runtime_error with the message to print (exit code -1 like main.cpp:147-150) on invalid input
Options parse(int argc, const char* const* argv);
std::string usage();

// models/<model>/[noiseN_][scaleSx].onnx  (main.cpp:201-204)
std::string model_path(const Options& o);
// the model of the stages of a --chain behind the first: --model at --scale and --chain-noise
std::string chain_model_path(const Options& o);
// the factor between input and network output: --scale, with --chain N its N-th power
int total_scale(const Options& o);
// "(model_with_underscores)(noiseN)(scaleS)(tta)"  (main.cpp:205-209); with --outscale F "(outscale<F as %g>)", with --outsize WxH "(WxH)" after (scaleS)
std::string output_suffix(const Options& o);
// output file name for one input (main.cpp:240-257): directory override, suffix, .png for stills / .mp4 for videos
std::string output_path(const Options& o, const std::string& input, bool single_frame);
std::string to_json(const Options& o);
// the output size of a `rows` x `cols` frame, one axis at a time (width: the columns): x scale, lround(x * outscale) with --outscale, W or H with --outsize
int out_dim(const Options& o, int dim, bool width);

}  // namespace w2x::cli
