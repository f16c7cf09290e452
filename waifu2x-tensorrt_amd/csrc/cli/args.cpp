#include "args.h"
#include "imageio.h"
#include "../light.h"
#include "../edge.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <sstream>
#include <stdexcept>

namespace w2x::cli {

namespace {

int to_int(const std::string& name, const std::string& v) {
    char* end = nullptr;
    long x = std::strtol(v.c_str(), &end, 10);
    if (v.empty() || *end) throw std::runtime_error(name + ": '" + v + "' is not an integer");
    return (int)x;
}

double to_double(const std::string& name, const std::string& v) {
    // accepts decimals and simple fractions ("1/16"), the way the README writes the blend choices
    auto slash = v.find('/');
    char* end = nullptr;
    if (slash != std::string::npos) {
        double a = std::strtod(v.substr(0, slash).c_str(), &end), b = std::strtod(v.substr(slash + 1).c_str(), nullptr);
        if (b == 0) throw std::runtime_error(name + ": bad fraction '" + v + "'");
        return a / b;
    }
    double x = std::strtod(v.c_str(), &end);
    if (v.empty() || *end) throw std::runtime_error(name + ": '" + v + "' is not a number");
    return x;
}

template <class T> void member(const std::string& name, const T& v, std::initializer_list<T> set) {
    if (std::find(set.begin(), set.end(), v) == set.end()) {
        std::ostringstream os; os << name << ": " << v << " not in {";
        bool first = true; for (const T& s : set) { os << (first ? "" : ",") << s; first = false; }
        os << "}";
        throw std::runtime_error(os.str());
    }
}

}  // namespace

std::string usage() {
    return "waifu2x (MI355X-native) - same command line as z3lx/waifu2x-tensorrt\n"
           "Usage: w2x [OPTIONS] SUBCOMMAND\n\n"
           "Options:\n"
           "  -h,--help                   Print this help message and exit\n"
           "  --model TEXT REQUIRED       {cunet/art,swin_unet/art,swin_unet/art_scan,swin_unet/photo}\n"
           "  --scale INT REQUIRED        {1,2,4}\n"
           "  --noise INT REQUIRED        {-1,0,1,2,3}\n"
           "  --batchSize INT REQUIRED    > 0\n"
           "  --tileSize INT REQUIRED     {64,128,256,400,640}\n"
           "  --device INT [0]            GPU device ID\n"
           "  --precision TEXT [fp16]     {fp16,tf32,fp32}\n"
           "  --devices INT [1]           (extension) number of GPUs: video frames round-robin, one image as N tile ranges\n"
           "  --split TEXT [shards]       (extension) {shards,strips}: one image over --devices N: every tile once with the seam bands exchanged / whole tile columns\n"
           "  --deep                      (extension) 16-bit PNGs keep 16 bits per sample through the engine and in the output\n"
           "  --models DIR [models]       (extension) root of the model directory tree\n\n"
           "Subcommands:\n"
           "  render                      Render image(s)/video(s)\n"
           "      -i,--input PATH ... REQUIRED   --recursive   -o,--output DIR   --nosuffix\n"
           "      --blend FLOAT [1/16] {1/8,1/16,1/32,0}   --tta   --codec TEXT [libx264]   --pix_fmt TEXT [yuv420p]   --crf INT [23] 0..51\n"
           "      --outscale FLOAT        (extension) output size = input size x FLOAT, 1 <= FLOAT <= --scale: the network output resized on the GPU\n"
           "      --outsize WxH           (extension) every output exactly W x H; each input w x h needs w <= W <= w x --scale, h <= H <= h x --scale\n"
           "                              (the two factors independent); works with --colorspace: YUV frames are resized on the GPU before they are encoded\n"
           "      --resize-filter TEXT [bicubic]  (extension) {bicubic,bilinear}: the antialiasing filter of --outscale / --outsize\n"
           "      --resize-light TEXT [gamma]  (extension) {gamma,srgb,bt709}: the light --outscale / --outsize average in - gamma: the encoded values as they are;\n"
           "                              srgb, bt709: the frame is decoded by that transfer curve, resized in linear light and encoded again (thin lines and fine\n"
           "                              texture keep their brightness).  Alpha is never touched.  Every route that takes --outscale / --outsize honours it\n"
           "      --edge TEXT [replicate] (extension) {replicate,wrap,mirror}: what lies beyond the frame edge - replicate: the edge pixel repeated; wrap: the frame\n"
           "                              is one period of a texture that tiles (seamless textures); mirror: reflection.  Stills with and without alpha, --gray,\n"
           "                              --rgb-in/out, --rgba-in/out, bgr24 video, --outscale / --outsize and --chain honour it; not with --colorspace\n"
           "      --colorspace TEXT       (extension) {bt601,bt709,bt2020}: videos read through ffmpeg stay YUV 4:2:0 at --pix_fmt\n"
           "                              (yuv420p or yuv420p10le) and are converted on the GPU; the output carries the colour tags\n"
           "      --color_range TEXT [tv] (extension) {tv,pc}: the range of the --colorspace frames\n"
           "      --chroma-loc TEXT [left] (extension) with --colorspace: {left,center,topleft}, where the chroma samples of the frames sit (left: MPEG-2 / H.264,\n"
           "                              center: JPEG / MJPEG / MPEG-1, topleft: BT.2020 / UHD); chroma is resampled on that grid both ways and the writer is\n"
           "                              handed -chroma_sample_location\n"
           "      --yuv-in FMT            (extension) with --colorspace: the raw format asked of the ffmpeg reader [--pix_fmt], one of\n"
           "                              {yuv420p,yuv420p10le,yuv422p,yuv422p10le,yuv444p,yuv444p10le,nv12,p010le}; converted on the GPU\n"
           "      --yuv-out FMT           (extension) with --colorspace: the raw format handed to the writer [--pix_fmt], same choices; --pix_fmt is then\n"
           "                              the encoder's format only (any, default FMT); neither option works with --outsize\n"
           "      --alpha-bleed INT [0]   (extension) 0..16: stills with an alpha channel: spread the colours of the visible pixels that many pixels under the\n"
           "                              transparent ones before upscaling (no dark fringe on cut-outs); not with --deep\n"
           "      --alpha-skip-uniform    (extension) a still whose alpha channel is one value (an opaque export) keeps it without running it through the network\n"
           "      --gray                  (extension) gray PNGs (colour type 0, 8- or 16-bit with --deep) stay one channel: one sample per pixel to the GPU and back,\n"
           "                              a gray PNG out; videos read through ffmpeg travel as raw gray frames.  Colour files, single images in formats\n"
           "                              only ffmpeg reads (JPEG ...) and gray + alpha PNGs (colour type 4: written as RGBA) are rendered as without it.  Not with --colorspace, not with --devices above 1\n"
           "      --rgb-in FMT, --rgb-out FMT\n"
           "                              (extension) {gbrp,gbrp10le,gbrp12le,gbrp16le,gbrpf32le}: videos read through ffmpeg travel as raw planar RGB frames of these\n"
           "                              formats, 8 to 16 bits or float in, any of them out (one given: the other side is gbrp); --outscale / --outsize apply.\n"
           "                              With --rgb-out and no --pix_fmt the encoder's format is the --rgb-out one.  Stills, single frames read through ffmpeg and\n"
           "                              the built-in AVI route are rendered as without them.  Not with --colorspace, not with --gray\n"
           "      --rgba-in FMT, --rgba-out FMT\n"
           "                              (extension) {gbrap,gbrap10le,gbrap12le,gbrap16le,gbrapf32le}: videos with an alpha channel read through ffmpeg travel as raw\n"
           "                              planar RGBA frames of these formats (one given: the other side is gbrap), colour and alpha rendered in one call per frame;\n"
           "                              --alpha-bleed (not on gbrapf32le input) and --alpha-skip-uniform apply to them, as do --outscale / --outsize and --devices.\n"
           "                              With --rgba-out and no --pix_fmt the encoder's format is the --rgba-out one.  Stills, single frames read through ffmpeg\n"
           "                              and the built-in AVI route are rendered as without them.  Not with --colorspace, --gray, --rgb-in or --rgb-out\n"
           "      --chain INT             (extension) {2,3,4}: the frame goes through INT engines one after the other on the GPU - x4 from a x2 model, x8, x16 - the\n"
           "                              first --model at --scale and --noise, the others --model at --scale and --chain-noise; --outscale / --outsize then range\n"
           "                              up to scale^INT (and down to a quarter of it).  Stills without alpha and videos as bgr24 or --rgb-in / --rgb-out frames, on one\n"
           "                              device.  Not with --colorspace, --gray, --rgba-in / --rgba-out, --alpha-bleed or --devices.  build: builds every stage's engine\n"
           "      --chain-noise INT [-1]  (extension) {-1,0,1,2,3}: the noise level of the stages behind the first; -1: they only scale\n"
           "      --chain-quantize        (extension) round the frame between two stages to the input's depth: the bytes of running the tool INT times\n"
           "      --dither TEXT [none]    (extension) {none,ordered,bluenoise}: dither every 8- to 16-bit sample written instead of rounding it - an 8 x 8 Bayer\n"
           "                              matrix or a 64 x 64 blue-noise table, on the GPU where the unrounded value is; smooth gradients leave without bands.\n"
           "                              Alpha and float output are never dithered.  Every route honours it\n"
           "      --dither-temporal       (extension) with --dither: videos move the pattern from frame to frame (default: the same pattern on every frame,\n"
           "                              which encoders prefer)\n"
           "      --tta-mode TEXT [mean]  (extension) {mean,reference}: with --tta, `mean` averages the 8 augmentations; `reference`\n"
           "                              reproduces the bytes of the reference's accumulation (img2img_render.cpp:313-316); --tta-compat = reference\n"
           "  build                       Build model\n"
           "  convert -i IN -o OUT        (extension) re-encode one still image (png/ppm), no GPU\n";
}

const char* const kYuvFormats[8] = {"yuv420p", "yuv420p10le", "yuv422p", "yuv422p10le", "yuv444p", "yuv444p10le", "nv12", "p010le"};

const char* const kRgbFormats[5] = {"gbrp", "gbrp10le", "gbrp12le", "gbrp16le", "gbrpf32le"};
int rgb_format_bits(const std::string& name) {
    const int bits[5] = {8, 10, 12, 16, 32};
    for (int k = 0; k < 5; ++k) if (name == kRgbFormats[k]) return bits[k];
    return 0;
}

const char* const kRgbaFormats[5] = {"gbrap", "gbrap10le", "gbrap12le", "gbrap16le", "gbrapf32le"};
int rgba_format_bits(const std::string& name) {
    const int bits[5] = {8, 10, 12, 16, 32};
    for (int k = 0; k < 5; ++k) if (name == kRgbaFormats[k]) return bits[k];
    return 0;
}

Options parse(int argc, const char* const* argv) {
    Options o;
    std::vector<std::string> a(argv + 1, argv + argc);
    bool seen_model = false, seen_scale = false, seen_noise = false, seen_batch = false, seen_tile = false, seen_outscale = false, seen_outsize = false, seen_filter = false, seen_colorspace = false, seen_range = false, seen_bleed = false, seen_skip = false, seen_pixfmt = false, seen_gray = false, seen_dither = false, seen_light = false, seen_edge = false, seen_chain = false, seen_chain_noise = false;
    auto value = [&](size_t& i) -> std::string {
        const std::string name = a[i];
        auto eq = name.find('=');
        if (name.rfind("--", 0) == 0 && eq != std::string::npos) { std::string v = name.substr(eq + 1); a[i] = name.substr(0, eq); return v; }
        if (i + 1 >= a.size()) throw std::runtime_error(name + ": 1 required value missing");
        return a[++i];
    };
    for (size_t i = 0; i < a.size(); ++i) {
        std::string k = a[i];
        if (k.rfind("--", 0) == 0 && k.find('=') != std::string::npos) k = k.substr(0, k.find('='));
        if (k == "-h" || k == "--help") { o.help = true; return o; }
        else if (k == "render" || k == "build" || k == "convert") {
            if (!o.command.empty()) throw std::runtime_error("Exactly 1 subcommand is required");
            o.command = k;
        }
        else if (k == "--model") { o.model = value(i); seen_model = true; }
        else if (k == "--scale") { o.scale = to_int(k, value(i)); seen_scale = true; }
        else if (k == "--noise") { o.noise = to_int(k, value(i)); seen_noise = true; }
        else if (k == "--batchSize") { o.batchSize = to_int(k, value(i)); seen_batch = true; }
        else if (k == "--tileSize") { o.tileSize = to_int(k, value(i)); seen_tile = true; }
        else if (k == "--device") o.device = to_int(k, value(i));
        else if (k == "--devices") o.devices = to_int(k, value(i));
        else if (k == "--split") o.split = value(i);
        else if (k == "--models") o.models = value(i);
        else if (k == "--precision") { o.precision = value(i); std::transform(o.precision.begin(), o.precision.end(), o.precision.begin(), ::tolower); }
        else if (k == "--print-config") o.printConfig = true;
        else if (k == "--deep") o.deep = true;
        else if (k == "-i" || k == "--input") {
            o.inputs.push_back(value(i));
            while (i + 1 < a.size() && a[i + 1].rfind("-", 0) != 0 && a[i + 1] != "render" && a[i + 1] != "build" && a[i + 1] != "convert") o.inputs.push_back(a[++i]);
        }
        else if (k == "--recursive") o.recursive = true;
        else if (k == "-o" || k == "--output") o.output = value(i);
        else if (k == "--nosuffix") o.nosuffix = true;
        else if (k == "--blend") o.blend = to_double(k, value(i));
        else if (k == "--tta") o.tta = true;
        else if (k == "--tta-mode") { o.ttaMode = value(i); std::transform(o.ttaMode.begin(), o.ttaMode.end(), o.ttaMode.begin(), ::tolower); }
        else if (k == "--tta-compat") o.ttaMode = "reference";
        else if (k == "--codec") o.codec = value(i);
        else if (k == "--pix_fmt") { o.pixFmt = value(i); seen_pixfmt = true; }
        else if (k == "--crf") o.crf = to_int(k, value(i));
        else if (k == "--outscale") { o.outscale = to_double(k, value(i)); seen_outscale = true; }
        else if (k == "--outsize") {
            const std::string v = value(i);
            int n = 0;
            if (std::sscanf(v.c_str(), "%dx%d%n", &o.outsizeW, &o.outsizeH, &n) != 2 || (size_t)n != v.size() || v.find_first_not_of("0123456789x") != std::string::npos)
                throw std::runtime_error("--outsize: '" + v + "' is not WxH (two positive integers)");
            if (o.outsizeW <= 0 || o.outsizeH <= 0) throw std::runtime_error("--outsize: " + v + ": width and height must be positive");
            seen_outsize = true;
        }
        else if (k == "--alpha-bleed") { o.alphaBleed = to_int(k, value(i)); seen_bleed = true; }
        else if (k == "--alpha-skip-uniform") { o.alphaSkipUniform = true; seen_skip = true; }
        else if (k == "--gray") { o.gray = true; seen_gray = true; }
        else if (k == "--chain") { o.chain = to_int(k, value(i)); seen_chain = true; }
        else if (k == "--chain-noise") { o.chainNoise = to_int(k, value(i)); seen_chain_noise = true; }
        else if (k == "--chain-quantize") o.chainQuantize = true;
        else if (k == "--dither") { o.dither = value(i); std::transform(o.dither.begin(), o.dither.end(), o.dither.begin(), ::tolower); seen_dither = true; }
        else if (k == "--dither-temporal") { o.ditherTemporal = true; seen_dither = true; }
        else if (k == "--edge") { o.edge = value(i); std::transform(o.edge.begin(), o.edge.end(), o.edge.begin(), ::tolower); seen_edge = true; }
        else if (k == "--resize-light") { o.resizeLight = value(i); std::transform(o.resizeLight.begin(), o.resizeLight.end(), o.resizeLight.begin(), ::tolower); seen_light = true; }
        else if (k == "--resize-filter") { o.resizeFilter = value(i); std::transform(o.resizeFilter.begin(), o.resizeFilter.end(), o.resizeFilter.begin(), ::tolower); seen_filter = true; }
        else if (k == "--colorspace") { o.colorspace = value(i); std::transform(o.colorspace.begin(), o.colorspace.end(), o.colorspace.begin(), ::tolower); seen_colorspace = true; }
        else if (k == "--color_range") { o.colorRange = value(i); std::transform(o.colorRange.begin(), o.colorRange.end(), o.colorRange.begin(), ::tolower); seen_range = true; }
        else if (k == "--chroma-loc") { o.chromaLoc = value(i); std::transform(o.chromaLoc.begin(), o.chromaLoc.end(), o.chromaLoc.begin(), ::tolower); }
        else if (k == "--yuv-in") o.yuvIn = value(i);
        else if (k == "--yuv-out") o.yuvOut = value(i);
        else if (k == "--rgb-in") o.rgbIn = value(i);
        else if (k == "--rgb-out") o.rgbOut = value(i);
        else if (k == "--rgba-in") o.rgbaIn = value(i);
        else if (k == "--rgba-out") o.rgbaOut = value(i);
        else throw std::runtime_error("The following argument was not expected: " + a[i]);
    }
    if (o.command.empty()) throw std::runtime_error("A subcommand is required");
    if (o.command == "convert") {
        if (o.inputs.size() != 1 || o.output.empty()) throw std::runtime_error("convert: exactly one -i and one -o are required");
        return o;
    }
    if (!seen_model) throw std::runtime_error("--model is required");
    if (!seen_scale) throw std::runtime_error("--scale is required");
    if (!seen_noise) throw std::runtime_error("--noise is required");
    if (!seen_batch) throw std::runtime_error("--batchSize is required");
    if (!seen_tile) throw std::runtime_error("--tileSize is required");
    member<std::string>("--model", o.model, {"cunet/art", "swin_unet/art", "swin_unet/art_scan", "swin_unet/photo"});
    member("--scale", o.scale, {1, 2, 4});
    member("--noise", o.noise, {-1, 0, 1, 2, 3});
    if (o.batchSize <= 0) throw std::runtime_error("--batchSize: number must be positive");
    member("--tileSize", o.tileSize, {64, 128, 256, 400, 640});
    if (o.device < 0) throw std::runtime_error("--device: number must be non-negative");
    if (o.devices < 1) throw std::runtime_error("--devices: number must be positive");
    member<std::string>("--split", o.split, {"shards", "strips"});
    member<std::string>("--precision", o.precision, {"fp16", "tf32", "fp32"});   // fp32: an addition (include/w2x/config.h)
    // --chain (extension): N stages of --model at --scale; the stages behind the first take --chain-noise
    if (seen_chain) {
        member("--chain", o.chain, {2, 3, 4});
        member("--chain-noise", o.chainNoise, {-1, 0, 1, 2, 3});
        if (o.command == "render" || o.command == "build") {
            if (o.scale == 1) throw std::runtime_error("--chain: needs --scale 2 or 4 (a chain of scale 1 stages leaves the size as it is)");
        }
        if (o.devices > 1) throw std::runtime_error("--chain: not with --devices " + std::to_string(o.devices) + " (a chained frame is rendered on one device)");
    } else if (seen_chain_noise || o.chainQuantize) throw std::runtime_error(std::string(seen_chain_noise ? "--chain-noise" : "--chain-quantize") + ": needs --chain");
    const bool seen_yuv_in = !o.yuvIn.empty(), seen_yuv_out = !o.yuvOut.empty(), seen_loc = !o.chromaLoc.empty();
    const bool seen_rgb_in = !o.rgbIn.empty(), seen_rgb_out = !o.rgbOut.empty();
    const bool seen_rgba_in = !o.rgbaIn.empty(), seen_rgba_out = !o.rgbaOut.empty();
    if (o.command == "render") {
        if (o.inputs.empty()) throw std::runtime_error("--input is required");
        for (const auto& p : o.inputs) if (!std::filesystem::exists(p)) throw std::runtime_error("--input: Path does not exist: " + p);
        if (!o.output.empty() && !std::filesystem::is_directory(o.output)) throw std::runtime_error("--output: Directory does not exist: " + o.output);
        const double choices[] = {1.0 / 8.0, 1.0 / 16.0, 1.0 / 32.0, 0.0};
        if (std::none_of(std::begin(choices), std::end(choices), [&](double c) { return c == o.blend; })) throw std::runtime_error("--blend: not in {1/8,1/16,1/32,0}");
        if (o.crf < 0 || o.crf > 51) throw std::runtime_error("--crf: Value not in range 0 to 51");
        member<std::string>("--tta-mode", o.ttaMode, {"mean", "reference"});
        if (o.ttaMode == "reference" && !o.tta) throw std::runtime_error("--tta-mode reference: needs --tta");
        if (seen_outscale) {
            if (!(o.outscale >= 1.0 && o.outscale <= total_scale(o))) {
                std::ostringstream os; os << "--outscale: " << o.outscale << " not in [1, " << total_scale(o) << "] (the output is a downsample of the --scale network's)";
                throw std::runtime_error(os.str());
            }
            if (seen_chain && o.outscale * 4 < total_scale(o)) {
                std::ostringstream os; os << "--outscale: " << o.outscale << " is below a quarter of the chain's factor " << total_scale(o) << " (the last stage's output shrinks by 4 at most)";
                throw std::runtime_error(os.str());
            }
            member<std::string>("--resize-filter", o.resizeFilter, {"bicubic", "bilinear"});
            if (o.devices > 1)
                for (const auto& p : o.inputs)
                    if (!std::filesystem::is_directory(p) && is_builtin_still(p)) throw std::runtime_error("--outscale: a still over --devices " + std::to_string(o.devices) + " is not supported: " + p);
        } else if (seen_outsize) {
            member<std::string>("--resize-filter", o.resizeFilter, {"bicubic", "bilinear"});
            if (o.devices > 1)
                for (const auto& p : o.inputs)
                    if (!std::filesystem::is_directory(p) && is_builtin_still(p)) throw std::runtime_error("--outsize: a still over --devices " + std::to_string(o.devices) + " is not supported: " + p);
        } else if (seen_filter) throw std::runtime_error("--resize-filter: needs --outscale or --outsize");
        if (seen_light) {                                                 // (a setting of the resize like the filter: every route that resizes honours it)
            if (!seen_outscale && !seen_outsize) throw std::runtime_error("--resize-light: needs --outscale or --outsize");
            int light_mode = 0;
            if (!light_parse_mode(o.resizeLight.c_str(), light_mode)) member<std::string>("--resize-light", o.resizeLight, {"gamma", "srgb", "bt709"});
        }
        if (seen_edge) {                                                  // (a setting of the engines: every route of the RGB family honours it)
            int edge_mode = 0;
            if (!edge_parse_mode(o.edge.c_str(), edge_mode)) member<std::string>("--edge", o.edge, {"replicate", "wrap", "mirror"});
            if (seen_colorspace) throw std::runtime_error("--edge: not together with --colorspace (YUV frames under an edge mode are not built)");
            if (edge_mode != kEdgeReplicate && o.devices > 1)
                for (const auto& p : o.inputs)
                    if (!std::filesystem::is_directory(p) && is_builtin_still(p)) throw std::runtime_error("--edge " + o.edge + ": a still over --devices " + std::to_string(o.devices) + " is not supported (strips and shards under an edge mode are not built): " + p);
        }
        if (seen_outscale && seen_outsize) throw std::runtime_error("--outsize: not together with --outscale (one of a factor and a size)");
        if (seen_colorspace) {
            member<std::string>("--colorspace", o.colorspace, {"bt601", "bt709", "bt2020"});
            member<std::string>("--color_range", o.colorRange, {"tv", "pc"});
            if (seen_loc) member<std::string>("--chroma-loc", o.chromaLoc, {"left", "center", "topleft"});
            for (const char* opt : {"--yuv-in", "--yuv-out"}) {
                const std::string& v = opt[6] == 'i' ? o.yuvIn : o.yuvOut;
                if (v.empty()) continue;
                member<std::string>(opt, v, {kYuvFormats[0], kYuvFormats[1], kYuvFormats[2], kYuvFormats[3], kYuvFormats[4], kYuvFormats[5], kYuvFormats[6], kYuvFormats[7]});
                if (seen_outsize) throw std::runtime_error(std::string(opt) + ": not together with --outsize (resized YUV output is yuv420p / yuv420p10le at --pix_fmt)");
            }
            if (seen_yuv_out) { if (!seen_pixfmt) o.pixFmt = o.yuvOut; }   // --pix_fmt is the encoder's format only
            else if (o.pixFmt != "yuv420p" && o.pixFmt != "yuv420p10le") throw std::runtime_error("--pix_fmt: with --colorspace one of {yuv420p,yuv420p10le}, got " + o.pixFmt);
            if (seen_outscale) throw std::runtime_error("--colorspace: not together with --outscale (a factor rarely gives the even sizes video wants: use --outsize WxH)");
        } else if (seen_range) throw std::runtime_error("--color_range: needs --colorspace");
        else if (seen_yuv_in || seen_yuv_out) throw std::runtime_error(std::string(seen_yuv_in ? "--yuv-in" : "--yuv-out") + ": needs --colorspace");
        else if (seen_loc) throw std::runtime_error("--chroma-loc: needs --colorspace");
        if (seen_gray) {
            if (seen_colorspace) throw std::runtime_error("--gray: not together with --colorspace (gray frames carry no chroma)");
            if (o.devices > 1) throw std::runtime_error("--gray: not with --devices " + std::to_string(o.devices) + " (gray frames are rendered on one device)");
        }
        for (const char* opt : {"--rgb-in", "--rgb-out"}) {
            const std::string& v = opt[6] == 'i' ? o.rgbIn : o.rgbOut;
            if (v.empty()) continue;
            member<std::string>(opt, v, {kRgbFormats[0], kRgbFormats[1], kRgbFormats[2], kRgbFormats[3], kRgbFormats[4]});
            if (seen_colorspace) throw std::runtime_error(std::string(opt) + ": not together with --colorspace (planar RGB frames are not converted to YUV)");
            if (seen_gray) throw std::runtime_error(std::string(opt) + ": not together with --gray (one raw frame format per run)");
        }
        if (seen_rgb_out && !seen_pixfmt) o.pixFmt = o.rgbOut;   // --pix_fmt is the encoder's format only
        for (const char* opt : {"--rgba-in", "--rgba-out"}) {
            const std::string& v = opt[7] == 'i' ? o.rgbaIn : o.rgbaOut;
            if (v.empty()) continue;
            member<std::string>(opt, v, {kRgbaFormats[0], kRgbaFormats[1], kRgbaFormats[2], kRgbaFormats[3], kRgbaFormats[4]});
            if (seen_colorspace) throw std::runtime_error(std::string(opt) + ": not together with --colorspace (planar RGBA frames are not converted to YUV)");
            if (seen_gray) throw std::runtime_error(std::string(opt) + ": not together with --gray (one raw frame format per run)");
            if (seen_rgb_in || seen_rgb_out) throw std::runtime_error(std::string(opt) + ": not together with " + (seen_rgb_in ? "--rgb-in" : "--rgb-out") + " (one raw frame format per run)");
        }
        if (seen_rgba_out && !seen_pixfmt) o.pixFmt = o.rgbaOut;
        if (seen_chain) {      // chained frames are interleaved or planar RGB on one device
            if (seen_colorspace) throw std::runtime_error("--chain: not together with --colorspace (a YUV chain is not built)");
            if (seen_gray) throw std::runtime_error("--chain: not together with --gray (a gray chain is not built)");
            if (seen_rgba_in || seen_rgba_out) throw std::runtime_error(std::string("--chain: not together with ") + (seen_rgba_in ? "--rgba-in" : "--rgba-out") + " (an RGBA chain is not built)");
            if (seen_bleed || seen_skip) throw std::runtime_error(std::string("--chain: not together with ") + (seen_bleed ? "--alpha-bleed" : "--alpha-skip-uniform") + " (an RGBA chain is not built)");
        }
        if (seen_dither) {
            member<std::string>("--dither", o.dither, {"none", "ordered", "bluenoise"});
            if (o.ditherTemporal && o.dither == "none") throw std::runtime_error("--dither-temporal: needs --dither ordered or --dither bluenoise");
        }
        if (seen_bleed) {
            if (!(o.alphaBleed >= 0 && o.alphaBleed <= 16)) throw std::runtime_error("--alpha-bleed: " + std::to_string(o.alphaBleed) + " not in [0, 16] (the radius in pixels)");
            if (o.alphaBleed > 0 && o.rgbaIn == kRgbaFormats[4]) throw std::runtime_error("--alpha-bleed: not together with --rgba-in " + o.rgbaIn + " (the bleed takes integer samples)");
            if (o.alphaBleed > 0 && o.deep) throw std::runtime_error("--alpha-bleed: not together with --deep (the bleed works on 8-bit colour; 16-bit stills keep the colours as stored)");
        }
    } else if (seen_dither) throw std::runtime_error(std::string(o.ditherTemporal ? "--dither-temporal" : "--dither") + ": only with render");
    else if (seen_light) throw std::runtime_error("--resize-light: only with render");
    else if (seen_edge) throw std::runtime_error("--edge: only with render");
    else if (seen_gray) throw std::runtime_error("--gray: only with render");
    else if (seen_rgb_in || seen_rgb_out) throw std::runtime_error(std::string(seen_rgb_in ? "--rgb-in" : "--rgb-out") + ": only with render");
    else if (seen_rgba_in || seen_rgba_out) throw std::runtime_error(std::string(seen_rgba_in ? "--rgba-in" : "--rgba-out") + ": only with render");
    else if (seen_outscale || seen_outsize || seen_filter || seen_colorspace || seen_range || seen_bleed || seen_skip || seen_yuv_in || seen_yuv_out || seen_loc)
        throw std::runtime_error(std::string(seen_loc ? "--chroma-loc" : seen_yuv_in ? "--yuv-in" : seen_yuv_out ? "--yuv-out" : seen_outscale ? "--outscale" : seen_outsize ? "--outsize" : seen_filter ? "--resize-filter" : seen_colorspace ? "--colorspace" :
                                             seen_range ? "--color_range" : seen_bleed ? "--alpha-bleed" : "--alpha-skip-uniform") + ": only with render");
    // cross-checks, main.cpp:142-145
    if (o.model == "cunet/art" && o.scale == 4) throw std::runtime_error("cunet/art does not support scale factor 4.");
    if (o.noise == -1 && o.scale == 1) throw std::runtime_error("Noise level -1 does not support scale factor 1.");
    return o;
}

static std::string model_file(const Options& o, int noise) {
    return o.models + "/" + o.model + "/" + (noise == -1 ? "" : "noise" + std::to_string(noise) + "_") +
           (o.scale == 1 ? "" : "scale" + std::to_string(o.scale) + "x") + ".onnx";
}
std::string model_path(const Options& o) { return model_file(o, o.noise); }
std::string chain_model_path(const Options& o) { return model_file(o, o.chainNoise); }
int total_scale(const Options& o) {
    int s = o.scale;
    for (int k = 1; k < o.chain; ++k) s *= o.scale;
    return s;
}

static std::string outscale_tag(const Options& o) {
    if (o.outsizeW > 0) return "(" + std::to_string(o.outsizeW) + "x" + std::to_string(o.outsizeH) + ")";
    if (o.outscale <= 0) return "";
    char buf[64]; std::snprintf(buf, sizeof buf, "(outscale%g)", o.outscale);
    return buf;
}

std::string output_suffix(const Options& o) {
    std::string m = o.model;
    std::replace(m.begin(), m.end(), '/', '_');
    return "(" + m + ")" + (o.noise == -1 ? "" : "(noise" + std::to_string(o.noise) + ")") +
           (o.scale == 1 ? "" : "(scale" + std::to_string(o.scale) + ")") + (o.chain > 1 ? "(chain" + std::to_string(o.chain) + ")" : "") + outscale_tag(o) + (o.tta ? "(tta)" : "");
}

int out_dim(const Options& o, int dim, bool width) {
    if (o.outsizeW > 0) return width ? o.outsizeW : o.outsizeH;
    return o.outscale > 0 ? (int)std::lround(dim * o.outscale) : dim * total_scale(o);
}

std::string output_path(const Options& o, const std::string& input, bool single_frame) {
    namespace fs = std::filesystem;
    fs::path file(input);
    if (!o.output.empty()) file = fs::path(o.output) / file.filename();
    if (!o.nosuffix) file.replace_filename(file.stem().string() + output_suffix(o) + file.extension().string());
    file.replace_extension(single_frame ? ".png" : ".mp4");
    return file.string();
}

std::string to_json(const Options& o) {
    auto q = [](const std::string& s) { std::string r = "\""; for (char c : s) { if (c == '"' || c == '\\') r += '\\'; r += c; } return r + "\""; };
    std::ostringstream os;
    os << "{\"command\": " << q(o.command) << ", \"model\": " << q(o.model) << ", \"scale\": " << o.scale << ", \"noise\": " << o.noise
       << ", \"batchSize\": " << o.batchSize << ", \"tileSize\": " << o.tileSize << ", \"device\": " << o.device << ", \"devices\": " << o.devices << ", \"split\": " << q(o.split)
       << ", \"precision\": " << q(o.precision) << ", \"recursive\": " << (o.recursive ? "true" : "false") << ", \"output\": " << q(o.output)
       << ", \"nosuffix\": " << (o.nosuffix ? "true" : "false") << ", \"blend\": " << o.blend << ", \"tta\": " << (o.tta ? "true" : "false") << ", \"tta_mode\": " << q(o.ttaMode)
       << ", \"outscale\": " << (o.outscale > 0 ? std::to_string(o.outscale) : std::string("null")) << ", \"outsize\": " << (o.outsizeW > 0 ? "[" + std::to_string(o.outsizeW) + ", " + std::to_string(o.outsizeH) + "]" : std::string("null"))
       << ", \"resize_filter\": " << q(o.resizeFilter) << ", \"resize_light\": " << q(o.resizeLight) << ", \"edge\": " << q(o.edge)
       << ", \"colorspace\": " << (o.colorspace.empty() ? std::string("null") : q(o.colorspace)) << ", \"color_range\": " << q(o.colorRange)
       << ", \"chroma_loc\": " << (o.chromaLoc.empty() ? std::string("null") : q(o.chromaLoc))
       << ", \"yuv_in\": " << (o.yuvIn.empty() ? std::string("null") : q(o.yuvIn)) << ", \"yuv_out\": " << (o.yuvOut.empty() ? std::string("null") : q(o.yuvOut))
       << ", \"alpha_bleed\": " << o.alphaBleed << ", \"alpha_skip_uniform\": " << (o.alphaSkipUniform ? "true" : "false") << ", \"gray\": " << (o.gray ? "true" : "false")
       << ", \"rgb_in\": " << (o.rgbIn.empty() ? std::string("null") : q(o.rgbIn)) << ", \"rgb_out\": " << (o.rgbOut.empty() ? std::string("null") : q(o.rgbOut))
       << ", \"rgba_in\": " << (o.rgbaIn.empty() ? std::string("null") : q(o.rgbaIn)) << ", \"rgba_out\": " << (o.rgbaOut.empty() ? std::string("null") : q(o.rgbaOut))
       << ", \"chain\": " << o.chain << ", \"chain_noise\": " << o.chainNoise << ", \"chain_quantize\": " << (o.chainQuantize ? "true" : "false")
       << ", \"chain_model_path\": " << (o.chain > 1 ? q(chain_model_path(o)) : std::string("null"))
       << ", \"dither\": " << q(o.dither) << ", \"dither_temporal\": " << (o.ditherTemporal ? "true" : "false")
       << ", \"codec\": " << q(o.codec) << ", \"pix_fmt\": " << q(o.pixFmt) << ", \"crf\": " << o.crf << ", \"inputs\": [";
    for (size_t i = 0; i < o.inputs.size(); ++i) os << (i ? ", " : "") << q(o.inputs[i]);
    os << "], \"model_path\": " << q(o.command == "convert" ? "" : model_path(o)) << ", \"suffix\": " << q(o.command == "convert" ? "" : output_suffix(o)) << ", \"outputs\": [";
    if (o.command == "render") for (size_t i = 0; i < o.inputs.size(); ++i) os << (i ? ", " : "") << q(output_path(o, o.inputs[i], true));
    os << "]}";
    return os.str();
}

}  // namespace w2x::cli
