// Resize in linear light, host side: the modes, the two curves, their constants as the kernels get them and the host statement of the two functions.
// No HIP: it builds with plain g++ (make asan) and is what the tests state the device code against.
//
// The rule.  A curve is four constants (t, k, a, g):
//     decode(e) = e / k              for e < t,      else ((e + a) / (1 + a))^g
//     encode(l) = k l                for l < t / k,  else (1 + a) l^(1/g) - a
//     Srgb  (IEC 61966-2-1):                                  t = 0.04045,      k = 12.92, a = 0.055,        g = 2.4
//     Bt709 (the Rec.709 / BT.2020 camera curve, inverted):   t = 0.0812428583, k = 4.5,   a = 0.0992968268, g = 1 / 0.45
// Both have a linear toe, so encode's slope is bounded (12.92, 4.5).  With a curve set, a resized frame is
//     1. L = decode(sat01(canvas value)) per colour sample, where the canvas is written (once per canvas pixel, not once per tap);
//     2. the resize of L as it is: the same tap tables, tap order, tile and LDS layout;
//     3. V = encode(sat01(L')) where the kernels otherwise take sat01 / quantise;
//     4. everything behind that on V: quantisation, dither threshold, BGR packing, the Y'CbCr matrix, the chroma-site filters, the NV12 interleave.
// Alpha is coverage and is never decoded or encoded; float destinations hold V; decode(0) = 0, decode(1) = 1, encode(0) = 0, encode(1) = 1 exactly; at the
// scaled size a resized call is the plain call (no round trip); Gamma, the default, is the engine that was never told about any of this.
//
// The arithmetic in fp32, every rounding stated (light_decode / light_encode below; the device functions of prepost_device.h are the same statements with the
// hardware's log2 / exp2):
//     decode: e < t ? e * (1/k) : exp2(g * log2(fma(e - 1, 1/(1+a), 1)))      ((e + a) / (1 + a) = 1 + (e - 1) / (1 + a): exactly 1 at e = 1)
//     encode: l < t/k ? k * l   : fma(a, p - 1, p),  p = exp2((1/g) * log2(l))   ((1 + a) p - a = p + a (p - 1): exactly 1 at p = 1)
// The constants and their reciprocals are made in double and rounded to fp32 once (light_args).
#pragma once
#include <cmath>
#include <cstring>

namespace w2x {

constexpr int kLightGamma = 0, kLightSrgb = 1, kLightBt709 = 2;
inline bool light_mode_ok(int mode) { return mode >= kLightGamma && mode <= kLightBt709; }

// What a linear-light launch gets beside its parameters: the curve as data.  mode kLightGamma: nothing is decoded or encoded and no kernel takes the struct.
struct LightArgs {
    int mode = kLightGamma;
    float t = 0.f, inv_k = 0.f;                                      // decode: the toe's end on the encoded axis, 1 / k
    float inv_1a = 0.f, g = 0.f;                                     //         1 / (1 + a), the exponent
    float tl = 0.f, k = 0.f;                                         // encode: the toe's end on the linear axis (t / k), k
    float a = 0.f, inv_g = 0.f;                                      //         a, 1 / g
};
inline LightArgs light_args(int mode) {
    LightArgs l;
    if (mode != kLightSrgb && mode != kLightBt709) return l;
    const double t = mode == kLightSrgb ? 0.04045 : 0.0812428583, k = mode == kLightSrgb ? 12.92 : 4.5;
    const double a = mode == kLightSrgb ? 0.055 : 0.0992968268, g = mode == kLightSrgb ? 2.4 : 1.0 / 0.45;
    l.mode = mode;
    l.t = (float)t; l.inv_k = (float)(1.0 / k); l.inv_1a = (float)(1.0 / (1.0 + a)); l.g = (float)g;
    l.tl = (float)(t / k); l.k = (float)k; l.a = (float)a; l.inv_g = (float)(1.0 / g);
    return l;
}
inline bool light_args_ok(const LightArgs& l) { return light_mode_ok(l.mode); }

// the host statement of the two functions (e, l in [0, 1]; the callers clamp); Gamma: the identity
inline float light_decode(const LightArgs& c, float e) {
    if (c.mode == kLightGamma) return e;
    const float lin = e * c.inv_k;
    const float base = std::fmaf(e - 1.f, c.inv_1a, 1.f);
    const float pw = std::exp2(c.g * std::log2(base));
    return e < c.t ? lin : pw;
}
inline float light_encode(const LightArgs& c, float l) {
    if (c.mode == kLightGamma) return l;
    const float lin = c.k * l;
    const float p = std::exp2(c.inv_g * std::log2(l));
    const float pw = std::fmaf(c.a, p - 1.f, p);
    return l < c.tl ? lin : pw;
}

// "gamma" | "srgb" | "bt709" <-> the mode; parse: false for anything else (mode untouched); name: nullptr for an unknown mode
inline const char* light_mode_name(int mode) { return mode == kLightGamma ? "gamma" : mode == kLightSrgb ? "srgb" : mode == kLightBt709 ? "bt709" : nullptr; }
inline bool light_parse_mode(const char* name, int& mode) {
    if (!name) return false;
    for (int m = kLightGamma; m <= kLightBt709; ++m)
        if (std::strcmp(name, light_mode_name(m)) == 0) { mode = m; return true; }
    return false;
}

}  // namespace w2x
