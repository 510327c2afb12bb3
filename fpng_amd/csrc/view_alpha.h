// view_alpha.h -- the alpha stage of fpng_amd_decode_batch(_device)_{planar,hwc}_views_alpha (include/fpng_amd.h): what a view does
// with the fourth plane of a 4-channel file -- composite the colour planes over an opaque background, or resize them premultiplied
// as Pillow's Image.resize of an RGBA image does.  The rule of the resize is resize.h's, untouched; the stage sits in the LOAD of
// its horizontal pass and in the STORE of its vertical pass.  The three functions below are the ONE text of the rule: the resize
// kernels (resize.hip, resize_color.hip) run them per tap and per result, the host twins fpng_amd_view_alpha_source and
// fpng_amd_view_alpha_result (decode_api.cpp) run them per byte, and the CPU tests judge those against Pillow.
//
// All of it is integer arithmetic on bytes (v: a colour byte, a: the alpha byte of the same sample, b: a background byte):
//
//   M(v, a)    = t = v * a + 128;  ((t >> 8) + t) >> 8                         RGBA -> RGBa: Pillow's MULDIV255
//   U(v, a)    = a == 0 || a == 255 ? v : min(255, (255 * v) / a)              RGBa -> RGBA: truncating, clipped
//   C(v, a, b) = t = v * a + b * (255 - a) + 128;  ((t >> 8) + t) >> 8         over an opaque background (a == 0 gives b)
//
// P_0 .. P_3: the crop's planes (a 3-channel file: P_3 = 255, and every op is op 0).
//   load   COMPOSITE:     P'_c = C(P_c, P_3, background[c]) for c < 3, P'_3 = 255
//          PREMULTIPLIED: P'_c = M(P_c, P_3) for c < 3, P'_3 = P_3
//   resize R' = the window of P' resized, per plane, by the rule of resize.h
//   store  PREMULTIPLIED: R_c = U(R'_c, R'_3) for c < 3, R_3 = R'_3            (COMPOSITE, none: R = R')
#pragma once
#include "fpng_amd.h"
#include "resize.h"

namespace fpng_amd {

constexpr uint32_t kAlphaComposite = 1, kAlphaPremultiplied = 2; // FPNG_AMD_ALPHA_*

// where a view's alpha record travels: DecResize::flags, whose bit 0 is the mirror flag -- the op in bits 1 and 2, the background's
// R, G, B in bits 8 .. 31.  A record without an op leaves the word what it was
constexpr uint32_t kResizeAlphaShift = 1, kResizeAlphaBits = 3u << kResizeAlphaShift, kResizeBgShift = 8;
FPNG_RESIZE_FN uint32_t resize_alpha_op(uint32_t flags) { return flags >> kResizeAlphaShift & 3u; }
FPNG_RESIZE_FN uint32_t resize_alpha_bg(uint32_t flags, uint32_t plane) { return plane < 3u ? flags >> (kResizeBgShift + 8u * plane) & 255u : 0u; }
inline uint32_t resize_alpha_flags(const fpng_amd_view_alpha &p)
{
    return p.op ? p.op << kResizeAlphaShift | (uint32_t)p.background[0] << kResizeBgShift | (uint32_t)p.background[1] << (kResizeBgShift + 8) | (uint32_t)p.background[2] << (kResizeBgShift + 16) : 0u;
}

FPNG_RESIZE_FN uint32_t alpha_mul(uint32_t v, uint32_t a)
{
    const uint32_t t = v * a + 128u;
    return ((t >> 8) + t) >> 8;
}
FPNG_RESIZE_FN uint32_t alpha_unmul(uint32_t v, uint32_t a)
{
    if (a == 0u || a == 255u) return v;
    const uint32_t q = 255u * v / a;
    return q > 255u ? 255u : q;
}
FPNG_RESIZE_FN uint32_t alpha_over(uint32_t v, uint32_t a, uint32_t b)
{
    const uint32_t t = v * a + b * (255u - a) + 128u;
    return ((t >> 8) + t) >> 8;
}

// ---- the kernels' load.  What plane `plane` of a view with this op is made of: kAlphaLoadRaw its own bytes, kAlphaLoadOver C of
//      them, kAlphaLoadMul M of them, kAlphaLoad255 the constant 255.  Only Over and Mul read the alpha plane ----
constexpr uint32_t kAlphaLoadRaw = 0, kAlphaLoadOver = 1, kAlphaLoadMul = 2, kAlphaLoad255 = 3;
FPNG_RESIZE_FN uint32_t alpha_load_mode(uint32_t op, uint32_t plane)
{
    if (op == kAlphaComposite) return plane < 3u ? kAlphaLoadOver : kAlphaLoad255;
    return op == kAlphaPremultiplied && plane < 3u ? kAlphaLoadMul : kAlphaLoadRaw;
}

// one output sample of the horizontal pass: 2^21 + the sum over its `count` taps of P'[t] * K[t * stride].  s: the plane's bytes at
// the first tap, a: the alpha plane's at the same offset (read in the modes Over and Mul only), bg: the plane's background byte.
// The mode is the same for all of a workgroup's threads
FPNG_RESIZE_FN int32_t alpha_pass_sum(uint32_t mode, const uint8_t *s, const uint8_t *a, uint32_t bg, uint32_t count, const int32_t *K, uint32_t stride)
{
    int32_t sum = 1 << (kResizeBits - 1);
    if (mode == kAlphaLoadOver)
        for (uint32_t t = 0; t < count; t++) sum += (int32_t)alpha_over(s[t], a[t], bg) * K[t * stride];
    else if (mode == kAlphaLoadMul)
        for (uint32_t t = 0; t < count; t++) sum += (int32_t)alpha_mul(s[t], a[t]) * K[t * stride];
    else if (mode == kAlphaLoad255)
        for (uint32_t t = 0; t < count; t++) sum += 255 * K[t * stride];
    else
        for (uint32_t t = 0; t < count; t++) sum += (int32_t)s[t] * K[t * stride];
    return sum;
}

// ---- the host's judgement and twins ----
inline const char *check_alpha_record(const fpng_amd_view_alpha &p)
{
    if (p.op > kAlphaPremultiplied) return "unknown fpng_amd_view_alpha::op (FPNG_AMD_ALPHA_COMPOSITE, _PREMULTIPLIED)";
    if (p.reserved[0] | p.reserved[1]) return "fpng_amd_view_alpha::reserved must be 0";
    if (p.background[3]) return "fpng_amd_view_alpha::background[3] must be 0 (the background is opaque)";
    if (p.op != kAlphaComposite && (p.background[0] | p.background[1] | p.background[2])) return "fpng_amd_view_alpha::background must be 0 without FPNG_AMD_ALPHA_COMPOSITE";
    return nullptr;
}

// step 1 (source) or step 3 (result) of the rule over four planes of w x h bytes, one behind the other; op 0: a copy
inline int alpha_twin_checked(const fpng_amd_view_alpha *p, uint32_t w, uint32_t h, const uint8_t *in, uint8_t *out, bool result, const char **why)
{
    *why = !p || !in || !out || !w || !h ? "null alpha, in or out, or an empty view" : check_alpha_record(*p);
    if (!*why && (uint64_t)w * h > SIZE_MAX / 4) *why = "4 * w * h, the bytes of in and of out, must fit size_t";
    if (*why) return FPNG_AMD_ERR_INVALID_ARG;
    const size_t n = (size_t)w * h;
    for (size_t k = 0; k < n; k++) {
        const uint32_t a = in[3 * n + k];
        for (uint32_t c = 0; c < 3; c++) {
            const uint32_t v = in[c * n + k];
            out[c * n + k] = (uint8_t)(result ? (p->op == kAlphaPremultiplied ? alpha_unmul(v, a) : v)
                                              : p->op == kAlphaComposite     ? alpha_over(v, a, p->background[c])
                                              : p->op == kAlphaPremultiplied ? alpha_mul(v, a)
                                                                             : v);
        }
        out[3 * n + k] = (uint8_t)(!result && p->op == kAlphaComposite ? 255u : a);
    }
    return FPNG_AMD_OK;
}

} // namespace fpng_amd
