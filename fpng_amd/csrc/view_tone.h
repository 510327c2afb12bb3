// view_tone.h -- the tone record of fpng_amd_decode_batch(_device)_planar_views_tone and _hwc_views_tone (include/fpng_amd.h: the
// rule): AutoContrast, Equalize and Contrast as RandAugment / TrivialAugment / AutoAugment apply them to a PIL image --
// ImageOps.autocontrast(img), ImageOps.equalize(img), ImageEnhance.Contrast(img).enhance(factor) -- each a statistic of the WHOLE view
// (its 256-bin histograms), a 256-entry table per channel and a point operation.  The stage sits behind the colour matrix and the
// warp and in front of the blur, solarize and posterize.  The pieces below are the ONE text, run by dec_view_tone_lut_kernel
// (view_tone.hip) for the tables and by the host functions fpng_amd_view_tone_lut / fpng_amd_view_tone_apply (decode_api.cpp) that the
// CPU tests judge against Pillow and an exact restatement.
//
//   W: the view's un-mirrored uint8 window as the post stage loads it -- B of view_post.h without a warp, the warp's gathered bytes
//      (fill samples included, as Pillow sees them after transform) with one.  Planes 0, 1, 2 only: a fourth one skips the stage.
//   h_c[v], c = 0, 1, 2: the count of byte v in plane c of W;  h_L[v]: the count of L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16,
//      Pillow's convert("L") (contrast only).  Counts are uint32: the host refuses a tone view whose w * h does not fit.
//   AUTOCONTRAST (cutoff 0), per channel: lo, hi the first and last v with h_c[v] > 0; hi <= lo: the identity; else in IEEE double,
//      NO contraction: scale = 255.0 / (hi - lo), offset = -lo * scale, lut[v] = clamp((int)(v * scale + offset), 0, 255), the cast
//      truncating toward zero.
//   EQUALIZE, per channel, in 64-bit integers: fewer than two non-zero bins: the identity; step = (sum h_c - h_c[last non-zero]) / 255,
//      floored; 0: the identity; else n = step / 2 and for v = 0 .. 255: lut[v] = min(255, n / step), n += h_c[v].  (The min is real:
//      Pillow clips the list it hands to point().)
//   CONTRAST with an fp32 factor, finite and >= 0: mean = (2 sum v h_L[v] + N) / (2 N), floored, N = w h -- Pillow's
//      int(sum / count + 0.5); all three channels share one table, in fp32 with EVERY operation rounded on its own:
//          t = (float)mean + factor * (float)((int)v - (int)mean)
//          0 <= factor <= 1: lut[v] = (uint8)t, truncating (t lies between mean and v);  else 0 if t <= 0, 255 if t >= 255, (uint8)t between.
//      This is Pillow's ImagingBlend of the solid mean image and the view as an x86-64 build computes it (separate fp32 multiply
//      and add; an aarch64 build may fuse them and differ in rare ties -- not offered).
//   W'_c = lut_c[W_c]; the blur, solarize, posterize, conversion, mirror and store proceed on W'.
#pragma once
#include "fpng_amd.h"
#include "resize.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace fpng_amd {

constexpr uint32_t kToneAutocontrast = 1u, kToneEqualize = 2u, kToneContrast = 3u; // FPNG_AMD_TONE_*
// a tone view's part of the decode scratch: uint32 h[4][256] (R, G, B, L), then uint8 lut[3][256]
constexpr uint32_t kToneHistWords = 4 * 256, kToneLutBytes = 3 * 256, kToneBytes = kToneHistWords * 4 + kToneLutBytes;

// Pillow's convert("L") of one pixel
FPNG_RESIZE_FN uint32_t tone_luma(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16; }

// AUTOCONTRAST: entry v of a channel whose first and last non-zero bins are lo and hi
FPNG_RESIZE_FN uint32_t tone_autocontrast_entry(uint32_t v, uint32_t lo, uint32_t hi)
{
#pragma clang fp contract(off)
    if (hi <= lo) return v;
    const double scale = 255.0 / (double)(hi - lo), offset = -(double)lo * scale;
    const int32_t ix = (int32_t)((double)v * scale + offset); // (within +-65025)
    return (uint32_t)(ix < 0 ? 0 : ix > 255 ? 255 : ix);
}

// EQUALIZE: the step of a channel of `bins` non-zero bins, `total` samples and `last` in the last non-zero bin; 0: the identity
FPNG_RESIZE_FN uint64_t tone_equalize_step(uint64_t total, uint64_t last, uint32_t bins) { return bins < 2 ? 0u : (total - last) / 255u; }
// entry v: before = h[0] + .. + h[v - 1]
FPNG_RESIZE_FN uint32_t tone_equalize_entry(uint32_t v, uint64_t before, uint64_t step)
{
    if (!step) return v;
    const uint64_t q = (step / 2 + before) / step;
    return (uint32_t)(q > 255u ? 255u : q);
}

// CONTRAST: the mean of L from sum = sum v h_L[v] and n = w h samples (n >= 1; 2 sum + n < 2^42)
FPNG_RESIZE_FN uint32_t tone_contrast_mean(uint64_t sum, uint64_t n) { return (uint32_t)((2 * sum + n) / (2 * n)); }
FPNG_RESIZE_FN uint32_t tone_contrast_entry(uint32_t v, uint32_t mean, float factor)
{
#pragma clang fp contract(off)
    const float d = (float)((int32_t)v - (int32_t)mean);
    const float p = factor * d;
    const float t = (float)(int32_t)mean + p;
    if (factor >= 0.0f && factor <= 1.0f) return (uint32_t)(int32_t)t & 255u; // (between mean and v)
    return t <= 0.0f ? 0u : t >= 255.0f ? 255u : (uint32_t)(int32_t)t;
}

// ---- host only: how the calls judge a record, and the rule for one view ----

static_assert(sizeof(fpng_amd_view_tone) == 16 && offsetof(fpng_amd_view_tone, factor) == 4 && offsetof(fpng_amd_view_tone, reserved) == 8 &&
                  FPNG_AMD_TONE_AUTOCONTRAST == kToneAutocontrast && FPNG_AMD_TONE_EQUALIZE == kToneEqualize && FPNG_AMD_TONE_CONTRAST == kToneContrast,
              "fpng_amd_view_tone layout");

// NULL, or why the calls refuse the record.  w, h: the view's window, where it is known (else 0: its size is not judged)
inline const char *check_tone_record(const fpng_amd_view_tone &p, uint32_t w, uint32_t h)
{
    if (p.op > kToneContrast) return "unknown fpng_amd_view_tone::op (FPNG_AMD_TONE_AUTOCONTRAST, _EQUALIZE, _CONTRAST)";
    if (p.reserved[0] | p.reserved[1]) return "fpng_amd_view_tone::reserved must be 0";
    if (p.op == kToneContrast) {
        if (!std::isfinite(p.factor) || !(p.factor >= 0.0f)) return "fpng_amd_view_tone::factor must be finite and >= 0 with FPNG_AMD_TONE_CONTRAST";
    } else if (p.factor != 0.0f) // (a NaN is not 0)
        return "fpng_amd_view_tone::factor must be 0 without FPNG_AMD_TONE_CONTRAST";
    if (p.op && (uint64_t)w * h > UINT32_MAX) return "a tone view's w * h must fit 32 bits (its histograms count in uint32)";
    return nullptr;
}

// the three tables of the record `p` (judged, op != 0 or not: 0 gives the identity) from the four histograms
inline void tone_lut(const fpng_amd_view_tone &p, const uint32_t hist[kToneHistWords], uint8_t lut[kToneLutBytes])
{
    if (p.op == kToneContrast) {
        uint64_t sum = 0, n = 0;
        for (uint32_t v = 0; v < 256; v++) sum += (uint64_t)v * hist[3 * 256 + v], n += hist[3 * 256 + v];
        const uint32_t mean = n ? tone_contrast_mean(sum, n) : 0u;
        for (uint32_t v = 0; v < 256; v++) lut[v] = lut[256 + v] = lut[512 + v] = (uint8_t)tone_contrast_entry(v, mean, p.factor);
        return;
    }
    for (uint32_t c = 0; c < 3; c++) {
        const uint32_t *const h = hist + c * 256;
        uint32_t lo = 255, hi = 0, bins = 0;
        uint64_t total = 0;
        for (uint32_t v = 0; v < 256; v++)
            if (h[v]) lo = bins++ ? lo : v, hi = v, total += h[v];
        const uint64_t step = tone_equalize_step(total, h[hi], bins);
        uint64_t before = 0;
        for (uint32_t v = 0; v < 256; before += h[v++])
            lut[c * 256 + v] = (uint8_t)(p.op == kToneAutocontrast ? tone_autocontrast_entry(v, lo, hi) : p.op == kToneEqualize ? tone_equalize_entry(v, before, step) : v);
    }
}

// the four histograms of the three planes of W (w x h bytes each, one behind the other)
inline void tone_histograms(uint32_t w, uint32_t h, const uint8_t *in, uint32_t hist[kToneHistWords])
{
    const size_t n = (size_t)w * h;
    for (uint32_t k = 0; k < kToneHistWords; k++) hist[k] = 0;
    for (size_t k = 0; k < n; k++) {
        const uint32_t r = in[k], g = in[n + k], b = in[2 * n + k];
        hist[r]++, hist[256 + g]++, hist[512 + b]++, hist[768 + tone_luma(r, g, b)]++;
    }
}

// fpng_amd_view_tone_lut / fpng_amd_view_tone_apply (decode_api.cpp) but for the error text, which comes back in *why: FPNG_AMD_OK, or
// FPNG_AMD_ERR_INVALID_ARG
inline int tone_lut_checked(const fpng_amd_view_tone *tone, const uint32_t *hist, uint8_t *lut, const char **why)
{
    *why = !tone || !hist || !lut ? "null tone, hist or lut" : check_tone_record(*tone, 0, 0);
    if (*why) return FPNG_AMD_ERR_INVALID_ARG;
    tone_lut(*tone, hist, lut);
    return FPNG_AMD_OK;
}

inline int tone_apply_checked(const fpng_amd_view_tone *tone, uint32_t w, uint32_t h, const uint8_t *in, uint8_t *out, const char **why)
{
    *why = !tone || !in || !out || !w || !h ? "null tone, in or out, or an empty view" : check_tone_record(*tone, w, h);
    if (!*why && (uint64_t)w * h > SIZE_MAX / 3) *why = "3 * w * h, the bytes of in and of out, must fit size_t"; // (a record without an op: any size)
    if (*why) return FPNG_AMD_ERR_INVALID_ARG;
    const size_t n = (size_t)w * h;
    uint32_t hist[kToneHistWords];
    uint8_t lut[kToneLutBytes];
    if (tone->op) tone_histograms(w, h, in, hist);
    else
        for (uint32_t k = 0; k < kToneHistWords; k++) hist[k] = 0;
    tone_lut(*tone, hist, lut);
    for (uint32_t c = 0; c < 3; c++)
        for (size_t k = 0; k < n; k++) out[c * n + k] = lut[c * 256 + in[c * n + k]];
    return FPNG_AMD_OK;
}

} // namespace fpng_amd
