// view_enhance.h -- the enhance record of fpng_amd_decode_batch(_device)_planar_views_enhance and _hwc_views_enhance
// (include/fpng_amd.h: the rule): Brightness, Color and Sharpness as RandAugment / TrivialAugment / AutoAugment apply them to a PIL
// image -- ImageEnhance.Brightness(img), .Color(img) and .Sharpness(img).enhance(factor) -- each Pillow's ImagingBlend of a DEGENERATE
// image and the view.  The stage sits behind the tone stage and in front of the blur, solarize and posterize.  The pieces below are
// the ONE text, run by the kMode == 3 instantiations of dec_view_post_kernel (view_post.hip) for every element and by the host
// function fpng_amd_view_enhance_apply (decode_api.cpp) that the CPU tests judge against Pillow and an exact restatement.
//
//   W': the bytes the tone stage hands on -- W itself for a view without a tone op.  Planes 0, 1, 2 only: a fourth one skips the stage.
//   E_c = blend(D_c, W'_c, factor), factor fp32, finite and >= 0, where blend(d, v, f) IS tone_contrast_entry(v, d, f) (view_tone.h):
//       t = (float)d + f * (float)((int)v - (int)d), every operation rounded on its own; 0 <= f <= 1: (uint8)t, truncating; else 0
//       for t <= 0, 255 for t >= 255, (uint8)t between.  f == 1 gives v.
//   BRIGHTNESS: D_c = 0 -- a point operation per channel, a 256-entry table.
//   COLOR:      D_c = L = tone_luma(W'_0, W'_1, W'_2), Pillow's convert("L"), for all three channels.
//   SHARPNESS:  D_c = ImageFilter.SMOOTH of plane c of W' over the un-mirrored w x h window.  w < 3 or h < 3: the identity.  A sample
//       on the window's outer frame (x = 0, x = w - 1, y = 0 or y = h - 1): D = W', so E = W' for every factor.  An interior sample:
//       S = the sum of its 3 x 3 neighbourhood + 4 x the centre (kernel 1 1 1 / 1 5 1 / 1 1 1), D = (2 S + 13) / 26, floored, in integers.
//       Pillow sums the nine products in fp32 with the weights (float)(k / 13.0), adds 0.5 and truncates.  S is an integer, so
//       S / 13 + 0.5 is an odd multiple of 1 / 26: at least 1 / 26 = 0.038 from every integer, while nine fp32 products and sums
//       of values below 256 are off by less than 0.001 in any order.  The truncation therefore lands where floor((2 S + 13) / 26)
//       does, whatever the order of summation.
//       The kernel is symmetric, so sharpening the un-mirrored window and mirroring at the store equals sharpening the mirrored
//       image; and E[refl(y)][refl(x)] is what sharpening the reflected neighbourhood gives, so the blur's reflected halo carries on
//       from E -- provided "a frame sample" is judged on the reflected, TRUE coordinate.
#pragma once
#include "fpng_amd.h"
#include "resize.h"
#include "view_tone.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace fpng_amd {

constexpr uint32_t kEnhanceBrightness = 1u, kEnhanceColor = 2u, kEnhanceSharpness = 3u; // FPNG_AMD_ENHANCE_*

// Pillow's ImagingBlend(degenerate, image, factor) for one byte: d of the degenerate image, v of the view
FPNG_RESIZE_FN uint32_t enhance_blend(uint32_t d, uint32_t v, float factor) { return tone_contrast_entry(v, d, factor); }

// ImageFilter.SMOOTH of an interior sample from s = the sum of its 3 x 3 neighbourhood + 4 x the centre (s <= 13 * 255)
FPNG_RESIZE_FN uint32_t enhance_smooth(uint32_t s) { return (2u * s + 13u) / 26u; }

// whether SHARPNESS filters a w x h window at all, and whether sample (x, y) of it -- TRUE coordinates -- is on its outer frame
FPNG_RESIZE_FN bool enhance_sharpens(uint32_t w, uint32_t h) { return w >= 3u && h >= 3u; }
FPNG_RESIZE_FN bool enhance_on_frame(uint32_t x, uint32_t y, uint32_t w, uint32_t h) { return x == 0u || y == 0u || x == w - 1u || y == h - 1u; }

// SHARPNESS for the interior sample at c of a plane whose rows are `stride` bytes apart
FPNG_RESIZE_FN uint32_t enhance_sharp_at(const uint8_t *c, int32_t stride, float factor)
{
    const uint32_t v = c[0];
    const uint32_t s = (uint32_t)c[-stride - 1] + c[-stride] + c[-stride + 1] + c[-1] + 5u * v + c[1] + c[stride - 1] + c[stride] + c[stride + 1];
    return enhance_blend(enhance_smooth(s), v, factor);
}

// post_refl (view_post.h) held inside the window: with a halo of R + 1 = min(w, h) the outermost ring's reflection is one past it
FPNG_RESIZE_FN uint32_t enhance_refl(int32_t j, uint32_t n)
{
    const int32_t r = j < 0 ? -j : j >= (int32_t)n ? 2 * ((int32_t)n - 1) - j : j;
    return (uint32_t)(r < 0 ? 0 : r >= (int32_t)n ? (int32_t)n - 1 : r);
}

// ---- host only: how the calls judge a record, and the rule for one view ----

static_assert(sizeof(fpng_amd_view_enhance) == 16 && offsetof(fpng_amd_view_enhance, factor) == 4 && offsetof(fpng_amd_view_enhance, reserved) == 8 &&
                  FPNG_AMD_ENHANCE_BRIGHTNESS == kEnhanceBrightness && FPNG_AMD_ENHANCE_COLOR == kEnhanceColor && FPNG_AMD_ENHANCE_SHARPNESS == kEnhanceSharpness,
              "fpng_amd_view_enhance layout");

// NULL, or why the calls refuse the record.  planes: those of the view's destination, where they are known (else 0: not judged)
inline const char *check_enhance_record(const fpng_amd_view_enhance &p, uint32_t planes)
{
    if (p.op > kEnhanceSharpness) return "unknown fpng_amd_view_enhance::op (FPNG_AMD_ENHANCE_BRIGHTNESS, _COLOR, _SHARPNESS)";
    if (p.reserved[0] | p.reserved[1]) return "fpng_amd_view_enhance::reserved must be 0";
    if (p.op) {
        if (!std::isfinite(p.factor) || !(p.factor >= 0.0f)) return "fpng_amd_view_enhance::factor must be finite and >= 0 with an op";
    } else if (p.factor != 0.0f) // (a NaN is not 0)
        return "fpng_amd_view_enhance::factor must be 0 without an op";
    if (p.op == kEnhanceColor && planes && planes < 3u) return "FPNG_AMD_ENHANCE_COLOR needs a destination of at least 3 planes";
    return nullptr;
}

// E of the three planes of W' (w x h bytes each, one behind the other) for the record `p` (judged; op 0: a copy)
inline void enhance_apply(const fpng_amd_view_enhance &p, uint32_t w, uint32_t h, const uint8_t *in, uint8_t *out)
{
    const size_t n = (size_t)w * h;
    const bool sharp = p.op == kEnhanceSharpness && enhance_sharpens(w, h);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const size_t k = (size_t)y * w + x;
            const uint32_t luma = p.op == kEnhanceColor ? tone_luma(in[k], in[n + k], in[2 * n + k]) : 0u;
            for (uint32_t c = 0; c < 3; c++) {
                const uint8_t *const at = in + c * n + k;
                uint32_t e = *at;
                if (p.op == kEnhanceBrightness) e = enhance_blend(0u, e, p.factor);
                else if (p.op == kEnhanceColor) e = enhance_blend(luma, e, p.factor);
                else if (sharp && !enhance_on_frame(x, y, w, h)) e = enhance_sharp_at(at, (int32_t)w, p.factor);
                out[c * n + k] = (uint8_t)e;
            }
        }
}

// fpng_amd_view_enhance_apply (decode_api.cpp) but for the error text, which comes back in *why: FPNG_AMD_OK, or FPNG_AMD_ERR_INVALID_ARG
inline int enhance_apply_checked(const fpng_amd_view_enhance *e, uint32_t w, uint32_t h, const uint8_t *in, uint8_t *out, const char **why)
{
    *why = !e || !in || !out || !w || !h ? "null enhance, in or out, or an empty view" : check_enhance_record(*e, 3);
    if (!*why && (w > (uint32_t)INT32_MAX || (uint64_t)w * h > SIZE_MAX / 3)) *why = "w must fit 31 bits, and 3 * w * h, the bytes of in and of out, size_t";
    if (*why) return FPNG_AMD_ERR_INVALID_ARG;
    enhance_apply(*e, w, h, in, out);
    return FPNG_AMD_OK;
}

} // namespace fpng_amd
