// view_warp.h -- the affine warp of fpng_amd_decode_batch(_device)_planar_views_warp and _hwc_views_warp (include/fpng_amd.h: the
// rule): what RandomRotation, RandomAffine and the ShearX/Y, TranslateX/Y and Rotate operations of RandAugment do to a PIL image --
// Image.transform(size, AFFINE, a, resample, fillcolor) -- between step 1 (the bytes B) and step 2 (blur) of the post rule.  The
// pieces below are the ONE text, run by dec_view_post_kernel (view_post.hip) in its load of the window and by the host function
// fpng_amd_view_warp_apply (decode_api.cpp) that the CPU tests judge against Pillow and an exact restatement.
//
//   M[q][i] = B[q][mirror ? w - 1 - i : i]: the warp reads the MIRRORED window (flip, then affine: torchvision's order); the mirror
//       is on the read index, because w - 1 - floor(v) != floor(w - v) at integers and no fixed-point coefficient holds it.
//   nearest (Pillow's affine_fixed): 16.16 integers from the host (warp_fix), sx = (A2 + x A0 + y A1) >> 16, sy likewise;
//       W[y][x] = M[sy][sx] inside 0 <= sx < w, 0 <= sy < h, else fill.
//   bilinear (Pillow's generic transform with bilinear_filter): IEEE double, NO contraction, the order of warp_locate below; the
//       byte is the value TRUNCATED.
// A pixel's position (warp_locate) is found once and serves all its planes (warp_sample).
#pragma once
#include "fpng_amd.h"
#include "resize.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace fpng_amd {

constexpr uint32_t kWarpAffine = 1u, kWarpBilinear = 2u; // FPNG_AMD_WARP_*

// what the kernel needs of a view's warp record: the host's fixed-point integers (64 bits wide: a coefficient of a 1-sample axis may
// pass the corner check and not fit 32; where Pillow's int holds them they are Pillow's) and the doubles themselves
struct DecWarp {
    int64_t A[6];
    double a[6];
    uint32_t flags; // FPNG_AMD_WARP_*; 0: no warp
    uint8_t fill[4];
};
static_assert(sizeof(DecWarp) == 104, "DecWarp layout");

// Pillow's check_fixed for one output corner
inline bool warp_corner_ok(const double a[6], double x, double y)
{
#pragma clang fp contract(off)
    return std::fabs(x * a[0] + y * a[1] + a[2]) < 32768.0 && std::fabs(x * a[3] + y * a[4] + a[5]) < 32768.0;
}

// FIX(v) = floor(v * 65536 + 0.5); A2 and A5 hold the half-sample steps.  Host only (|a| < 2^17 after the corner check).
inline void warp_fix(const double a[6], int64_t A[6])
{
#pragma clang fp contract(off)
    const auto fix = [](double v) { return (int64_t)std::floor(v * 65536.0 + 0.5); };
    A[0] = fix(a[0]), A[1] = fix(a[1]), A[3] = fix(a[3]), A[4] = fix(a[4]);
    A[2] = fix(a[2] + a[0] * 0.5 + a[1] * 0.5), A[5] = fix(a[5] + a[3] * 0.5 + a[4] * 0.5);
}

// where output sample (x, y) of a w x h window reads: columns of B (the mirror applied) and rows; nearest uses (x0, y0) only
struct WarpAt {
    uint32_t inside, x0, x1, y0, y1; // (y1 == y0 where Pillow's v2 = v1: the row below is outside)
    double dx, dy;
};

FPNG_RESIZE_FN WarpAt warp_locate(const DecWarp &r, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t mirror)
{
#pragma clang fp contract(off)
    WarpAt at = {};
    if (!(r.flags & kWarpBilinear)) {
        const int64_t sx = (r.A[2] + (int64_t)x * r.A[0] + (int64_t)y * r.A[1]) >> 16, sy = (r.A[5] + (int64_t)x * r.A[3] + (int64_t)y * r.A[4]) >> 16;
        if (sx < 0 || sx >= (int64_t)w || sy < 0 || sy >= (int64_t)h) return at;
        at.inside = 1, at.x0 = mirror ? w - 1u - (uint32_t)sx : (uint32_t)sx, at.y0 = (uint32_t)sy;
        return at;
    }
    const double xc = (double)x + 0.5, yc = (double)y + 0.5;
    double xs = (r.a[0] * xc + r.a[1] * yc) + r.a[2], ys = (r.a[3] * xc + r.a[4] * yc) + r.a[5];
    if (xs < 0.0 || xs >= (double)w || ys < 0.0 || ys >= (double)h) return at;
    xs -= 0.5, ys -= 0.5;
    const double fx = std::floor(xs), fy = std::floor(ys);
    const int32_t xi = (int32_t)fx, yi = (int32_t)fy; // (-1 .. w, -1 .. h)
    at.inside = 1, at.dx = xs - fx, at.dy = ys - fy;
    const uint32_t x0 = (uint32_t)(xi < 0 ? 0 : xi >= (int32_t)w ? (int32_t)w - 1 : xi), x1 = (uint32_t)(xi + 1 < 0 ? 0 : xi + 1 >= (int32_t)w ? (int32_t)w - 1 : xi + 1);
    at.x0 = mirror ? w - 1u - x0 : x0, at.x1 = mirror ? w - 1u - x1 : x1;
    at.y0 = (uint32_t)(yi < 0 ? 0 : yi >= (int32_t)h ? (int32_t)h - 1 : yi);
    at.y1 = yi + 1 >= 0 && yi + 1 < (int32_t)h ? (uint32_t)(yi + 1) : at.y0;
    return at;
}

// the byte of W at `at` for the plane p of B (rows of w bytes)
FPNG_RESIZE_FN uint32_t warp_sample(const WarpAt &at, uint32_t flags, const uint8_t *p, uint32_t w, uint32_t fill)
{
#pragma clang fp contract(off)
    if (!at.inside) return fill;
    const uint8_t *const r0 = p + (uint64_t)at.y0 * w;
    if (!(flags & kWarpBilinear)) return r0[at.x0];
    const uint8_t *const r1 = p + (uint64_t)at.y1 * w;
    const int32_t p00 = r0[at.x0], p01 = r0[at.x1], p10 = r1[at.x0], p11 = r1[at.x1];
    const double v1 = (double)p00 + (double)(p01 - p00) * at.dx, v2 = (double)p10 + (double)(p11 - p10) * at.dx;
    const double v = v1 + (v2 - v1) * at.dy;
    return (uint32_t)(int32_t)v;
}

// ---- host only: how the calls judge a record and make the kernel's, and the rule for one plane ----

static_assert(sizeof(fpng_amd_view_warp) == 64 && offsetof(fpng_amd_view_warp, a) == 8 && offsetof(fpng_amd_view_warp, fill) == 56 && offsetof(fpng_amd_view_warp, reserved1) == 60 &&
                  FPNG_AMD_WARP_AFFINE == kWarpAffine && FPNG_AMD_WARP_BILINEAR == kWarpBilinear,
              "fpng_amd_view_warp layout");

// NULL, or why the calls refuse the record.  w, h: the view's window, where it is known (else 0: the corners are not judged)
inline const char *check_warp_record(const fpng_amd_view_warp &p, uint32_t w, uint32_t h)
{
    if (p.flags & ~(uint32_t)(kWarpAffine | kWarpBilinear)) return "unknown fpng_amd_view_warp::flags bits (FPNG_AMD_WARP_AFFINE, _BILINEAR)";
    if ((p.flags & kWarpBilinear) && !(p.flags & kWarpAffine)) return "FPNG_AMD_WARP_BILINEAR needs FPNG_AMD_WARP_AFFINE";
    if (p.reserved0 | p.reserved1) return "fpng_amd_view_warp::reserved0 and reserved1 must be 0";
    for (int k = 0; k < 6; k++)
        if (!std::isfinite(p.a[k])) return "fpng_amd_view_warp::a: every coefficient must be finite";
    if (!p.flags) {
        for (int k = 0; k < 6; k++)
            if (p.a[k] != 0.0) return "fpng_amd_view_warp::a and fill must be 0 without FPNG_AMD_WARP_AFFINE";
        if (p.fill[0] | p.fill[1] | p.fill[2] | p.fill[3]) return "fpng_amd_view_warp::a and fill must be 0 without FPNG_AMD_WARP_AFFINE";
        return nullptr;
    }
    if (w && h)
        for (int k = 0; k < 4; k++)
            if (!warp_corner_ok(p.a, k & 1 ? (double)w : 0.0, k & 2 ? (double)h : 0.0))
                return "fpng_amd_view_warp::a: the four corners of the window must map to positions below 32768 in magnitude (Pillow's check_fixed)";
    return nullptr;
}

// whether the record makes its view a warp view: a flag, and coefficients other than the identity's.  The identity under either
// filter is W = M, so its view is left to the post call -- bit for bit what the call without a warp writes, in every dtype (a float
// view without post flags keeps the colour rule's unrounded value, which a pass through the bytes would lose)
inline bool warp_moves(const fpng_amd_view_warp &p)
{
    return p.flags && !(p.a[0] == 1.0 && p.a[1] == 0.0 && p.a[2] == 0.0 && p.a[3] == 0.0 && p.a[4] == 1.0 && p.a[5] == 0.0);
}

inline DecWarp warp_record(const fpng_amd_view_warp &p)
{
    DecWarp r = {};
    r.flags = warp_moves(p) ? p.flags : 0u;
    for (int k = 0; k < 6; k++) r.a[k] = p.a[k];
    for (int k = 0; k < 4; k++) r.fill[k] = p.fill[k];
    if (r.flags) warp_fix(p.a, r.A);
    return r;
}

// W of the rule for one plane: in is B (w x h, un-mirrored), out W.  The record has been judged.  flags == 0: out = M.
inline void warp_apply_plane(const fpng_amd_view_warp &p, uint32_t w, uint32_t h, uint32_t mirror, const uint8_t *in, uint8_t *out, uint8_t fill)
{
    DecWarp r = warp_record(p);
    if (p.flags && !r.flags) r.flags = p.flags, warp_fix(p.a, r.A); // (the identity goes through the gather here: W = M is its result)
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            if (!r.flags) {
                out[(size_t)y * w + x] = in[(size_t)y * w + (mirror ? w - 1 - x : x)];
                continue;
            }
            const WarpAt at = warp_locate(r, x, y, w, h, mirror);
            out[(size_t)y * w + x] = (uint8_t)warp_sample(at, r.flags, in, w, fill);
        }
}

// fpng_amd_view_warp_apply (decode_api.cpp) but for the error text, which comes back in *why: FPNG_AMD_OK, or FPNG_AMD_ERR_INVALID_ARG
inline int warp_apply_checked(const fpng_amd_view_warp *warp, uint32_t w, uint32_t h, uint32_t mirror, const uint8_t *in, uint8_t *out, uint8_t fill, const char **why)
{
    *why = !warp || !in || !out || !w || !h ? "null warp, in or out, or an empty plane" : check_warp_record(*warp, w, h);
    if (*why) return FPNG_AMD_ERR_INVALID_ARG;
    warp_apply_plane(*warp, w, h, mirror, in, out, fill);
    return FPNG_AMD_OK;
}

} // namespace fpng_amd
