// resize.h -- the resize of fpng_amd_decode_batch(_device)_planar_resize (include/fpng_amd.h): the ONE text of the weight rule,
// shared by dec_resize_kernel (resize.hip), which computes its tile's weights with it, and by the host function
// fpng_amd_resize_weights (decode_api.cpp) that the CPU tests judge against a Python restatement of the rule.
//
// The rule is Pillow's 8-bit resampler -- what torchvision's PIL backend computes for resized_crop(..., interpolation=BILINEAR or
// BICUBIC).  A filter f is a kernel function k_f and a base support s_f: bilinear is the triangle tri with s_f = 1, bicubic the
// Keys cubic (a = -0.5) with s_f = 2.  Per axis (`in` -> `out` samples), in IEEE double, operations in the order written, no fused
// multiply-add:
//
//   scale = in / out;  fs = max(scale, 1.0);  support = s_f * fs;  ss = 1.0 / fs
//   for o in 0 .. out - 1:
//       center = (o + 0.5) * scale
//       first  = max((int)(center - support + 0.5), 0)                  (int): truncation toward zero
//       count  = min((int)(center + support + 0.5), in) - first
//       k[t]   = k_f(((t + first) - center + 0.5) * ss)   t = 0 .. count - 1
//                  tri(a)   = |a| < 1 ? 1 - |a| : 0
//                  cubic(a) = x = |a|;  x < 1 ? ((1.5 * x - 2.5) * x) * x + 1 : x < 2 ? (((x - 5) * x + 8) * x - 4) * -0.5 : 0
//       ww     = k[0] + k[1] + ... (in this order);  k[t] = k[t] / ww  (if ww != 0)
//       K[o][t] = k[t] < 0 ? (int)(-0.5 + k[t] * 4194304.0) : (int)(0.5 + k[t] * 4194304.0)          2^22
//
//   one pass:  out[o] = clamp((2^21 + sum_t in[first_o + t] * K[o][t]) >> 22, 0, 255)        (>>: arithmetic, a negative sum gives 0)
//
// The horizontal pass gives BYTES, the vertical pass reads those.  Taps never leave the `in` samples (first >= 0, first + count <=
// in); in == out is the identity (one weight of 2^22, any other tap 0).  The triangle's weights are not negative and sum to 2^22
// give or take `count` units; the cubic's may be negative (the clamp is then live at both ends) and the sum of their magnitudes
// is 1.167 * 2^22 at the scale limit and at most 1.27 * 2^22 anywhere (near in == out, where few taps share the sum), so a pass's
// sum 2^21 + 255 * sum |K| stays inside int32.  With in <= 32 * out
// (bilinear) and in <= 16 * out (bicubic): support <= 32 and count <= kResizeMaxTaps.
//
// The filters of the RESAMPLE record -- Pillow's NEAREST, BOX, HAMMING and LANCZOS -- have their rule further down ("the filters of the
// RESAMPLE record"): the three convolutions under this one with signed kernel arguments and their own supports, limits in * max(s_f, 1)
// <= 32 * out, and NEAREST as an index table.
//
// A WINDOW (x, y, w, h) of the resized image (fpng_amd_resize_view) is the same weights evaluated at o = x + i: the source it needs
// is the box first(x) .. first(x + w - 1) + count(x + w - 1) per axis (first and first + count do not decrease with o).
//
// Double add, multiply, divide, compare and conversion are correctly rounded on the host and on gfx950; what could differ is a
// multiply and an add contracted into one fused operation, which hipcc does in device code by default: contraction is off in here.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FPNG_RESIZE_FN __host__ __device__ inline
#else
#define FPNG_RESIZE_FN inline
#endif

namespace fpng_amd {

constexpr uint32_t kResizeMaxTaps = 65;  // count at the scale limit
constexpr uint32_t kResizeMaxScale = 32; // in <= kResizeMaxScale * out (bilinear); bicubic: half of it, the same support
constexpr uint32_t kResizeMirror = 1u;   // FPNG_AMD_RESIZE_MIRROR
constexpr uint32_t kResizeBits = 22;     // the weights' fixed point
constexpr uint32_t kResizeBilinear = 0, kResizeBicubic = 1, kResizeFilters = 2; // FPNG_AMD_FILTER_*
// The filters of the RESAMPLE record (fpng_amd_view_resample: FPNG_AMD_RESAMPLE_* + 1), as they travel in DecResize::filter behind
// the two above -- the second half of this file has their rule
constexpr uint32_t kResizeNearest = 2, kResizeBox = 3, kResizeHamming = 4, kResizeLanczos = 5, kResizeAllFilters = 6;
// What a views launch's records ask of its kernel: 0 -- all bilinear, the instantiation with the triangle alone; 1 -- some bicubic;
// 2 -- some RESAMPLE filter, the instantiation that takes every filter as a value.  A launch's kind: the most of its records'
constexpr uint32_t kResizeLaunchKinds = 3;
inline uint32_t resize_launch_kind(uint32_t filter) { return filter < kResizeFilters ? filter : 2u; }

// 2 * s_f, the filter's base support in HALF units (the box filter's is 0.5).  NEAREST has no support: the 2 of the triangle,
// which bounds it -- a sample's one tap lies inside the triangle's taps of the same sample
FPNG_RESIZE_FN uint32_t resize_base_support2(uint32_t filter)
{
    return filter == kResizeBicubic ? 4u : filter == kResizeBox ? 1u : filter == kResizeLanczos ? 6u : 2u;
}
// s_f (the filters with a whole one)
FPNG_RESIZE_FN uint32_t resize_base_support(uint32_t filter) { return resize_base_support2(filter) / 2u; }

// in * max(s_f, 1) <= kResizeMaxScale * out
FPNG_RESIZE_FN bool resize_scale_ok(uint32_t in, uint32_t out, uint32_t filter = kResizeBilinear)
{
    const uint32_t s2 = resize_base_support2(filter);
    return in && out && (uint64_t)in * (s2 < 2u ? 2u : s2) <= 2ull * kResizeMaxScale * out;
}

// taps an output sample of this axis has at most (what the kernel sizes its tile's weights with): count < 2 * support + 1, and one
// more for the roundings of center -/+ support.  NEAREST: its one tap
FPNG_RESIZE_FN uint32_t resize_max_taps(uint32_t in, uint32_t out, uint32_t filter = kResizeBilinear)
{
    if (filter == kResizeNearest) return 1u;
    const uint64_t s2 = resize_base_support2(filter);
    const uint32_t twice = in > out ? (uint32_t)((s2 * in + out - 1) / out) : (uint32_t)s2; // ceil(2 * support)
    const uint32_t taps = twice + 2u;
    return taps < kResizeMaxTaps ? taps : kResizeMaxTaps;
}

// the filters' kernel functions (x = |a|)
FPNG_RESIZE_FN double resize_tri(double x)
{
#pragma clang fp contract(off)
    return x < 1.0 ? 1.0 - x : 0.0;
}
FPNG_RESIZE_FN double resize_cubic(double x)
{
#pragma clang fp contract(off)
    if (x < 1.0) return ((1.5 * x - 2.5) * x) * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5;
    return 0.0;
}

// Output sample o of an axis of `in` -> `out` samples: its first tap, and its `count` weights to K[0], K[stride], K[2 * stride] ...
// Returns count (at most cap).  (Two walks over the taps -- their sum first, then every tap again, divided: the same operations on the same
// values give the same k[t] both times, and no thread keeps 65 doubles.)
// The taps of output sample o: lo .. hi - 1 of the `in` samples (hi >= lo), with the sample's centre and the kernel's scale.  The ONE
// place first and count come from: resize_weights_of (the kernel's tile, the host's weights) and resize_taps_of (the host's source
// box) both call it, so a box holds its window's taps by construction.
struct ResizeTaps {
    double center, ss;
    int64_t lo, hi;
};
FPNG_RESIZE_FN ResizeTaps resize_taps(uint32_t filter, uint32_t in, uint32_t out, uint32_t o)
{
#pragma clang fp contract(off)
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = filter == kResizeBicubic ? 2.0 * fs : fs, ss = 1.0 / fs;
    const double center = ((double)o + 0.5) * scale;
    int64_t lo = (int64_t)(center - support + 0.5), hi = (int64_t)(center + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > (int64_t)in) hi = (int64_t)in;
    if (hi < lo) hi = lo;
    return {center, ss, lo, hi};
}

// kFilter: the filter, known where this is compiled (the bilinear text is what it was before there was a second filter)
template <uint32_t kFilter>
FPNG_RESIZE_FN uint32_t resize_weights_of(uint32_t in, uint32_t out, uint32_t o, uint32_t *first, int32_t *K, uint32_t stride, uint32_t cap = kResizeMaxTaps)
{
#pragma clang fp contract(off)
    const ResizeTaps taps = resize_taps(kFilter, in, out, o);
    const double center = taps.center, ss = taps.ss;
    const int64_t lo = taps.lo;
    int64_t n = taps.hi - lo;
    if (n > (int64_t)cap) n = (int64_t)cap; // (never with resize_scale_ok() and cap = resize_max_taps(): the caller's K has room for cap)
    const uint32_t count = (uint32_t)n;
    double ww = 0.0;
    for (uint32_t t = 0; t < count; t++) {
        double a = ((double)((int64_t)t + lo) - center + 0.5) * ss;
        if (a < 0.0) a = -a;
        ww += kFilter == kResizeBicubic ? resize_cubic(a) : resize_tri(a);
    }
    for (uint32_t t = 0; t < count; t++) {
        double a = ((double)((int64_t)t + lo) - center + 0.5) * ss;
        if (a < 0.0) a = -a;
        double k = kFilter == kResizeBicubic ? resize_cubic(a) : resize_tri(a);
        if (ww != 0.0) k = k / ww;
        K[(size_t)t * stride] = k < 0.0 ? (int32_t)(-0.5 + k * 4194304.0) : (int32_t)(0.5 + k * 4194304.0);
    }
    *first = (uint32_t)lo;
    return count;
}

// the same with the filter as a value
FPNG_RESIZE_FN uint32_t resize_weights_of(uint32_t filter, uint32_t in, uint32_t out, uint32_t o, uint32_t *first, int32_t *K, uint32_t stride, uint32_t cap = kResizeMaxTaps)
{
    return filter == kResizeBicubic ? resize_weights_of<kResizeBicubic>(in, out, o, first, K, stride, cap) : resize_weights_of<kResizeBilinear>(in, out, o, first, K, stride, cap);
}

// ---- the filters of the RESAMPLE record: Pillow's BOX, HAMMING, LANCZOS and NEAREST ----
// BOX, HAMMING and LANCZOS are convolutions under the rule at the top, unchanged, each with a kernel function of the SIGNED argument
// (the box is not symmetric) and its base support:
//
//   box(a)     = a > -0.5 && a <= 0.5 ? 1 : 0                                                         s_f = 0.5
//   hamming(a) = x = |a|;  x == 0 ? 1 : x >= 1 ? 0 : (x = x * pi;  sin(x) / x * (c0 + c1 * cos(x)))    s_f = 1
//                c0 = (double)0.54f, c1 = (double)0.46f: Pillow writes the two constants as floats
//   lanczos(a) = -3 <= a && a < 3 ? sinc(a) * sinc(a / 3) : 0;  sinc(x) = x == 0 ? 1 : (x = x * pi;  sin(x) / x)      s_f = 3
//
// sin and cos are resize_sin and resize_cos below: ONE text that the kernels and the host compile, in double, contraction off, so
// the two sides agree bit for bit.  Pillow calls its C library's, which is another program: the two may differ in the last bit of a
// value, and such a difference flips a weight only where k * 2^22 lies within about 1e-9 of a half-integer (the CPU tests sweep
// some 10^7 weights against Pillow without meeting one).
//
// NEAREST is no convolution: Pillow's resize sends it through its affine scale path.  Per axis a = (double)in / out, xo = a * 0.5,
// and for o = 0 .. out - 1: idx[o] = (int)xo, then xo += a.  The running sum is part of the rule ((int)((o + 0.5) * a) differs for a
// fifth of the size pairs below 400), so idx[o] takes o additions to know: the host builds a view's indices
// (resize_nearest_indices) and the kernels read them (DecResize::nearest).  In the passes NEAREST is one tap of weight 2^22 at
// idx[o]: (2^21 + v * 2^22) >> 22 = v.

// The argument reduction and the two polynomials are those of fdlibm's e_rem_pio2.c, k_sin.c and k_cos.c (Copyright (C) 1993 by
// Sun Microsystems, Inc.  Developed at SunSoft, a Sun Microsystems, Inc. business.  Permission to use, copy, modify, and distribute
// this software is freely granted, provided that this notice is preserved), for |x| <= 3 pi, which is all the filters ask: errors
// below 1 ulp.
struct ResizeArg { // |x| = n * pi / 2 + y0 + y1, |y0 + y1| <= pi / 4
    double y0, y1;
    uint32_t n;
};
FPNG_RESIZE_FN ResizeArg resize_rem_pio2(double ax) // 0 <= ax < 2^20 * pi / 2; here at most 3 pi
{
#pragma clang fp contract(off)
    constexpr double inv_pio2 = 6.36619772367581382433e-01; // 53 bits of 2 / pi
    constexpr double pio2_1 = 1.57079632673412561417e+00;   // the first 33 bits of pi / 2
    constexpr double pio2_2 = 6.07710050630396597660e-11;   // the second 33 bits
    constexpr double pio2_2t = 2.02226624879595063154e-21;  // pi / 2 - (pio2_1 + pio2_2)
    const int32_t n = (int32_t)(ax * inv_pio2 + 0.5);
    const double fn = (double)n;
    const double t = ax - fn * pio2_1; // (exact: fn has few bits, pio2_1 33)
    double w = fn * pio2_2;
    const double r = t - w;
    w = fn * pio2_2t - ((t - r) - w);
    const double y0 = r - w;
    return {y0, (r - y0) - w, (uint32_t)n};
}
FPNG_RESIZE_FN double resize_kernel_sin(double x, double y) // sin(x + y), |x| <= pi / 4, y the tail of x
{
#pragma clang fp contract(off)
    constexpr double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                     S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double z = x * x, v = z * x;
    const double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
FPNG_RESIZE_FN double resize_kernel_cos(double x, double y) // cos(x + y), the same
{
#pragma clang fp contract(off)
    constexpr double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                     C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double z = x * x;
    const double r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    const double ax = x < 0.0 ? -x : x;
    if (ax < 0.3) return 1.0 - (0.5 * z - (z * r - x * y));
    // (qx: |x| / 4 cut to the upper word of the double, 0.28125 above 0.78125 -- 1 - qx is then exact)
    const uint64_t bits = __builtin_bit_cast(uint64_t, ax);
    const double qx = ax > 0.78125 ? 0.28125 : __builtin_bit_cast(double, (bits & 0xFFFFFFFF00000000ull) - (0x00200000ull << 32));
    const double hz = 0.5 * z - qx, a = 1.0 - qx;
    return a - (hz - (z * r - x * y));
}
FPNG_RESIZE_FN double resize_sin(double x)
{
#pragma clang fp contract(off)
    const ResizeArg q = resize_rem_pio2(x < 0.0 ? -x : x);
    const double s = q.n & 1u ? resize_kernel_cos(q.y0, q.y1) : resize_kernel_sin(q.y0, q.y1);
    return ((q.n & 2u) != 0) != (x < 0.0) ? -s : s;
}
FPNG_RESIZE_FN double resize_cos(double x)
{
#pragma clang fp contract(off)
    const ResizeArg q = resize_rem_pio2(x < 0.0 ? -x : x);
    const double c = q.n & 1u ? resize_kernel_sin(q.y0, q.y1) : resize_kernel_cos(q.y0, q.y1);
    return ((q.n + 1u) & 2u) ? -c : c;
}

constexpr double kResizePi = 3.14159265358979323846; // M_PI

FPNG_RESIZE_FN double resize_sinc(double x)
{
#pragma clang fp contract(off)
    if (x == 0.0) return 1.0;
    x = x * kResizePi;
    return resize_sin(x) / x;
}
// k_f(a) of BOX, HAMMING and LANCZOS, a signed
FPNG_RESIZE_FN double resample_kernel(uint32_t filter, double a)
{
#pragma clang fp contract(off)
    if (filter == kResizeBox) return a > -0.5 && a <= 0.5 ? 1.0 : 0.0;
    if (filter == kResizeHamming) {
        double x = a < 0.0 ? -a : a;
        if (x == 0.0) return 1.0;
        if (x >= 1.0) return 0.0;
        x = x * kResizePi;
        return resize_sin(x) / x * ((double)0.54f + (double)0.46f * resize_cos(x));
    }
    return -3.0 <= a && a < 3.0 ? resize_sinc(a) * resize_sinc(a / 3) : 0.0; // kResizeLanczos
}

// resize_taps for BOX, HAMMING and LANCZOS: the same text with the support in half units
FPNG_RESIZE_FN ResizeTaps resample_taps(uint32_t filter, uint32_t in, uint32_t out, uint32_t o)
{
#pragma clang fp contract(off)
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = (0.5 * (double)resize_base_support2(filter)) * fs, ss = 1.0 / fs;
    const double center = ((double)o + 0.5) * scale;
    int64_t lo = (int64_t)(center - support + 0.5), hi = (int64_t)(center + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > (int64_t)in) hi = (int64_t)in;
    if (hi < lo) hi = lo;
    return {center, ss, lo, hi};
}

// resize_weights_of for every filter but NEAREST, the filter a value: the launches that hold a view with a RESAMPLE filter run this
// text for all of their views (bilinear and bicubic: the operations of resize_weights_of<>, so the same weights)
FPNG_RESIZE_FN uint32_t resample_weights_of(uint32_t filter, uint32_t in, uint32_t out, uint32_t o, uint32_t *first, int32_t *K, uint32_t stride, uint32_t cap = kResizeMaxTaps)
{
#pragma clang fp contract(off)
    if (filter < kResizeFilters) return resize_weights_of(filter, in, out, o, first, K, stride, cap);
    const ResizeTaps taps = resample_taps(filter, in, out, o);
    const double center = taps.center, ss = taps.ss;
    const int64_t lo = taps.lo;
    int64_t n = taps.hi - lo;
    if (n > (int64_t)cap) n = (int64_t)cap; // (never with resize_scale_ok() and cap = resize_max_taps())
    const uint32_t count = (uint32_t)n;
    double ww = 0.0;
    for (uint32_t t = 0; t < count; t++) ww += resample_kernel(filter, ((double)((int64_t)t + lo) - center + 0.5) * ss);
    for (uint32_t t = 0; t < count; t++) {
        double k = resample_kernel(filter, ((double)((int64_t)t + lo) - center + 0.5) * ss);
        if (ww != 0.0) k = k / ww;
        K[(size_t)t * stride] = k < 0.0 ? (int32_t)(-0.5 + k * 4194304.0) : (int32_t)(0.5 + k * 4194304.0);
    }
    *first = (uint32_t)lo;
    return count;
}

// NEAREST: idx[o] of output samples o0 .. o0 + n - 1 of an axis to to[0 .. n - 1] -- o0 + n additions from sample 0.  false: an
// index outside the `in` samples (never)
FPNG_RESIZE_FN bool resize_nearest_indices(uint32_t in, uint32_t out, uint32_t o0, uint32_t n, uint32_t *to)
{
#pragma clang fp contract(off)
    const double a = (double)in / (double)out;
    double xo = a * 0.5;
    bool ok = true;
    for (uint64_t o = 0; o < (uint64_t)o0 + n; o++, xo += a) {
        if (o < o0) continue;
        const int64_t idx = (int64_t)xo;
        ok = ok && idx >= 0 && idx < (int64_t)in;
        to[o - o0] = (uint32_t)(idx < 0 ? 0 : idx < (int64_t)in ? idx : (int64_t)in - 1);
    }
    return ok;
}

// first and count of resize_weights_of without the weights (with resize_scale_ok() its cap never applies)
FPNG_RESIZE_FN uint32_t resize_taps_of(uint32_t filter, uint32_t in, uint32_t out, uint32_t o, uint32_t *first)
{
    const ResizeTaps taps = filter < kResizeFilters ? resize_taps(filter, in, out, o) : resample_taps(filter, in, out, o);
    *first = (uint32_t)taps.lo;
    return (uint32_t)(taps.hi - taps.lo);
}

// first tap and the tap behind the last one of output samples o0 .. o0 + n - 1 of an axis (n >= 1): the source samples a window needs
FPNG_RESIZE_FN void resize_source_span(uint32_t filter, uint32_t in, uint32_t out, uint32_t o0, uint32_t n, uint32_t *begin, uint32_t *end)
{
    if (filter == kResizeNearest) { // (idx does not decrease with o)
        uint32_t idx[2] = {0, 0};
        resize_nearest_indices(in, out, o0, 1, &idx[0]);
        resize_nearest_indices(in, out, o0 + n - 1, 1, &idx[1]);
        *begin = idx[0], *end = idx[1] + 1;
        return;
    }
    uint32_t first = 0, last = 0;
    resize_taps_of(filter, in, out, o0, &first);
    const uint32_t count = resize_taps_of(filter, in, out, o0 + n - 1, &last);
    *begin = first, *end = last + count;
}

// one pass's sum -> its byte
FPNG_RESIZE_FN uint32_t resize_clip8(int32_t sum)
{
    const int32_t v = sum >> kResizeBits;
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// ---- the kernel's tile (resize.hip) and what the host sizes its launch with ----
constexpr uint32_t kResizeTileW = 64, kResizeTileH = 16; // output samples per workgroup
constexpr uint32_t kResizeBlock = 256;

// source rows that the kResizeTileH output rows of one tile reach at most: first is the truncation of (q + 0.5) * scale - support
// + 0.5 and the last tap's end that of (q' + 0.5) * scale + support + 0.5 with q' - q <= kResizeTileH - 1, so their distance is
// below (kResizeTileH - 1) * scale + 2 * support + 1; two more for the roundings.  (Any kResizeTileH consecutive samples: a
// window's tiles start anywhere.)
FPNG_RESIZE_FN uint32_t resize_tile_rows(uint32_t in, uint32_t out, uint32_t filter = kResizeBilinear)
{
    const uint64_t reach2 = 2 * (kResizeTileH - 1) + 2 * resize_base_support2(filter); // ((tile - 1) + 2 * s_f) in half units
    const uint64_t span = in > out ? (reach2 * in + 2ull * out - 1) / (2ull * out) : (reach2 + 1) / 2; // ceil((tile - 1) * scale + 2 * support)
    const uint64_t rows = span + 3;
    return (uint32_t)(rows < in ? rows : in);
}

// bytes of LDS one tile needs: the x weights (taps x kResizeTileW), the y weights (taps x kResizeTileH), first and count of both
// axes, the horizontal pass's bytes (rows x kResizeTileW)
FPNG_RESIZE_FN uint32_t resize_tile_lds(uint32_t taps_x, uint32_t taps_y, uint32_t rows)
{
    return (taps_x * kResizeTileW + taps_y * kResizeTileH + 2u * (kResizeTileW + kResizeTileH)) * 4u + rows * kResizeTileW;
}

// a view's work for dec_resize_kernel: the window (x, y, w, h) of its crop (in_w x in_h) resized to full_w x full_h becomes the
// caller's planes (dst: DecJob's rules -- row 0 of plane 0, signed byte pitches).  src is the first byte of the BOX of the crop
// that the window's taps reach, inside the uint8 planes that the file's job decoded (rows src_pitch bytes apart, planes
// src_plane_pitch: those of the job's own box, which holds the boxes of all of the file's views -- with one view they are the
// view's box, tight); box_x / box_y: the view's box's origin within its crop, so a tap at crop column f is byte f - box_x of its row
struct DecResize {
    const uint8_t *src;
    uint8_t *dst;
    int64_t plane_pitch;
    uint64_t src_plane_pitch;
    int32_t pitch;
    uint32_t in_w, in_h, full_w, full_h, flags, planes;
    uint32_t taps_x, taps_y, rows; // what the tile's LDS is laid out with (resize_max_taps, resize_tile_rows)
    uint32_t filter;
    uint32_t x, y, w, h;
    uint32_t box_x, box_y;
    uint32_t src_pitch;
    // a NEAREST view's indices, else NULL: idx of the window's w columns, then of its h rows, as samples of the crop (the host's
    // resize_nearest_indices; the kernels with the RESAMPLE filters read them, no other kernel looks)
    const uint32_t *nearest;
};
static_assert(sizeof(DecResize) == 112 && offsetof(DecResize, src_plane_pitch) == 24 && offsetof(DecResize, pitch) == 32 && offsetof(DecResize, src_pitch) == 100 &&
                  offsetof(DecResize, nearest) == 104,
              "DecResize layout");

// Step 1 of the resize kernels in a launch that holds RESAMPLE filters: first, count and weights of sample o of an axis, which is
// sample i of the view's window on that axis (idx: the axis' part of DecResize::nearest)
FPNG_RESIZE_FN uint32_t resample_tile_weights(uint32_t filter, uint32_t in, uint32_t out, uint32_t o, const uint32_t *idx, uint32_t i, uint32_t *first, int32_t *K, uint32_t stride,
                                              uint32_t cap)
{
    if (filter == kResizeNearest) {
        *first = idx[i], K[0] = 1 << kResizeBits;
        return 1u;
    }
    return resample_weights_of(filter, in, out, o, first, K, stride, cap);
}

// tiles of kResizeTileW x kResizeTileH samples that a w x h window has per plane
FPNG_RESIZE_FN uint64_t resize_tiles(uint32_t w, uint32_t h)
{
    return (uint64_t)((w + kResizeTileW - 1) / kResizeTileW) * ((h + kResizeTileH - 1) / kResizeTileH);
}

} // namespace fpng_amd
