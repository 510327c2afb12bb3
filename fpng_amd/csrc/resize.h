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

// s_f, the filter's base support
FPNG_RESIZE_FN uint32_t resize_base_support(uint32_t filter) { return filter == kResizeBicubic ? 2u : 1u; }

FPNG_RESIZE_FN bool resize_scale_ok(uint32_t in, uint32_t out, uint32_t filter = kResizeBilinear)
{
    return in && out && (uint64_t)in * resize_base_support(filter) <= (uint64_t)kResizeMaxScale * out;
}

// taps an output sample of this axis has at most (what the kernel sizes its tile's weights with): count < 2 * support + 1, and one
// more for the roundings of center -/+ support
FPNG_RESIZE_FN uint32_t resize_max_taps(uint32_t in, uint32_t out, uint32_t filter = kResizeBilinear)
{
    const uint64_t sf = resize_base_support(filter);
    const uint32_t twice = in > out ? (uint32_t)((2ull * sf * in + out - 1) / out) : (uint32_t)(2u * sf); // ceil(2 * support)
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

// first and count of resize_weights_of without the weights (with resize_scale_ok() its cap never applies)
FPNG_RESIZE_FN uint32_t resize_taps_of(uint32_t filter, uint32_t in, uint32_t out, uint32_t o, uint32_t *first)
{
    const ResizeTaps taps = resize_taps(filter, in, out, o);
    *first = (uint32_t)taps.lo;
    return (uint32_t)(taps.hi - taps.lo);
}

// first tap and the tap behind the last one of output samples o0 .. o0 + n - 1 of an axis (n >= 1): the source samples a window needs
FPNG_RESIZE_FN void resize_source_span(uint32_t filter, uint32_t in, uint32_t out, uint32_t o0, uint32_t n, uint32_t *begin, uint32_t *end)
{
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
    const uint64_t reach = kResizeTileH - 1 + 2 * resize_base_support(filter); // (tile - 1) + 2 * s_f
    const uint64_t span = in > out ? (reach * in + out - 1) / out : reach; // ceil((tile - 1) * scale + 2 * support)
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
};
static_assert(sizeof(DecResize) == 104 && offsetof(DecResize, src_plane_pitch) == 24 && offsetof(DecResize, pitch) == 32 && offsetof(DecResize, src_pitch) == 100, "DecResize layout");

// tiles of kResizeTileW x kResizeTileH samples that a w x h window has per plane
FPNG_RESIZE_FN uint64_t resize_tiles(uint32_t w, uint32_t h)
{
    return (uint64_t)((w + kResizeTileW - 1) / kResizeTileW) * ((h + kResizeTileH - 1) / kResizeTileH);
}

} // namespace fpng_amd
