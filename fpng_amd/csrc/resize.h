// resize.h -- the resize of fpng_amd_decode_batch(_device)_planar_resize (include/fpng_amd.h): the ONE text of the weight rule,
// shared by dec_resize_kernel (resize.hip), which computes its tile's weights with it, and by the host function
// fpng_amd_resize_weights (decode_api.cpp) that the CPU tests judge against a Python restatement of the rule.
//
// The rule is Pillow's 8-bit resampler with the triangle (bilinear) filter -- what torchvision's PIL backend computes for
// resized_crop(..., interpolation=BILINEAR): per axis (`in` -> `out` samples), in IEEE double, operations in the order written,
// no fused multiply-add:
//
//   scale = in / out;  fs = max(scale, 1.0);  support = fs;  ss = 1.0 / fs
//   for o in 0 .. out - 1:
//       center = (o + 0.5) * scale
//       first  = max((int)(center - support + 0.5), 0)                  (int): truncation toward zero
//       count  = min((int)(center + support + 0.5), in) - first
//       k[t]   = tri(((t + first) - center + 0.5) * ss)   t = 0 .. count - 1;   tri(a) = |a| < 1 ? 1 - |a| : 0
//       ww     = k[0] + k[1] + ... (in this order);  k[t] = k[t] / ww  (if ww != 0)
//       K[o][t] = (int)(0.5 + k[t] * 4194304.0)                          2^22
//
//   one pass:  out[o] = clamp((2^21 + sum_t in[first_o + t] * K[o][t]) >> 22, 0, 255)
//
// The horizontal pass gives BYTES, the vertical pass reads those.  Taps never leave the `in` samples (first >= 0, first + count <=
// in); in == out is the identity (one weight of 2^22, any other tap 0).  The weights are not negative and sum to 2^22 give or take `count` units,
// so a pass's sum stays below 2^31.  With in <= 32 * out: support <= 32 and count <= kResizeMaxTaps.
//
// Double add, multiply, divide, compare and conversion are correctly rounded on the host and on gfx950; what could differ is a
// multiply and an add contracted into one fused operation, which hipcc does in device code by default: contraction is off in here.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FPNG_RESIZE_FN __host__ __device__ inline
#else
#define FPNG_RESIZE_FN inline
#endif

namespace fpng_amd {

constexpr uint32_t kResizeMaxTaps = 65;  // count at the scale limit
constexpr uint32_t kResizeMaxScale = 32; // in <= kResizeMaxScale * out
constexpr uint32_t kResizeMirror = 1u;   // FPNG_AMD_RESIZE_MIRROR
constexpr uint32_t kResizeBits = 22;     // the weights' fixed point

FPNG_RESIZE_FN bool resize_scale_ok(uint32_t in, uint32_t out) { return in && out && (uint64_t)in <= (uint64_t)kResizeMaxScale * out; }

// taps an output sample of this axis has at most (what the kernel sizes its tile's weights with): count < 2 * support + 1, and one
// more for the roundings of center -/+ support
FPNG_RESIZE_FN uint32_t resize_max_taps(uint32_t in, uint32_t out)
{
    const uint32_t twice = in > out ? (uint32_t)((2ull * in + out - 1) / out) : 2u; // ceil(2 * support)
    const uint32_t taps = twice + 2u;
    return taps < kResizeMaxTaps ? taps : kResizeMaxTaps;
}

// Output sample o of an axis of `in` -> `out` samples: its first tap, and its `count` weights to K[0], K[stride], K[2 * stride] ...
// Returns count (at most cap).  (Two walks over the taps -- their sum first, then every tap again, divided: the same operations on the same
// values give the same k[t] both times, and no thread keeps 65 doubles.)
FPNG_RESIZE_FN uint32_t resize_weights_of(uint32_t in, uint32_t out, uint32_t o, uint32_t *first, int32_t *K, uint32_t stride, uint32_t cap = kResizeMaxTaps)
{
#pragma clang fp contract(off)
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs, ss = 1.0 / fs;
    const double center = ((double)o + 0.5) * scale;
    int64_t lo = (int64_t)(center - support + 0.5), hi = (int64_t)(center + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > (int64_t)in) hi = (int64_t)in;
    int64_t n = hi - lo;
    if (n < 0) n = 0;
    if (n > (int64_t)cap) n = (int64_t)cap; // (never with resize_scale_ok() and cap = resize_max_taps(): the caller's K has room for cap)
    const uint32_t count = (uint32_t)n;
    double ww = 0.0;
    for (uint32_t t = 0; t < count; t++) {
        double a = ((double)((int64_t)t + lo) - center + 0.5) * ss;
        if (a < 0.0) a = -a;
        ww += a < 1.0 ? 1.0 - a : 0.0;
    }
    for (uint32_t t = 0; t < count; t++) {
        double a = ((double)((int64_t)t + lo) - center + 0.5) * ss;
        if (a < 0.0) a = -a;
        double k = a < 1.0 ? 1.0 - a : 0.0;
        if (ww != 0.0) k = k / ww;
        K[(size_t)t * stride] = (int32_t)(0.5 + k * 4194304.0);
    }
    *first = (uint32_t)lo;
    return count;
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
// below (kResizeTileH - 1) * scale + 2 * support + 1; two more for the roundings
FPNG_RESIZE_FN uint32_t resize_tile_rows(uint32_t in, uint32_t out)
{
    const uint64_t span = in > out ? ((uint64_t)(kResizeTileH + 1) * in + out - 1) / out : (uint64_t)kResizeTileH + 1; // ceil((tile - 1) * scale + 2 * support)
    const uint64_t rows = span + 3;
    return (uint32_t)(rows < in ? rows : in);
}

// bytes of LDS one tile needs: the x weights (taps x kResizeTileW), the y weights (taps x kResizeTileH), first and count of both
// axes, the horizontal pass's bytes (rows x kResizeTileW)
FPNG_RESIZE_FN uint32_t resize_tile_lds(uint32_t taps_x, uint32_t taps_y, uint32_t rows)
{
    return (taps_x * kResizeTileW + taps_y * kResizeTileH + 2u * (kResizeTileW + kResizeTileH)) * 4u + rows * kResizeTileW;
}

// a file's work for dec_resize_kernel: its crop's uint8 planes (src, tight: rows of crop w bytes, planes of crop w * h) become the
// caller's planes (dst: DecJob's rules -- row 0 of plane 0, signed byte pitches)
struct DecResize {
    const uint8_t *src;
    uint8_t *dst;
    int64_t plane_pitch;
    int32_t pitch;
    uint32_t in_w, in_h, out_w, out_h, flags, planes;
    uint32_t taps_x, taps_y, rows; // what the tile's LDS is laid out with (resize_max_taps, resize_tile_rows)
    uint32_t pad_[2];
};
static_assert(sizeof(DecResize) == 72, "DecResize layout");

} // namespace fpng_amd
