// encode_resize.h -- the front stage of fpng_amd_encode_submit_renditions (include/fpng_amd.h): a RENDITION of a device image --
// img.crop(box).resize((w, h), filter) as Pillow computes it -- resampled from the source AS IT LIES (any of the four descriptor
// kinds: interleaved in every FPNG_AMD_SRC_* format with a signed pitch, planar uint8 with signed row and plane pitches, planar
// floats through quantize.h; and the YUV surfaces of fpng_amd_encode_submit_yuv through yuv.h) into tight R,G,B[,A] rows that the unchanged encode chain then reads like any fpng_amd_image.
//
// The rule of the resize is resize.h's, untouched, with `in` = the BOX's size: taps never leave the box.  The alpha rule is
// view_alpha.h's PREMULTIPLIED op (M on load, U on store).  What is new is the source accessor below and the tight interleaved
// store; both the kernel (encode_resize.hip) and the host twin fpng_amd_rendition_pixels (api.cpp) compile this text.
//
// One workgroup of enc_resize_kernel handles one (rendition, tile of kResizeTileW x kResizeTileH output pixels), ALL channels, as
// dec_resize_hwc_kernel does: per channel the horizontal pass into LDS bytes T and the vertical pass out of them, a thread's result
// bytes of its rows kept in registers, a byte per channel; behind the last channel they go to LDS as O[row][column * chans + chan],
// in the place of the weights and T, and a wave per row stores the row's run of whole pixels.  So a tile needs resize_tile_lds()
// bytes, or O's if that is more (enc_resize_tile_lds), whatever the channel count: 55 KB at the bilinear 32 x limit.  Where a
// 4-byte interleaved source's tile stays small with T once per channel, the horizontal pass is FUSED: all channels from one load
// per tap (enc_resize_fused, enc_row_sums4).
#pragma once
#include "kernels.h"
#include "quantize.h"
#include "resize.h"
#include "view_alpha.h"
#include "yuv.h"

namespace fpng_amd {

// how a source's channel bytes lie: EncResize::layout
constexpr uint32_t kEncSrcBytes3 = 0;  // interleaved, 3 source bytes per pixel, any start byte and pitch
constexpr uint32_t kEncSrcBytes4 = 1;  // interleaved, 4 source bytes per pixel, base and pitch multiples of 4: one aligned dword per pixel
constexpr uint32_t kEncSrcPlanar = 2;  // planar uint8
constexpr uint32_t kEncSrcFloat = 3;   // + kF32 / kF16 / kBF16: planar floats, quantised per element (quantize.h)
constexpr uint32_t kEncSrcYuv = 6;     // + FPNG_AMD_YUV_*: a YUV surface, converted per pixel (yuv.h)
constexpr uint32_t kEncSrcLayouts = 10;

// the constants of a submission's sources, behind the records in the kernel's memory: the float kind's, the YUV kind's
struct EncConsts {
    FloatQuant fq;
    YuvMatrix ym;
};

// a rendition's work for enc_resize_kernel.  src: channel data of pixel (0, 0) of the BOX -- the first byte of its source pixel
// (interleaved), or its element in the R plane (planar); pitch: signed bytes between rows; plane_pitch: signed bytes from one
// channel's plane to the next (planar); sel: kSrcFormats' selector, byte k = the source byte of channel k (interleaved).
// YUV surfaces: src = the luma plane's top row of the FRAME, plane_pitch = the chroma offset, and the box's origin travels in
// sel (x) and reserved (y) -- a 4:2:0 pixel's chroma index depends on its ABSOLUTE coordinates, so a box with an odd origin cannot
// be folded into src as the other layouts fold theirs.
// dst: the tight rows, w * chans bytes each.  premul: view_alpha.h's PREMULTIPLIED op is in force (4 channels, not NEAREST, not
// the identity: the host's rule).  nearest: a NEAREST rendition's indices, the w columns' and then the h rows', as samples of the
// box (the host's resize_nearest_indices), else NULL
struct EncResize {
    const uint8_t *src;
    uint8_t *dst;
    int64_t pitch, plane_pitch;
    const uint32_t *nearest;
    uint32_t layout, sel, chans, filter;
    uint32_t in_w, in_h, w, h;
    uint32_t premul;
    uint32_t taps_x, taps_y, rows; // what the tile's LDS is laid out with (resize_max_taps, resize_tile_rows)
    uint32_t fused;                // enc_resize_fused(): the horizontal pass makes all channels at once, T has a plane of `rows` rows per channel
    uint32_t reserved;             // YUV surfaces: the box's first row in the frame
};
static_assert(sizeof(EncResize) == 96 && offsetof(EncResize, nearest) == 32 && offsetof(EncResize, layout) == 40 && offsetof(EncResize, rows) == 84 && offsetof(EncResize, fused) == 88,
              "EncResize layout");

typedef uint32_t __attribute__((may_alias, aligned(4))) enc_u32_any;
typedef uint16_t __attribute__((may_alias, aligned(2))) enc_u16_any;

// THE ACCESSOR: channel c (the file's: R, G, B, A = 0 .. 3) of pixel (x, y) of the box, as the byte the file's pixel is made of.
// Only bytes of that pixel are read (kEncSrcBytes4: the aligned dword that is the pixel); L: the record's layout, known where
// this is compiled
template <uint32_t L> FPNG_RESIZE_FN uint32_t enc_src_channel(const EncResize &r, const EncConsts &k, uint32_t c, uint32_t x, uint32_t y)
{
    if constexpr (L >= kEncSrcYuv) {
        return yuv_channel<L - kEncSrcYuv>(r.src, r.pitch, r.plane_pitch, k.ym, c, r.sel + x, r.reserved + y);
    } else if constexpr (L == kEncSrcBytes3) {
        return (r.src + (int64_t)y * r.pitch + (uint64_t)x * 3u)[r.sel >> (8u * c) & 0xFFu];
    } else if constexpr (L == kEncSrcBytes4) {
        return *(const enc_u32_any *)(r.src + (int64_t)y * r.pitch + (uint64_t)x * 4u) >> (8u * (r.sel >> (8u * c) & 3u)) & 0xFFu;
    } else {
        const uint8_t *const row = r.src + (int64_t)c * r.plane_pitch + (int64_t)y * r.pitch;
        if constexpr (L == kEncSrcPlanar) return row[x];
        else {
            constexpr uint32_t DT = L - kEncSrcFloat;
            // (k lies in memory -- the kernel's in global memory behind its records: an index into a kernel ARGUMENT would put
            //  the argument into private memory)
            const float sc = k.fq.scale[c], bi = k.fq.bias[c];
            const uint32_t bits = DT == kF32 ? *(const enc_u32_any *)(row + (uint64_t)x * 4u) : (uint32_t) * (const enc_u16_any *)(row + (uint64_t)x * 2u);
            return quantize(widen<DT>(bits), sc, bi);
        }
    }
}

// one output sample of the horizontal pass: 2^21 + the sum over its `count` taps, columns first .. first + count - 1 of row y of
// the box, of P'_c * K[t * stride] -- P' = M(P_c, P_3) for a colour channel of a premultiplied rendition, else the channel's byte
template <uint32_t L, bool kMul> FPNG_RESIZE_FN int32_t enc_row_sum_of(const EncResize &r, const EncConsts &k, uint32_t c, uint32_t y, uint32_t first, uint32_t count, const int32_t *K, uint32_t stride)
{
    int32_t sum = 1 << (kResizeBits - 1);
    for (uint32_t t = 0; t < count; t++) {
        uint32_t v = enc_src_channel<L>(r, k, c, first + t, y);
        if constexpr (kMul) v = alpha_mul(v, enc_src_channel<L>(r, k, 3u, first + t, y));
        sum += (int32_t)v * K[t * stride];
    }
    return sum;
}
template <uint32_t L> FPNG_RESIZE_FN int32_t enc_row_sum_layout(const EncResize &r, const EncConsts &k, uint32_t c, uint32_t y, uint32_t first, uint32_t count, const int32_t *K, uint32_t stride)
{
    if constexpr (L >= kEncSrcYuv) return enc_row_sum_of<L, false>(r, k, c, y, first, count, K, stride); // (three channels: never premultiplied)
    else return r.premul && c < 3u ? enc_row_sum_of<L, true>(r, k, c, y, first, count, K, stride) : enc_row_sum_of<L, false>(r, k, c, y, first, count, K, stride);
}
// the same with the layout as a value (the same for all of a workgroup's threads).  kYuv: the record's layout is one of the YUV
// surfaces' (all records of a submission are, or none is).  They have a text of their own so that the kernel of the other
// layouts stays the one it was: with the four surfaces in ONE switch enc_resize_kernel needs 177 vector registers instead of 136
template <bool kYuv> FPNG_RESIZE_FN int32_t enc_row_sum(const EncResize &r, const EncConsts &k, uint32_t c, uint32_t y, uint32_t first, uint32_t count, const int32_t *K, uint32_t stride)
{
    if constexpr (kYuv) {
        switch (r.layout) {
        case kEncSrcYuv + kYuvNV12: return enc_row_sum_layout<kEncSrcYuv + kYuvNV12>(r, k, c, y, first, count, K, stride);
        case kEncSrcYuv + kYuvP016: return enc_row_sum_layout<kEncSrcYuv + kYuvP016>(r, k, c, y, first, count, K, stride);
        case kEncSrcYuv + kYuv444: return enc_row_sum_layout<kEncSrcYuv + kYuv444>(r, k, c, y, first, count, K, stride);
        default: return enc_row_sum_layout<kEncSrcYuv + kYuv444_16>(r, k, c, y, first, count, K, stride);
        }
    }
    switch (r.layout) {
    case kEncSrcBytes3: return enc_row_sum_layout<kEncSrcBytes3>(r, k, c, y, first, count, K, stride);
    case kEncSrcBytes4: return enc_row_sum_layout<kEncSrcBytes4>(r, k, c, y, first, count, K, stride);
    case kEncSrcPlanar: return enc_row_sum_layout<kEncSrcPlanar>(r, k, c, y, first, count, K, stride);
    case kEncSrcFloat + kF32: return enc_row_sum_layout<kEncSrcFloat + kF32>(r, k, c, y, first, count, K, stride);
    case kEncSrcFloat + kF16: return enc_row_sum_layout<kEncSrcFloat + kF16>(r, k, c, y, first, count, K, stride);
    default: return enc_row_sum_layout<kEncSrcFloat + kBF16>(r, k, c, y, first, count, K, stride);
    }
}

// kEncSrcBytes4, the FUSED horizontal pass: the sums of ALL channels of one output sample from ONE load per tap -- the aligned dword
// that is the pixel holds them all.  The same products in the same order as enc_row_sum's, channel by channel (a 3-channel
// source's c3 is made of a byte nobody asked for and is not looked at)
struct EncSums4 {
    int32_t c0, c1, c2, c3;
};
FPNG_RESIZE_FN EncSums4 enc_row_sums4(const EncResize &r, uint32_t y, uint32_t first, uint32_t count, const int32_t *K, uint32_t stride)
{
    const uint8_t *const row = r.src + (int64_t)y * r.pitch + (uint64_t)first * 4u;
    const uint32_t sh0 = 8u * (r.sel & 3u), sh1 = 8u * (r.sel >> 8 & 3u), sh2 = 8u * (r.sel >> 16 & 3u), sh3 = 8u * (r.sel >> 24 & 3u);
    EncSums4 s = {1 << (kResizeBits - 1), 1 << (kResizeBits - 1), 1 << (kResizeBits - 1), 1 << (kResizeBits - 1)};
    for (uint32_t t = 0; t < count; t++) {
        const uint32_t px = *(const enc_u32_any *)(row + (size_t)t * 4u);
        const int32_t k = K[t * stride];
        uint32_t v0 = px >> sh0 & 0xFFu, v1 = px >> sh1 & 0xFFu, v2 = px >> sh2 & 0xFFu;
        const uint32_t v3 = px >> sh3 & 0xFFu;
        if (r.premul) v0 = alpha_mul(v0, v3), v1 = alpha_mul(v1, v3), v2 = alpha_mul(v2, v3);
        s.c0 += (int32_t)v0 * k, s.c1 += (int32_t)v1 * k, s.c2 += (int32_t)v2 * k, s.c3 += (int32_t)v3 * k;
    }
    return s;
}

// step 3 of view_alpha.h's rule on a pixel's result bytes (channel c in byte c): R_c = U(R'_c, R'_3), R_3 = R'_3
FPNG_RESIZE_FN uint32_t enc_unmul_pixel(uint32_t px)
{
    const uint32_t a = px >> 24;
    return alpha_unmul(px & 255u, a) | alpha_unmul(px >> 8 & 255u, a) << 8 | alpha_unmul(px >> 16 & 255u, a) << 16 | a << 24;
}

// the LDS bytes of one tile: resize_tile_lds(), whose bytes the tile's result bytes O take over once the passes are done (a tile
// of few taps and rows needs less than O does)
// fused: T holds a plane of `rows` rows per channel instead of one that the channels take turns in
FPNG_RESIZE_FN uint32_t enc_resize_tile_lds(uint32_t taps_x, uint32_t taps_y, uint32_t rows, uint32_t chans, bool fused)
{
    const uint32_t passes = resize_tile_lds(taps_x, taps_y, rows) + (fused ? (chans - 1u) * rows * kResizeTileW : 0u), o = kResizeTileH * kResizeTileW * chans;
    return passes > o ? passes : o;
}
constexpr uint32_t kEncResizeMaxLds = 65536u; // what a launch may ask for (launch_dec_resize_hwc's bound)
// How the channels share the LDS: a 4-byte interleaved source whose tile, with T once per channel, stays within 32 KB (reductions up
// to about 8 x; so that as many workgroups fit a compute unit as before) runs the FUSED horizontal pass -- one load per tap for all
// channels (enc_row_sums4).  Every other rendition's channels take turns in one T (enc_row_sum), whatever its scale: the limits'
// 55 KB tiles among them, and every YUV surface (no fused pass for those layouts)
constexpr uint32_t kEncResizeFusedLds = 32768u;
FPNG_RESIZE_FN bool enc_resize_fused(uint32_t layout, uint32_t taps_x, uint32_t taps_y, uint32_t rows, uint32_t chans)
{
    return layout == kEncSrcBytes4 && enc_resize_tile_lds(taps_x, taps_y, rows, chans, true) <= kEncResizeFusedLds;
}

// where the renditions of one submission lie in the lane's scratch: every base a multiple of 16 (the row walk reads aligned
// 16-byte pieces), rows tight, and kEncResizeSlack bytes behind the last one for the walk's aligned reads past a row's end
constexpr uint64_t kEncResizeAlign = 16, kEncResizeSlack = 256;
FPNG_RESIZE_FN uint64_t enc_resize_place(uint64_t *cursor, uint32_t w, uint32_t h, uint32_t chans)
{
    const uint64_t at = (*cursor + kEncResizeAlign - 1) & ~(kEncResizeAlign - 1);
    *cursor = at + (uint64_t)w * h * chans;
    return at;
}
FPNG_RESIZE_FN uint64_t enc_resize_scratch_bytes(uint64_t cursor) { return ((cursor + kEncResizeAlign - 1) & ~(kEncResizeAlign - 1)) + kEncResizeSlack; }

// An exact grid as launch_dec_resize_hwc's, a workgroup per (record, tile): pre (device) and h_pre (host, the same words) hold n + 1
// entries, the TILES of the submission's records in front of each of recs[0 .. n].  lds_bytes: the most enc_resize_tile_lds() of the
// records.  consts (device): the submission's constants (read for float sources and YUV surfaces only).  yuv: the records are
// those of YUV frames (enc_resize_kernel<true>).  false: a record without or with too
// many tiles, or lds_bytes above kEncResizeMaxLds; nothing is launched.
bool launch_enc_resize(hipStream_t s, const EncResize *recs, const uint64_t *pre, const uint64_t *h_pre, uint32_t n, uint32_t lds_bytes, const EncConsts *consts, bool yuv = false);

} // namespace fpng_amd
