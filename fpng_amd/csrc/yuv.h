// yuv.h -- a pixel of a YUV video surface -> the PNG's R,G,B bytes: the ONE text of the rule of fpng_amd_encode_submit_yuv
// (include/fpng_amd.h), compiled by the row walk and the stored form (kernels.hip), by the renditions' source accessor
// (encode_resize.h) and by the host twin fpng_amd_yuv_pixels (api.cpp) that the CPU tests judge against the rule.
//
// Surfaces (FPNG_AMD_YUV_*; one base pointer, ONE row pitch for all planes, one signed chroma offset -- how a decoder hands a
// surface out):
//   NV12     8-bit luma plane, then one plane of interleaved Cb,Cr at half resolution in both directions
//   P016     the same with 16-bit little-endian elements (P010 / P012: their bits are MSB-aligned)
//   444      three 8-bit planes Y, Cb, Cr, chroma_offset apart
//   444_16   three 16-bit planes Y, Cb, Cr
//
// Pixel (x, y) of a w x h frame:
//   Y  = e(luma, x, y)
//   4:2:0:  Cb = e(chroma, 2 (x >> 1), y >> 1),  Cr = e(chroma, 2 (x >> 1) + 1, y >> 1)
//   4:4:4:  Cb = e(plane 1, x, y),               Cr = e(plane 2, x, y)
//   e of an 8-bit element = (float)byte;  e of a 16-bit element = (float)word * 2^-8 (exact: one matrix serves 8-, 10-, 12- and
//   16-bit content)
//   t_c    = fmaf(m[c][2], Cr, fmaf(m[c][1], Cb, fmaf(m[c][0], Y, m[c][3])))      c = R, G, B   (resize_color.h: color_mix)
//   byte_c = (uint8) rint(fminf(fmaxf(t_c, 0), 255)), ties to even                             (quantize.h: round_to_byte)
//
// The chroma of a 4:2:0 surface is REPLICATED: the four pixels of a 2 x 2 block share one Cb,Cr pair.  There is no interpolation
// and no chroma siting option.  With finite matrix entries of magnitude <= 65536 (the host refuses anything else) and elements
// below 256, |t_c| < 2^26: never infinite, never NaN.
#pragma once
#include "kernels.h"
#include "quantize.h"
#include "resize_color.h"

namespace fpng_amd {

constexpr uint32_t kYuvNV12 = 0, kYuvP016 = 1, kYuv444 = 2, kYuv444_16 = 3;
static_assert(FPNG_AMD_YUV_NV12 == kYuvNV12 && FPNG_AMD_YUV_P016 == kYuvP016 && FPNG_AMD_YUV_444 == kYuv444 && FPNG_AMD_YUV_444_16 == kYuv444_16 &&
                  FPNG_AMD_YUV_SURFACES == (uint32_t)kYuvSurfaces, "the surfaces' numbering");

constexpr bool yuv_is_420(uint32_t surface) { return surface < kYuv444; }
constexpr uint32_t yuv_elem_bytes(uint32_t surface) { return (surface & 1u) ? 2u : 1u; }
// planes with a buffer resource of their own in the row walk: luma + the interleaved chroma plane, or Y, Cb, Cr
constexpr int yuv_planes(uint32_t surface) { return yuv_is_420(surface) ? 2 : 3; }
// bytes of a chroma row (4:2:0: an odd width's last pixel has a full Cb,Cr pair)
FPNG_QUANT_FN uint64_t yuv_chroma_row_bytes(uint32_t surface, uint32_t w)
{
    return (yuv_is_420(surface) ? 2ull * (((uint64_t)w + 1u) >> 1) : (uint64_t)w) * yuv_elem_bytes(surface);
}

typedef uint16_t __attribute__((may_alias, aligned(2))) yuv_u16_any;

// e(): the element whose bits (16-bit surfaces: a little-endian word) are v
template <uint32_t S> FPNG_QUANT_FN float yuv_elem(uint32_t v) { return yuv_elem_bytes(S) == 2 ? (float)v * 0.00390625f : (float)v; }
// byte_c for row (m0, m1, m2, m3) of the matrix
FPNG_QUANT_FN uint32_t yuv_byte(float m0, float m1, float m2, float m3, float y, float cb, float cr) { return round_to_byte(color_mix(m0, m1, m2, m3, y, cb, cr)); }

// element i of a plane's row in memory
template <uint32_t S> FPNG_QUANT_FN uint32_t yuv_load(const uint8_t *row, uint64_t i)
{
    if constexpr (yuv_elem_bytes(S) == 2) return *(const yuv_u16_any *)(row + 2u * i);
    else return row[i];
}

// THE ACCESSOR: Y, Cb, Cr of pixel (x, y) of the FRAME (absolute coordinates: the chroma index of a 4:2:0 surface depends on them)
// whose luma plane's top row begins at `luma`.  Only elements of that pixel (4:2:0: of its 2 x 2 block's chroma pair) are read
template <uint32_t S> FPNG_QUANT_FN void yuv_fetch(const uint8_t *luma, int64_t pitch, int64_t chroma_offset, uint32_t x, uint32_t y, float &Y, float &Cb, float &Cr)
{
    const uint8_t *const ly = luma + (int64_t)y * pitch;
    Y = yuv_elem<S>(yuv_load<S>(ly, x));
    if constexpr (yuv_is_420(S)) {
        const uint8_t *const c = luma + chroma_offset + (int64_t)(y >> 1) * pitch;
        Cb = yuv_elem<S>(yuv_load<S>(c, 2u * (uint64_t)(x >> 1))), Cr = yuv_elem<S>(yuv_load<S>(c, 2u * (uint64_t)(x >> 1) + 1u));
    } else {
        Cb = yuv_elem<S>(yuv_load<S>(ly + chroma_offset, x)), Cr = yuv_elem<S>(yuv_load<S>(ly + 2 * chroma_offset, x));
    }
}
// file channel c (0, 1, 2 = R, G, B) of that pixel.  (The row of the matrix is selected, not indexed: ym may be a kernel argument,
// and an index into one by a lane's value would put a copy of it into private memory.)
template <uint32_t S> FPNG_QUANT_FN uint32_t yuv_channel(const uint8_t *luma, int64_t pitch, int64_t chroma_offset, const YuvMatrix &ym, uint32_t c, uint32_t x, uint32_t y)
{
    float Y, Cb, Cr;
    yuv_fetch<S>(luma, pitch, chroma_offset, x, y, Y, Cb, Cr);
    const float m0 = c == 0 ? ym.m[0][0] : c == 1 ? ym.m[1][0] : ym.m[2][0], m1 = c == 0 ? ym.m[0][1] : c == 1 ? ym.m[1][1] : ym.m[2][1];
    const float m2 = c == 0 ? ym.m[0][2] : c == 1 ? ym.m[1][2] : ym.m[2][2], m3 = c == 0 ? ym.m[0][3] : c == 1 ? ym.m[1][3] : ym.m[2][3];
    return yuv_byte(m0, m1, m2, m3, Y, Cb, Cr);
}

} // namespace fpng_amd
