// yuv_store.h -- the R,G,B bytes of a decoded view -> the elements of a YUV video surface: the ONE text of the rule of
// fpng_amd_decode_batch(_device)_yuv_views (include/fpng_amd.h), compiled by dec_yuv_store_kernel (yuv_store.hip) and by the host
// twin fpng_amd_yuv_surface (decode_api.cpp) that the CPU tests judge against a numpy restatement of the rule.  The surfaces and
// their layout words are yuv.h's, which reads them back on the encode side.
//
// P: the view's three uint8 planes R, G, B (w x h).  f: the call's 3 x 4 fp32 matrix, rows Y, Cb, Cr, columns R, G, B, offset.
// d: the depth -- 8 on the 8-bit surfaces; 10, 12 or 16 on the 16-bit ones.  IEEE binary32, one fused multiply-add where written:
//
//   t_c(r, g, b) = fmaf(f[c][2], b, fmaf(f[c][1], g, fmaf(f[c][0], r, f[c][3])))        (resize_color.h: color_mix)
//   elem_d(t)    = rint(fminf(fmaxf(t * 2^(d-8), 0), 2^d - 1)), ties to even            (t * 2^(d-8) is exact)
//   Y(x, y)      = elem_d(t_0(P_R[y][x], P_G[y][x], P_B[y][x]))
//   4:4:4:  Cb(x, y) = elem_d(t_1(the same pixel)),  Cr(x, y) = elem_d(t_2(the same pixel))
//   4:2:0:  chroma sample (i, j), i < ceil(w / 2), j < ceil(h / 2):
//           S_k = P_k[min(2j, h-1)][min(2i, w-1)] + P_k[min(2j, h-1)][min(2i+1, w-1)]
//               + P_k[min(2j+1, h-1)][min(2i, w-1)] + P_k[min(2j+1, h-1)][min(2i+1, w-1)]       (integer, 0 .. 1020)
//           m_k = (float)S_k * 0.25f                                                            (exact)
//           Cb = elem_d(t_1(m_R, m_G, m_B)),  Cr = elem_d(t_2(m_R, m_G, m_B))
//
// A 16-bit element is stored as elem_d << (16 - d), little-endian, MSB-aligned: the word that yuv.h reads back as word * 2^-8.
// The chroma of a 4:2:0 surface is the MEAN of its 2 x 2 block (centre siting): at an odd edge the existing pixels count twice.
// There is no chroma siting option.  Nothing is clamped to 16..235 beyond the clamp to the element range.  With finite matrix
// entries of magnitude <= 65536 (the host refuses anything else) |t_c| < 2^26: never infinite, never NaN.
#pragma once
#include "yuv.h"

namespace fpng_amd {

// the depth as the rule's three constants: 2^(d-8), 2^d - 1 (both exact in fp32) and the store's shift
struct YuvDepth {
    float scale, top;
    uint32_t shift;
};
inline YuvDepth yuv_depth(uint32_t surface, uint32_t d)
{
    return {(float)(1u << (d - 8u)), (float)((1u << d) - 1u), yuv_elem_bytes(surface) == 2 ? 16u - d : 0u};
}
// the depths a surface has (0: its own)
inline uint32_t yuv_store_depth(uint32_t surface, uint32_t depth)
{
    if (yuv_elem_bytes(surface) == 1) return depth == 0 || depth == 8 ? 8u : 0u;
    return depth == 0 ? 16u : depth == 10 || depth == 12 || depth == 16 ? depth : 0u;
}

// elem_d(t)
FPNG_QUANT_FN uint32_t yuv_store_elem(float t, float scale, float top)
{
    t = fminf(fmaxf(t * scale, 0.0f), top); // (NaN -> 0)
    return (uint32_t)(int32_t)rintf(t);
}
// elem_d(t_c(r, g, b)) for row (m0, m1, m2, m3) of the matrix
FPNG_QUANT_FN uint32_t yuv_store_mix(float m0, float m1, float m2, float m3, float r, float g, float b, float scale, float top)
{
    return yuv_store_elem(color_mix(m0, m1, m2, m3, r, g, b), scale, top);
}
// m_k of a block's integer sum
FPNG_QUANT_FN float yuv_store_mean(uint32_t sum) { return (float)sum * 0.25f; }

// ---- the host twin's walk: the rule element by element (the kernel walks strips of eight pixels, yuv_store.hip) ----
template <uint32_t S> inline void yuv_store_put(uint8_t *row, uint64_t i, uint32_t e, uint32_t shift)
{
    if constexpr (yuv_elem_bytes(S) == 2) {
        const uint16_t word = (uint16_t)(e << shift);
        row[2 * i] = (uint8_t)word, row[2 * i + 1] = (uint8_t)(word >> 8);
    } else
        row[i] = (uint8_t)e;
}
// rgb: tight h x w x 3 bytes; luma, pitch, chroma_offset: the surface's layout words (judged)
template <uint32_t S> inline void yuv_store_surface(const uint8_t *rgb, uint32_t w, uint32_t h, const YuvMatrix &f, const YuvDepth &dp, uint8_t *luma, int64_t pitch, int64_t chroma_offset)
{
    const auto px = [&](uint32_t x, uint32_t y, uint32_t k) -> uint32_t { return rgb[((size_t)y * w + x) * 3 + k]; };
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const float r = (float)px(x, y, 0), g = (float)px(x, y, 1), b = (float)px(x, y, 2);
            uint8_t *const ly = luma + (int64_t)y * pitch;
            yuv_store_put<S>(ly, x, yuv_store_mix(f.m[0][0], f.m[0][1], f.m[0][2], f.m[0][3], r, g, b, dp.scale, dp.top), dp.shift);
            if constexpr (!yuv_is_420(S)) {
                yuv_store_put<S>(ly + chroma_offset, x, yuv_store_mix(f.m[1][0], f.m[1][1], f.m[1][2], f.m[1][3], r, g, b, dp.scale, dp.top), dp.shift);
                yuv_store_put<S>(ly + 2 * chroma_offset, x, yuv_store_mix(f.m[2][0], f.m[2][1], f.m[2][2], f.m[2][3], r, g, b, dp.scale, dp.top), dp.shift);
            }
        }
    if constexpr (yuv_is_420(S))
        for (uint32_t j = 0; j < (h + 1) / 2; j++)
            for (uint32_t i = 0; i < (w + 1) / 2; i++) {
                const uint32_t x0 = 2 * i, x1 = x0 + 1 < w ? x0 + 1 : w - 1, y0 = 2 * j, y1 = y0 + 1 < h ? y0 + 1 : h - 1;
                float m[3];
                for (uint32_t k = 0; k < 3; k++) m[k] = yuv_store_mean(px(x0, y0, k) + px(x1, y0, k) + px(x0, y1, k) + px(x1, y1, k));
                uint8_t *const c = luma + chroma_offset + (int64_t)j * pitch;
                yuv_store_put<S>(c, 2ull * i, yuv_store_mix(f.m[1][0], f.m[1][1], f.m[1][2], f.m[1][3], m[0], m[1], m[2], dp.scale, dp.top), dp.shift);
                yuv_store_put<S>(c, 2ull * i + 1, yuv_store_mix(f.m[2][0], f.m[2][1], f.m[2][2], f.m[2][3], m[0], m[1], m[2], dp.scale, dp.top), dp.shift);
            }
}

// ---- the kernel's work ----
// A view for dec_yuv_store_kernel: its three uint8 planes in the decode scratch, which the views call's resize has just written
// (src: row 0 of R, 16-byte aligned; rows src_pitch bytes apart, a multiple of 16; planes src_plane_pitch), and the caller's
// surface (luma, pitch, chroma_offset: fpng_amd_yuv_dest's words, judged)
struct DecYuvStore {
    const uint8_t *src;
    uint8_t *luma;
    int64_t pitch, chroma_offset;
    uint64_t src_plane_pitch;
    uint32_t src_pitch, w, h, pad_;
};
static_assert(sizeof(DecYuvStore) == 56, "DecYuvStore layout");

// the scratch planes' row pitch
constexpr uint32_t yuv_stage_pitch(uint32_t w) { return (w + 15u) & ~15u; }

// A lane owns a STRIP of kYuvStrip pixels of a row (4:2:0: of a pair of rows); a workgroup kYuvBlockX strips along the row by
// kYuvBlockY rows (pairs of rows): a wave's stores are contiguous.  The workgroups a w x h view has
constexpr uint32_t kYuvStrip = 8, kYuvBlockX = 64, kYuvBlockY = 4, kYuvBlock = kYuvBlockX * kYuvBlockY;
FPNG_QUANT_FN uint64_t yuv_store_blocks(uint32_t surface, uint32_t w, uint32_t h)
{
    const uint32_t strips = (w + kYuvStrip - 1) / kYuvStrip, rows = yuv_is_420(surface) ? (h + 1) / 2 : h;
    return (uint64_t)((strips + kYuvBlockX - 1) / kYuvBlockX) * ((rows + kYuvBlockY - 1) / kYuvBlockY);
}

// An exact grid over the launch's records: pre[k] (k = 0 .. n), h_pre its host copy: the workgroups of the batch's records in front
// of record k.  false: a record without or with too many workgroups; nothing is launched
bool launch_dec_yuv_store(hipStream_t s, const DecYuvStore *recs, const uint64_t *pre, const uint64_t *h_pre, uint32_t n, uint32_t surface, const YuvMatrix &f, const YuvDepth &dp);

} // namespace fpng_amd
