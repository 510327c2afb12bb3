// yuv_store.hip -- the last stage of fpng_amd_decode_batch(_device)_yuv_views: a view's three uint8 planes, which the views call's
// resize has written into the decode scratch, become the elements of the caller's YUV surface (yuv_store.h: the rule, and the
// text the host's fpng_amd_yuv_surface runs).  Purely memory-bound, no LDS, no barrier; every launch is idempotent -- a group that
// needed more synchronisation rounds comes through again.
//
// A lane owns a strip of kYuvStrip = 8 pixels: on the 4:2:0 surfaces of a PAIR of rows, on the 4:4:4 ones of one row.
//   loads   4:2:0: six aligned 8-byte loads, two rows of three planes; 4:4:4: three.  The scratch planes start on 16 bytes and
//           their rows are a multiple of 16 apart (yuv_stage_pitch), so a strip's 8 bytes are aligned and lie inside its row's
//           pitch even where the row ends inside them; the bytes behind a row's end are whatever the scratch held.
//   edges   4:2:0: a strip with fewer than 8 pixels replicates its last pixel over the rest of the 8 bytes, and a strip without a
//           second row takes its first row twice: the block sums then are the rule's, min() and all.
//   compute 16 luma and 4 chroma pairs (4:4:4: 8 + 8 + 8 elements) in registers.  The matrix is a kernel argument -- scalar
//           registers -- and its rows are named, never indexed by a lane's value.
//   stores  a full strip whose destination piece is aligned: two 8-byte luma pieces and one 8-byte Cb,Cr piece (16-bit surfaces:
//           16-byte pieces).  Lanes run along a row: a wave's stores are contiguous.  The last strip of a row with fewer than 8
//           pixels, and any piece that is not aligned to its size -- 8-bit planes may start at any byte -- is stored element by
//           element, the strip's own elements and nothing else.
// A workgroup is kYuvBlockX = 64 strips along the row by kYuvBlockY = 4 rows (pairs): ONE exact grid over all records of the launch,
// pre counting the workgroups of the records in front, as the resize kernels run.  The strip is the issue's 8 pixels: the 8-bit
// surfaces' pieces are half the 16 bytes a store moves best per byte; 16 pixels a lane would double the registers of the
// 16-bit surfaces' lanes for the same pieces there.
#include <hip/hip_runtime.h>

#include "exact_grid.h"
#include "yuv_store.h"

namespace fpng_amd {

namespace {

// (the scratch and the surfaces are global memory: typed so, a pointer read out of a record loads and stores as one, not as a flat one)
typedef uint64_t __attribute__((may_alias, aligned(8))) yuv_u64_a;
typedef uint32_t yuv_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) yuv_u64_a g_u64;
typedef __attribute__((address_space(1))) yuv_u32x4 g_u32x4;
typedef __attribute__((address_space(1))) yuv_u16_any g_u16;
typedef __attribute__((address_space(1))) uint8_t g_u8;

// bytes n .. 7 of v become byte n - 1 (1 <= n <= 7)
__device__ __forceinline__ uint64_t yuv_pad8(uint64_t v, uint32_t n)
{
    const uint64_t keep = (1ull << (8u * n)) - 1ull;
    const uint64_t last = (v >> (8u * (n - 1u))) & 255ull;
    return (v & keep) | ((last * 0x0101010101010101ull) & ~keep);
}

// elements e[0 .. count - 1] (count <= 8) of surface S to p: one piece when all eight are there and p is aligned to it
template <uint32_t S> __device__ __forceinline__ void yuv_store_piece(uint8_t *p, const uint32_t (&e)[8], uint32_t count, uint32_t shift)
{
    if constexpr (yuv_elem_bytes(S) == 2) {
        if (count == 8u && !((uintptr_t)p & 15u)) {
            yuv_u32x4 q;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) q[k] = ((e[2 * k] << shift) & 0xFFFFu) | (e[2 * k + 1] << (shift + 16u));
            *(g_u32x4 *)p = q;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 8; k++)
                if (k < count) *(g_u16 *)(p + 2u * k) = (uint16_t)(e[k] << shift);
        }
    } else {
        if (count == 8u && !((uintptr_t)p & 7u)) {
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) lo |= e[k] << (8u * k), hi |= e[k + 4] << (8u * k);
            *(g_u64 *)p = (uint64_t)lo | ((uint64_t)hi << 32);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 8; k++)
                if (k < count) ((g_u8 *)p)[k] = (uint8_t)e[k];
        }
    }
}

template <uint32_t S> __global__ __launch_bounds__(kYuvBlock) void dec_yuv_store_kernel(const DecYuvStore *recs, const uint64_t *pre, uint32_t n, YuvMatrix f, YuvDepth dp)
{
    constexpr bool k420 = yuv_is_420(S);
    constexpr uint32_t kElem = yuv_elem_bytes(S);
    uint64_t g;
    const uint32_t lo = exact_grid_find(pre, n, blockIdx.x, g);
    const DecYuvStore &r = recs[lo];
    const uint32_t w = r.w, h = r.h;
    const uint32_t strips = (w + kYuvStrip - 1) / kYuvStrip, rows = k420 ? (h + 1) / 2 : h;
    const uint32_t blocks_x = (strips + kYuvBlockX - 1) / kYuvBlockX;
    const uint64_t rel = exact_grid_within(pre, lo, g);
    if (rel >= yuv_store_blocks(S, w, h)) return; // (never, with the host's pre)
    const uint32_t i = (uint32_t)(rel % blocks_x) * kYuvBlockX + threadIdx.x % kYuvBlockX;
    const uint32_t j = (uint32_t)(rel / blocks_x) * kYuvBlockY + threadIdx.x / kYuvBlockX;
    if (i >= strips || j >= rows) return;
    const uint32_t x0 = i * kYuvStrip, count = w - x0 < kYuvStrip ? w - x0 : kYuvStrip; // the strip's pixels: 1 .. 8
    const float scale = dp.scale, top = dp.top;
    const uint32_t shift = dp.shift;
    if constexpr (k420) {
        const uint32_t y0 = 2u * j;
        const bool two = y0 + 1u < h;
        const uint8_t *const p0 = r.src + (uint64_t)y0 * r.src_pitch + x0, *const p1 = two ? p0 + r.src_pitch : p0;
        uint64_t v[2][3];
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) {
            v[0][c] = *(const g_u64 *)(p0 + c * r.src_plane_pitch), v[1][c] = *(const g_u64 *)(p1 + c * r.src_plane_pitch);
            if (count < kYuvStrip) v[0][c] = yuv_pad8(v[0][c], count), v[1][c] = yuv_pad8(v[1][c], count);
        }
        uint8_t *const ly = r.luma + (int64_t)y0 * r.pitch + (int64_t)x0 * kElem;
#pragma unroll
        for (uint32_t q = 0; q < 2; q++) {
            if (q && !two) break;
            uint32_t e[8];
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                const float cr = (float)(uint32_t)(v[q][0] >> (8u * k) & 255u), cg = (float)(uint32_t)(v[q][1] >> (8u * k) & 255u), cb = (float)(uint32_t)(v[q][2] >> (8u * k) & 255u);
                e[k] = yuv_store_mix(f.m[0][0], f.m[0][1], f.m[0][2], f.m[0][3], cr, cg, cb, scale, top);
            }
            yuv_store_piece<S>(ly + (int64_t)q * r.pitch, e, count, shift);
        }
        uint32_t e[8];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            float m[3];
#pragma unroll
            for (uint32_t c = 0; c < 3; c++) {
                const uint32_t a = (uint32_t)(v[0][c] >> (16u * k)) & 0xFFFFu, b = (uint32_t)(v[1][c] >> (16u * k)) & 0xFFFFu;
                m[c] = yuv_store_mean((a & 255u) + (a >> 8) + (b & 255u) + (b >> 8));
            }
            e[2 * k] = yuv_store_mix(f.m[1][0], f.m[1][1], f.m[1][2], f.m[1][3], m[0], m[1], m[2], scale, top);
            e[2 * k + 1] = yuv_store_mix(f.m[2][0], f.m[2][1], f.m[2][2], f.m[2][3], m[0], m[1], m[2], scale, top);
        }
        // (the chroma row's element 2 (x >> 1) of pixel x: element x0 of strip x0; an odd count's last pixel has a full pair)
        yuv_store_piece<S>(r.luma + r.chroma_offset + (int64_t)j * r.pitch + (int64_t)x0 * kElem, e, (count + 1u) & ~1u, shift);
    } else {
        const uint8_t *const p0 = r.src + (uint64_t)j * r.src_pitch + x0;
        uint64_t v[3];
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) v[c] = *(const g_u64 *)(p0 + c * r.src_plane_pitch);
        uint8_t *const ly = r.luma + (int64_t)j * r.pitch + (int64_t)x0 * kElem;
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) {
            // (the row of the matrix is named by the unrolled c, a constant)
            const float m0 = f.m[c][0], m1 = f.m[c][1], m2 = f.m[c][2], m3 = f.m[c][3];
            uint32_t e[8];
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                const float cr = (float)(uint32_t)(v[0] >> (8u * k) & 255u), cg = (float)(uint32_t)(v[1] >> (8u * k) & 255u), cb = (float)(uint32_t)(v[2] >> (8u * k) & 255u);
                e[k] = yuv_store_mix(m0, m1, m2, m3, cr, cg, cb, scale, top);
            }
            yuv_store_piece<S>(ly + (int64_t)c * r.chroma_offset, e, count, shift);
        }
    }
}

} // namespace

bool launch_dec_yuv_store(hipStream_t s, const DecYuvStore *recs, const uint64_t *pre, const uint64_t *h_pre, uint32_t n, uint32_t surface, const YuvMatrix &f, const YuvDepth &dp)
{
    using Kernel = void (*)(const DecYuvStore *, const uint64_t *, uint32_t, YuvMatrix, YuvDepth);
    static const Kernel kernels[kYuvSurfaces] = {dec_yuv_store_kernel<kYuvNV12>, dec_yuv_store_kernel<kYuvP016>, dec_yuv_store_kernel<kYuv444>, dec_yuv_store_kernel<kYuv444_16>};
    if (surface >= (uint32_t)kYuvSurfaces) return false;
    return exact_grid_walk(h_pre, n, kYuvBlock, [&](uint32_t r0, uint32_t r1, uint32_t groups) {
        hipLaunchKernelGGL(kernels[surface], dim3(groups), dim3(kYuvBlock), 0, s, recs + r0, pre + r0, r1 - r0, f, dp);
    });
}

} // namespace fpng_amd
