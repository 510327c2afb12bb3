// encode_resize.hip -- the front stage of fpng_amd_encode_submit_renditions: enc_resize_kernel resamples a box of a source image,
// where and how it lies, into the tight R,G,B[,A] rows that the encode chain reads (encode_resize.h has the record, the source
// accessor and the LDS formula; resize.h the rule of the weights; view_alpha.h the alpha rule).
//
// One workgroup per (rendition, tile of kResizeTileW x kResizeTileH output pixels), on an exact one-dimensional grid over the
// prefix sums of the renditions' tiles:
//   1. a thread per column / row of the tile computes the first tap, tap count and weights of its sample into LDS
//      (resample_tile_weights, every filter a value: the text the host's twin runs): Kx[t][column], Ky[t][row] -- once, not per channel;
//   2. per channel the horizontal pass over the box rows that the tile's Ky reach -- a wave per row, a lane per column, the taps
//      through the source accessor (neighbouring lanes read neighbouring pixels), the weights from LDS without bank conflicts -- into
//      LDS bytes T[row][column], then the vertical pass out of T, a thread's result bytes of its four rows kept in four registers,
//      a byte per channel.  A premultiplied rendition's colour channels are M(v, a) of two channels of the same source pixel on
//      load, and U(R'_c, R'_3) of the four result bytes of a register before the store.  FUSED (EncResize::fused, the host's
//      enc_resize_fused: a 4-byte interleaved source whose tile holds T once per channel within 32 KB): the horizontal pass makes
//      all channels from ONE dword load per tap (enc_row_sums4) into a T plane each, and the vertical passes follow without a
//      barrier between them;
//   3. the registers go to LDS as O[row][column * chans + chan], in the place of the weights and T, and a wave per row writes the
//      row's run of whole pixels in memory order: single bytes up to the first 4-byte boundary, dwords, single bytes behind the last.
// The sums are integers, so their order is free; no atomics, nothing between workgroups.  Nothing is read but bytes of the box's
// pixels (4-byte sources: the aligned dword that is the pixel) and nothing written but the rendition's own w * h * chans bytes.
#include <hip/hip_runtime.h>

#include "encode_resize.h"
#include "exact_grid.h"
#include "resize_tile.h"

#include <algorithm>

namespace fpng_amd {

namespace {

// kYuv: the submission's sources are YUV surfaces (enc_row_sum<true>)
template <bool kYuv> __global__ __launch_bounds__(kResizeBlock) void enc_resize_kernel(const EncResize *recs, const uint64_t *pre, uint32_t n, const EncConsts *__restrict__ consts_in)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t enc_resize_lds[];
    uint64_t g;
    const uint32_t lo = exact_grid_find(pre, n, blockIdx.x, g);
    const EncResize r = recs[lo];
    const EncConsts &consts = *consts_in;
    const uint32_t C = r.chans;
    const uint32_t tile = (uint32_t)exact_grid_within(pre, lo, g);
    if ((uint64_t)tile >= resize_tiles(r.w, r.h)) return; // (never, with the host's pre)
    uint32_t ox0, oq0, nw, nq;
    resize_tile_at(tile, r.w, r.h, ox0, oq0, nw, nq);
    FPNG_RESIZE_TILE_LDS(enc_resize_lds, r.taps_x, r.taps_y);
    uint8_t *const O = enc_resize_lds; // (once the passes are done, in the place of everything else)
    const uint32_t tid = threadIdx.x;
    // ---- 1. the tile's weights: samples of the box (in_w x in_h) resized to w x h ----
    if (tid < kResizeTileW) {
        uint32_t first = 0, count = 0;
        if (tid < nw) count = resample_tile_weights(r.filter, r.in_w, r.w, ox0 + tid, r.nearest, ox0 + tid, &first, Kx + tid, kResizeTileW, r.taps_x);
        fx[tid] = first, cx[tid] = count;
    } else if (tid < kResizeTileW + kResizeTileH) {
        const uint32_t q = tid - kResizeTileW;
        uint32_t first = 0, count = 0;
        if (q < nq) count = resample_tile_weights(r.filter, r.in_h, r.h, oq0 + q, r.nearest ? r.nearest + r.w : nullptr, oq0 + q, &first, Ky + q, kResizeTileH, r.taps_y);
        fy[q] = first, cy[q] = count;
    }
    __syncthreads();
    // ---- 2. per channel: the horizontal pass into T, the vertical pass out of it into a byte of res[k] -- row wave + 4 k of the
    //      tile, column o, channel c in byte c ----
    const uint32_t row0 = fy[0];
    const uint32_t nrows = std::min(fy[nq - 1] + cy[nq - 1] - row0, r.rows); // (the host's bound holds: T has r.rows rows)
    const uint32_t o = tid % kResizeTileW, wave = tid / kResizeTileW;
    constexpr uint32_t kWaves = kResizeBlock / kResizeTileW, kRowsPerWave = kResizeTileH / kWaves;
    uint32_t res[kRowsPerWave] = {};
    // the vertical pass of channel c out of its horizontal bytes Tc
    auto vertical = [&](const uint8_t *Tc, uint32_t c) {
        if (o >= nw) return;
#pragma unroll
        for (uint32_t k = 0; k < kRowsPerWave; k++) {
            const uint32_t q = wave + k * kWaves;
            if (q >= nq) break;
            const uint32_t first = fy[q] - row0;
            const uint32_t count = first < nrows ? std::min(cy[q], nrows - first) : 0u;
            int32_t sum = 1 << (kResizeBits - 1);
            for (uint32_t t = 0; t < count; t++) sum += (int32_t)Tc[(first + t) * kResizeTileW + o] * Ky[t * kResizeTileH + q];
            res[k] |= resize_clip8(sum) << (8 * c);
        }
    };
    const uint32_t first_x = fx[o], count_x = cx[o]; // (a column past the rendition's edge: no taps)
    if (r.fused) { // (a 4-byte source whose tile holds T once per channel: one load per tap for all of them)
        const uint32_t plane = r.rows * kResizeTileW;
        for (uint32_t j = wave; j < nrows; j += kWaves) {
            const EncSums4 s = enc_row_sums4(r, row0 + j, first_x, count_x, Kx + o, kResizeTileW);
            uint8_t *const t = T + j * kResizeTileW + o;
            t[0] = (uint8_t)resize_clip8(s.c0), t[plane] = (uint8_t)resize_clip8(s.c1), t[2 * plane] = (uint8_t)resize_clip8(s.c2);
            if (C == 4) t[3 * plane] = (uint8_t)resize_clip8(s.c3);
        }
        __syncthreads();
        for (uint32_t c = 0; c < C; c++) vertical(T + c * plane, c);
    } else
        for (uint32_t c = 0; c < C; c++) {
            if (c) __syncthreads(); // (the channel before has been read out of T)
            for (uint32_t j = wave; j < nrows; j += kWaves) T[j * kResizeTileW + o] = (uint8_t)resize_clip8(enc_row_sum<kYuv>(r, consts, c, row0 + j, first_x, count_x, Kx + o, kResizeTileW));
            __syncthreads();
            vertical(T, c);
        }
    if (r.premul) {
#pragma unroll
        for (uint32_t k = 0; k < kRowsPerWave; k++) res[k] = enc_unmul_pixel(res[k]);
    }
    __syncthreads(); // (weights, taps and T have been read for the last time: O takes their place)
    const uint32_t o_stride = kResizeTileW * C; // bytes of a row of O
    if (o < nw) {
#pragma unroll
        for (uint32_t k = 0; k < kRowsPerWave; k++) {
            const uint32_t q = wave + k * kWaves;
            if (q >= nq) break;
            uint8_t *const p = O + q * o_stride + o * C;
            if (C == 4) *(uint32_t *)p = res[k];
            else p[0] = (uint8_t)res[k], p[1] = (uint8_t)(res[k] >> 8), p[2] = (uint8_t)(res[k] >> 16);
        }
    }
    __syncthreads();
    // ---- 3. the store: a wave per row, the row's run of nw whole pixels in memory order ----
    const uint32_t n_el = nw * C;
    for (uint32_t q = wave; q < nq; q += kWaves) {
        const uint8_t *const Oq = O + q * o_stride;
        uint8_t *const D = r.dst + (uint64_t)(oq0 + q) * ((uint64_t)r.w * C) + (uint64_t)ox0 * C;
        resize_tile_run<1>(D, n_el, o, [&](uint32_t e) { D[e] = Oq[e]; },
                           [&](uint32_t e) { *(uint32_t *)(D + e) = Oq[e] | (uint32_t)Oq[e + 1] << 8 | (uint32_t)Oq[e + 2] << 16 | (uint32_t)Oq[e + 3] << 24; });
    }
}

} // namespace

bool launch_enc_resize(hipStream_t s, const EncResize *recs, const uint64_t *pre, const uint64_t *h_pre, uint32_t n, uint32_t lds_bytes, const EncConsts *consts, bool yuv)
{
    if (lds_bytes > kEncResizeMaxLds) return false;
    return exact_grid_walk(h_pre, n, kResizeBlock, [&](uint32_t r0, uint32_t r1, uint32_t groups) {
        hipLaunchKernelGGL(yuv ? enc_resize_kernel<true> : enc_resize_kernel<false>, dim3(groups), dim3(kResizeBlock), lds_bytes, s, recs + r0, pre + r0, r1 - r0, consts);
    });
}

} // namespace fpng_amd
