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

#include <algorithm>

namespace fpng_amd {

namespace {

// kYuv: the submission's sources are YUV surfaces (enc_row_sum<true>)
template <bool kYuv> __global__ __launch_bounds__(kResizeBlock) void enc_resize_kernel(const EncResize *recs, const uint64_t *pre, uint32_t n, const EncConsts *__restrict__ consts_in)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t enc_resize_lds[];
    const uint64_t g = pre[0] + blockIdx.x;
    uint32_t lo = 0, hi = n; // pre[lo] <= g < pre[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pre[mid] <= g) lo = mid;
        else hi = mid;
    }
    const EncResize r = recs[lo];
    const EncConsts &consts = *consts_in;
    const uint32_t C = r.chans;
    const uint32_t tile = (uint32_t)(g - pre[lo]);
    if ((uint64_t)tile >= resize_tiles(r.w, r.h)) return; // (never, with the host's pre)
    const uint32_t tiles_x = (r.w + kResizeTileW - 1) / kResizeTileW;
    const uint32_t ox0 = tile % tiles_x * kResizeTileW, oq0 = tile / tiles_x * kResizeTileH;
    const uint32_t nq = std::min(kResizeTileH, r.h - oq0), nw = std::min(kResizeTileW, r.w - ox0);
    int32_t *const Kx = (int32_t *)enc_resize_lds, *const Ky = Kx + r.taps_x * kResizeTileW;
    uint32_t *const fx = (uint32_t *)(Ky + r.taps_y * kResizeTileH), *const cx = fx + kResizeTileW, *const fy = cx + kResizeTileW, *const cy = fy + kResizeTileH;
    uint8_t *const T = (uint8_t *)(cy + kResizeTileH), *const O = enc_resize_lds; // (O: once the passes are done, in the place of everything else)
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
        const uint32_t head = std::min(n_el, (0u - (uint32_t)(uintptr_t)D) & 3u);
        const uint32_t nd = (n_el - head) / 4u, tail0 = head + nd * 4u;
        if (o < head) D[o] = Oq[o];
        for (uint32_t d = o; d < nd; d += kResizeTileW) {
            const uint32_t e = head + d * 4u;
            *(uint32_t *)(D + e) = Oq[e] | (uint32_t)Oq[e + 1] << 8 | (uint32_t)Oq[e + 2] << 16 | (uint32_t)Oq[e + 3] << 24;
        }
        if (tail0 + o < n_el) D[tail0 + o] = Oq[tail0 + o];
    }
}

} // namespace

bool launch_enc_resize(hipStream_t s, const EncResize *recs, const uint64_t *pre, const uint64_t *h_pre, uint32_t n, uint32_t lds_bytes, const EncConsts *consts, bool yuv)
{
    // (a launch holds fewer than 2^32 threads: fewer than 2^24 workgroups)
    constexpr uint64_t kMaxGrid = (1ull << 32) / kResizeBlock - 1;
    if (lds_bytes > kEncResizeMaxLds) return false;
    for (uint32_t r0 = 0; r0 < n;) {
        uint32_t r1 = r0 + 1;
        if (h_pre[r1] <= h_pre[r0] || h_pre[r1] - h_pre[r0] > kMaxGrid) return false;
        while (r1 < n && h_pre[r1 + 1] > h_pre[r1] && h_pre[r1 + 1] - h_pre[r0] <= kMaxGrid) r1++;
        hipLaunchKernelGGL(yuv ? enc_resize_kernel<true> : enc_resize_kernel<false>, dim3((uint32_t)(h_pre[r1] - h_pre[r0])), dim3(kResizeBlock), lds_bytes, s, recs + r0, pre + r0, r1 - r0, consts);
        r0 = r1;
    }
    return true;
}

} // namespace fpng_amd
