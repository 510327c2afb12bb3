// view_tone.hip -- the two kernels in front of the post stage of fpng_amd_decode_batch(_device)_planar_views_tone and _hwc_views_tone
// (view_tone.h: the rule, and the text the host's fpng_amd_view_tone_lut runs): a tone view's histograms and its tables.
//
// dec_view_tone_hist_kernel: tone views only, a workgroup per (tone view, chunk of kToneChunk consecutive samples of its window),
//   the exact grid with refs[].pre counting chunks.  A sample is loaded exactly as dec_view_post_kernel loads it: the plain byte of
//   the un-mirrored window in the scratch, or warp_locate / warp_sample for a view with a warp (fill samples count).  The window has
//   just been written by the resize and is read from L2.  A workgroup counts into four 256-bin uint32 histograms in LDS (4 KB) with
//   LDS atomics -- the three channels' for autocontrast and equalize, the luma's alone for contrast -- and then adds its non-zero
//   bins to the view's uint32[4][256] in the scratch with global atomics: integer adds, so the result does not depend on the order.
//   A chunk is eight tiles' worth (8192 samples): up to 24576 LDS atomics against at most 768 global ones.  The caller zeroes the
//   views' histograms on the stream in front of the launch.
// dec_view_tone_lut_kernel: a workgroup of 256 threads per tone view, thread v writes lut[c][v].  Equalize's running n is an
//   inclusive LDS scan of the 64-bit counts, lo / hi / the number of non-zero bins are LDS atomics, the luma sum is the same scan's
//   last element; the entries are view_tone.h's.
#include "view_post.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace fpng_amd {

namespace {

constexpr uint32_t kToneLutBlock = 256;

__global__ __launch_bounds__(kResizeBlock) void dec_view_tone_hist_kernel(const DecViewPost *recs, const DecToneRef *refs, uint32_t n)
{
    __shared__ uint32_t H[kToneHistWords];
    uint64_t g;
    const uint32_t lo = exact_grid_find(refs, n, blockIdx.x, g); // (refs[].pre: exact_grid_pre of view_post.h)
    const DecViewPost &r = recs[refs[lo].rec];
    const uint32_t w = r.w, h = r.h, op = r.tone_op;
    const uint64_t total = (uint64_t)w * h, first = exact_grid_within(refs, lo, g) * kToneChunk; // (total < 2^32: the host)
    if (!op || !r.tone || first >= total) return;                                    // (never, with the host's refs)
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < kToneHistWords; k += kResizeBlock) H[k] = 0;
    __syncthreads();
    const uint32_t i0 = (uint32_t)first, i1 = (uint32_t)std::min<uint64_t>(total, first + kToneChunk);
    const uint32_t wflags = r.warp.flags, mirror = r.mirror;
    const uint8_t *const src = r.src;
    for (uint32_t i = i0 + tid; i < i1; i += kResizeBlock) {
        uint32_t c[3];
        if (wflags) {
            const WarpAt at = warp_locate(r.warp, i % w, i / w, w, h, mirror);
#pragma unroll
            for (uint32_t p = 0; p < 3; p++) c[p] = warp_sample(at, wflags, src + p * total, w, r.warp.fill[p]) & 255u;
        } else {
#pragma unroll
            for (uint32_t p = 0; p < 3; p++) c[p] = src[p * total + i];
        }
        if (op == kToneContrast) atomicAdd(&H[3 * 256 + (tone_luma(c[0], c[1], c[2]) & 255u)], 1u);
        else {
#pragma unroll
            for (uint32_t p = 0; p < 3; p++) atomicAdd(&H[p * 256 + c[p]], 1u);
        }
    }
    __syncthreads();
    for (uint32_t k = tid; k < kToneHistWords; k += kResizeBlock)
        if (const uint32_t v = H[k]) atomicAdd(r.tone + k, v);
}

// the inclusive sums of x over the workgroup's 256 threads (*total: the last one).  Every thread of the workgroup calls it.
__device__ __forceinline__ uint64_t tone_scan(uint64_t x, uint64_t (*P)[kToneLutBlock], uint32_t v, uint64_t *total)
{
    uint32_t cur = 0;
    P[0][v] = x;
    __syncthreads();
    for (uint32_t d = 1; d < kToneLutBlock; d <<= 1) {
        P[cur ^ 1][v] = P[cur][v] + (v >= d ? P[cur][v - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    const uint64_t mine = P[cur][v];
    *total = P[cur][kToneLutBlock - 1];
    __syncthreads(); // (P is free again)
    return mine;
}

__global__ __launch_bounds__(kToneLutBlock) void dec_view_tone_lut_kernel(const DecViewPost *recs, const DecToneRef *refs)
{
    __shared__ uint64_t P[2][kToneLutBlock];
    __shared__ uint32_t ends[3]; // lo, hi, the non-zero bins of a channel
    const DecViewPost &r = recs[refs[blockIdx.x].rec];
    const uint32_t op = r.tone_op, v = threadIdx.x;
    if (!op || !r.tone) return; // (never; uniform)
    const uint32_t *const hist = r.tone;
    uint8_t *const lut = (uint8_t *)(r.tone + kToneHistWords);
    if (op == kToneContrast) {
        uint64_t sum;
        tone_scan((uint64_t)v * hist[3 * 256 + v], P, v, &sum);
        const uint32_t mean = tone_contrast_mean(sum, (uint64_t)r.w * r.h);
        const uint8_t e = (uint8_t)tone_contrast_entry(v, mean, r.tone_factor);
        lut[v] = lut[256 + v] = lut[512 + v] = e;
        return;
    }
    for (uint32_t c = 0; c < 3; c++) {
        const uint32_t hv = hist[c * 256 + v];
        if (v == 0) ends[0] = 255u, ends[1] = 0u, ends[2] = 0u;
        uint64_t total;
        const uint64_t upto = tone_scan(hv, P, v, &total); // (its barriers stand between the line above and the atomics below)
        if (hv) atomicMin(&ends[0], v), atomicMax(&ends[1], v), atomicAdd(&ends[2], 1u);
        __syncthreads();
        const uint32_t first = ends[0], last = ends[1], bins = ends[2];
        uint32_t e;
        if (op == kToneAutocontrast) e = tone_autocontrast_entry(v, first, last);
        else e = tone_equalize_entry(v, upto - hv, tone_equalize_step(total, hist[c * 256 + last], bins));
        lut[c * 256 + v] = (uint8_t)e;
        __syncthreads(); // (ends is read; the next channel sets it again)
    }
}

} // namespace

bool launch_dec_view_tone(hipStream_t s, const DecViewPost *recs, const DecToneRef *refs, const DecToneRef *h_refs, uint32_t n)
{
    if (!exact_grid_walk(h_refs, n, kResizeBlock, [&](uint32_t r0, uint32_t r1, uint32_t groups) { hipLaunchKernelGGL(dec_view_tone_hist_kernel, dim3(groups), dim3(kResizeBlock), 0, s, recs, refs + r0, r1 - r0); }))
        return false;
    if (n) hipLaunchKernelGGL(dec_view_tone_lut_kernel, dim3(n), dim3(kToneLutBlock), 0, s, recs, refs);
    return true;
}

} // namespace fpng_amd
