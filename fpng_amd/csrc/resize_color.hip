// resize_color.hip -- the second stage of fpng_amd_decode_batch(_device)_planar_views_color and _hwc_views_color: the resize of
// resize.hip's dec_resize_hwc_kernel -- one workgroup per (record, tile of kResizeTileW x kResizeTileH samples of the window), ALL
// planes, the exact grid with pre counting tiles -- with the view's 3 x 4 colour matrix (resize_color.h: color_apply, the text the
// host's fpng_amd_color_apply runs) between the resize's bytes and the element that is stored.  A workgroup per plane, as the planar
// kernels of resize.hip run, cannot mix channels; this one has a pixel's three bytes in one thread.
//   1. the tile's weights, first taps and tap counts -- once, not once per plane;
//   2. per plane the two integer passes through the same T bytes (the same sums, guards and resize_clip8 as dec_resize_tile), a
//      thread's result BYTES of its four rows kept in four registers, a byte per plane: the R_c[y + q][x + i] of the plain call;
//   3. the store.
//      Planar destinations (kHwc = false): straight out of those registers -- a thread has all channels of its pixels, plane c's
//      element is color_apply(m[c], r, g, b) and the wave's lanes are neighbouring columns of one row of one plane, in either
//      mirror direction, as in dec_resize_tile.  No LDS behind the passes, and resize_tile_lds() bytes of it.
//      Channels-last destinations (kHwc = true): a thread turns each of its pixels into its elements in the same way and puts
//      their BITS into LDS, a row of the tile per wave in the place of the weights (within resize_hwc_tile_lds() bytes); the wave
//      then walks the row's run in memory order as dec_resize_hwc_kernel does -- pixel_elems, reversed, positions >= planes never
//      written, dwords where the run allows -- copying what it finds.  (Applying the matrix per ELEMENT of the run instead, its
//      row chosen by the element's channel, needs the pixel's three bytes and twelve selects per element.)
// A fourth channel (alpha, or the 255 of a 3-channel file) skips the matrix.  The kernels of resize.hip are not touched: the two
// passes are repeated here.
// kAlpha (view_alpha.h): the load of step 2 makes P'; a PREMULTIPLIED view runs the passes for all
// FOUR planes, whatever the destination's count, and divides the three colour bytes by R'_3 in front of the matrix.
#include "decode.h"
#include "exact_grid.h"
#include "float_store.h"
#include "resize.h"
#include "resize_color.h"
#include "resize_hwc.h"
#include "resize_tile.h"
#include "view_alpha.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace fpng_amd {

namespace {

// kResample: as dec_resize_tile's (resize.hip)
template <int kDtype, bool kAnyFilter, bool kHwc, bool kAlpha = false, bool kResample = false>
__global__ __launch_bounds__(kResizeBlock) void dec_resize_color_kernel(const DecResizeColor *recs, const uint64_t *pre, uint32_t n, DecFloat flt)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t resize_lds[];
    uint64_t g;
    const uint32_t lo = exact_grid_find(pre, n, blockIdx.x, g);
    const DecResize r = recs[lo].d.r;
    const uint32_t C = r.planes;
    const uint32_t tile = (uint32_t)exact_grid_within(pre, lo, g);
    if ((uint64_t)tile >= resize_tiles(r.w, r.h)) return; // (never, with the host's pre)
    uint32_t ox0, oq0, nw, nq;
    resize_tile_at(tile, r.w, r.h, ox0, oq0, nw, nq);
    FPNG_RESIZE_TILE_LDS(resize_lds, r.taps_x, r.taps_y);
    const uint32_t tid = threadIdx.x;
    [[maybe_unused]] const uint32_t filter = kAnyFilter ? r.filter : kResizeBilinear;
    // ---- 1. the tile's weights ----
    if (tid < kResizeTileW) {
        uint32_t first = r.box_x, count = 0;
        if constexpr (kResample) {
            if (tid < nw) count = resample_tile_weights(r.filter, r.in_w, r.full_w, r.x + ox0 + tid, r.nearest, ox0 + tid, &first, Kx + tid, kResizeTileW, r.taps_x);
        } else if (tid < nw) count = resize_weights_of(filter, r.in_w, r.full_w, r.x + ox0 + tid, &first, Kx + tid, kResizeTileW, r.taps_x);
        fx[tid] = first - r.box_x, cx[tid] = count;
    } else if (tid < kResizeTileW + kResizeTileH) {
        const uint32_t q = tid - kResizeTileW;
        uint32_t first = r.box_y, count = 0;
        if constexpr (kResample) {
            if (q < nq) count = resample_tile_weights(r.filter, r.in_h, r.full_h, r.y + oq0 + q, r.nearest + r.w, oq0 + q, &first, Ky + q, kResizeTileH, r.taps_y);
        } else if (q < nq) count = resize_weights_of(filter, r.in_h, r.full_h, r.y + oq0 + q, &first, Ky + q, kResizeTileH, r.taps_y);
        fy[q] = first - r.box_y, cy[q] = count;
    }
    __syncthreads();
    // ---- 2. per plane: the horizontal pass into T, the vertical pass out of it into a byte of res[k] -- row wave + 4 k of the
    //      tile, column o, plane b in byte b ----
    const uint32_t row0 = fy[0];
    const uint32_t nrows = std::min(fy[nq - 1] + cy[nq - 1] - row0, r.rows); // (the host's bound holds: T has r.rows rows)
    const uint32_t o = tid % kResizeTileW, wave = tid / kResizeTileW;
    constexpr uint32_t kWaves = kResizeBlock / kResizeTileW, kRowsPerWave = kResizeTileH / kWaves;
    uint32_t res[kRowsPerWave] = {};
    [[maybe_unused]] const uint32_t a_op = kAlpha ? resize_alpha_op(r.flags) : 0u;
    const uint32_t n_planes = kAlpha && a_op == kAlphaPremultiplied ? 4u : C;
    for (uint32_t plane = 0; plane < n_planes; plane++) {
        if (plane) __syncthreads(); // (the plane before has been read out of T)
        const uint8_t *const S = r.src + (uint64_t)plane * r.src_plane_pitch;
        {
            const uint32_t first = fx[o], count = cx[o];
            for (uint32_t j = wave; j < nrows; j += kWaves) {
                const uint8_t *s = S + (uint64_t)(row0 + j) * r.src_pitch + first;
                int32_t sum = 1 << (kResizeBits - 1);
                if constexpr (kAlpha) // (the sum over P'; the alpha plane's byte: the same offset, 3 - plane planes on)
                    sum = alpha_pass_sum(alpha_load_mode(a_op, plane), s, s + (uint64_t)(3u - plane) * r.src_plane_pitch, resize_alpha_bg(r.flags, plane), count, Kx + o, kResizeTileW);
                else
                    for (uint32_t t = 0; t < count; t++) sum += (int32_t)s[t] * Kx[t * kResizeTileW + o];
                T[j * kResizeTileW + o] = (uint8_t)resize_clip8(sum);
            }
        }
        __syncthreads();
        if (o < nw) {
#pragma unroll
            for (uint32_t k = 0; k < kRowsPerWave; k++) {
                const uint32_t q = wave + k * kWaves;
                if (q >= nq) break;
                const uint32_t first = fy[q] - row0;
                const uint32_t count = first < nrows ? std::min(cy[q], nrows - first) : 0u;
                int32_t sum = 1 << (kResizeBits - 1);
                for (uint32_t t = 0; t < count; t++) sum += (int32_t)T[(first + t) * kResizeTileW + o] * Ky[t * kResizeTileH + q];
                res[k] |= resize_clip8(sum) << (8 * plane);
            }
        }
    }
    if constexpr (kAlpha)
        if (a_op == kAlphaPremultiplied) { // (step 3 of the alpha rule: in front of the matrix)
#pragma unroll
            for (uint32_t k = 0; k < kRowsPerWave; k++) {
                const uint32_t a = res[k] >> 24;
                res[k] = alpha_unmul(res[k] & 255u, a) | alpha_unmul(res[k] >> 8 & 255u, a) << 8 | alpha_unmul(res[k] >> 16 & 255u, a) << 16 | a << 24;
            }
        }
    // ---- 3. the store ----
    // (the view's matrix: the same for all of the workgroup's threads; every index below is a constant)
    const float m00 = recs[lo].m[0][0], m01 = recs[lo].m[0][1], m02 = recs[lo].m[0][2], m03 = recs[lo].m[0][3];
    const float m10 = recs[lo].m[1][0], m11 = recs[lo].m[1][1], m12 = recs[lo].m[1][2], m13 = recs[lo].m[1][3];
    const float m20 = recs[lo].m[2][0], m21 = recs[lo].m[2][1], m22 = recs[lo].m[2][2], m23 = recs[lo].m[2][3];
    constexpr uint32_t kElem = kDtype < 0 ? 1u : dec_float_bytes((uint32_t)kDtype);
    const bool mirror = r.flags & kResizeMirror;
    if constexpr (!kHwc) {
        if (o >= nw) return;
        const uint32_t col = mirror ? r.w - 1 - (ox0 + o) : ox0 + o;
        uint8_t *const D = r.dst + (int64_t)col * kElem;
#pragma unroll
        for (uint32_t k = 0; k < kRowsPerWave; k++) {
            const uint32_t q = wave + k * kWaves;
            if (q >= nq) break;
            const float rr = (float)(res[k] & 255u), gg = (float)(res[k] >> 8 & 255u), bb = (float)(res[k] >> 16 & 255u), aa = (float)(res[k] >> 24);
            uint8_t *const p = D + (int64_t)(oq0 + q) * r.pitch;
            elem_store<kDtype>(p, float_elem_bits<kDtype>(color_apply(m00, m01, m02, m03, rr, gg, bb), flt.scale[0], flt.bias[0]));
            elem_store<kDtype>(p + r.plane_pitch, float_elem_bits<kDtype>(color_apply(m10, m11, m12, m13, rr, gg, bb), flt.scale[1], flt.bias[1]));
            elem_store<kDtype>(p + 2 * r.plane_pitch, float_elem_bits<kDtype>(color_apply(m20, m21, m22, m23, rr, gg, bb), flt.scale[2], flt.bias[2]));
            if (C == 4) elem_store<kDtype>(p + 3 * r.plane_pitch, float_elem_bits<kDtype>(aa, flt.scale[3], flt.bias[3]));
        }
    } else {
        const uint32_t P = recs[lo].d.pixel_elems, reversed = recs[lo].d.hwc_flags & kHwcReversed;
        __syncthreads(); // (weights, taps and T have been read for the last time: the waves' row buffers take their place)
        // A wave and its own rows of the tile, one at a time: every lane turns its pixel into elements -- the channel a constant, no
        // select -- and puts their bits into the wave's row buffer, element k of pixel i at i * C + k; then the wave walks the row's
        // run in memory order out of the buffer.  Nothing but the wave itself touches its buffer: LDS operations of one wave
        // complete in order, and the wavefront fences keep the compiler from moving them across.
        const uint32_t row_buf = kResizeTileW * C * kElem + (kElem < 4 ? 4u : 0u); // (4 of them <= kResizeTileH * kResizeTileW * C)
        uint8_t *const W = resize_lds + wave * row_buf;
        const uint32_t d0 = mirror ? r.w - ox0 - nw : ox0; // the run's first pixel of the destination's row
        const uint32_t n_el = (nw - 1) * P + C;            // the run's elements, up to the last one that is written
        const bool dwords = kElem < 4 && P == C;           // every element of the run is written, and they are narrower than a dword
        const uint32_t i = mirror ? nw - 1 - o : o;        // this lane's pixel of the run
#pragma unroll
        for (uint32_t k = 0; k < kRowsPerWave; k++) {
            const uint32_t q = wave + k * kWaves;
            if (q >= nq) break; // (the same for all of the wave's lanes)
            uint8_t *const D = r.dst + (int64_t)(oq0 + q) * r.pitch + (int64_t)((uint64_t)d0 * P * kElem);
            // (dword runs: the buffer's elements start at D's offset within its dword, so that a dword of memory is one of LDS)
            uint8_t *const B = W + (dwords ? (uint32_t)(uintptr_t)D & 3u : 0u);
            if (o < nw) {
                const float rr = (float)(res[k] & 255u), gg = (float)(res[k] >> 8 & 255u), bb = (float)(res[k] >> 16 & 255u), aa = (float)(res[k] >> 24);
                uint8_t *const px = B + (size_t)i * C * kElem;
                const uint32_t last = (C - 1) * kElem; // (reversed: file channel c is element C - 1 - c of its pixel)
                elem_store<kDtype>(px + (reversed ? last : 0u), float_elem_bits<kDtype>(color_apply(m00, m01, m02, m03, rr, gg, bb), flt.scale[0], flt.bias[0]));
                elem_store<kDtype>(px + (reversed ? last - kElem : kElem), float_elem_bits<kDtype>(color_apply(m10, m11, m12, m13, rr, gg, bb), flt.scale[1], flt.bias[1]));
                elem_store<kDtype>(px + (reversed ? last - 2 * kElem : 2 * kElem), float_elem_bits<kDtype>(color_apply(m20, m21, m22, m23, rr, gg, bb), flt.scale[2], flt.bias[2]));
                if (C == 4) elem_store<kDtype>(px + (reversed ? 0u : 3 * kElem), float_elem_bits<kDtype>(aa, flt.scale[3], flt.bias[3]));
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            auto copy1 = [&](uint32_t e, uint32_t at) __attribute__((always_inline)) { // element e of the run: element `at` of the buffer
                if constexpr (kDtype < 0) D[e] = B[at];
                else if constexpr (kDtype == 0) *(f32_a *)(D + (size_t)e * 4) = *(const float *)(B + (size_t)at * 4);
                else *(u16_a *)(D + (size_t)e * 2) = *(const uint16_t *)(B + (size_t)at * 2);
            };
            if (!dwords) {
                for (uint32_t e = o; e < n_el; e += kResizeTileW) {
                    if (P == C) copy1(e, e);
                    else if ((e & 3u) < C) copy1(e, (e >> 2) * C + (e & 3u)); // (P == 4: position e % 4; 3 is the caller's)
                }
            } else {
                resize_tile_run<kElem < 4 ? kElem : 1u>(D, n_el, o, [&](uint32_t e) { copy1(e, e); }, [&](uint32_t e) {
                    const size_t at = (size_t)e * kElem;
                    *(uint32_t *)(D + at) = *(const uint32_t *)(B + at);
                });
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // (the next row's elements go into the same buffer)
        }
    }
}

// The instantiations by index: alpha (0 / 1), channels-last (0 / 1), the launch's kind of filters (resize.h: triangle alone, both
// filters, resample), element (0: bytes, 1 + dtype).  kAnyFilter is the kind >= 1, kResample the kind == 2.
constexpr uint32_t color_index(uint32_t alpha, uint32_t hwc, uint32_t kind, uint32_t elem) { return ((alpha * 2 + hwc) * kResizeLaunchKinds + kind) * (kDecFloatTypes + 1) + elem; }
template <uint32_t I> struct ColorAt {
    static constexpr uint32_t kKind = I / (kDecFloatTypes + 1) % kResizeLaunchKinds, kForm = I / (kDecFloatTypes + 1) / kResizeLaunchKinds;
    static constexpr auto value = dec_resize_color_kernel<(int)(I % (kDecFloatTypes + 1)) - 1, kKind >= 1, kForm % 2 != 0, kForm / 2 != 0, kKind == 2>;
};

} // namespace

bool launch_dec_resize_color(hipStream_t s, const DecResizeColor *recs, const uint64_t *pre, const uint64_t *h_pre, uint32_t n, uint32_t lds_bytes, const DecFloat *flt, uint32_t filters,
                             bool hwc, bool any_alpha)
{
    static constexpr auto kernels = exact_grid_table<ColorAt, color_index(1, 1, kResizeLaunchKinds - 1, kDecFloatTypes) + 1>();
    if (lds_bytes > 65536u || filters >= kResizeLaunchKinds) return false;
    return exact_grid_walk(h_pre, n, kResizeBlock, [&](uint32_t r0, uint32_t r1, uint32_t groups) {
        hipLaunchKernelGGL(kernels[color_index(any_alpha, hwc, filters, flt ? flt->dtype + 1 : 0)], dim3(groups), dim3(kResizeBlock), lds_bytes, s, recs + r0, pre + r0, r1 - r0, flt ? *flt : DecFloat{});
    });
}

} // namespace fpng_amd
