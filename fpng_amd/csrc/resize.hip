// resize.hip -- the second stage of fpng_amd_decode_batch(_device)_planar_resize, _planar_resize_view and _planar_views: uint8
// planes of the file, which the crop kernels of decode.hip (dec_unfilter_crop_kernel<-1, *>, dec_stored_crop_kernel<-1>) left in the
// decode scratch, are resized by the rule of resize.h (bilinear or bicubic; in the _views_resample calls also Pillow's nearest, box,
// Hamming and Lanczos), mirrored where asked, and written once -- bytes, or
// the float call's elements.  What is written is a WINDOW (x, y, w, h) of the crop resized to full_w x full_h (the plain resize
// call: the whole of it); the scratch holds the box of the crop that the window's taps reach, so a tap at crop column f is byte
// f - box_x of its row -- as a sub-rectangle of the planes of ONE box per file that holds the boxes of all of the file's views (the
// views call; the other calls have one view per file, whose box those planes are).
//
// One workgroup per (file, plane, tile of kResizeTileW x kResizeTileH samples of the window):
//   1. a thread per column / row of the tile computes the first tap, tap count and weights of sample x + column / y + row of the
//      full image (resize_weights_of, the text the host's fpng_amd_resize_weights_filter runs) into LDS: Kx[t][column], Ky[t][row];
//   2. the horizontal pass over the source rows the tile's Ky reach -- a wave per row, a lane per column, the row's bytes from
//      global memory (neighbouring lanes read neighbouring bytes: the same cache lines), the weights from LDS without bank
//      conflicts (consecutive lanes, consecutive dwords) -- into LDS bytes T[row][column];
//   3. the vertical pass out of T (a wave reads 64 consecutive bytes of a row, Ky[t][row] is one address for the wave: a
//      broadcast), then the mirror as an index of the store, the fmaf and the conversion of the float call, and stores that are
//      contiguous along a row for the wave in either direction.
// The sums are integers, so their order is free; no atomics, nothing between workgroups.  LDS is sized by the launch for the
// largest tile of its files (resize_tile_lds): ~8 KB for a 1080p crop -> 224 x 224, 55 KB at the bilinear 32 x limit, 41 KB at the
// bicubic 16 x limit.
#include "decode.h"
#include "exact_grid.h"
#include "float_store.h"
#include "resize.h"
#include "resize_hwc.h"
#include "resize_tile.h"
#include "view_alpha.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace fpng_amd {

namespace {

// One tile of one plane of one record: the kernels below find the three and hand them over.
// kAnyFilter: the launch's records may ask for the bicubic filter; false: all of them are bilinear (the plain resize call's launches,
// and a view call's whose files are), and the kernel holds the triangle's weight code alone.
// kAlpha: the launch's records may carry the COMPOSITE alpha op (view_alpha.h; the _views_alpha calls' launches that hold such a
// view): the load of the horizontal pass makes P' of the plane's and the alpha plane's bytes at the same offset.  A workgroup has
// one plane, so the PREMULTIPLIED op, whose store divides a colour plane's result by the alpha plane's, never comes here: a planar
// call with such a view runs dec_resize_color_kernel under identity matrices (decode_api.cpp: normalise_views).  false: the kernel
// that was there before there was an alpha stage
// kResample: the launch's records may carry a RESAMPLE filter (resize.h: NEAREST, BOX, HAMMING, LANCZOS): step 1 takes every record's
// weights from resample_tile_weights, the filter a value (kAnyFilter is then not looked at); false: the kernel as it was
template <int kDtype, bool kAnyFilter, bool kAlpha = false, bool kResample = false>
__device__ __forceinline__ void dec_resize_tile(const DecResize &r, uint32_t plane, uint32_t tile, const DecFloat &flt)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t resize_lds[];
    uint32_t ox0, oq0, nw, nq;
    resize_tile_at(tile, r.w, r.h, ox0, oq0, nw, nq);
    FPNG_RESIZE_TILE_LDS(resize_lds, r.taps_x, r.taps_y);
    const uint32_t tid = threadIdx.x;
    [[maybe_unused]] const uint32_t filter = kAnyFilter ? r.filter : kResizeBilinear;
    // ---- 1. the tile's weights (first: relative to the view's box, which the host made of these samples' own first and count --
    //      resize_taps -- so first >= box_x and first >= box_y, whatever the file's other views are) ----
    if (tid < kResizeTileW) {
        uint32_t first = r.box_x, count = 0;
        if constexpr (kResample) {
            if (ox0 + tid < r.w) count = resample_tile_weights(r.filter, r.in_w, r.full_w, r.x + ox0 + tid, r.nearest, ox0 + tid, &first, Kx + tid, kResizeTileW, r.taps_x);
        } else if (ox0 + tid < r.w) count = resize_weights_of(filter, r.in_w, r.full_w, r.x + ox0 + tid, &first, Kx + tid, kResizeTileW, r.taps_x);
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
    // ---- 2. the horizontal pass ----
    const uint32_t row0 = fy[0];
    const uint32_t nrows = std::min(fy[nq - 1] + cy[nq - 1] - row0, r.rows); // (the host's bound holds: T has r.rows rows)
    const uint32_t o = tid % kResizeTileW, wave = tid / kResizeTileW;
    const uint8_t *const P = r.src + (uint64_t)plane * r.src_plane_pitch;
    // (COMPOSITE, or no op: a PREMULTIPLIED view needs R'_3 next to its colour planes and goes to an all-planes kernel -- the host's rule)
    [[maybe_unused]] const uint32_t a_mode = kAlpha ? alpha_load_mode(resize_alpha_op(r.flags), plane) : kAlphaLoadRaw;
    {
        const uint32_t first = fx[o], count = cx[o];
        for (uint32_t j = wave; j < nrows; j += kResizeBlock / kResizeTileW) {
            const uint8_t *s = P + (uint64_t)(row0 + j) * r.src_pitch + first;
            int32_t sum = 1 << (kResizeBits - 1);
            if constexpr (kAlpha) // (the sum over P'; the alpha plane's byte: the same offset, 3 - plane planes on)
                sum = alpha_pass_sum(a_mode, s, s + (uint64_t)(3u - plane) * r.src_plane_pitch, resize_alpha_bg(r.flags, plane), count, Kx + o, kResizeTileW);
            else
                for (uint32_t t = 0; t < count; t++) sum += (int32_t)s[t] * Kx[t * kResizeTileW + o];
            T[j * kResizeTileW + o] = (uint8_t)resize_clip8(sum);
        }
    }
    __syncthreads();
    // ---- 3. the vertical pass, the mirror, the element ----
    if (ox0 + o >= r.w) return; // (o >= nw, in the spelling this kernel was compiled with: the other one moves its instructions)
    const uint32_t col = r.flags & kResizeMirror ? r.w - 1 - (ox0 + o) : ox0 + o;
    constexpr uint32_t kElem = kDtype < 0 ? 1u : dec_float_bytes((uint32_t)kDtype);
    float sc, bi; // (plane b of the record is the FILE's channel b, whatever the planes' order in memory)
    float_scale_bias(flt, plane, sc, bi);
    uint8_t *const D = r.dst + (int64_t)plane * r.plane_pitch + (int64_t)col * kElem;
    for (uint32_t q = wave; q < nq; q += kResizeBlock / kResizeTileW) {
        const uint32_t first = fy[q] - row0;
        const uint32_t count = first < nrows ? std::min(cy[q], nrows - first) : 0u;
        int32_t sum = 1 << (kResizeBits - 1);
        for (uint32_t t = 0; t < count; t++) sum += (int32_t)T[(first + t) * kResizeTileW + o] * Ky[t * kResizeTileH + q];
        elem_store<kDtype>(D + (int64_t)(oq0 + q) * r.pitch, byte_elem_bits<kDtype>(resize_clip8(sum), sc, bi));
    }
}

// The rectangular grid of the calls with one output per file: (the launch's largest record's tiles, 4 planes, records); the surplus
// workgroups of smaller records leave at once.
template <int kDtype, bool kAnyFilter>
__global__ __launch_bounds__(kResizeBlock) void dec_resize_kernel(const DecResize *recs, DecFloat flt)
{
    const DecResize r = recs[blockIdx.z];
    if (blockIdx.y >= r.planes || (uint64_t)blockIdx.x >= resize_tiles(r.w, r.h)) return; // (the grid is the launch's largest file)
    dec_resize_tile<kDtype, kAnyFilter>(r, blockIdx.y, blockIdx.x, flt);
}

// The exact grid of the views call, whose records mix sizes and plane counts by design: one dimension, a workgroup per (record,
// plane, tile) and none in surplus.  pre[k] (k = 0 .. n): the workgroups of the batch's records in front of this launch's record k
// (planes x tiles each, never 0), so workgroup b of the launch is number pre[0] + b of the batch and belongs to the last record
// whose pre is not above that; the launch has pre[n] - pre[0] workgroups.  The search is the same for all of a workgroup's threads.
template <int kDtype, bool kAnyFilter, bool kAlpha = false, bool kResample = false>
__global__ __launch_bounds__(kResizeBlock) void dec_resize_exact_kernel(const DecResize *recs, const uint64_t *pre, uint32_t n, DecFloat flt)
{
    uint64_t g;
    const uint32_t lo = exact_grid_find(pre, n, blockIdx.x, g);
    const DecResize r = recs[lo];
    const uint32_t rel = (uint32_t)exact_grid_within(pre, lo, g), tiles = (uint32_t)resize_tiles(r.w, r.h); // (planes x tiles < 2^24: the host's rule)
    const uint32_t plane = rel / tiles;
    if (plane >= r.planes) return; // (never, with the host's pre)
    dec_resize_tile<kDtype, kAnyFilter, kAlpha, kResample>(r, plane, rel - plane * tiles, flt);
}

// The exact-grid launchers' instantiations by index: alpha (0 / 1), the launch's kind of filters (resize.h: triangle alone, both
// filters, resample), element (0: bytes, 1 + dtype).  kAnyFilter is the kind >= 1, kResample the kind == 2.
constexpr uint32_t exact_index(uint32_t alpha, uint32_t kind, uint32_t elem) { return (alpha * kResizeLaunchKinds + kind) * (kDecFloatTypes + 1) + elem; }
template <uint32_t I> struct ExactAt {
    static constexpr uint32_t kKind = I / (kDecFloatTypes + 1) % kResizeLaunchKinds;
    static constexpr auto value = dec_resize_exact_kernel<(int)(I % (kDecFloatTypes + 1)) - 1, kKind >= 1, I / (kDecFloatTypes + 1) / kResizeLaunchKinds != 0, kKind == 2>;
};

} // namespace

bool launch_dec_resize_exact(hipStream_t s, const DecResize *recs, const uint64_t *pre, const uint64_t *h_pre, uint32_t n, uint32_t lds_bytes, const DecFloat *flt, uint32_t filters,
                             bool any_alpha)
{
    static constexpr auto kernels = exact_grid_table<ExactAt, exact_index(1, kResizeLaunchKinds - 1, kDecFloatTypes) + 1>();
    if (lds_bytes > 65536u || filters >= kResizeLaunchKinds) return false;
    return exact_grid_walk(h_pre, n, kResizeBlock, [&](uint32_t r0, uint32_t r1, uint32_t groups) {
        hipLaunchKernelGGL(kernels[exact_index(any_alpha, filters, flt ? flt->dtype + 1 : 0)], dim3(groups), dim3(kResizeBlock), lds_bytes, s, recs + r0, pre + r0, r1 - r0, flt ? *flt : DecFloat{});
    });
}

bool launch_dec_resize(hipStream_t s, const DecResize *recs, uint32_t n, uint32_t max_tiles, uint32_t lds_bytes, const DecFloat *flt, bool any_filter)
{
    using Kernel = void (*)(const DecResize *, DecFloat);
    static const Kernel kernels[2][kDecFloatTypes + 1] = {{dec_resize_kernel<-1, false>, dec_resize_kernel<0, false>, dec_resize_kernel<1, false>, dec_resize_kernel<2, false>},
                                                          {dec_resize_kernel<-1, true>, dec_resize_kernel<0, true>, dec_resize_kernel<1, true>, dec_resize_kernel<2, true>}};
    // (a launch holds fewer than 2^32 threads, its z dimension at most 65535 workgroups)
    const uint64_t per_file = (uint64_t)max_tiles * 4 * kResizeBlock;
    if (!max_tiles || per_file >= (1ull << 32) || lds_bytes > 65536u) return false;
    const uint32_t step = (uint32_t)std::min<uint64_t>(32768u, ((1ull << 32) - 1) / per_file);
    for (uint32_t j0 = 0; j0 < n; j0 += step)
        hipLaunchKernelGGL(kernels[any_filter][flt ? flt->dtype + 1 : 0], dim3(max_tiles, 4, std::min(step, n - j0)), dim3(kResizeBlock), lds_bytes, s, recs + j0, flt ? *flt : DecFloat{});
    return true;
}

// ---- the channels-last destinations of fpng_amd_decode_batch(_device)_hwc_views (resize_hwc.h) ----
namespace {

// One workgroup per (record, tile of kResizeTileW x kResizeTileH samples of the window), ALL planes: the exact grid of
// dec_resize_exact_kernel with pre counting tiles.
//   1. the tile's weights, first taps and tap counts as in dec_resize_tile -- once, not once per plane;
//   2. per plane the two passes of dec_resize_tile (the same integer sums, resize_clip8 after each, the same guards) through the
//      same T bytes, a thread's result BYTES of its four rows kept in four registers, a byte per plane; behind the last plane they
//      go to LDS as O[row][column * planes + plane], in the place of the weights and T, which are done with -- so a tile needs no
//      more LDS than the planar kernel's, and as many workgroups fit a compute unit (with 3 or 4 KB on top of the 20 KB of a 10 x
//      reduction one fewer did, and the kernel ran 8 % longer: profiles/views_hwc_timing.txt);
//   3. a wave per row of the tile walks the row's run of the destination in memory order: element e is position e % pixel_elems of
//      pixel e / pixel_elems (positions >= planes belong to the caller: skipped), neighbouring lanes write neighbouring elements.
//      The mirror is an index into O -- the tile's columns ox0 .. ox0 + nw - 1 of the window are pixels w - ox0 - nw .. w - ox0 - 1
//      of the destination, back to front -- the reversed order an index into the pixel; the fmaf and the conversion are
//      dec_resize_tile's.  Where every element of the run is written (pixel_elems == planes) and the elements are narrower than a
//      dword, the run goes out as single elements up to the first 4-byte boundary, dwords, and single elements behind the last one.
// kAlpha (view_alpha.h): the load of step 2 makes P' as dec_resize_tile's does; a PREMULTIPLIED view runs the passes for all FOUR planes,
// whatever the destination's count -- R'_3 is then byte 3 of the same register -- and divides the three colour bytes by it before
// they go to O.
// kResample: as dec_resize_tile's
template <int kDtype, bool kAnyFilter, bool kAlpha = false, bool kResample = false>
__global__ __launch_bounds__(kResizeBlock) void dec_resize_hwc_kernel(const DecResizeHwc *recs, const uint64_t *pre, uint32_t n, DecFloat flt)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t resize_lds[];
    uint64_t g;
    const uint32_t lo = exact_grid_find(pre, n, blockIdx.x, g);
    const DecResize r = recs[lo].r;
    const uint32_t P = recs[lo].pixel_elems, reversed = recs[lo].hwc_flags & kHwcReversed, C = r.planes;
    const uint32_t tile = (uint32_t)exact_grid_within(pre, lo, g);
    if ((uint64_t)tile >= resize_tiles(r.w, r.h)) return; // (never, with the host's pre)
    uint32_t ox0, oq0, nw, nq;
    resize_tile_at(tile, r.w, r.h, ox0, oq0, nw, nq);
    FPNG_RESIZE_TILE_LDS(resize_lds, r.taps_x, r.taps_y);
    uint8_t *const O = resize_lds; // (once the passes are done, in the place of everything else)
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
    const uint32_t o_stride = kResizeTileW * C; // bytes of a row of O
    constexpr uint32_t kWaves = kResizeBlock / kResizeTileW, kRowsPerWave = kResizeTileH / kWaves;
    uint32_t res[kRowsPerWave] = {};
    [[maybe_unused]] const uint32_t a_op = kAlpha ? resize_alpha_op(r.flags) : 0u;
    const uint32_t n_planes = kAlpha && a_op == kAlphaPremultiplied ? 4u : C;
    for (uint32_t plane = 0; plane < n_planes; plane++) {
        if (plane) __syncthreads(); // (the plane before has been read out of T)
        const uint8_t *const S = r.src + (uint64_t)plane * r.src_plane_pitch;
        {
            const uint32_t first = fx[o], count = cx[o];
            for (uint32_t j = wave; j < nrows; j += kResizeBlock / kResizeTileW) {
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
        if (a_op == kAlphaPremultiplied) { // (step 3 of the rule; a destination of three planes drops R_3 behind it)
#pragma unroll
            for (uint32_t k = 0; k < kRowsPerWave; k++) {
                const uint32_t a = res[k] >> 24;
                res[k] = alpha_unmul(res[k] & 255u, a) | alpha_unmul(res[k] >> 8 & 255u, a) << 8 | alpha_unmul(res[k] >> 16 & 255u, a) << 16 | (C == 4 ? a << 24 : 0u);
            }
        }
    __syncthreads(); // (weights, taps and T have been read for the last time: O takes their place)
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
    // ---- 3. the store: a wave per row, the row's run in memory order ----
    constexpr uint32_t kElem = kDtype < 0 ? 1u : dec_float_bytes((uint32_t)kDtype);
    const bool mirror = r.flags & kResizeMirror;
    const uint32_t d0 = mirror ? r.w - ox0 - nw : ox0; // the run's first pixel of the destination's row
    const uint32_t n_el = (nw - 1) * P + C;            // the run's elements, up to the last one that is written
    for (uint32_t q = wave; q < nq; q += kResizeBlock / kResizeTileW) {
        const uint8_t *const Oq = O + q * o_stride;
        uint8_t *const D = r.dst + (int64_t)(oq0 + q) * r.pitch + (int64_t)((uint64_t)d0 * P * kElem);
        // element e of the run as the bits of its kElem bytes (e's position within its pixel is below C)
        auto bits = [&](uint32_t e) -> uint32_t {
            const uint32_t i = P == 4 ? e >> 2 : e / 3u, k = e - i * P; // (P is 3 or 4)
            const uint32_t c = reversed ? C - 1 - k : k;              // the FILE's channel
            float sc, bi;
            float_scale_bias(flt, c, sc, bi);
            return byte_elem_bits<kDtype>(Oq[(mirror ? nw - 1 - i : i) * C + c], sc, bi);
        };
        auto store1 = [&](uint32_t e) { elem_store<kDtype>(D + (size_t)e * kElem, bits(e)); };
        if (kElem == 4 || P != C) {
            for (uint32_t e = o; e < n_el; e += kResizeTileW)
                if (P == C || (e & 3u) < C) store1(e); // (P == 4: position e % 4; 3 is the caller's)
        } else {
            constexpr uint32_t kPer = 4u / kElem; // elements per dword
            const uint32_t head = std::min(n_el, (uint32_t)((0u - (uint32_t)(uintptr_t)D) & 3u) / kElem); // (D is a multiple of kElem)
            const uint32_t nd = (n_el - head) / kPer, tail0 = head + nd * kPer;
            if (o < head) store1(o);
            for (uint32_t d = o; d < nd; d += kResizeTileW) {
                const uint32_t e = head + d * kPer;
                uint32_t word;
                if constexpr (kPer == 4) word = bits(e) | bits(e + 1) << 8 | bits(e + 2) << 16 | bits(e + 3) << 24;
                else word = bits(e) | bits(e + 1) << 16;
                *(uint32_t *)(D + (size_t)e * kElem) = word;
            }
            if (tail0 + o < n_el) store1(tail0 + o);
        }
    }
}

template <uint32_t I> struct HwcAt { // (exact_index)
    static constexpr uint32_t kKind = I / (kDecFloatTypes + 1) % kResizeLaunchKinds;
    static constexpr auto value = dec_resize_hwc_kernel<(int)(I % (kDecFloatTypes + 1)) - 1, kKind >= 1, I / (kDecFloatTypes + 1) / kResizeLaunchKinds != 0, kKind == 2>;
};

} // namespace

bool launch_dec_resize_hwc(hipStream_t s, const DecResizeHwc *recs, const uint64_t *pre, const uint64_t *h_pre, uint32_t n, uint32_t lds_bytes, const DecFloat *flt, uint32_t filters,
                           bool any_alpha)
{
    static constexpr auto kernels = exact_grid_table<HwcAt, exact_index(1, kResizeLaunchKinds - 1, kDecFloatTypes) + 1>();
    if (lds_bytes > 65536u || filters >= kResizeLaunchKinds) return false;
    return exact_grid_walk(h_pre, n, kResizeBlock, [&](uint32_t r0, uint32_t r1, uint32_t groups) {
        hipLaunchKernelGGL(kernels[exact_index(any_alpha, filters, flt ? flt->dtype + 1 : 0)], dim3(groups), dim3(kResizeBlock), lds_bytes, s, recs + r0, pre + r0, r1 - r0, flt ? *flt : DecFloat{});
    });
}

} // namespace fpng_amd
