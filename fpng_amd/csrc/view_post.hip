// view_post.hip -- the third stage of fpng_amd_decode_batch(_device)_planar_views_post and _hwc_views_post: a view's blur, solarize
// and posterize (view_post.h: the rule, and the text the host's fpng_amd_view_post_apply runs) on the un-mirrored uint8 window that
// dec_resize_color_kernel<-1, *, false> has written into the decode scratch, and the store into the caller's destination.  One
// workgroup per (record, tile of kResizeTileW x kResizeTileH samples of the window), ALL planes, the exact grid with pre counting
// tiles, as dec_resize_color_kernel runs.  Per colour plane, with R the view's radius:
//   1. the tile and a halo of R samples on every side into LDS, the window's border reflected (post_refl): (16 + 2R) rows of
//      (64 + 2R) bytes -- at R = 16 48 x 96;
//   2. the horizontal pass out of those into LDS bytes, the tile's rows and the halo above and below (the horizontal pass of a
//      reflected row IS that row of H);
//   3. the vertical pass out of those, then solarize and posterize: a thread's bytes of its four rows go into four registers, a
//      byte per plane, as in dec_resize_color_kernel.
// R = 0 (point operations only) reads the scratch straight into the registers: no LDS, no barrier.  A fourth plane (alpha, or the
// 255 of a 3-channel file) is copied.
// A view with a WARP (the _views_warp calls; view_warp.h: the rule) reads W in the place of B: sample (q, i) of W is gathered from the
// window -- one byte, or four and a blend in doubles -- wherever the text above loads B[q][i], the halo's reflected samples
// included, and the mirror moves from the store into the gather's read index.  The kWarp instantiations run those calls: a
// sample's position is found once (warp_locate) and serves its planes, so stage 1 fills the halos of all three colour planes in one
// sweep (S holds three); the fourth plane is gathered too.  Whether a record has a warp is uniform across its workgroup.  The
// window is at most a few hundred KB and has just been written: the gather reads it out of L2.
// A view with a TONE op (the _views_tone calls; view_tone.h: the rule) reads W' = lut[W]: the kMode == 2 instantiations run those
// calls.  They copy the view's three 256-byte tables, which dec_view_tone_lut_kernel has written into the scratch, into LDS (the
// identity for a view of the call without an op) and look every sample up where the text above loads B or gathers W -- the halo
// fill, the warp's halo fill and both R = 0 paths.  The fourth plane is not looked up.
// A view with an ENHANCE op (the _views_enhance calls; view_enhance.h: the rule) reads E = blend(D, W'): the kMode == 3
// instantiations run those calls, and do everything the kMode == 2 ones do.  BRIGHTNESS (D = 0) is composed into the tables as they
// are copied into LDS.  COLOR (D = the sample's luma) needs the three planes of a sample together: stage 1 fills all three planes of
// S in one sweep without a warp too, and both R = 0 paths are one that fetches a sample's three bytes.  SHARPNESS (D = SMOOTH, a
// 3 x 3 filter) loads the tile with a halo of R + 1 -- S has rows of 98 bytes, 50 of them, here -- and one more pass per plane writes
// E for the tile and a halo of R into a one-plane buffer behind the tables, rows of 96 bytes, out of which the horizontal pass
// reads; with R = 0 E goes straight into the registers.  A sample of the halo is a frame sample by its reflected, TRUE coordinate.
// With R = min(w, h) - 1 the outermost ring reflects to one past the window: its index is held inside (enhance_refl), for those
// samples are neighbours of frame samples only, whose D does not read them.
//   4. the store: a thread has all channels of its pixels; every element is stored on its own -- planar destinations as
//      dec_resize_color_kernel's, lanes along a row of a plane; channels-last ones by element, position c or planes - 1 - c of the
//      pixel, positions >= planes never written.
// LDS reads of the passes are bytes at consecutive addresses along a wave's lanes: four lanes a bank, one address each -- no conflict.
// The kernel is symmetric, so taps -d and d share one product: sum = 2^21 + s[0] k[0] + sum_d (s[-d] + s[d]) k[d] -- the same integer.
#include "decode.h"
#include "exact_grid.h"
#include "float_store.h"
#include "resize.h"
#include "resize_hwc.h"
#include "resize_tile.h"
#include "view_post.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace fpng_amd {

namespace {

constexpr uint32_t kPostHaloW = kResizeTileW + 2 * kPostMaxRadius, kPostHaloH = kResizeTileH + 2 * kPostMaxRadius; // 96 x 48

// kMode: 0 the post calls', 1 the warp calls' (gathers), 2 the tone calls' (gathers and applies a table), 3 the enhance calls' (gathers,
// applies a table and blends against a degenerate image)
template <int kDtype, bool kHwc, int kMode> __global__ __launch_bounds__(kResizeBlock) void dec_view_post_kernel(const DecViewPost *recs, const uint64_t *pre, uint32_t n, DecFloat flt)
{
    constexpr bool kWarp = kMode >= 1, kTone = kMode >= 2, kEnh = kMode == 3;
    constexpr uint32_t kSW = kPostHaloW + (kEnh ? 2 : 0), kSH = kPostHaloH + (kEnh ? 2 : 0); // (kEnh: sharpness reads one sample further)
    constexpr uint32_t kHalo = kSH * kSW, kEHalo = kPostHaloH * kPostHaloW;
    // the tile and its halo, rows of kSW bytes (kWarp: per colour plane); kTone: behind them the view's tables, lut[c][v]; kEnh: behind
    // those E of one plane, the tile and the blur's halo, rows of kPostHaloW bytes
    __shared__ __attribute__((aligned(16))) uint8_t S[(kWarp ? 3 : 1) * kHalo + (kTone ? kToneLutBytes : 0) + (kEnh ? kEHalo : 0)];
    __shared__ __attribute__((aligned(16))) uint8_t Hb[kPostHaloH * kResizeTileW]; // the horizontal pass: rows of kResizeTileW bytes
    __shared__ int32_t K[kPostMaxRadius + 1];                                   // k[d]: taps -d and d share it
    uint64_t g;
    const uint32_t lo = exact_grid_find(pre, n, blockIdx.x, g);
    const DecViewPost &r = recs[lo];
    const uint32_t w = r.w, h = r.h, C = r.planes, flags = r.flags;
    const uint32_t tile = (uint32_t)exact_grid_within(pre, lo, g);
    if ((uint64_t)tile >= resize_tiles(w, h)) return; // (never, with the host's pre)
    uint32_t ox0, oq0, nw, nq;
    resize_tile_at(tile, w, h, ox0, oq0, nw, nq);
    // (the host's records: 1 .. 16 with blur, and below w and h -- the bounds of S and of one reflection, held here too)
    const uint32_t R = (flags & kPostBlur) ? std::min(std::min(r.radius, kPostMaxRadius), std::min(w, h) - 1u) : 0u;
    const uint32_t tid = threadIdx.x, o = tid % kResizeTileW, wave = tid / kResizeTileW;
    constexpr uint32_t kWaves = kResizeBlock / kResizeTileW, kRowsPerWave = kResizeTileH / kWaves;
    const uint64_t plane_bytes = (uint64_t)w * h;
    const uint32_t threshold = r.threshold, bits = r.bits;
    const uint32_t wflags = kWarp ? r.warp.flags : 0u, mirror = r.mirror;
    uint32_t res[kRowsPerWave] = {};
    uint8_t *const T = S + (kTone ? 3 * kHalo : 0u); // (kTone only)
    if constexpr (kTone) {
        const uint8_t *const lut = r.tone_op ? (const uint8_t *)(r.tone + kToneHistWords) : nullptr;
        if constexpr (kEnh) { // (BRIGHTNESS: a point operation behind the table's)
            const bool bright = r.enhance_op == kEnhanceBrightness;
            const float f = r.enhance_factor;
            for (uint32_t k = tid; k < kToneLutBytes; k += kResizeBlock) {
                const uint32_t t = lut ? lut[k] : k & 255u;
                T[k] = (uint8_t)(bright ? enhance_blend(0u, t, f) : t);
            }
        } else
            for (uint32_t k = tid; k < kToneLutBytes; k += kResizeBlock) T[k] = lut ? lut[k] : (uint8_t)k;
        __syncthreads();
    }
    // (the byte of W' for the byte b of plane p of W)
    const auto tone = [&](uint32_t p, uint32_t b) -> uint32_t {
        if constexpr (kTone) return T[p * 256 + b];
        else return b;
    };
    if constexpr (kEnh) {
        const uint32_t eop = r.enhance_op, np = std::min(C, 3u);
        const float ef = r.enhance_factor;
        const uint32_t X = eop == kEnhanceSharpness && enhance_sharpens(w, h) ? 1u : 0u, Rh = R + X; // (the halo that stage 1 loads)
        uint8_t *const Eb = T + kToneLutBytes;
        // the bytes of E -- but for SHARPNESS: of W' -- of the sample (x, y) of the window, true coordinates, in planes 0 .. np - 1
        const auto sample3 = [&](uint32_t x, uint32_t y, uint32_t v[3]) {
            if (wflags) {
                const WarpAt at = warp_locate(r.warp, x, y, w, h, mirror);
#pragma unroll
                for (uint32_t p = 0; p < 3; p++) v[p] = p < np ? T[p * 256 + warp_sample(at, wflags, r.src + p * plane_bytes, w, r.warp.fill[p])] : 0u;
            } else {
#pragma unroll
                for (uint32_t p = 0; p < 3; p++) v[p] = p < np ? T[p * 256 + r.src[p * plane_bytes + (uint64_t)y * w + x]] : 0u;
            }
            if (eop == kEnhanceColor && np == 3) {
                const uint32_t luma = tone_luma(v[0], v[1], v[2]);
#pragma unroll
                for (uint32_t p = 0; p < 3; p++) v[p] = enhance_blend(luma, v[p], ef);
            }
        };
        // E of the sample at c of a plane of S whose true coordinates are (tx, ty) (X only)
        const auto sharp = [&](const uint8_t *c, uint32_t tx, uint32_t ty) -> uint32_t { return enhance_on_frame(tx, ty, w, h) ? c[0] : enhance_sharp_at(c, (int32_t)kSW, ef); };
        if (Rh) {
            if (R && tid <= R) K[tid] = r.k[tid];
            const uint32_t sw = nw + 2 * Rh, sh = nq + 2 * Rh; // (<= kSW, kSH)
            // ---- 1. the tile and its halo, all colour planes of a sample at once ----
            for (uint32_t j = wave; j < sh; j += kWaves) {
                const uint32_t y = enhance_refl((int32_t)(oq0 + j) - (int32_t)Rh, h);
                for (uint32_t i = o; i < sw; i += kResizeTileW) {
                    uint32_t v[3];
                    sample3(enhance_refl((int32_t)(ox0 + i) - (int32_t)Rh, w), y, v);
#pragma unroll
                    for (uint32_t p = 0; p < 3; p++)
                        if (p < np) S[p * kHalo + j * kSW + i] = (uint8_t)v[p];
                }
            }
            __syncthreads();
            for (uint32_t plane = 0; plane < np; plane++) {
                const uint8_t *const Sp = S + plane * kHalo;
                const uint8_t *from = Sp; // (what the horizontal pass reads: rows of `stride` bytes, the tile and a halo of R)
                uint32_t stride = kSW;
                if (X && !R) { // ---- 1b. E into the registers, the point operations ----
                    if (o < nw) {
#pragma unroll
                        for (uint32_t k = 0; k < kRowsPerWave; k++) {
                            const uint32_t q = wave + k * kWaves;
                            if (q >= nq) break;
                            res[k] |= post_point(sharp(Sp + (q + 1) * kSW + o + 1, ox0 + o, oq0 + q), flags, threshold, bits) << (8 * plane);
                        }
                    }
                    continue;
                }
                if (X) { // ---- 1b. E of the tile and a halo of R (the plane before has been read out of Eb: a barrier since) ----
                    for (uint32_t j = wave; j < nq + 2 * R; j += kWaves) {
                        const uint32_t ty = post_refl((int32_t)(oq0 + j) - (int32_t)R, h);
                        for (uint32_t i = o; i < nw + 2 * R; i += kResizeTileW)
                            Eb[j * kPostHaloW + i] = (uint8_t)sharp(Sp + (j + 1) * kSW + i + 1, post_refl((int32_t)(ox0 + i) - (int32_t)R, w), ty);
                    }
                    from = Eb, stride = kPostHaloW;
                    __syncthreads(); // (and the plane before has been read out of Hb)
                } else if (plane)
                    __syncthreads(); // (the plane before has been read out of Hb)
                // ---- 2. the horizontal pass ----
                if (o < nw)
                    for (uint32_t j = wave; j < nq + 2 * R; j += kWaves) {
                        const uint8_t *const s = from + j * stride + o + R;
                        int32_t sum = (1 << (kResizeBits - 1)) + (int32_t)s[0] * K[0];
#pragma unroll 4
                        for (uint32_t d = 1; d <= R; d++) sum += ((int32_t)s[-(int32_t)d] + (int32_t)s[d]) * K[d];
                        Hb[j * kResizeTileW + o] = (uint8_t)resize_clip8(sum);
                    }
                __syncthreads();
                // ---- 3. the vertical pass, the point operations ----
                if (o < nw) {
#pragma unroll
                    for (uint32_t k = 0; k < kRowsPerWave; k++) {
                        const uint32_t q = wave + k * kWaves;
                        if (q >= nq) break;
                        const uint8_t *const s = Hb + (q + R) * kResizeTileW + o;
                        int32_t sum = (1 << (kResizeBits - 1)) + (int32_t)s[0] * K[0];
#pragma unroll 4
                        for (uint32_t d = 1; d <= R; d++) sum += ((int32_t)s[-(int32_t)(d * kResizeTileW)] + (int32_t)s[d * kResizeTileW]) * K[d];
                        res[k] |= post_point(resize_clip8(sum), flags, threshold, bits) << (8 * plane);
                    }
                }
            }
        } else if (o < nw) {
#pragma unroll
            for (uint32_t k = 0; k < kRowsPerWave; k++) {
                const uint32_t q = wave + k * kWaves;
                if (q >= nq) break;
                uint32_t v[3];
                sample3(ox0 + o, oq0 + q, v);
#pragma unroll
                for (uint32_t p = 0; p < 3; p++)
                    if (p < np) res[k] |= post_point(v[p], flags, threshold, bits) << (8 * p);
            }
        }
    } else if (R) {
        if (tid <= R) K[tid] = r.k[tid];
        const uint32_t sw = nw + 2 * R, sh = nq + 2 * R; // (<= kPostHaloW, kPostHaloH)
        for (uint32_t plane = 0; plane < C && plane < 3; plane++) {
            const uint8_t *const src = r.src + plane * plane_bytes;
            uint8_t *const Sp = S + (kWarp ? plane * kHalo : 0u);
            if (plane) __syncthreads(); // (the plane before has been read out of S and Hb)
            // ---- 1. the tile and its halo ----
            if (kWarp && wflags) {
                if (!plane) { // (all colour planes of a sample from one position)
                    const uint32_t np = std::min(C, 3u);
                    for (uint32_t j = wave; j < sh; j += kWaves) {
                        const uint32_t y = post_refl((int32_t)(oq0 + j) - (int32_t)R, h);
                        for (uint32_t i = o; i < sw; i += kResizeTileW) {
                            const WarpAt at = warp_locate(r.warp, post_refl((int32_t)(ox0 + i) - (int32_t)R, w), y, w, h, mirror);
                            for (uint32_t p = 0; p < np; p++) S[p * kHalo + j * kPostHaloW + i] = (uint8_t)tone(p, warp_sample(at, wflags, r.src + p * plane_bytes, w, r.warp.fill[p]));
                        }
                    }
                }
            } else
                for (uint32_t j = wave; j < sh; j += kWaves) {
                    const uint8_t *const row = src + (uint64_t)post_refl((int32_t)(oq0 + j) - (int32_t)R, h) * w;
                    for (uint32_t i = o; i < sw; i += kResizeTileW) Sp[j * kPostHaloW + i] = (uint8_t)tone(plane, row[post_refl((int32_t)(ox0 + i) - (int32_t)R, w)]);
                }
            __syncthreads();
            // ---- 2. the horizontal pass ----
            if (o < nw)
                for (uint32_t j = wave; j < sh; j += kWaves) {
                    const uint8_t *const s = Sp + j * kPostHaloW + o + R; // (the sample itself; taps -d and d: one product)
                    int32_t sum = (1 << (kResizeBits - 1)) + (int32_t)s[0] * K[0];
#pragma unroll 4
                    for (uint32_t d = 1; d <= R; d++) sum += ((int32_t)s[-(int32_t)d] + (int32_t)s[d]) * K[d];
                    Hb[j * kResizeTileW + o] = (uint8_t)resize_clip8(sum);
                }
            __syncthreads();
            // ---- 3. the vertical pass, the point operations ----
            if (o < nw) {
#pragma unroll
                for (uint32_t k = 0; k < kRowsPerWave; k++) {
                    const uint32_t q = wave + k * kWaves;
                    if (q >= nq) break;
                    const uint8_t *const s = Hb + (q + R) * kResizeTileW + o;
                    int32_t sum = (1 << (kResizeBits - 1)) + (int32_t)s[0] * K[0];
#pragma unroll 4
                    for (uint32_t d = 1; d <= R; d++) sum += ((int32_t)s[-(int32_t)(d * kResizeTileW)] + (int32_t)s[d * kResizeTileW]) * K[d];
                    res[k] |= post_point(resize_clip8(sum), flags, threshold, bits) << (8 * plane);
                }
            }
        }
    } else if (o < nw && kWarp && wflags) {
#pragma unroll
        for (uint32_t k = 0; k < kRowsPerWave; k++) {
            const uint32_t q = wave + k * kWaves;
            if (q >= nq) break;
            const WarpAt at = warp_locate(r.warp, ox0 + o, oq0 + q, w, h, mirror);
            for (uint32_t plane = 0; plane < C && plane < 3; plane++)
                res[k] |= post_point(tone(plane, warp_sample(at, wflags, r.src + plane * plane_bytes, w, r.warp.fill[plane])), flags, threshold, bits) << (8 * plane);
            if (C == 4) res[k] |= warp_sample(at, wflags, r.src + 3 * plane_bytes, w, r.warp.fill[3]) << 24;
        }
    } else if (o < nw) {
        for (uint32_t plane = 0; plane < C && plane < 3; plane++) {
#pragma unroll
            for (uint32_t k = 0; k < kRowsPerWave; k++) {
                const uint32_t q = wave + k * kWaves;
                if (q >= nq) break;
                res[k] |= post_point(tone(plane, r.src[plane * plane_bytes + (uint64_t)(oq0 + q) * w + ox0 + o]), flags, threshold, bits) << (8 * plane);
            }
        }
    }
    if (o >= nw) return; // (no barrier behind this line)
    if (C == 4 && kWarp && wflags) {
        if (R || kEnh) { // (without blur: gathered above -- but for the enhance calls')
#pragma unroll
            for (uint32_t k = 0; k < kRowsPerWave; k++) {
                const uint32_t q = wave + k * kWaves;
                if (q >= nq) break;
                res[k] |= warp_sample(warp_locate(r.warp, ox0 + o, oq0 + q, w, h, mirror), wflags, r.src + 3 * plane_bytes, w, r.warp.fill[3]) << 24;
            }
        }
    } else if (C == 4) {
#pragma unroll
        for (uint32_t k = 0; k < kRowsPerWave; k++) {
            const uint32_t q = wave + k * kWaves;
            if (q >= nq) break;
            res[k] |= (uint32_t)r.src[3 * plane_bytes + (uint64_t)(oq0 + q) * w + ox0 + o] << 24;
        }
    }
    // ---- 4. the store ----
    constexpr uint32_t kElem = kDtype < 0 ? 1u : dec_float_bytes((uint32_t)kDtype);
    const uint32_t col = mirror && !wflags ? w - 1 - (ox0 + o) : ox0 + o; // (a warp has mirrored its reads)
    // (file channel c: plane c, or element c -- reversed: planes - 1 - c -- of its pixel)
    int64_t at[4], first;
    if constexpr (!kHwc) {
        first = (int64_t)col * kElem;
#pragma unroll
        for (uint32_t c = 0; c < 4; c++) at[c] = (int64_t)c * r.plane_pitch;
    } else {
        const bool reversed = r.hwc_flags & kHwcReversed;
        first = (int64_t)((uint64_t)col * r.pixel_elems * kElem);
#pragma unroll
        for (uint32_t c = 0; c < 4; c++) at[c] = (int64_t)((reversed ? C - 1 - c : c) * kElem);
    }
#pragma unroll
    for (uint32_t k = 0; k < kRowsPerWave; k++) {
        const uint32_t q = wave + k * kWaves;
        if (q >= nq) break;
        uint8_t *const p = r.dst + (int64_t)(oq0 + q) * r.pitch + first;
        elem_store<kDtype>(p + at[0], byte_elem_bits<kDtype>(res[k] & 255u, flt.scale[0], flt.bias[0]));
        elem_store<kDtype>(p + at[1], byte_elem_bits<kDtype>(res[k] >> 8 & 255u, flt.scale[1], flt.bias[1]));
        elem_store<kDtype>(p + at[2], byte_elem_bits<kDtype>(res[k] >> 16 & 255u, flt.scale[2], flt.bias[2]));
        if (C == 4) elem_store<kDtype>(p + at[3], byte_elem_bits<kDtype>(res[k] >> 24, flt.scale[3], flt.bias[3]));
    }
}

// The instantiations by index: kMode (0 .. 3), channels-last (0 / 1), element (0: bytes, 1 + dtype)
constexpr uint32_t post_index(uint32_t mode, uint32_t hwc, uint32_t elem) { return (mode * 2 + hwc) * (kDecFloatTypes + 1) + elem; }
template <uint32_t I> struct PostAt {
    static constexpr auto value = dec_view_post_kernel<(int)(I % (kDecFloatTypes + 1)) - 1, I / (kDecFloatTypes + 1) % 2 != 0, (int)(I / (kDecFloatTypes + 1) / 2)>;
};

} // namespace

bool launch_dec_view_post(hipStream_t s, const DecViewPost *recs, const uint64_t *pre, const uint64_t *h_pre, uint32_t n, const DecFloat *flt, bool hwc, int mode)
{
    static constexpr auto kernels = exact_grid_table<PostAt, post_index(3, 1, kDecFloatTypes) + 1>();
    if (mode < 0 || mode > 3) return false;
    return exact_grid_walk(h_pre, n, kResizeBlock, [&](uint32_t r0, uint32_t r1, uint32_t groups) {
        hipLaunchKernelGGL(kernels[post_index(mode, hwc, flt ? flt->dtype + 1 : 0)], dim3(groups), dim3(kResizeBlock), 0, s, recs + r0, pre + r0, r1 - r0, flt ? *flt : DecFloat{});
    });
}

} // namespace fpng_amd
