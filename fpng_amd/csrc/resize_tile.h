// resize_tile.h -- what the tile kernels of the resize share in front of and behind their passes (resize.hip: dec_resize_tile,
// dec_resize_hwc_kernel; resize_color.hip: dec_resize_color_kernel; encode_resize.hip: enc_resize_kernel; view_post.hip's kernel takes
// the geometry): a workgroup of kResizeBlock threads and a tile of kResizeTileW x kResizeTileH samples of a w x h window.  Device
// code only.
// resize_tile_at: where the tile lies in the window; FPNG_RESIZE_TILE_LDS: its arrays in LDS; resize_tile_run: a row's run to memory.
// Step 1 (the weights) and the two passes stay written out in each kernel: moved into functions of this header they compile to
// other instructions in every kernel (profiles/view_kernels_isa_diff.txt has what was tried).
#pragma once
#include "resize.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace fpng_amd {

// Tile number `tile` (below resize_tiles(w, h)) of a w x h window
__device__ __forceinline__ void resize_tile_at(uint32_t tile, uint32_t w, uint32_t h, uint32_t &ox0, uint32_t &oq0, uint32_t &nw, uint32_t &nq)
{
    const uint32_t tiles_x = (w + kResizeTileW - 1) / kResizeTileW;
    ox0 = tile % tiles_x * kResizeTileW, oq0 = tile / tiles_x * kResizeTileH;
    nq = std::min(kResizeTileH, h - oq0), nw = std::min(kResizeTileW, w - ox0);
}

// The carve of the launch's dynamic LDS `lds`: declares Kx[t][column] and Ky[t][row], the weights; fx, cx, fy and cy, first tap and
// tap count per column and per row; T[source row][column], the horizontal pass's bytes.  (A macro, so that the pointers are the
// kernel's own locals: a function that computes them changes the kernels' instructions.)  This is the layout that resize.h's
// resize_tile_lds() sizes, in its order -- (taps_x * kResizeTileW + taps_y * kResizeTileH) weights and 2 * (kResizeTileW +
// kResizeTileH) firsts and counts of four bytes each, then rows * kResizeTileW bytes of T.  A change to one is a change to the other.
#define FPNG_RESIZE_TILE_LDS(lds, taps_x, taps_y)                                                                                                            \
    int32_t *const Kx = (int32_t *)(lds), *const Ky = Kx + (taps_x) * kResizeTileW;                                                                          \
    uint32_t *const fx = (uint32_t *)(Ky + (taps_y) * kResizeTileH), *const cx = fx + kResizeTileW, *const fy = cx + kResizeTileW, *const cy = fy + kResizeTileH; \
    uint8_t *const T = (uint8_t *)(cy + kResizeTileH)

// A row's run of n_el elements of kElem bytes (1 or 2) at D, a multiple of kElem, in memory order: lane o of the row's wave stores
// single elements up to the first 4-byte boundary -- one(e) -- the dwords -- word(e), e the dword's first element -- and single
// elements behind the last dword.  How element e is made is the caller's: computed bits, a copy out of LDS.
template <uint32_t kElem, class One, class Word> __device__ __forceinline__ void resize_tile_run(const uint8_t *D, uint32_t n_el, uint32_t o, const One &one, const Word &word)
{
    constexpr uint32_t kPer = 4u / kElem; // elements per dword
    const uint32_t head = std::min(n_el, (uint32_t)((0u - (uint32_t)(uintptr_t)D) & 3u) / kElem);
    const uint32_t nd = (n_el - head) / kPer, tail0 = head + nd * kPer;
    if (o < head) one(o);
    for (uint32_t d = o; d < nd; d += kResizeTileW) word(head + d * kPer);
    if (tail0 + o < n_el) one(tail0 + o);
}

} // namespace fpng_amd
