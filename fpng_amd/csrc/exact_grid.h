// exact_grid.h -- the exact one-dimensional grid of the view-stage kernels (resize.hip, resize_color.hip, view_post.hip,
// view_tone.hip, yuv_store.hip, encode_resize.hip): a workgroup per unit of work of every record and none in surplus.
// pre[k] (k = 0 .. n): the workgroups of the batch's records in front of record k (never 0 per record), so workgroup b of a launch
// over records r0 .. r1 - 1 is number pre[r0] + b of the batch and belongs to the last record whose pre is not above that.
// exact_grid_find / exact_grid_within: what the kernels run, host and device; exact_grid_walk: the host's cut of pre[] into launches;
// exact_grid_table: a launcher's instantiations by index.  An element of pre[] is a uint64_t, or a record that carries one
// (exact_grid_pre: view_post.h's DecToneRef).  The host part compiles with any C++17 compiler.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FPNG_GRID_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define FPNG_GRID_FN inline
#endif

namespace fpng_amd {

FPNG_GRID_FN uint64_t exact_grid_pre(const uint64_t &e) { return e; }

// Workgroup b of the launch whose records' prefixes are pre[0 .. n] (n >= 1, b < pre[n] - pre[0]) is number g = pre[0] + b of the
// batch: its record lo, pre[lo] <= g < pre[lo + 1], is returned, and exact_grid_within(pre, lo, g) = g - pre[lo] is the workgroup's
// number within that record (a function of its own, so that a kernel subtracts where it needs the number: behind the record's
// load).  The same for all of a workgroup's threads.
template <class E> FPNG_GRID_FN uint32_t exact_grid_find(const E *pre, uint32_t n, uint32_t b, uint64_t &g)
{
    g = exact_grid_pre(pre[0]) + b;
    uint32_t lo = 0, hi = n; // pre[lo] <= g < pre[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (exact_grid_pre(pre[mid]) <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}
template <class E> FPNG_GRID_FN uint64_t exact_grid_within(const E *pre, uint32_t lo, uint64_t g) { return g - exact_grid_pre(pre[lo]); }

// (a launch holds fewer than 2^32 threads: at 256 a workgroup fewer than 2^24 workgroups, far below the 2^31 of a grid's dimension)
constexpr uint64_t exact_grid_limit(uint32_t block) { return (1ull << 32) / block - 1; }

// The launches of records 0 .. n - 1: launch(r0, r1, workgroups) for consecutive pieces [r0, r1) that cover [0, n) in order, each of
// at most `limit` workgroups (0: exact_grid_limit(block)) and greedy -- one more record would exceed the limit.  false, and NOTHING
// launched, where a record has no workgroups (pre does not increase) or more than the limit; n = 0: true and no launch.
template <class E, class Launch> bool exact_grid_walk(const E *h_pre, uint32_t n, uint32_t block, Launch &&launch, uint64_t limit = 0)
{
    if (!limit) limit = exact_grid_limit(block);
    const auto at = [&](uint32_t k) { return exact_grid_pre(h_pre[k]); };
    for (uint32_t k = 0; k < n; k++)
        if (at(k + 1) <= at(k) || at(k + 1) - at(k) > limit) return false;
    for (uint32_t r0 = 0, r1; r0 < n; r0 = r1) {
        for (r1 = r0 + 1; r1 < n && at(r1 + 1) - at(r0) <= limit;) r1++;
        launch(r0, r1, (uint32_t)(at(r1) - at(r0)));
    }
    return true;
}

// table[i] = At<i>::value for i < kCount: At decodes the index into the template arguments, next to the function that encodes it
template <template <uint32_t> class At, size_t... I> constexpr auto exact_grid_table(std::index_sequence<I...>)
{
    return std::array<std::decay_t<decltype(At<0>::value)>, sizeof...(I)>{At<(uint32_t)I>::value...};
}
template <template <uint32_t> class At, uint32_t kCount> constexpr auto exact_grid_table() { return exact_grid_table<At>(std::make_index_sequence<kCount>{}); }

} // namespace fpng_amd
