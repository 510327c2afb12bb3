// png_views_gather.h -- the request of some files of an fpng_amd_png_views request: the per-file ranges of every array that is given,
// compacted (png_views_api.cpp sends the fpng-written files of a batch through the existing views path with it).  Host-only and
// free of HIP: tests/cpp/png_views_gather_host.cpp builds it alone.
#pragma once
#include "fpng_amd.h"

#include <cstdint>
#include <vector>

namespace fpng_amd {

// the records of `all` (NULL: not given) of the files picked[0 .. n_picked): file f's are all[first[f]] .. all[first[f] + count[f] - 1].
// -> out.data(), or NULL where all is
template <class T> const T *gather_views(const T *all, const uint32_t *picked, uint32_t n_picked, const uint32_t *first, const uint32_t *count, std::vector<T> &out)
{
    if (!all) return nullptr;
    out.clear();
    for (uint32_t k = 0; k < n_picked; k++) out.insert(out.end(), all + first[picked[k]], all + first[picked[k]] + count[picked[k]]);
    return out.data();
}

// A request for some of the files: what the pointers of rq point into
struct GatheredPngViews {
    std::vector<uint32_t> first, view_count; // (first: per file of `all`, its first record)
    std::vector<fpng_amd_crop> crops;
    std::vector<fpng_amd_resize_view> views;
    std::vector<fpng_amd_view_dest> dests;
    std::vector<fpng_amd_view_dest_hwc> hwc;
    std::vector<fpng_amd_view_color> colors;
    std::vector<fpng_amd_view_post> posts;
    std::vector<fpng_amd_view_warp> warps;
    std::vector<fpng_amd_view_tone> tones;
    std::vector<fpng_amd_view_enhance> enhances;
    std::vector<fpng_amd_view_alpha> alphas;
    std::vector<fpng_amd_view_resample> resamples;
    fpng_amd_png_views rq = {};

    // all: a request over n files whose counts are good (each >= 1, their sum fits 32 bits); picked: n_picked of its files, in
    // any order.  fmt, flags and reserved are all's
    void gather(const fpng_amd_png_views &all, uint32_t n, const uint32_t *picked, uint32_t n_picked)
    {
        first.resize(n), index.resize(n), one.assign(n, 1u);
        for (uint32_t i = 0, at = 0; i < n; at += all.view_count[i++]) first[i] = at, index[i] = i;
        const uint32_t *f = first.data(), *c = all.view_count;
        rq = all;
        rq.view_count = gather_views(all.view_count, picked, n_picked, index.data(), one.data(), view_count); // (file f's one count, at f)
        rq.crops = gather_views(all.crops, picked, n_picked, f, c, crops);
        rq.views = gather_views(all.views, picked, n_picked, f, c, views);
        rq.dests = gather_views(all.dests, picked, n_picked, f, c, dests);
        rq.hwc = gather_views(all.hwc, picked, n_picked, f, c, hwc);
        rq.colors = gather_views(all.colors, picked, n_picked, f, c, colors);
        rq.posts = gather_views(all.posts, picked, n_picked, f, c, posts);
        rq.warps = gather_views(all.warps, picked, n_picked, f, c, warps);
        rq.tones = gather_views(all.tones, picked, n_picked, f, c, tones);
        rq.enhances = gather_views(all.enhances, picked, n_picked, f, c, enhances);
        rq.alphas = gather_views(all.alphas, picked, n_picked, f, c, alphas);
        rq.resamples = gather_views(all.resamples, picked, n_picked, f, c, resamples);
    }

private:
    std::vector<uint32_t> index, one;
};

} // namespace fpng_amd
