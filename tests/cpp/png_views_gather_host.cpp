// png_views_gather_host.cpp -- fpng_amd/csrc/png_views_gather.h alone: files {1, 3} of a 5-file request with 2, 1, 3, 1, 2 views and
// every array given are compacted, and each array's records are compared with the ranges they came from.  Every record of the full
// request carries its own index, so a record from the wrong place shows.  Prints "ok" and exits 0, or says what differs.
#include "png_views_gather.h"

#include <cstdio>
#include <cstring>

using namespace fpng_amd;

template <class T> static int same(const char *what, const T *got, const T *all, const uint32_t *from, uint32_t n)
{
    for (uint32_t k = 0; k < n; k++)
        if (memcmp(&got[k], &all[from[k]], sizeof(T)) != 0) {
            printf("%s: record %u is not record %u of the request\n", what, k, from[k]);
            return 1;
        }
    return 0;
}

int main()
{
    const uint32_t counts[5] = {2, 1, 3, 1, 2}, total = 9, picked[2] = {1, 3};
    const uint32_t from[2] = {2, 6}; // file 1's one view is view 2, file 3's view 6
    fpng_amd_crop crops[total];
    fpng_amd_resize_view views[total];
    fpng_amd_view_dest dests[total];
    fpng_amd_view_dest_hwc hwc[total];
    fpng_amd_view_color colors[total];
    fpng_amd_view_post posts[total];
    fpng_amd_view_warp warps[total];
    fpng_amd_view_tone tones[total];
    fpng_amd_view_enhance enhances[total];
    fpng_amd_view_alpha alphas[total];
    fpng_amd_view_resample resamples[total];
    memset(crops, 0, sizeof crops), memset(views, 0, sizeof views), memset(dests, 0, sizeof dests), memset(hwc, 0, sizeof hwc), memset(colors, 0, sizeof colors);
    memset(posts, 0, sizeof posts), memset(warps, 0, sizeof warps), memset(tones, 0, sizeof tones), memset(enhances, 0, sizeof enhances), memset(alphas, 0, sizeof alphas);
    memset(resamples, 0, sizeof resamples);
    for (uint32_t v = 0; v < total; v++) {
        crops[v].x = 100 + v, views[v].full_w = 200 + v, dests[v].pixels_cap = 300 + v, hwc[v].pixels_cap = 400 + v, colors[v].m[0][0] = 500.0f + v;
        posts[v].blur_radius = 600 + v, warps[v].a[0] = 700.0 + v, tones[v].op = 800 + v, enhances[v].op = 900 + v, alphas[v].op = 1000 + v, resamples[v].filter = 1100 + v;
    }
    fpng_amd_float_format fmt = {};
    fpng_amd_png_views all = {counts, crops, views, dests, hwc, &fmt, colors, posts, warps, tones, enhances, alphas, resamples, FPNG_AMD_PNG_GENERAL_ONLY, 0};
    GatheredPngViews sub;
    sub.gather(all, 5, picked, 2);
    const fpng_amd_png_views &rq = sub.rq;
    int bad = 0;
    if (rq.view_count[0] != 1 || rq.view_count[1] != 1 || sub.view_count.size() != 2) printf("view_count: not {1, 1}\n"), bad = 1;
    if (sub.crops.size() != 2 || sub.resamples.size() != 2 || sub.hwc.size() != 2) printf("sizes: not 2 records per array\n"), bad = 1;
    bad |= same("crops", rq.crops, crops, from, 2) | same("views", rq.views, views, from, 2) | same("dests", rq.dests, dests, from, 2) | same("hwc", rq.hwc, hwc, from, 2);
    bad |= same("colors", rq.colors, colors, from, 2) | same("posts", rq.posts, posts, from, 2) | same("warps", rq.warps, warps, from, 2) | same("tones", rq.tones, tones, from, 2);
    bad |= same("enhances", rq.enhances, enhances, from, 2) | same("alphas", rq.alphas, alphas, from, 2) | same("resamples", rq.resamples, resamples, from, 2);
    if (rq.fmt != &fmt || rq.flags != FPNG_AMD_PNG_GENERAL_ONLY || rq.reserved != 0) printf("fmt, flags or reserved changed\n"), bad = 1;
    // files with several views, in another order, and arrays that are not given
    const uint32_t picked2[3] = {4, 0, 2}, from2[7] = {7, 8, 0, 1, 3, 4, 5};
    all.dests = nullptr, all.tones = nullptr;
    sub.gather(all, 5, picked2, 3);
    if (sub.rq.view_count[0] != 2 || sub.rq.view_count[1] != 2 || sub.rq.view_count[2] != 3) printf("view_count: not {2, 2, 3}\n"), bad = 1;
    if (sub.rq.dests || sub.rq.tones) printf("an array that was not given is given\n"), bad = 1;
    bad |= same("crops (2)", sub.rq.crops, crops, from2, 7) | same("hwc (2)", sub.rq.hwc, hwc, from2, 7) | same("warps (2)", sub.rq.warps, warps, from2, 7);
    if (!bad) printf("ok\n");
    return bad;
}
