// view_plan_resample.cpp -- what the views stage's host plan (fpng_amd/csrc/view_plan.h) makes of the RESAMPLE records of the
// _views_resample calls, for four files with 3, 2, 1 and 2 views of which the second becomes no job.  Held here, through the set-up
// block as the device gets it: the effective filter in DecResize::filter -- the record's where it has one, else the view's own; taps,
// rows and LDS by the effective filter's bounds; a file's box the union of its views' boxes under their effective filters; the
// NEAREST views' index tables -- w + h words each, Pillow's running sum, every index inside the view's box -- carved inside the
// set-up block and reached through the placed DecResize::nearest, and no table for any other view or for the file without a job; a
// record without a filter leaves its view's record what the plan without RESAMPLE records makes.  Per layout one line "ok <layout>".
// Host-only: built with the system's C++ compiler under the address and undefined-behaviour sanitizers, no HIP runtime linked,
// nothing loaded into an interpreter.
#include "view_plan.h"

#include <cstdio>
#include <cstdlib>

using namespace fpng_amd;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond);     \
            return 1;                                                            \
        }                                                                        \
    } while (0)

namespace {

struct Carver { // decode_api.cpp's Scratch without the device: 256-byte aligned pieces
    size_t need = 0;
    size_t carve(size_t n)
    {
        const size_t o = need;
        need += (n + 255) & ~(size_t)255;
        return o;
    }
};

constexpr uint32_t kFiles = 4, kViews = 8, kNoJob = 1;
const uint32_t kCounts[kFiles] = {3, 2, 1, 2};
const fpng_amd_crop kCrops[kViews] = {{0, 0, 96, 64}, {10, 5, 300, 200}, {0, 0, 50, 50}, {3, 5, 40, 30}, {100, 100, 64, 48}, {7, 9, 200, 120}, {0, 0, 33, 17}, {5, 5, 20, 10}};
const fpng_amd_resize_view kSizes[kViews] = {{3, 2, 0, 0, 3, 2, 0, 1},        {150, 100, 3, 2, 130, 70, 1, 1}, {25, 25, 0, 0, 25, 25, 0, 0}, {20, 15, 0, 0, 20, 15, 1, 1},
                                             {128, 96, 10, 7, 100, 40, 0, 0}, {100, 60, 0, 0, 100, 60, 0, 1},  {33, 17, 0, 0, 33, 17, 1, 0}, {70, 7, 3, 1, 65, 5, 1, 1}};
// file 0: NEAREST at exactly 32 x over a bicubic view, none, LANCZOS; file 1 (no job): NEAREST, BOX; file 2: HAMMING; file 3: none, NEAREST
const uint32_t kFilters[kViews] = {FPNG_AMD_RESAMPLE_NEAREST, 0, FPNG_AMD_RESAMPLE_LANCZOS, FPNG_AMD_RESAMPLE_NEAREST, FPNG_AMD_RESAMPLE_BOX, FPNG_AMD_RESAMPLE_HAMMING, 0,
                                   FPNG_AMD_RESAMPLE_NEAREST};

int build(bool hwc, const fpng_amd_view_resample *resamples, std::vector<std::vector<uint8_t>> &pixels, ViewPlan &plan, std::vector<DecCrop> &boxes)
{
    static fpng_amd_view_dest dests[kViews];
    static fpng_amd_view_dest_hwc hwcs[kViews];
    for (uint32_t v = 0; v < kViews; v++) {
        dests[v] = {}, hwcs[v] = {};
        dests[v].d_pixels = pixels[v].data(), dests[v].pixels_cap = pixels[v].size();
        hwcs[v].d_pixels = pixels[v].data(), hwcs[v].pixels_cap = pixels[v].size();
    }
    ViewRequest rq;
    rq.family = resamples ? ViewFamily::Resample : ViewFamily::Plain, rq.view_count = kCounts, rq.crops = kCrops, rq.views = kSizes, rq.resamples = resamples;
    if (hwc) rq.hwc = hwcs;
    else rq.dests = dests;
    plan.begin(rq, kFiles, 1);
    for (uint32_t i = 0; i < kFiles; i++) {
        const DecCrop box = plan.file_box(i);
        boxes.push_back(box);
        fpng_amd_png f = {};
        fpng_amd_png_planar x = {};
        const Refusal no = plan.file_records(i, f, x, 3, box, 3);
        CHECK(!no && plan.file_recs.size() == kCounts[i]);
        if (i != kNoJob) plan.add_job(i, 3, box); // (file kNoJob: its records, and its NEAREST view's indices, are dropped)
    }
    plan.close();
    return 0;
}

int run(bool hwc)
{
    std::vector<std::vector<uint8_t>> pixels(kViews);
    for (uint32_t v = 0; v < kViews; v++) pixels[v].resize((size_t)kSizes[v].w * kSizes[v].h * 4);
    fpng_amd_view_resample resamples[kViews] = {};
    for (uint32_t v = 0; v < kViews; v++) resamples[v].filter = kFilters[v];
    ViewPlan p, q;
    std::vector<DecCrop> boxes, plain_boxes;
    if (int rc = build(hwc, resamples, pixels, p, boxes)) return rc;
    if (int rc = build(hwc, nullptr, pixels, q, plain_boxes)) return rc;
    const uint32_t n_recs = kViews - kCounts[kNoJob];
    CHECK(p.resize.size() == n_recs && q.resize.size() == n_recs);

    // through the set-up block
    Carver sc;
    sc.carve(1000); // (what lies in front of the block)
    const size_t o_jobs = sc.carve(3 * 64);
    p.carve_records(sc);
    const size_t o_tail = sc.carve(100), setup_len = o_tail + 100 - o_jobs;
    p.carve_scratch(sc);
    std::vector<uint8_t> base(sc.need), h_setup(setup_len, 0);
    p.place(base.data());
    p.write_setup(h_setup.data(), o_jobs);
    CHECK(p.at.nearest >= o_jobs && p.at.nearest + p.nearest.size() * 4 <= o_tail); // (the tables lie inside the block)

    size_t words = 0;
    for (uint32_t i = 0, v = 0, rec = 0; i < kFiles; i++) {
        // the file's box: the union of its views' boxes, each under its effective filter
        uint64_t x0 = UINT64_MAX, y0 = UINT64_MAX, x1 = 0, y1 = 0;
        for (uint32_t k = 0; k < kCounts[i]; k++) {
            const DecCrop b = view_box({kCrops[v + k].x, kCrops[v + k].y, kCrops[v + k].w, kCrops[v + k].h}, kSizes[v + k], &resamples[v + k]);
            x0 = std::min<uint64_t>(x0, b.x), y0 = std::min<uint64_t>(y0, b.y), x1 = std::max<uint64_t>(x1, (uint64_t)b.x + b.w), y1 = std::max<uint64_t>(y1, (uint64_t)b.y + b.h);
        }
        CHECK(boxes[i].x == x0 && boxes[i].y == y0 && boxes[i].w == x1 - x0 && boxes[i].h == y1 - y0);
        for (uint32_t k = 0; k < kCounts[i]; k++, v++) {
            if (i == kNoJob) continue;
            const fpng_amd_resize_view &z = kSizes[v];
            const uint32_t filter = kFilters[v] ? kFilters[v] + 1 : z.filter;
            // the record as the kernel reads it
            DecResize r;
            memcpy(&r, h_setup.data() + (p.at.recs - o_jobs) + rec * p.rec_bytes(), sizeof r);
            CHECK(!memcmp(&r, &p.resize[rec], sizeof r));
            CHECK(r.filter == filter && view_filter(z, &resamples[v]) == filter && resize_scale_ok(r.in_w, r.full_w, filter) && resize_scale_ok(r.in_h, r.full_h, filter));
            CHECK(r.taps_x == resize_max_taps(r.in_w, r.full_w, filter) && r.taps_y == resize_max_taps(r.in_h, r.full_h, filter) && r.rows == resize_tile_rows(r.in_h, r.full_h, filter));
            CHECK(r.taps_x <= kResizeMaxTaps && r.taps_y <= kResizeMaxTaps && p.lds[rec] <= 65536u);
            if (filter == kResizeNearest) {
                CHECK(r.taps_x == 1 && r.taps_y == 1 && r.nearest == (const uint32_t *)(base.data() + p.at.nearest) + words);
                const uint32_t *table = (const uint32_t *)(h_setup.data() + (p.at.nearest - o_jobs)) + words; // (what the pointer reaches once the block is uploaded)
                std::vector<uint32_t> want((size_t)z.w + z.h);
                CHECK(resize_nearest_indices(r.in_w, r.full_w, z.x, z.w, want.data()) && resize_nearest_indices(r.in_h, r.full_h, z.y, z.h, want.data() + z.w));
                CHECK(!memcmp(table, want.data(), want.size() * 4));
                // (every index inside the view's box, whose origin the record carries; the box inside the job's planes)
                const DecCrop b = view_box({0, 0, r.in_w, r.in_h}, z, &resamples[v]);
                CHECK(r.box_x == b.x && r.box_y == b.y && table[0] == b.x && table[z.w - 1] + 1 == b.x + b.w && table[z.w] == b.y && table[z.w + z.h - 1] + 1 == b.y + b.h);
                for (uint32_t t = 1; t < z.w; t++) CHECK(table[t] >= table[t - 1] && table[t] < r.in_w);
                for (uint32_t t = 1; t < z.h; t++) CHECK(table[z.w + t] >= table[z.w + t - 1] && table[z.w + t] < r.in_h);
                words += want.size();
            } else
                CHECK(r.nearest == nullptr);
            if (!kFilters[v]) { // (a record without a filter: the view's record of the plan without RESAMPLE records, but for where its file's box lies)
                DecResize a = p.resize[rec], c = q.resize[rec];
                a.src = c.src = nullptr, a.src_pitch = c.src_pitch = 0, a.src_plane_pitch = c.src_plane_pitch = 0;
                CHECK(!memcmp(&a, &c, sizeof a) && p.lds[rec] == q.lds[rec] && p.tiles[rec] == q.tiles[rec]);
            }
            rec++;
        }
    }
    CHECK(words == p.nearest.size() && words == (size_t)(3 + 2) + (65 + 5)); // (views 0 and 7; view 3's file became no job)
    CHECK(q.nearest.empty() && p.plane_pre == q.plane_pre && p.tile_pre == q.tile_pre);
    printf("ok %s\n", hwc ? "hwc" : "planar");
    return 0;
}

} // namespace

int main()
{
    for (bool hwc : {false, true})
        if (int rc = run(hwc)) return rc;
    return 0;
}
