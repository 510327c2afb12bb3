// view_plan_alpha.cpp -- what the views stage's host plan (fpng_amd/csrc/view_plan.h) makes of the alpha records of the _views_alpha
// calls, for four files with 3, 2, 1 and 2 views: file 0 has four channels and three planes in its destinations, file 1 three
// channels, file 2 four channels and no record with an op, file 3 four channels and four planes.  Held here: the op and the
// background travel in DecResize::flags next to the mirror flag, and every other field of the record is the one of the plan
// without alpha records; a record of a 3-channel file normalises to op 0; the job of a 4-channel file with an alpha view decodes
// four planes into the scratch whatever its destinations have, no other job decodes more than its destinations' planes, and the
// intermediate planes grow by exactly those fourth planes.  Per layout one line "ok <layout>".  Host-only: built with the system's
// C++ compiler, no HIP runtime linked, nothing loaded into an interpreter.
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

constexpr uint32_t kFiles = 4, kViews = 8;
const uint32_t kCounts[kFiles] = {3, 2, 1, 2}, kFileChans[kFiles] = {4, 3, 4, 4}, kPlanes[kFiles] = {3, 4, 3, 4};
const fpng_amd_crop kCrops[kViews] = {{0, 0, 96, 64}, {10, 5, 300, 200}, {0, 0, 50, 50}, {3, 5, 40, 30}, {100, 100, 64, 48}, {7, 9, 200, 120}, {0, 0, 33, 17}, {5, 5, 20, 10}};
const fpng_amd_resize_view kSizes[kViews] = {{48, 32, 0, 0, 48, 32, 0, 0},    {150, 100, 3, 2, 130, 70, 1, 1}, {25, 25, 0, 0, 25, 25, 0, 0}, {20, 15, 0, 0, 20, 15, 1, 1},
                                             {128, 96, 10, 7, 100, 40, 0, 0}, {100, 60, 0, 0, 100, 60, 0, 1},  {33, 17, 0, 0, 33, 17, 1, 0}, {40, 20, 0, 0, 40, 20, 1, 1}};

struct Built {
    ViewPlan plan;
    std::vector<uint32_t> job_planes;
    std::vector<size_t> job_out;
};

int build(bool hwc, const fpng_amd_view_alpha *alphas, std::vector<std::vector<uint8_t>> &pixels, Built &b)
{
    static fpng_amd_view_dest dests[kViews];
    static fpng_amd_view_dest_hwc hwcs[kViews];
    for (uint32_t v = 0; v < kViews; v++) {
        dests[v] = {}, hwcs[v] = {};
        dests[v].d_pixels = pixels[v].data(), dests[v].pixels_cap = pixels[v].size();
        hwcs[v].d_pixels = pixels[v].data(), hwcs[v].pixels_cap = pixels[v].size();
    }
    ViewRequest rq;
    rq.family = alphas ? ViewFamily::Alpha : ViewFamily::Plain, rq.view_count = kCounts, rq.crops = kCrops, rq.views = kSizes, rq.alphas = alphas;
    if (hwc) rq.hwc = hwcs;
    else rq.dests = dests;
    b.plan.begin(rq, kFiles, 1);
    for (uint32_t i = 0; i < kFiles; i++) {
        const DecCrop box = b.plan.file_box(i);
        fpng_amd_png f = {};
        fpng_amd_png_planar x = {};
        const uint32_t in_scratch = b.plan.job_planes(i, kFileChans[i], kPlanes[i]);
        const Refusal no = b.plan.file_records(i, f, x, kPlanes[i], box, kFileChans[i]);
        CHECK(!no && b.plan.file_recs.size() == kCounts[i]);
        b.job_planes.push_back(in_scratch);
        b.job_out.push_back(b.plan.add_job(i, kPlanes[i], box, in_scratch));
    }
    b.plan.close();
    return 0;
}

int run(bool hwc)
{
    std::vector<std::vector<uint8_t>> pixels(kViews);
    for (uint32_t v = 0; v < kViews; v++) pixels[v].resize((size_t)kSizes[v].w * kSizes[v].h * 4);
    // file 0: composite, none, premultiplied; file 1 (three channels): both ops; file 2: none; file 3: none, composite over black
    fpng_amd_view_alpha alphas[kViews] = {};
    alphas[0].op = FPNG_AMD_ALPHA_COMPOSITE, alphas[0].background[0] = 255, alphas[0].background[1] = 128, alphas[0].background[2] = 1;
    alphas[2].op = FPNG_AMD_ALPHA_PREMULTIPLIED;
    alphas[3].op = FPNG_AMD_ALPHA_COMPOSITE, alphas[3].background[0] = 9, alphas[4].op = FPNG_AMD_ALPHA_PREMULTIPLIED;
    alphas[7].op = FPNG_AMD_ALPHA_COMPOSITE;
    for (uint32_t v = 0; v < kViews; v++) CHECK(!check_alpha_record(alphas[v]));
    Built with, without;
    if (int rc = build(hwc, alphas, pixels, with)) return rc;
    if (int rc = build(hwc, nullptr, pixels, without)) return rc;
    const ViewPlan &p = with.plan, &q = without.plan;
    CHECK(p.resize.size() == kViews && q.resize.size() == kViews);

    // the op and the background in the flags, next to the mirror flag; a 3-channel file's records normalise to op 0
    const uint32_t want_op[kViews] = {1, 0, 2, 0, 0, 0, 0, 1};
    for (uint32_t v = 0; v < kViews; v++) {
        const DecResize &r = p.resize[v];
        CHECK(resize_alpha_op(r.flags) == want_op[v]);
        CHECK((r.flags & kResizeMirror) == (kSizes[v].flags & kResizeMirror));
        if (!want_op[v]) CHECK(r.flags == kSizes[v].flags);
        // (every other field: the plan's without alpha records, but for where the job's planes lie in the scratch)
        DecResize a = r, c = q.resize[v];
        a.flags = c.flags = 0, a.src = c.src = nullptr;
        CHECK(!memcmp(&a, &c, sizeof a));
        CHECK(p.lds[v] == q.lds[v] && p.tiles[v] == q.tiles[v]);
    }
    CHECK(resize_alpha_bg(p.resize[0].flags, 0) == 255 && resize_alpha_bg(p.resize[0].flags, 1) == 128 && resize_alpha_bg(p.resize[0].flags, 2) == 1);
    CHECK(resize_alpha_bg(p.resize[0].flags, 3) == 0 && p.resize[2].flags >> kResizeBgShift == 0);
    CHECK(p.resize[7].flags == (kResizeMirror | kAlphaComposite << kResizeAlphaShift)); // (a black background: an op all the same)
    CHECK(p.plane_pre == q.plane_pre && p.tile_pre == q.tile_pre); // (the launches' grids do not know of the stage)

    // the planes in the scratch
    const uint32_t want_planes[kFiles] = {4, 4, 3, 4};
    size_t extra = 0;
    for (uint32_t i = 0; i < kFiles; i++) {
        CHECK(with.job_planes[i] == want_planes[i] && without.job_planes[i] == kPlanes[i]);
        CHECK(with.job_out[i] == without.job_out[i] + extra);
        if (want_planes[i] != kPlanes[i]) {
            const DecCrop box = views_box(kCrops + p.first_view(i), kSizes + p.first_view(i), kCounts[i]);
            extra += (((size_t)box.w * box.h * 4 + 15) & ~(size_t)15) - (((size_t)box.w * box.h * 3 + 15) & ~(size_t)15);
        }
    }
    CHECK(extra && p.mid_total == q.mid_total + extra);
    // a view's planes stay inside its job's: the alpha plane of file 0's views is plane 3 of a box of four
    for (uint32_t i = 0; i < kFiles; i++)
        for (uint32_t v = p.job_rec[i]; v < p.job_rec[i + 1]; v++) {
            const DecResize &r = p.resize[v];
            const size_t end = (i + 1 < kFiles ? with.job_out[i + 1] : p.mid_total);
            const uint32_t read = resize_alpha_op(r.flags) ? 4 : r.planes;
            CHECK((size_t)(uintptr_t)r.src >= with.job_out[i] && (size_t)(uintptr_t)r.src + (read - 1) * r.src_plane_pitch < end);
        }
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
