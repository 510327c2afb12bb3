// view_plan_build.cpp -- builds the views stage's host records (fpng_amd/csrc/view_plan.h: ViewPlan, everything up to and including
// the set-up block) for a batch of four files with 2, 1, 3 and 1 views whose second file gets no job, for planar and channels-last
// destinations and for the plain, the colour and the post family (whose views mix direct, blur, warp, tone and enhance views), and
// holds the index arrays against each other: job ranges are contiguous and cover every record, direct plus post records are all
// records, every tone ref points at a post record with a tone op inside its job's range, prefix sums increase and end at the tile
// totals, and what went into the set-up block is what the plan holds.  Every buffer is a heap block of exactly the size the plan
// asked for: a write past one is the address sanitizer's to find.  Per configuration one line "ok <layout> <family>".  Host-only:
// built with the system's C++ compiler and its sanitizers, no HIP runtime linked, nothing loaded into an interpreter.
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

constexpr uint32_t kFiles = 4, kViews = 7, kPlanes = 3;
const uint32_t kCounts[kFiles] = {2, 1, 3, 1};
// (crop, full size, window, mirror, filter) per view: one tile, several tiles, a window of a larger full size
const fpng_amd_crop kCrops[kViews] = {{0, 0, 96, 64}, {10, 5, 300, 200}, {0, 0, 50, 50}, {3, 5, 40, 30}, {100, 100, 64, 48}, {7, 9, 200, 120}, {0, 0, 33, 17}};
const fpng_amd_resize_view kSizes[kViews] = {{48, 32, 0, 0, 48, 32, 0, 0},   {150, 100, 3, 2, 130, 70, 1, 1}, {25, 25, 0, 0, 25, 25, 0, 0}, {20, 15, 0, 0, 20, 15, 1, 1},
                                             {128, 96, 10, 7, 100, 40, 0, 0}, {100, 60, 0, 0, 100, 60, 0, 1},   {33, 17, 0, 0, 33, 17, 1, 0}};

template <class T> bool increasing(const std::vector<T> &v)
{
    for (size_t k = 1; k < v.size(); k++)
        if (!(v[k - 1] < v[k])) return false;
    return true;
}

int run(bool hwc, ViewFamily family)
{
    // the request, normalised as decode_api.cpp does it: post records only with matrices
    std::vector<std::vector<uint8_t>> pixels(kViews);
    fpng_amd_view_dest dests[kViews] = {};
    fpng_amd_view_dest_hwc hwcs[kViews] = {};
    fpng_amd_view_color colors[kViews] = {};
    fpng_amd_view_post posts[kViews] = {};
    fpng_amd_view_warp warps[kViews] = {};
    fpng_amd_view_tone tones[kViews] = {};
    fpng_amd_view_enhance enhances[kViews] = {};
    for (uint32_t v = 0; v < kViews; v++) {
        pixels[v].resize((size_t)kSizes[v].w * kSizes[v].h * 4);
        dests[v].d_pixels = pixels[v].data(), dests[v].pixels_cap = pixels[v].size();
        hwcs[v].d_pixels = pixels[v].data(), hwcs[v].pixels_cap = pixels[v].size(), hwcs[v].pixel_elems = v & 1 ? 4 : 0, hwcs[v].flags = v & 2 ? 1 : 0;
        colors[v].m[0][0] = colors[v].m[1][1] = colors[v].m[2][2] = 1.0f + 0.125f * v;
    }
    // view 0 direct, 1 blur, (2: the file without a job, a tone view), 3 warp, 4 tone, 5 direct, 6 tone + enhance
    posts[1].flags = kPostBlur, posts[1].blur_radius = 2, posts[1].blur_sigma = 1.5;
    tones[2].op = 2;
    warps[3].flags = 1, warps[3].a[0] = 1.0, warps[3].a[1] = 0.25, warps[3].a[4] = 1.0;
    tones[4].op = 1;
    tones[6].op = 3, tones[6].factor = 1.5f, enhances[6].op = 1, enhances[6].factor = 0.5f;
    const bool want_post[kViews] = {false, true, true, true, true, false, true}, want_tone[kViews] = {false, false, true, false, true, false, true};
    ViewRequest rq;
    rq.family = family, rq.view_count = kCounts, rq.crops = kCrops, rq.views = kSizes;
    if (hwc) rq.hwc = hwcs;
    else rq.dests = dests;
    if (family >= ViewFamily::Color) rq.colors = colors;
    if (family >= ViewFamily::Post) rq.posts = posts, rq.warps = warps, rq.tones = tones, rq.enhances = enhances;
    const bool post_call = rq.posts != nullptr;

    // ---- parse ----
    ViewPlan plan;
    plan.begin(rq, kFiles, 1);
    CHECK(plan.active() && plan.multi() && plan.hwc() == hwc);
    std::vector<uint32_t> job_file;
    std::vector<size_t> job_out;
    for (uint32_t i = 0; i < kFiles; i++) {
        const DecCrop box = plan.file_box(i);
        CHECK(box.w && box.h);
        fpng_amd_png f = {};
        fpng_amd_png_planar x = {};
        const Refusal no = plan.file_records(i, f, x, kPlanes, box);
        CHECK(!no);
        CHECK(plan.file_recs.size() == kCounts[i]);
        if (i == 1) continue; // (this file does not become a job: its records never join the plan)
        job_out.push_back(plan.add_job(i, kPlanes, box));
        job_file.push_back(i);
    }
    plan.close();
    const size_t nj = job_file.size(), nr = plan.resize.size();

    // ---- place and plan: the set-up block is job records, the plan's records and a tail ----
    Carver sc;
    sc.carve(1000); // (what lies in front of the block)
    const size_t o_jobs = sc.carve(nj * 64);
    plan.carve_records(sc);
    const size_t o_tail = sc.carve(100), setup_len = o_tail + 100 - o_jobs;
    plan.carve_scratch(sc);
    uint8_t *const base = (uint8_t *)malloc(sc.need), *const h_setup = (uint8_t *)malloc(setup_len);
    if (!base || !h_setup) return 3;
    memset(h_setup, 0, setup_len);
    plan.place(base);
    plan.write_setup(h_setup, o_jobs);

    // job ranges are contiguous and cover every record
    CHECK(nr == 2 + 3 + 1 && plan.job_rec.size() == nj + 1 && plan.job_rec.front() == 0 && plan.job_rec.back() == nr);
    for (size_t k = 0; k < nj; k++) CHECK(plan.job_rec[k + 1] - plan.job_rec[k] == kCounts[job_file[k]]);
    CHECK(increasing(job_out) && plan.mid_total % 16 == 0);
    CHECK(plan.tiles.size() == nr && plan.lds.size() == nr && plan.plane_pre.size() == nr + 1 && increasing(plan.plane_pre));
    uint64_t all_tiles = 0;
    for (size_t q = 0; q < nr; q++) {
        CHECK(plan.tiles[q] == resize_tiles(plan.resize[q].w, plan.resize[q].h) && plan.tiles[q] >= 1);
        all_tiles += plan.tiles[q];
        CHECK(plan.resize[q].src >= plan.d_mid && plan.resize[q].src < plan.d_mid + plan.mid_total);
    }
    CHECK(plan.plane_pre.back() == all_tiles * kPlanes);
    if (plan.per_tile()) CHECK(plan.tile_pre.size() == nr + 1 && increasing(plan.tile_pre) && plan.tile_pre.back() == all_tiles && plan.hwc_px.size() == nr);
    if (rq.colors) CHECK(plan.color_view.size() == nr);
    // the view of record q: the records skip the views of the file without a job
    std::vector<uint32_t> view_of;
    for (size_t k = 0; k < nj; k++)
        for (uint32_t v = 0; v < kCounts[job_file[k]]; v++) view_of.push_back(plan.first_view(job_file[k]) + v);
    CHECK(view_of.size() == nr);
    for (size_t q = 0; q < nr && rq.colors; q++) CHECK(plan.color_view[q] == view_of[q]);

    const uint8_t *const h_recs = h_setup + (plan.at.recs - o_jobs);
    const uint64_t *const h_pre = (const uint64_t *)(h_setup + (plan.at.pre - o_jobs));
    CHECK(plan.at.recs >= o_jobs + nj * 64 && plan.at.tone_refs + plan.tone_refs.size() * sizeof(DecToneRef) <= o_tail);
    if (!post_call) {
        CHECK(plan.post_recs.empty() && plan.tone_refs.empty() && plan.post_of.empty() && plan.n_tone() == 0);
        for (size_t q = 0; q < nr; q++) {
            DecResize r;
            memcpy(&r, h_recs + q * plan.rec_bytes(), sizeof r);
            CHECK(r.w == kSizes[view_of[q]].w && r.h == kSizes[view_of[q]].h && r.dst == pixels[view_of[q]].data() && r.src == plan.resize[q].src);
            if (rq.colors) {
                DecResizeColor c;
                memcpy(&c, h_recs + q * sizeof c, sizeof c);
                CHECK(c.m[1][1] == colors[view_of[q]].m[1][1]);
            }
            if (hwc) {
                DecResizeHwc d;
                memcpy(&d, h_recs + q * plan.rec_bytes(), sizeof d);
                CHECK(d.pixel_elems == (view_of[q] & 1 ? 4u : kPlanes) && d.hwc_flags == (view_of[q] & 2 ? 1u : 0u));
            }
        }
        const std::vector<uint64_t> &pre = plan.per_tile() ? plan.tile_pre : plan.plane_pre;
        CHECK(!memcmp(h_pre, pre.data(), pre.size() * 8));
    } else {
        // direct plus post records are all records; each kind keeps the views' order
        const size_t np = plan.post_recs.size(), nd = nr - np;
        CHECK(plan.post_of.size() == nr && plan.job_post.size() == nj + 1 && plan.job_post.front() == 0 && plan.job_post.back() == np);
        size_t seen = 0;
        for (size_t k = 0; k < nj; k++)
            for (uint32_t q = plan.job_rec[k]; q < plan.job_rec[k + 1]; q++) {
                CHECK((plan.post_of[q] >= 0) == want_post[view_of[q]]);
                if (plan.post_of[q] < 0) continue;
                CHECK((size_t)plan.post_of[q] == seen && seen >= plan.job_post[k] && seen < plan.job_post[k + 1]);
                const DecViewPost &pr = plan.post_recs[seen++];
                CHECK(pr.dst == pixels[view_of[q]].data() && pr.src == plan.resize[q].dst && pr.src >= plan.d_mid && pr.src + (size_t)pr.w * pr.h * kPlanes <= plan.d_mid + plan.mid_total);
                CHECK(((pr.src - plan.d_mid) & 15) == 0 && (pr.tone_op != 0) == want_tone[view_of[q]] && (pr.tone != nullptr) == (pr.tone_op != 0));
            }
        CHECK(seen == np && np == 4 && nd == 2);
        // prefix sums increase and end at the tile totals
        CHECK(plan.dir_pre.size() == nd + 1 && plan.post_pre.size() == np + 1 && increasing(plan.dir_pre) && increasing(plan.post_pre));
        CHECK(plan.dir_pre.front() == 0 && plan.post_pre.front() == 0 && plan.dir_pre.back() + plan.post_pre.back() == all_tiles);
        CHECK(!memcmp(h_pre, plan.dir_pre.data(), (nd + 1) * 8) && !memcmp(h_pre + nd + 1, plan.post_pre.data(), (np + 1) * 8));
        CHECK(!memcmp(h_setup + (plan.at.post - o_jobs), plan.post_recs.data(), np * sizeof(DecViewPost)));
        // the records of the block: the direct ones in front
        size_t di = 0, pi = 0;
        for (size_t q = 0; q < nr; q++) {
            DecResizeColor c;
            memcpy(&c, h_recs + (plan.post_of[q] >= 0 ? nd + pi++ : di++) * sizeof c, sizeof c);
            CHECK(c.d.r.w == kSizes[view_of[q]].w && c.d.r.src == plan.resize[q].src && c.d.r.dst == plan.resize[q].dst && c.m[0][0] == colors[view_of[q]].m[0][0]);
            CHECK(plan.post_of[q] >= 0 ? (c.d.pixel_elems == 0 && !(c.d.r.flags & kResizeMirror)) : (c.d.r.dst == pixels[view_of[q]].data()));
        }
        // every tone ref points at a post record with a tone op, inside its job's range; the chunks' sums close
        const size_t nt = plan.n_tone();
        CHECK(nt == 2 && plan.tone_refs.size() == nt + 1 && plan.job_tone.size() == nj + 1 && plan.job_tone.front() == 0 && plan.job_tone.back() == nt);
        uint64_t chunks = 0;
        for (size_t k = 0; k < nj; k++)
            for (uint32_t t = plan.job_tone[k]; t < plan.job_tone[k + 1]; t++) {
                const DecToneRef &ref = plan.tone_refs[t];
                CHECK(ref.rec >= plan.job_post[k] && ref.rec < plan.job_post[k + 1] && plan.post_recs[ref.rec].tone_op != 0 && ref.pre == chunks);
                CHECK((uint8_t *)plan.post_recs[ref.rec].tone == plan.d_tone + t * kToneBytes);
                chunks += tone_chunks(plan.post_recs[ref.rec].w, plan.post_recs[ref.rec].h);
            }
        CHECK(plan.tone_refs.back().pre == chunks && chunks >= nt);
        CHECK(plan.d_tone + nt * kToneBytes <= base + sc.need);
        CHECK(!memcmp(h_setup + (plan.at.tone_refs - o_jobs), plan.tone_refs.data(), (nt + 1) * sizeof(DecToneRef)));
    }
    free(h_setup), free(base);
    printf("ok %s %d\n", hwc ? "hwc" : "planar", (int)family);
    return 0;
}

// a call without views: the plan holds nothing and asks for nothing
int run_empty()
{
    ViewPlan plan;
    plan.begin(ViewRequest(), kFiles, 1);
    plan.close();
    Carver sc;
    plan.carve_records(sc), plan.carve_scratch(sc);
    plan.place(nullptr), plan.write_setup(nullptr, 0);
    CHECK(!plan.active() && sc.need == 0 && plan.job_rec.capacity() == 0 && plan.plane_pre.capacity() == 0 && plan.view_ofs.capacity() == 0);
    printf("ok empty\n");
    return 0;
}

} // namespace

int main()
{
    for (int hwc = 0; hwc < 2; hwc++)
        for (ViewFamily family : {ViewFamily::Plain, ViewFamily::Color, ViewFamily::Enhance})
            if (int rc = run(hwc != 0, family)) return rc;
    return run_empty();
}
