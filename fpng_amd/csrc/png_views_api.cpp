// png_views_api.cpp -- fpng_amd_decode_batch(_device)_png_views: views of ordinary PNG files.  The request is judged as the views
// call of its family judges it (view_request.h), the files are routed as fpng_amd_decode_batch(_device)_png routes them -- by the
// same code: png_tier.h -- fpng-written ones through the existing views path, with their part of the request, and the general
// tier's files run in groups: inflate (only the rows that the file's box needs are kept), the states back, a ViewPlan of the
// group's good files with their real channel counts, png_unfilter_box_kernel into the plan's planes, the states back, and the
// plan's own launches.  Everything that can refuse the CALL is judged from the heads and the request before the first kernel of
// the general tier runs.  What is this call's own lives here: the request's refusals, the pre-judging of every file (box, room,
// share of the plan's scratch), the two plans of a group and its boxes, the job runs.  Heads, routing, groups, the scratch layout
// in front of the plan, the file records and the results' fold are the tier's (png_tier.h, png_tier_plan.h).
#include "decode.h"
#include "encoder.h"
#include "png_decode.h"
#include "png_tier.h"
#include "png_views_gather.h"
#include "view_request.h"

#include "fpng.h"

#include <cstring>
#include <vector>

using namespace fpng_amd;

namespace {

static_assert(sizeof(fpng_amd_png_views) == 112 && offsetof(fpng_amd_png_views, colors) == 48 && offsetof(fpng_amd_png_views, flags) == 104, "fpng_amd_png_views layout");
static_assert(FPNG_AMD_DECODE_PNG_CROP_OUTSIDE == 68 && FPNG_AMD_DECODE_CROP_OUTSIDE == 67 && FPNG_AMD_DECODE_UNSUPPORTED_PNG == 67, "67 means UNSUPPORTED_PNG here");

// the scratch behind a group's records, bytes and scanlines: ViewPlan's carve calls
struct Carver {
    size_t need;
    size_t carve(size_t n) { const size_t o = need; need += align256(n); return o; }
};

// the request as the views calls carry it; the family: the last stage array given
ViewRequest as_request(const fpng_amd_png_views &q)
{
    ViewRequest rq;
    rq.fmt = q.fmt, rq.crops = q.crops, rq.views = q.views, rq.view_count = q.view_count, rq.dests = q.dests, rq.hwc = q.hwc;
    rq.colors = q.colors, rq.posts = q.posts, rq.warps = q.warps, rq.tones = q.tones, rq.enhances = q.enhances, rq.alphas = q.alphas, rq.resamples = q.resamples;
    rq.family = q.resamples ? ViewFamily::Resample : q.alphas ? ViewFamily::Alpha : q.enhances ? ViewFamily::Enhance : q.tones ? ViewFamily::Tone
                : q.warps   ? ViewFamily::Warp     : q.posts  ? ViewFamily::Post  : q.colors   ? ViewFamily::Color   : ViewFamily::Plain;
    return rq;
}

// does decode_device_png at 4 channels give this file an alpha that can be below 255?  (the plan's 4-channel files)
bool has_alpha_plane(uint32_t color, uint32_t trns_len) { return color == 4 || color == 6 || (color == 3 && trns_len) || (color == 0 && trns_len >= 2) || (color == 2 && trns_len >= 6); }

// The plan of files g0 .. g1 - 1 of `general`: those whose `good` entry is set (NULL: all), with chans[k - g0] channels.  The
// destinations have been judged: a refusal here is the same one.  job_of: per file its job, or -1
int build_plan(ViewPlan &plan, const ViewRequest &rq, uint32_t n, uint32_t elem, const fpng_amd_png_planar *files, const std::vector<TierFile> &general, size_t g0, size_t g1,
               const uint8_t *good, const uint32_t *chans, std::vector<int32_t> &job_of, std::vector<size_t> &out_ofs, std::vector<uint32_t> &planes_of)
{
    plan.begin(rq, n, elem);
    job_of.assign(g1 - g0, -1), out_ofs.assign(g1 - g0, 0), planes_of.assign(g1 - g0, 0);
    int32_t jobs = 0;
    for (size_t k = g0; k < g1; k++) {
        if (good && !good[k - g0]) continue;
        const TierFile &q = general[k];
        const fpng_amd_png_planar &x = files[q.file];
        const fpng_amd_png plain = {x.data, x.size, 0, nullptr, 0};
        const DecCrop box = plan.file_box(q.file);
        if (const Refusal no = plan.file_records(q.file, plain, x, x.num_chans, box, chans[k - g0])) return fail(no.code, no.why);
        planes_of[k - g0] = plan.job_planes(q.file, chans[k - g0], x.num_chans);
        out_ofs[k - g0] = plan.add_job(q.file, x.num_chans, box, planes_of[k - g0]);
        job_of[k - g0] = jobs++;
    }
    plan.close();
    return FPNG_AMD_OK;
}

int png_views(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const fpng_amd_png_views *rq_in, fpng_amd_decode_result *results, bool device_data)
{
    // 0. what needs no file, no encoder and no device: the record's own words, then everything the family's views call judges
    if (!rq_in) return fail(FPNG_AMD_ERR_INVALID_ARG, "null request");
    if (rq_in->reserved) return fail(FPNG_AMD_ERR_INVALID_ARG, "fpng_amd_png_views::reserved must be 0");
    if (rq_in->flags & ~FPNG_AMD_PNG_GENERAL_ONLY) return fail(FPNG_AMD_ERR_INVALID_ARG, "unknown fpng_amd_png_views::flags bits (FPNG_AMD_PNG_GENERAL_ONLY)");
    if (!rq_in->dests == !rq_in->hwc) return fail(FPNG_AMD_ERR_INVALID_ARG, "exactly one of fpng_amd_png_views::dests and hwc");
    const ViewRequest asked = as_request(*rq_in);
    StagesUsed used;
    if (int rc = check_views_request(files, n, asked, results, used)) return rc;
    if (!e || !files || !n || !results) return fail(FPNG_AMD_ERR_INVALID_ARG, "null/empty batch");
    // (the files' and the destinations' own words, as the planar family judges them behind the encoder: decode_files_planar)
    DecFloat flt;
    uint32_t elem;
    if (int rc = check_float_format(asked.fmt, flt, elem)) return rc;
    for (uint32_t i = 0; i < n; i++)
        if (files[i].num_chans != 3 && files[i].num_chans != 4) return fail(FPNG_AMD_ERR_INVALID_ARG, "num_chans must be 3 or 4");
    if (int rc = check_view_dests(asked, used.total, elem)) return rc;
    ViewDefaults made;
    const ViewRequest rq = normalise_views(asked, used, made);
    const uint32_t flags = rq_in->flags;
    std::memset(results, 0, (size_t)n * sizeof *results);
    HIP_TRY(hipSetDevice(e->device));
    int rc = drain(e);
    if (rc) return rc;
    hipStream_t s = e->stream;

    // 1. the heads: one fetch
    std::vector<PngSpan> spans(n);
    for (uint32_t i = 0; i < n; i++) spans[i] = {files[i].data, files[i].size};
    std::vector<uint8_t> heads;
    if ((rc = fetch_png_heads(e, spans.data(), n, device_data, heads))) return rc;

    // 2. IHDR, crops, boxes and every destination's pitches and room, of every file, from the heads and the request alone: what
    //    refuses the call refuses it here, before anything of the general tier is launched.  `judged` keeps a file's record for
    //    the general tier, whichever way it gets there
    ViewPlan pre; // (only its per-file calls are used: nothing becomes a job)
    pre.begin(rq, n, elem);
    std::vector<TierFile> judged(n);
    std::vector<int32_t> ihdr_status(n, (int32_t)fpng::FPNG_DECODE_INVALID_ARG);
    std::vector<uint32_t> ihdr_chans(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        if (!files[i].data || !files[i].size) continue;
        TierFile &g = judged[i];
        g.file = i, g.data = files[i].data, g.size = files[i].size;
        uint32_t st = pngi::check_ihdr(heads.data() + (size_t)i * kPngHead, files[i].size, g.w, g.h, g.color, g.bpp, ihdr_chans[i]);
        if (!st && (uint64_t)g.w * g.h * files[i].num_chans > UINT32_MAX) st = fpng::FPNG_DECODE_FAILED_DIMENSIONS_TOO_LARGE;
        for (uint32_t v = pre.first_view(i), end = v + pre.views_of(i); !st && v < end; v++) { // (the crop rule of the views calls: dec_crop_tiles)
            const fpng_amd_crop &c = rq.crops[v];
            if ((uint64_t)c.x + c.w > g.w || (uint64_t)c.y + c.h > g.h) st = FPNG_AMD_DECODE_PNG_CROP_OUTSIDE;
        }
        ihdr_status[i] = (int32_t)st;
        if (st) continue; // (not decoded: needs no room)
        const DecCrop box = pre.file_box(i);
        g.box = {box.x, box.y, box.w, box.h};
        const fpng_amd_png plain = {files[i].data, files[i].size, 0, nullptr, 0};
        if (const Refusal no = pre.file_records(i, plain, files[i], files[i].num_chans, box, 0)) return fail(no.code, no.why);
        g.scan_bytes = ((uint64_t)g.box.y + g.box.h) * (1 + (uint64_t)g.w * g.bpp);
        // (its share of the plan's device scratch, at most: the box's planes, the post views' windows, the tone views' histograms and tables)
        g.share = align256((((size_t)g.box.w * g.box.h * 4 + 15) & ~(size_t)15) + 256);
        for (uint32_t v = pre.first_view(i), end = v + pre.views_of(i); v < end; v++)
            if (pre.is_post_view(v)) {
                g.share += (((size_t)rq.views[v].w * rq.views[v].h * files[i].num_chans + 15) & ~(size_t)15);
                if (rq.tones && rq.tones[v].op) g.share += kToneBytes;
            }
    }

    // 3. routing: fpng's files through the existing views path with their part of the request; what it leaves comes to the general
    //    tier.  Everything has been judged above, whichever way a file gets there
    std::vector<TierFile> general;
    auto to_general = [&](uint32_t i, bool) -> int {
        fpng_amd_decode_result &r = results[i];
        r.w = judged[i].w, r.h = judged[i].h, r.channels_in_file = ihdr_chans[i], r.status = ihdr_status[i];
        if (!r.status) general.push_back(judged[i]);
        return FPNG_AMD_OK;
    };
    auto run_fast = [&](const std::vector<uint32_t> &fast, std::vector<fpng_amd_decode_result> &sub_res) -> int {
        GatheredPngViews sub;
        sub.gather(*rq_in, n, fast.data(), (uint32_t)fast.size());
        std::vector<fpng_amd_png_planar> sub_files(fast.size());
        for (size_t k = 0; k < fast.size(); k++) sub_files[k] = files[fast[k]];
        if (int rc = decode_files_views(e, sub_files.data(), (uint32_t)sub_files.size(), sub_res.data(), device_data, as_request(sub.rq))) return rc;
        for (fpng_amd_decode_result &r : sub_res) // (67 is UNSUPPORTED_PNG in this call)
            if (r.status == FPNG_AMD_DECODE_CROP_OUTSIDE) r.status = FPNG_AMD_DECODE_PNG_CROP_OUTSIDE;
        return FPNG_AMD_OK;
    };
    if ((rc = route_png_files(spans.data(), n, heads.data(), flags & FPNG_AMD_PNG_GENERAL_ONLY, results, to_general, run_fast))) return rc;
    if (general.empty()) return FPNG_AMD_OK;

    // 4. groups of files whose kept scanlines, bytes (host-resident files) and share of the plan's scratch fit the limit
    const std::vector<TierGroup> groups = png_groups(general, !device_data);
    if ((rc = begin_png_groups(e, true))) return rc;

    // 5. per group
    TierUpload up;
    std::vector<pngi::State> states;
    std::vector<pngi::Box> boxes;
    std::vector<uint8_t> good;
    std::vector<uint32_t> chans, planes_of;
    std::vector<int32_t> job_of;
    std::vector<size_t> out_ofs;
    for (const TierGroup &g : groups) {
        const size_t m = g.g1 - g.g0;
        const bool stamp = e->profiling && &g == &groups[0];
        // the scratch: records, states, boxes, bytes, scanlines, then the plan's.  The plan is built twice: now with every file as a
        // 4-channel one, which needs the most, for the room -- the buffer must not move once the scanlines are in it -- and
        // behind the inflate kernel with the files that are good and the channels they have
        const TierLayout at = png_group_layout(m, g, true);
        const size_t o_plan = at.end;
        chans.assign(m, 4);
        Carver room = {o_plan};
        {
            ViewPlan most;
            if ((rc = build_plan(most, rq, n, elem, files, general, g.g0, g.g1, nullptr, chans.data(), job_of, out_ofs, planes_of))) return rc;
            most.carve_records(room), most.carve_scratch(room);
        }
        // a. records (and, host-resident files, their bytes) up
        if ((rc = upload_group(e, &general[g.g0], m, at, room.need, !device_data, 0, up))) return rc;
        uint8_t *base = e->d_decode.p;
        pngi::File *d_recs = (pngi::File *)(base + at.recs);
        pngi::State *d_states = (pngi::State *)(base + at.states);
        pngi::Box *d_boxes = (pngi::Box *)(base + at.boxes);
        // b. inflate; c. the states back: which files are good so far, and which have an alpha plane
        if (stamp) HIP_TRY(hipEventRecord(e->png_ev[0], s));
        launch_png_inflate(s, d_recs, d_states, (uint32_t)m);
        HIP_TRY(hipGetLastError());
        if (stamp) HIP_TRY(hipEventRecord(e->png_ev[1], s));
        states.resize(m);
        HIP_TRY(hipMemcpyAsync(states.data(), d_states, m * sizeof(pngi::State), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        good.assign(m, 0);
        for (size_t k = 0; k < m; k++) good[k] = states[k].status == 0, chans[k] = has_alpha_plane(general[g.g0 + k].color, states[k].trns_len) ? 4u : 3u;
        // d. the group's plan, a fresh one, in the room sized above; e. its set-up block and the boxes up
        ViewPlan plan;
        if ((rc = build_plan(plan, rq, n, elem, files, general, g.g0, g.g1, good.data(), chans.data(), job_of, out_ofs, planes_of))) return rc;
        const uint32_t jobs = (uint32_t)(plan.job_rec.empty() ? 0 : plan.job_rec.size() - 1);
        if (jobs) {
            Carver sc = {o_plan};
            plan.carve_records(sc);
            const size_t setup_len = sc.need - o_plan;
            plan.carve_scratch(sc);
            if (sc.need > e->d_decode.cap) return fail(FPNG_AMD_ERR_UNSUPPORTED, "png views: the group's plan outgrew its room");
            plan.place(base);
            if ((rc = e->h_dec_fetch.ensure(setup_len + m * sizeof(pngi::Box)))) return rc;
            uint8_t *const h_setup = e->h_dec_fetch.p;
            std::memset(h_setup, 0, setup_len);
            plan.write_setup(h_setup, o_plan);
            boxes.assign(m, pngi::Box());
            for (size_t k = 0; k < m; k++)
                if (job_of[k] >= 0) {
                    const fpng_amd_crop &b = general[g.g0 + k].box;
                    boxes[k] = {plan.d_mid + out_ofs[k], b.x, b.y, b.w, b.h, planes_of[k], 0};
                }
            std::memcpy(h_setup + setup_len, boxes.data(), m * sizeof(pngi::Box));
            HIP_TRY(hipMemcpyAsync(base + o_plan, h_setup, setup_len, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_boxes, h_setup + setup_len, m * sizeof(pngi::Box), hipMemcpyHostToDevice, s));
            // f. the box kernel (files whose status is not 0 return at once); g. the states back
            if (stamp) HIP_TRY(hipEventRecord(e->png_ev[3], s));
            launch_png_unfilter_box(s, d_recs, d_states, d_boxes, (uint32_t)m);
            HIP_TRY(hipGetLastError());
            if (stamp) HIP_TRY(hipEventRecord(e->png_ev[2], s));
            HIP_TRY(hipMemcpyAsync(states.data(), d_states, m * sizeof(pngi::State), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (stamp) e->png_ev_recorded = true;
            // h. the views of the files that are still good: the plan's launches over each run of consecutive jobs
            for (size_t k = 0; k < m;) {
                if (job_of[k] < 0 || states[k].status) {
                    k++;
                    continue;
                }
                const uint32_t j0 = (uint32_t)job_of[k];
                uint32_t j1 = j0;
                for (; k < m && (job_of[k] < 0 || !states[k].status); k++) // (files without a job lie between jobs, not inside one)
                    if (job_of[k] >= 0) j1 = (uint32_t)job_of[k] + 1;
                if ((rc = plan.enqueue(s, j0, j1, rq.fmt ? &flt : nullptr))) return rc;
            }
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(s)); // (the next group reuses the scratch and the pinned block)
        } else if (stamp) { // (no file of the first group reached the box kernel)
            HIP_TRY(hipEventRecord(e->png_ev[3], s));
            HIP_TRY(hipEventRecord(e->png_ev[2], s));
            e->png_ev_recorded = true;
        }
        for (size_t k = 0; k < m; k++) fold_state(results[general[g.g0 + k].file], general[g.g0 + k], states[k]);
    }
    return FPNG_AMD_OK;
}

} // namespace

extern "C" int fpng_amd_decode_batch_png_views(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const fpng_amd_png_views *rq, fpng_amd_decode_result *results)
{
    return png_views(e, files, n, rq, results, false);
}

extern "C" int fpng_amd_decode_batch_device_png_views(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const fpng_amd_png_views *rq, fpng_amd_decode_result *results)
{
    return png_views(e, files, n, rq, results, true);
}
