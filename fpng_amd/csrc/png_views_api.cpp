// png_views_api.cpp -- fpng_amd_decode_batch(_device)_png_views: views of ordinary PNG files.  The request is judged as the views
// call of its family judges it (view_request.h), the files are routed as fpng_amd_decode_batch(_device)_png routes them
// (png_decode_api.cpp) -- fpng-written ones through the existing views path, with their part of the request -- and the general
// tier's files run in groups: inflate (only the rows that the file's box needs are kept), the states back, a ViewPlan of the
// group's good files with their real channel counts, png_unfilter_box_kernel into the plan's planes, the states back, and the
// plan's own launches.  Everything that can refuse the CALL is judged from the heads and the request before the first kernel of
// the general tier runs.
#include "decode.h"
#include "encoder.h"
#include "png_decode.h"
#include "png_views_gather.h"
#include "view_request.h"

#include "fpng.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace fpng_amd;

namespace {

static_assert(sizeof(fpng_amd_png_views) == 112 && offsetof(fpng_amd_png_views, colors) == 48 && offsetof(fpng_amd_png_views, flags) == 104, "fpng_amd_png_views layout");
static_assert(sizeof(pngi::Box) == 32, "the box kernel's record");
static_assert(FPNG_AMD_DECODE_PNG_CROP_OUTSIDE == 68 && FPNG_AMD_DECODE_CROP_OUTSIDE == 67 && FPNG_AMD_DECODE_UNSUPPORTED_PNG == 67, "67 means UNSUPPORTED_PNG here");

constexpr uint32_t kPngHead = 64; // (png_decode_api.cpp: what comes back of a device-resident file)
constexpr size_t kDefaultScratchLimit = (size_t)1 << 30;

bool looks_fpng(const uint8_t *head, uint32_t size)
{
    static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    if (size < 58 || memcmp(head, sig, 8) != 0 || pngi::be32(head + 8) != 13) return false;
    if (head[24] != 8 || (head[25] != 2 && head[25] != 6)) return false;
    return pngi::be32(head + 33) == 5 && memcmp(head + 37, "fdEC", 4) == 0;
}

size_t scratch_limit()
{
    if (const char *v = getenv("FPNG_AMD_PNG_SCRATCH_LIMIT")) {
        const long long n = atoll(v);
        if (n > 0) return (size_t)n;
    }
    return kDefaultScratchLimit;
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

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

// the files' and the destinations' own words, as the planar family judges them behind the encoder (decode_api.cpp: decode_files_planar)
int check_planar_words(const fpng_amd_png_planar *files, uint32_t n, const ViewRequest &rq, uint64_t n_views, DecFloat &flt, uint32_t &elem)
{
    flt = {}, elem = 1;
    if (const fpng_amd_float_format *fmt = rq.fmt) {
        if (fmt->dtype >= kDecFloatTypes) return fail(FPNG_AMD_ERR_INVALID_ARG, "unknown element type (FPNG_AMD_F32, _F16, _BF16)");
        if (fmt->reserved) return fail(FPNG_AMD_ERR_INVALID_ARG, "fpng_amd_float_format::reserved must be 0");
        for (int c = 0; c < 4; c++)
            if (!std::isfinite(fmt->scale[c]) || !std::isfinite(fmt->bias[c])) return fail(FPNG_AMD_ERR_INVALID_ARG, "scale and bias must be finite");
        flt.dtype = fmt->dtype, elem = dec_float_bytes(fmt->dtype);
        std::memcpy(flt.scale, fmt->scale, sizeof flt.scale), std::memcpy(flt.bias, fmt->bias, sizeof flt.bias);
    }
    for (uint32_t i = 0; i < n; i++)
        if (files[i].num_chans != 3 && files[i].num_chans != 4) return fail(FPNG_AMD_ERR_INVALID_ARG, "num_chans must be 3 or 4");
    for (uint64_t v = 0; rq.hwc && v < n_views; v++) {
        const fpng_amd_view_dest_hwc &x = rq.hwc[v];
        if (((uintptr_t)x.d_pixels | (uint64_t)x.row_pitch) & (elem - 1)) return fail(FPNG_AMD_ERR_INVALID_ARG, "d_pixels and row_pitch must be multiples of the element size");
        if (x.row_pitch <= -(int64_t)0x80000000ll || x.row_pitch >= (int64_t)0x80000000ll) return fail(FPNG_AMD_ERR_INVALID_ARG, "|row_pitch| >= 2^31");
    }
    for (uint64_t v = 0; rq.dests && v < n_views; v++) {
        const fpng_amd_view_dest &x = rq.dests[v];
        if (((uintptr_t)x.d_pixels | (uint64_t)x.row_pitch | (uint64_t)x.plane_pitch) & (elem - 1))
            return fail(FPNG_AMD_ERR_INVALID_ARG, "d_pixels, row_pitch and plane_pitch must be multiples of the element size");
        if (x.row_pitch <= -(int64_t)0x80000000ll || x.row_pitch >= (int64_t)0x80000000ll) return fail(FPNG_AMD_ERR_INVALID_ARG, "|row_pitch| >= 2^31");
    }
    return FPNG_AMD_OK;
}

// does decode_device_png at 4 channels give this file an alpha that can be below 255?  (the plan's 4-channel files)
bool has_alpha_plane(uint32_t color, uint32_t trns_len) { return color == 4 || color == 6 || (color == 3 && trns_len) || (color == 0 && trns_len >= 2) || (color == 2 && trns_len >= 6); }

struct General { // a file of the general tier
    uint32_t file;
    uint32_t w, h, color, bpp;
    DecCrop box;         // what is decoded of it: the ONE box of its views
    uint64_t scan_bytes; // the rows kept: (box.y + box.h) * (1 + w * bpp)
    size_t share;        // of the plan's device scratch, at most: the box's planes, the post views' windows, the tone views' histograms and tables
};

// The plan of files g0 .. g1 - 1 of `general`: those whose `good` entry is set (NULL: all), with chans[k - g0] channels.  The
// destinations have been judged: a refusal here is the same one.  job_of: per file its job, or -1
int build_plan(ViewPlan &plan, const ViewRequest &rq, uint32_t n, uint32_t elem, const fpng_amd_png_planar *files, const std::vector<General> &general, size_t g0, size_t g1,
               const uint8_t *good, const uint32_t *chans, std::vector<int32_t> &job_of, std::vector<size_t> &out_ofs, std::vector<uint32_t> &planes_of)
{
    plan.begin(rq, n, elem);
    job_of.assign(g1 - g0, -1), out_ofs.assign(g1 - g0, 0), planes_of.assign(g1 - g0, 0);
    int32_t jobs = 0;
    for (size_t k = g0; k < g1; k++) {
        if (good && !good[k - g0]) continue;
        const General &q = general[k];
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
    DecFloat flt;
    uint32_t elem;
    if (int rc = check_planar_words(files, n, asked, used.total, flt, elem)) return rc;
    ViewDefaults made;
    const ViewRequest rq = normalise_views(asked, used, made);
    const uint32_t flags = rq_in->flags;
    std::memset(results, 0, (size_t)n * sizeof *results);
    HIP_TRY(hipSetDevice(e->device));
    int rc = drain(e);
    if (rc) return rc;
    hipStream_t s = e->stream;

    // 1. the heads: one fetch
    std::vector<uint8_t> heads((size_t)n * kPngHead, 0);
    if (device_data) {
        const size_t o_refs = align256((size_t)n * kPngHead), total = o_refs + (size_t)n * sizeof(DecFileRef);
        if ((rc = e->h_dec_fetch.ensure(total)) || (rc = e->d_decode.ensure(total))) return rc;
        DecFileRef *h_refs = (DecFileRef *)(e->h_dec_fetch.p + o_refs);
        for (uint32_t i = 0; i < n; i++) h_refs[i] = {(const uint8_t *)files[i].data, files[i].data ? files[i].size : 0u, 0};
        uint8_t *d_refs = e->d_decode.p + o_refs;
        HIP_TRY(hipMemcpyAsync(d_refs, h_refs, (size_t)n * sizeof(DecFileRef), hipMemcpyHostToDevice, s));
        launch_dec_fetch(s, (const DecFileRef *)d_refs, n, kPngHead, 0, e->d_decode.p);
        HIP_TRY(hipMemcpyAsync(e->h_dec_fetch.p, e->d_decode.p, (size_t)n * kPngHead, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::memcpy(heads.data(), e->h_dec_fetch.p, heads.size());
        for (uint32_t i = 0; i < n; i++) // (the fetch leaves what lies behind a short file's end as it was)
            if (files[i].size < kPngHead) std::memset(heads.data() + (size_t)i * kPngHead + files[i].size, 0, kPngHead - files[i].size);
    } else
        for (uint32_t i = 0; i < n; i++)
            if (files[i].data) std::memcpy(heads.data() + (size_t)i * kPngHead, files[i].data, std::min(files[i].size, kPngHead));

    // 2. IHDR, crops, boxes and every destination's pitches and room, of every file, from the heads and the request alone: what
    //    refuses the call refuses it here, before anything of the general tier is launched.  `judged` keeps a file's record for
    //    the general tier, whichever way it gets there
    ViewPlan pre; // (only its per-file calls are used: nothing becomes a job)
    pre.begin(rq, n, elem);
    std::vector<General> judged(n);
    std::vector<int32_t> ihdr_status(n, (int32_t)fpng::FPNG_DECODE_INVALID_ARG);
    std::vector<uint32_t> ihdr_chans(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        if (!files[i].data || !files[i].size) continue;
        General &g = judged[i];
        g = {i, 0, 0, 0, 0, {0, 0, 0, 0}, 0, 0};
        uint32_t st = pngi::check_ihdr(heads.data() + (size_t)i * kPngHead, files[i].size, g.w, g.h, g.color, g.bpp, ihdr_chans[i]);
        if (!st && (uint64_t)g.w * g.h * files[i].num_chans > UINT32_MAX) st = fpng::FPNG_DECODE_FAILED_DIMENSIONS_TOO_LARGE;
        for (uint32_t v = pre.first_view(i), end = v + pre.views_of(i); !st && v < end; v++) { // (the crop rule of the views calls: dec_crop_tiles)
            const fpng_amd_crop &c = rq.crops[v];
            if ((uint64_t)c.x + c.w > g.w || (uint64_t)c.y + c.h > g.h) st = FPNG_AMD_DECODE_PNG_CROP_OUTSIDE;
        }
        ihdr_status[i] = (int32_t)st;
        if (st) continue; // (not decoded: needs no room)
        g.box = pre.file_box(i);
        const fpng_amd_png plain = {files[i].data, files[i].size, 0, nullptr, 0};
        if (const Refusal no = pre.file_records(i, plain, files[i], files[i].num_chans, g.box, 0)) return fail(no.code, no.why);
        g.scan_bytes = ((uint64_t)g.box.y + g.box.h) * (1 + (uint64_t)g.w * g.bpp);
        g.share = align256((((size_t)g.box.w * g.box.h * 4 + 15) & ~(size_t)15) + 256);
        for (uint32_t v = pre.first_view(i), end = v + pre.views_of(i); v < end; v++)
            if (pre.is_post_view(v)) {
                g.share += (((size_t)rq.views[v].w * rq.views[v].h * files[i].num_chans + 15) & ~(size_t)15);
                if (rq.tones && rq.tones[v].op) g.share += kToneBytes;
            }
    }

    // 3. routing: fpng's files through the existing views path with their part of the request; what it leaves comes to the general tier
    std::vector<uint32_t> fast;
    std::vector<General> general;
    auto to_general = [&](uint32_t i) {
        fpng_amd_decode_result &r = results[i];
        r.w = judged[i].w, r.h = judged[i].h, r.channels_in_file = ihdr_chans[i], r.status = ihdr_status[i];
        if (!r.status) general.push_back(judged[i]);
    };
    for (uint32_t i = 0; i < n; i++) {
        if (!files[i].data || !files[i].size) results[i].status = fpng::FPNG_DECODE_INVALID_ARG;
        else if (!(flags & FPNG_AMD_PNG_GENERAL_ONLY) && looks_fpng(heads.data() + (size_t)i * kPngHead, files[i].size)) fast.push_back(i);
        else to_general(i);
    }
    if (!fast.empty()) {
        GatheredPngViews sub;
        sub.gather(*rq_in, n, fast.data(), (uint32_t)fast.size());
        std::vector<fpng_amd_png_planar> sub_files(fast.size());
        std::vector<fpng_amd_decode_result> sub_res(fast.size());
        for (size_t k = 0; k < fast.size(); k++) sub_files[k] = files[fast[k]];
        if ((rc = decode_files_views(e, sub_files.data(), (uint32_t)sub_files.size(), sub_res.data(), device_data, as_request(sub.rq)))) return rc;
        for (size_t k = 0; k < fast.size(); k++) {
            results[fast[k]] = sub_res[k];
            if (sub_res[k].status == FPNG_AMD_DECODE_CROP_OUTSIDE) results[fast[k]].status = FPNG_AMD_DECODE_PNG_CROP_OUTSIDE;
            if (sub_res[k].status == fpng::FPNG_DECODE_NOT_FPNG || sub_res[k].status == FPNG_AMD_DECODE_UNDECIDED) to_general(fast[k]);
        }
    }
    if (general.empty()) return FPNG_AMD_OK;

    // 4. groups of files whose kept scanlines, bytes (host-resident files) and share of the plan's scratch fit the limit
    const size_t limit = scratch_limit();
    struct Group {
        size_t g0, g1, scan, bytes;
    };
    std::vector<Group> groups;
    for (size_t k = 0; k < general.size();) {
        Group g = {k, k, 0, 0};
        size_t share = 0;
        for (; g.g1 < general.size(); g.g1++) {
            const size_t scan = align256(general[g.g1].scan_bytes), bytes = device_data ? 0 : align256(files[general[g.g1].file].size);
            if (g.g1 != g.g0 && g.scan + g.bytes + share + scan + bytes + general[g.g1].share > limit) break;
            g.scan += scan, g.bytes += bytes, share += general[g.g1].share;
        }
        groups.push_back(g);
        k = g.g1;
    }
    const bool prof = e->profiling;
    e->png_ev_recorded = false, e->png_ev_split = true;
    if (prof)
        for (hipEvent_t &ev : e->png_ev)
            if (!ev) HIP_TRY(hipEventCreate(&ev));

    // 5. per group
    std::vector<pngi::File> recs;
    std::vector<pngi::State> states;
    std::vector<pngi::Box> boxes;
    std::vector<uint8_t> good;
    std::vector<uint32_t> chans, planes_of;
    std::vector<int32_t> job_of;
    std::vector<size_t> out_ofs;
    for (const Group &g : groups) {
        const size_t m = g.g1 - g.g0;
        const bool stamp = prof && &g == &groups[0];
        // the scratch: records, states, boxes, bytes, scanlines, then the plan's.  The plan is built twice: now with every file as a
        // 4-channel one, which needs the most, for the room -- the buffer must not move once the scanlines are in it -- and
        // behind the inflate kernel with the files that are good and the channels they have
        const size_t o_states = align256(m * sizeof(pngi::File)), o_boxes = o_states + align256(m * sizeof(pngi::State)), o_bytes = o_boxes + align256(m * sizeof(pngi::Box)),
                     o_scan = o_bytes + g.bytes, o_plan = o_scan + g.scan;
        chans.assign(m, 4);
        {
            ViewPlan most;
            if ((rc = build_plan(most, rq, n, elem, files, general, g.g0, g.g1, nullptr, chans.data(), job_of, out_ofs, planes_of))) return rc;
            Carver sc = {o_plan};
            most.carve_records(sc), most.carve_scratch(sc);
            if ((rc = e->d_decode.ensure(sc.need))) return rc;
        }
        uint8_t *base = e->d_decode.p;
        pngi::File *d_recs = (pngi::File *)base;
        pngi::State *d_states = (pngi::State *)(base + o_states);
        pngi::Box *d_boxes = (pngi::Box *)(base + o_boxes);
        uint8_t *d_bytes = base + o_bytes, *d_scan = base + o_scan;
        // a. records (and, host-resident files, their bytes) up
        recs.assign(m, pngi::File());
        size_t at_bytes = 0, at_scan = 0;
        for (size_t k = 0; k < m; k++) {
            const General &q = general[g.g0 + k];
            const fpng_amd_png_planar &f = files[q.file];
            pngi::File &r = recs[k];
            if (device_data) r.data = (const uint8_t *)f.data;
            else {
                HIP_TRY(hipMemcpyAsync(d_bytes + at_bytes, f.data, f.size, hipMemcpyHostToDevice, s));
                r.data = d_bytes + at_bytes, at_bytes += align256(f.size);
            }
            r.scan = d_scan + at_scan, at_scan += align256(q.scan_bytes);
            r.out = nullptr, r.scan_bytes = q.scan_bytes, r.need_bytes = (uint64_t)q.h * (1 + (uint64_t)q.w * q.bpp), r.size = f.size;
            r.w = q.w, r.h = q.h, r.color = q.color, r.bpp = q.bpp, r.dst_c = 0;
        }
        HIP_TRY(hipMemcpyAsync(d_recs, recs.data(), m * sizeof(pngi::File), hipMemcpyHostToDevice, s));
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
                    const DecCrop &b = general[g.g0 + k].box;
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
        for (size_t k = 0; k < m; k++) {
            const General &q = general[g.g0 + k];
            fpng_amd_decode_result &r = results[q.file];
            r.status = (int32_t)states[k].status;
            if (q.color == 3 && states[k].trns_len && states[k].status != pngi::kBadChunk && states[k].status != pngi::kUnsupported) r.channels_in_file = 4;
        }
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
