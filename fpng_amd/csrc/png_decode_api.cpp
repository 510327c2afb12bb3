// png_decode_api.cpp -- fpng_amd_decode_batch(_device)_png: ordinary PNG files to interleaved pixels.  What is this call's own: its
// argument checks, how it judges a file of the general tier (png_inflate_core.h: check_ihdr, and the room for the pixels), the fpng
// path it sends fpng's files through -- fpng_amd_decode_batch(_device), as they are -- and a group's two kernels (png_inflate.hip).
// The tier's host path -- heads, routing, groups, scratch layout, records, results -- is png_tier.h's and png_tier_plan.h's, which
// fpng_amd_decode_batch(_device)_png_views (png_views_api.cpp) goes by as well.
#include "decode.h"
#include "encoder.h"
#include "png_decode.h"
#include "png_tier.h"

#include "fpng.h"

#include <cstring>
#include <vector>

using namespace fpng_amd;

namespace {

static_assert(pngi::kNotPng == fpng::FPNG_DECODE_FAILED_NOT_PNG && pngi::kHeaderCrc == fpng::FPNG_DECODE_FAILED_HEADER_CRC32 &&
                  pngi::kBadDims == fpng::FPNG_DECODE_FAILED_INVALID_DIMENSIONS && pngi::kDimsTooLarge == fpng::FPNG_DECODE_FAILED_DIMENSIONS_TOO_LARGE &&
                  pngi::kBadChunk == fpng::FPNG_DECODE_FAILED_CHUNK_PARSING && pngi::kBadIdat == fpng::FPNG_DECODE_FAILED_INVALID_IDAT &&
                  pngi::kUnsupported == FPNG_AMD_DECODE_UNSUPPORTED_PNG,
              "the tier's statuses are the public ones");

int decode_png(fpng_amd_encoder *e, const fpng_amd_png *files, uint32_t n, uint32_t desired, uint32_t flags, fpng_amd_decode_result *results, bool device_data)
{
    if (!e || !files || !n || !results) return fail(FPNG_AMD_ERR_INVALID_ARG, "null/empty batch");
    if (desired != 3 && desired != 4) return fail(FPNG_AMD_ERR_INVALID_ARG, "desired_chans must be 3 or 4");
    if (flags & ~FPNG_AMD_PNG_GENERAL_ONLY) return fail(FPNG_AMD_ERR_INVALID_ARG, "unknown flags");
    std::memset(results, 0, (size_t)n * sizeof *results);
    HIP_TRY(hipSetDevice(e->device));
    int rc = drain(e);
    if (rc) return rc;
    hipStream_t s = e->stream;

    // 1. the heads
    std::vector<PngSpan> spans(n);
    for (uint32_t i = 0; i < n; i++) spans[i] = {files[i].data, files[i].size};
    std::vector<uint8_t> heads;
    if ((rc = fetch_png_heads(e, spans.data(), n, device_data, heads))) return rc;

    // 2. IHDR and routing.  The general tier's files are judged, and their room checked, before anything of the tier is launched; a
    //    file that the fpng path left UNDECIDED has had its room checked there
    std::vector<TierFile> general;
    auto judge = [&](uint32_t i, bool checked_room) -> int {
        const fpng_amd_png &f = files[i];
        fpng_amd_decode_result &r = results[i];
        TierFile g = {};
        g.file = i, g.data = f.data, g.size = f.size, g.out = f.d_pixels;
        uint32_t chans = 0;
        const uint32_t st = pngi::check_ihdr(heads.data() + (size_t)i * kPngHead, f.size, g.w, g.h, g.color, g.bpp, chans);
        r.w = g.w, r.h = g.h, r.channels_in_file = chans, r.status = (int32_t)st;
        if (st) return FPNG_AMD_OK;
        const uint64_t need = (uint64_t)g.w * g.h * desired;
        if (need > UINT32_MAX) {
            r.status = fpng::FPNG_DECODE_FAILED_DIMENSIONS_TOO_LARGE;
            return FPNG_AMD_OK;
        }
        if (!checked_room && (!f.d_pixels || f.pixels_cap < need)) return fail(FPNG_AMD_ERR_BUFFER_TOO_SMALL, "d_pixels / pixels_cap < w * h * desired_chans");
        g.scan_bytes = (uint64_t)g.h * (1 + (uint64_t)g.w * g.bpp);
        general.push_back(g);
        return FPNG_AMD_OK;
    };
    auto run_fast = [&](const std::vector<uint32_t> &fast, std::vector<fpng_amd_decode_result> &sub_res) -> int {
        std::vector<fpng_amd_png> sub(fast.size());
        for (size_t k = 0; k < fast.size(); k++) sub[k] = files[fast[k]];
        return device_data ? fpng_amd_decode_batch_device(e, sub.data(), (uint32_t)sub.size(), desired, sub_res.data())
                           : fpng_amd_decode_batch(e, sub.data(), (uint32_t)sub.size(), desired, sub_res.data());
    };
    if ((rc = route_png_files(spans.data(), n, heads.data(), flags & FPNG_AMD_PNG_GENERAL_ONLY, results, judge, run_fast))) return rc;
    if (general.empty()) return FPNG_AMD_OK;

    // 3. the groups, and room for the largest of them
    const std::vector<TierGroup> groups = png_groups(general, !device_data);
    size_t need = 0;
    for (const TierGroup &g : groups) need = std::max(need, png_group_layout(g.g1 - g.g0, g, false).end);
    if ((rc = e->d_decode.ensure(need)) || (rc = begin_png_groups(e, false))) return rc;

    // 4. per group: records (and, host-resident files, their bytes) up, the two kernels, the states back
    TierUpload up;
    std::vector<pngi::State> states;
    for (const TierGroup &g : groups) {
        const size_t m = g.g1 - g.g0;
        const TierLayout at = png_group_layout(m, g, false);
        if ((rc = upload_group(e, &general[g.g0], m, at, at.end, !device_data, desired, up))) return rc;
        pngi::State *d_states = (pngi::State *)(e->d_decode.p + at.states);
        const bool stamp = e->profiling && &g == &groups[0];
        launch_png_decode(s, (const pngi::File *)(e->d_decode.p + at.recs), d_states, (uint32_t)m, stamp ? e->png_ev : nullptr);
        HIP_TRY(hipGetLastError());
        states.resize(m);
        HIP_TRY(hipMemcpyAsync(states.data(), d_states, m * sizeof(pngi::State), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s)); // (the next group reuses the scratch, the vectors above are free again)
        if (stamp) e->png_ev_recorded = true;
        for (size_t k = 0; k < m; k++) fold_state(results[general[g.g0 + k].file], general[g.g0 + k], states[k]);
    }
    return FPNG_AMD_OK;
}

} // namespace

extern "C" int fpng_amd_decode_batch_png(fpng_amd_encoder *e, const fpng_amd_png *files, uint32_t n, uint32_t desired, uint32_t flags, fpng_amd_decode_result *results)
{
    return decode_png(e, files, n, desired, flags, results, false);
}

extern "C" int fpng_amd_decode_batch_device_png(fpng_amd_encoder *e, const fpng_amd_png *files, uint32_t n, uint32_t desired, uint32_t flags, fpng_amd_decode_result *results)
{
    return decode_png(e, files, n, desired, flags, results, true);
}

extern "C" int fpng_amd_decode_png_last_kernel_ms(fpng_amd_encoder *e, float ms[2])
{
    if (!e || !ms) return fail(FPNG_AMD_ERR_INVALID_ARG, "null argument");
    ms[0] = ms[1] = 0.f;
    if (!e->png_ev_recorded) return FPNG_AMD_OK;
    HIP_TRY(hipEventSynchronize(e->png_ev[2]));
    HIP_TRY(hipEventElapsedTime(&ms[0], e->png_ev[0], e->png_ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms[1], e->png_ev[e->png_ev_split ? 3 : 1], e->png_ev[2]));
    return FPNG_AMD_OK;
}
