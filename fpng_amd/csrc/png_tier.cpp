// png_tier.cpp -- the general decode tier's host path behind the png and the png_views calls (png_tier.h): of every file only the head
// is read on the host, files with fpng's marker chunk go through the fpng path as they are, and everything else, and what that path
// leaves, runs in groups that fit the scratch limit (png_tier_plan.h).
#include "png_tier.h"

#include "decode.h"
#include "encoder.h"

#include "fpng.h"

using namespace fpng_amd;

int fpng_amd::fetch_png_heads(fpng_amd_encoder *e, const PngSpan *files, uint32_t n, bool device_data, std::vector<uint8_t> &heads)
{
    heads.assign((size_t)n * kPngHead, 0);
    if (!device_data) {
        for (uint32_t i = 0; i < n; i++)
            if (files[i].data) std::memcpy(heads.data() + (size_t)i * kPngHead, files[i].data, std::min(files[i].size, kPngHead));
        return FPNG_AMD_OK;
    }
    // (heads first, the file references behind them on a 256-byte boundary: the same layout on both sides)
    hipStream_t s = e->stream;
    const size_t o_refs = align256((size_t)n * kPngHead), total = o_refs + (size_t)n * sizeof(DecFileRef);
    int rc;
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
    return FPNG_AMD_OK;
}

int fpng_amd::route_png_files(const PngSpan *files, uint32_t n, const uint8_t *heads, bool general_only, fpng_amd_decode_result *results, const PngJudge &judge, const PngFastPath &run_fast)
{
    int rc;
    std::vector<uint32_t> fast;
    for (uint32_t i = 0; i < n; i++) {
        if (!files[i].data || !files[i].size) results[i].status = fpng::FPNG_DECODE_INVALID_ARG;
        else if (!general_only && looks_fpng(heads + (size_t)i * kPngHead, files[i].size)) fast.push_back(i);
        else if ((rc = judge(i, false)))
            return rc;
    }
    if (fast.empty()) return FPNG_AMD_OK;
    // fpng's files: their path, as it is; what it leaves to others comes to the general tier
    std::vector<fpng_amd_decode_result> sub(fast.size());
    if ((rc = run_fast(fast, sub))) return rc;
    for (size_t k = 0; k < fast.size(); k++) {
        results[fast[k]] = sub[k];
        if (sub[k].status == fpng::FPNG_DECODE_NOT_FPNG || sub[k].status == FPNG_AMD_DECODE_UNDECIDED)
            if ((rc = judge(fast[k], sub[k].status == FPNG_AMD_DECODE_UNDECIDED))) return rc;
    }
    return FPNG_AMD_OK;
}

int fpng_amd::begin_png_groups(fpng_amd_encoder *e, bool split)
{
    e->png_ev_recorded = false, e->png_ev_split = split;
    if (e->profiling)
        for (hipEvent_t &ev : e->png_ev)
            if (!ev) HIP_TRY(hipEventCreate(&ev));
    return FPNG_AMD_OK;
}

int fpng_amd::upload_group(fpng_amd_encoder *e, const TierFile *tier, size_t m, const TierLayout &at, size_t need, bool upload, uint32_t dst_c, TierUpload &up)
{
    if (int rc = e->d_decode.ensure(need)) return rc;
    uint8_t *base = e->d_decode.p;
    up.recs.resize(m);
    fill_records(tier, m, at, base, upload, dst_c, up.recs.data(), up.copies);
    for (const TierCopy &c : up.copies) HIP_TRY(hipMemcpyAsync(base + c.ofs, c.src, c.size, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(base + at.recs, up.recs.data(), m * sizeof(pngi::File), hipMemcpyHostToDevice, e->stream));
    return FPNG_AMD_OK;
}
