// png_decode_api.cpp -- host side of the general decode tier (png_inflate.hip): fpng_amd_decode_batch(_device)_png.  Of every file
// only the head is read here: the IHDR is judged (png_inflate_core.h: check_ihdr) and the file is routed -- files that carry fpng's
// marker chunk behind the IHDR go through fpng_amd_decode_batch(_device) as they are, everything else, and what that path leaves
// (NOT_FPNG, UNDECIDED), goes to the two kernels, in groups whose filtered scanlines fit the scratch limit.
#include "decode.h"
#include "encoder.h"
#include "png_decode.h"

#include "fpng.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace fpng_amd;

namespace {

static_assert(pngi::kNotPng == fpng::FPNG_DECODE_FAILED_NOT_PNG && pngi::kHeaderCrc == fpng::FPNG_DECODE_FAILED_HEADER_CRC32 &&
                  pngi::kBadDims == fpng::FPNG_DECODE_FAILED_INVALID_DIMENSIONS && pngi::kDimsTooLarge == fpng::FPNG_DECODE_FAILED_DIMENSIONS_TOO_LARGE &&
                  pngi::kBadChunk == fpng::FPNG_DECODE_FAILED_CHUNK_PARSING && pngi::kBadIdat == fpng::FPNG_DECODE_FAILED_INVALID_IDAT &&
                  pngi::kUnsupported == FPNG_AMD_DECODE_UNSUPPORTED_PNG,
              "the tier's statuses are the public ones");
static_assert(sizeof(pngi::File) == 64 && sizeof(pngi::State) == 32, "the kernels' records");

constexpr uint32_t kPngHead = 64; // bytes of a device-resident file that come back: signature, IHDR, the next chunk's length and type
constexpr size_t kDefaultScratchLimit = (size_t)1 << 30;

// fpng's own files: 8-bit RGB / RGBA with the marker chunk right behind the IHDR (where every fpng encoder puts it)
bool looks_fpng(const uint8_t *head, uint32_t size)
{
    static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    if (size < 58 || memcmp(head, sig, 8) != 0 || pngi::be32(head + 8) != 13) return false;
    if (head[24] != 8 || (head[25] != 2 && head[25] != 6)) return false;
    return pngi::be32(head + 33) == 5 && memcmp(head + 37, "fdEC", 4) == 0;
}

struct General { // a file of the general tier
    uint32_t file;
    uint32_t w, h, color, bpp;
    uint64_t scan_bytes;
};

size_t scratch_limit()
{
    if (const char *v = getenv("FPNG_AMD_PNG_SCRATCH_LIMIT")) {
        const long long n = atoll(v);
        if (n > 0) return (size_t)n;
    }
    return kDefaultScratchLimit;
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

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
    std::vector<uint8_t> heads((size_t)n * kPngHead, 0);
    if (device_data) {
        // (heads first, the file references behind them on a 256-byte boundary: the same layout on both sides)
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

    // 2. IHDR and routing.  The general tier's files are judged, and their room checked, before anything is launched
    std::vector<uint32_t> fast;
    std::vector<General> general;
    auto judge = [&](uint32_t i, bool checked_room) -> int {
        const fpng_amd_png &f = files[i];
        fpng_amd_decode_result &r = results[i];
        General g = {i, 0, 0, 0, 0, 0};
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
    for (uint32_t i = 0; i < n; i++) {
        if (!files[i].data || !files[i].size) {
            results[i].status = fpng::FPNG_DECODE_INVALID_ARG;
            continue;
        }
        if (!(flags & FPNG_AMD_PNG_GENERAL_ONLY) && looks_fpng(heads.data() + (size_t)i * kPngHead, files[i].size)) fast.push_back(i);
        else if ((rc = judge(i, false)))
            return rc;
    }

    // 3. fpng's files: the batch path, as it is; what it leaves to others comes to the general tier
    if (!fast.empty()) {
        std::vector<fpng_amd_png> sub(fast.size());
        std::vector<fpng_amd_decode_result> sub_res(fast.size());
        for (size_t k = 0; k < fast.size(); k++) sub[k] = files[fast[k]];
        rc = device_data ? fpng_amd_decode_batch_device(e, sub.data(), (uint32_t)sub.size(), desired, sub_res.data())
                         : fpng_amd_decode_batch(e, sub.data(), (uint32_t)sub.size(), desired, sub_res.data());
        if (rc) return rc;
        for (size_t k = 0; k < fast.size(); k++) {
            results[fast[k]] = sub_res[k];
            if (sub_res[k].status == fpng::FPNG_DECODE_NOT_FPNG || sub_res[k].status == FPNG_AMD_DECODE_UNDECIDED)
                if ((rc = judge(fast[k], sub_res[k].status == FPNG_AMD_DECODE_UNDECIDED))) return rc;
        }
    }
    if (general.empty()) return FPNG_AMD_OK;

    // 4. groups of files whose scanlines (and, host-resident files, whose bytes) fit the scratch limit (a file that alone exceeds it is a group of its own)
    const size_t limit = scratch_limit();
    struct Group {
        size_t g0, g1, scan, bytes;
    };
    std::vector<Group> groups;
    size_t need = 0;
    for (size_t k = 0; k < general.size();) {
        Group g = {k, k, 0, 0};
        // (host-resident files: their bytes are staged and uploaded per group, so they count against the limit as well)
        for (; g.g1 < general.size(); g.g1++) {
            const size_t scan = align256(general[g.g1].scan_bytes), bytes = device_data ? 0 : align256(files[general[g.g1].file].size);
            if (g.g1 != g.g0 && g.scan + g.bytes + scan + bytes > limit) break;
            g.scan += scan, g.bytes += bytes;
        }
        const size_t m = g.g1 - g.g0;
        need = std::max(need, align256(m * sizeof(pngi::File)) + align256(m * sizeof(pngi::State)) + g.bytes + g.scan);
        groups.push_back(g);
        k = g.g1;
    }
    if ((rc = e->d_decode.ensure(need))) return rc;
    const bool prof = e->profiling;
    e->png_ev_recorded = false, e->png_ev_split = false;
    if (prof)
        for (hipEvent_t &ev : e->png_ev)
            if (!ev) HIP_TRY(hipEventCreate(&ev));

    // 5. per group: records (and, host-resident files, their bytes) up, the two kernels, the states back
    std::vector<pngi::File> recs;
    std::vector<pngi::State> states;
    for (const Group &g : groups) {
        const size_t m = g.g1 - g.g0;
        uint8_t *base = e->d_decode.p;
        pngi::File *d_recs = (pngi::File *)base;
        pngi::State *d_states = (pngi::State *)(base + align256(m * sizeof(pngi::File)));
        uint8_t *d_bytes = (uint8_t *)d_states + align256(m * sizeof(pngi::State)), *d_scan = d_bytes + g.bytes;
        recs.assign(m, pngi::File());
        size_t at_bytes = 0, at_scan = 0;
        for (size_t k = 0; k < m; k++) {
            const General &q = general[g.g0 + k];
            const fpng_amd_png &f = files[q.file];
            pngi::File &r = recs[k];
            if (device_data) r.data = (const uint8_t *)f.data;
            else {
                // (straight from the caller's memory, which stays as it is until the call returns: no second copy on the host)
                HIP_TRY(hipMemcpyAsync(d_bytes + at_bytes, f.data, f.size, hipMemcpyHostToDevice, s));
                r.data = d_bytes + at_bytes, at_bytes += align256(f.size);
            }
            r.scan = d_scan + at_scan, at_scan += align256(q.scan_bytes);
            r.out = f.d_pixels, r.scan_bytes = q.scan_bytes, r.size = f.size;
            r.w = q.w, r.h = q.h, r.color = q.color, r.bpp = q.bpp, r.dst_c = desired;
        }
        HIP_TRY(hipMemcpyAsync(d_recs, recs.data(), m * sizeof(pngi::File), hipMemcpyHostToDevice, s));
        const bool stamp = prof && &g == &groups[0];
        launch_png_decode(s, d_recs, d_states, (uint32_t)m, stamp ? e->png_ev : nullptr);
        HIP_TRY(hipGetLastError());
        states.resize(m);
        HIP_TRY(hipMemcpyAsync(states.data(), d_states, m * sizeof(pngi::State), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s)); // (the next group reuses the scratch, the vectors above are free again)
        if (stamp) e->png_ev_recorded = true;
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
