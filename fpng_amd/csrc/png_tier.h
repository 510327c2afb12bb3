// png_tier.h -- the general decode tier's host path where it needs the encoder and its stream (png_tier.cpp): the heads of a call's
// files, the routing between the fpng path and the tier, the events, a group's way into the scratch.  The rules are png_tier_plan.h's;
// the png and the png_views calls keep what is their own: how a file is judged, what runs the fpng path, the kernels of a group.
#pragma once
#include "png_tier_plan.h"

#include <functional>
#include <vector>

struct fpng_amd_encoder;

namespace fpng_amd {

struct PngSpan { // a file of either call: fpng_amd_png's and fpng_amd_png_planar's data and size
    const void *data;
    uint32_t size;
};

// heads: n * kPngHead bytes, zero behind a file's end (and for a file without data).  device_data: one fetch kernel and one copy back
int fetch_png_heads(fpng_amd_encoder *e, const PngSpan *files, uint32_t n, bool device_data, std::vector<uint8_t> &heads);

// judge(i, undecided): file i is the general tier's -- sets results[i] from its head and, if it is to be decoded, appends it to the
//     tier's files; anything but FPNG_AMD_OK refuses the call.  undecided: the fpng path ran it and left it FPNG_AMD_DECODE_UNDECIDED
// run_fast(fast, sub): the fpng path over files fast[0 ..], their results to sub[0 ..]
using PngJudge = std::function<int(uint32_t i, bool undecided)>;
using PngFastPath = std::function<int(const std::vector<uint32_t> &fast, std::vector<fpng_amd_decode_result> &sub)>;
// Null and empty files get FPNG_DECODE_INVALID_ARG.  Files with fpng's marker (unless general_only) go through run_fast; all others
// are judged at once, in the call's order, and what run_fast leaves NOT_FPNG or UNDECIDED is judged behind them
int route_png_files(const PngSpan *files, uint32_t n, const uint8_t *heads, bool general_only, fpng_amd_decode_result *results, const PngJudge &judge, const PngFastPath &run_fast);

// in front of a call's groups: nothing is recorded yet; split: the host works between the two kernels (fpng_amd_decode_png_last_kernel_ms)
int begin_png_groups(fpng_amd_encoder *e, bool split);

struct TierUpload { // what upload_group fills, kept by the caller across its groups
    std::vector<pngi::File> recs;
    std::vector<TierCopy> copies;
};
// The m files at `tier`, placed at `at`: the scratch grows to `need` bytes (at least at.end; it is not moved again before the group is
// done), the files' bytes go up (upload), then the records in one copy.  dst_c: fill_records'
int upload_group(fpng_amd_encoder *e, const TierFile *tier, size_t m, const TierLayout &at, size_t need, bool upload, uint32_t dst_c, TierUpload &up);

} // namespace fpng_amd
