// png_tier_plan.h -- the general decode tier's host rules that need neither the encoder nor the device: what counts as an fpng file,
// the scratch limit, the groups, a group's layout in the scratch, the kernels' file records, a state's fold into a result.  The png
// calls (png_decode_api.cpp) and the png_views calls (png_views_api.cpp) both go by it; png_tier.h has the part that needs the
// stream.  Host-only and free of HIP: tests/cpp/png_tier_plan_host.cpp builds it alone.
#pragma once
#include "fpng_amd.h"
#include "png_inflate_core.h"

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace fpng_amd {

static_assert(sizeof(pngi::File) == 64 && sizeof(pngi::State) == 32 && sizeof(pngi::Box) == 32, "the kernels' records");

constexpr uint32_t kPngHead = 64; // bytes of a device-resident file that come back: signature, IHDR, the next chunk's length and type

// fpng's own files: 8-bit RGB / RGBA with the marker chunk right behind the IHDR (where every fpng encoder puts it)
inline bool looks_fpng(const uint8_t *head, uint32_t size)
{
    static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    if (size < 58 || memcmp(head, sig, 8) != 0 || pngi::be32(head + 8) != 13) return false;
    if (head[24] != 8 || (head[25] != 2 && head[25] != 6)) return false;
    return pngi::be32(head + 33) == 5 && memcmp(head + 37, "fdEC", 4) == 0;
}

inline size_t scratch_limit() // FPNG_AMD_PNG_SCRATCH_LIMIT, read at every call
{
    if (const char *v = getenv("FPNG_AMD_PNG_SCRATCH_LIMIT")) {
        const long long n = atoll(v);
        if (n > 0) return (size_t)n;
    }
    return (size_t)1 << 30;
}
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// a file of the general tier: what its head and the call say of it
struct TierFile {
    uint32_t file;       // its index in the call
    uint32_t w, h, color, bpp;
    uint64_t scan_bytes; // the rows kept: h * (1 + w * bpp), or the (box.y + box.h) rows that a views call's box needs
    fpng_amd_crop box;   // the views calls: what is decoded of it, the ONE box of its views
    size_t share;        // the views calls: of the plan's device scratch, at most; the png calls: 0
    const void *data;    // the file as the caller gave it
    uint32_t size;
    uint8_t *out;        // the png calls: its pixels; the views calls: NULL
};
// files g0 .. g1 - 1 of the tier run together; scan, bytes: their scanlines and (upload) their bytes, each file's rounded up to 256
struct TierGroup {
    size_t g0, g1, scan, bytes;
};
// THE grouping rule.  A file counts align256(scan_bytes) + its share + (upload: host-resident files, whose bytes are staged and
// uploaded per group) align256(size); it joins the group while the sum stays at or under the limit, and a file that alone exceeds
// the limit is a group of its own.  limit: FPNG_AMD_PNG_SCRATCH_LIMIT's, unless a test says otherwise
inline std::vector<TierGroup> png_groups(const std::vector<TierFile> &tier, bool upload, size_t limit = scratch_limit())
{
    std::vector<TierGroup> groups;
    for (size_t k = 0; k < tier.size();) {
        TierGroup g = {k, k, 0, 0};
        size_t share = 0;
        for (; g.g1 < tier.size(); g.g1++) {
            const TierFile &q = tier[g.g1];
            const size_t scan = align256(q.scan_bytes), bytes = upload ? align256(q.size) : 0;
            if (g.g1 != g.g0 && g.scan + g.bytes + share + scan + bytes + q.share > limit) break;
            g.scan += scan, g.bytes += bytes, share += q.share;
        }
        groups.push_back(g);
        k = g.g1;
    }
    return groups;
}

// A group of m files in the scratch, as offsets: records, states, (the views calls' boxes,) the uploaded bytes, the scanlines, each
// on a 256-byte boundary.  end: the first free byte -- what the png calls need, and where the views calls' plan begins
struct TierLayout {
    size_t recs, states, boxes, bytes, scan, end;
};
inline TierLayout png_group_layout(size_t m, const TierGroup &g, bool with_boxes)
{
    const size_t states = align256(m * sizeof(pngi::File)), boxes = states + align256(m * sizeof(pngi::State));
    const size_t bytes = boxes + (with_boxes ? align256(m * sizeof(pngi::Box)) : 0);
    return {0, states, boxes, bytes, bytes + g.bytes, bytes + g.bytes + g.scan};
}

// a host-to-device copy that the caller of fill_records makes: size bytes from src to the scratch's byte ofs
struct TierCopy {
    const void *src;
    size_t ofs, size;
};
// The kernels' records of the m files at `tier`, a group placed at `at` in the scratch at `base`.  dst_c: 3 or 4, the png calls --
// pixels to TierFile::out, every row kept; 0, the views calls -- no pixels, and the stream must still yield the whole image's rows.
// upload: the files' bytes go to the scratch (copies says from where to where: straight from the caller's memory, which stays as
// it is until the call returns, no second copy on the host); else they are read where they are
inline void fill_records(const TierFile *tier, size_t m, const TierLayout &at, uint8_t *base, bool upload, uint32_t dst_c, pngi::File *recs, std::vector<TierCopy> &copies)
{
    copies.clear();
    size_t at_bytes = at.bytes, at_scan = at.scan;
    for (size_t k = 0; k < m; k++) {
        const TierFile &q = tier[k];
        pngi::File &r = recs[k];
        r = pngi::File();
        if (upload) copies.push_back({q.data, at_bytes, q.size}), r.data = base + at_bytes, at_bytes += align256(q.size);
        else r.data = (const uint8_t *)q.data;
        r.scan = base + at_scan, at_scan += align256(q.scan_bytes);
        r.out = dst_c ? q.out : nullptr, r.scan_bytes = q.scan_bytes, r.size = q.size;
        r.need_bytes = dst_c ? 0 : (uint64_t)q.h * (1 + (uint64_t)q.w * q.bpp);
        r.w = q.w, r.h = q.h, r.color = q.color, r.bpp = q.bpp, r.dst_c = dst_c;
    }
}

// a file's result once its kernels have run: the status, and a palette file with a tRNS chunk has four channels
inline void fold_state(fpng_amd_decode_result &r, const TierFile &q, const pngi::State &st)
{
    r.status = (int32_t)st.status;
    if (q.color == 3 && st.trns_len && st.status != pngi::kBadChunk && st.status != pngi::kUnsupported) r.channels_in_file = 4;
}

} // namespace fpng_amd
