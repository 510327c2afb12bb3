// png_tier_plan_host.cpp -- fpng_amd/csrc/png_tier_plan.h alone: the grouping rule against a restatement of it written here, the
// scratch layout against the formulas of the two calls written out as numbers, the file records of a group in a heap block of
// exactly the layout's size (so that the address sanitizer sees a record that points outside), what counts as an fpng file, and
// the fold of a file's state into its result.  Prints "ok" and exits 0, or says what differs.
#include "png_tier_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

using namespace fpng_amd;

static int bad = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) printf("line %d: %s\n", __LINE__, #cond), bad = 1; \
    } while (0)

static size_t r256(size_t n) { return (n + 255) / 256 * 256; }

// the rule, restated: a file joins while the sum stays at or under the limit; a file that alone exceeds it is a group of its own
static std::vector<std::pair<size_t, size_t>> restated(const std::vector<TierFile> &t, bool upload, size_t limit)
{
    std::vector<std::pair<size_t, size_t>> out;
    size_t start = 0, sum = 0;
    for (size_t i = 0; i < t.size(); i++) {
        const size_t need = r256(t[i].scan_bytes) + (upload ? r256(t[i].size) : 0) + t[i].share;
        if (i != start && sum + need > limit) out.push_back({start, i}), start = i, sum = 0;
        sum += need;
    }
    if (!t.empty()) out.push_back({start, t.size()});
    return out;
}

static std::vector<TierFile> tier_of(const std::vector<uint64_t> &scan, const std::vector<uint32_t> &sizes = {})
{
    std::vector<TierFile> t(scan.size());
    for (size_t i = 0; i < scan.size(); i++) t[i].file = (uint32_t)i, t[i].scan_bytes = scan[i], t[i].size = sizes.empty() ? 1000u : sizes[i];
    return t;
}

static bool breaks_are(const std::vector<TierGroup> &g, const std::vector<std::pair<size_t, size_t>> &want)
{
    if (g.size() != want.size()) return false;
    for (size_t i = 0; i < g.size(); i++)
        if (g[i].g0 != want[i].first || g[i].g1 != want[i].second) return false;
    return true;
}

static void grouping()
{
    std::vector<TierFile> t = tier_of({256, 512, 256, 1024});
    CHECK(breaks_are(png_groups(t, false, 1024), {{0, 3}, {3, 4}})); // (a sum equal to the limit joins)
    CHECK(breaks_are(png_groups(t, false, 1023), {{0, 2}, {2, 3}, {3, 4}})); // (the last file alone exceeds the limit)
    CHECK(breaks_are(png_groups(t, false, 256), {{0, 1}, {1, 2}, {2, 3}, {3, 4}}));
    std::vector<TierGroup> g = png_groups(t, false, 1024);
    CHECK(g.size() == 2 && g[0].scan == 1024 && g[0].bytes == 0 && g[1].scan == 1024 && g[1].bytes == 0);
    // scan_bytes of 1 and 257 count as 256 and 512
    std::vector<TierFile> odd = tier_of({1, 257});
    g = png_groups(odd, false, 768);
    CHECK(g.size() == 1 && g[0].scan == 768);
    CHECK(breaks_are(png_groups(odd, false, 767), {{0, 1}, {1, 2}}));
    g = png_groups(odd, false, 1);
    CHECK(g.size() == 2 && g[0].scan == 256 && g[1].scan == 512);
    // the host form: the files' bytes count as well, each rounded up
    std::vector<TierFile> host = tier_of({256, 512, 256, 1024}, {1, 300, 256, 0});
    g = png_groups(host, true, (size_t)1 << 30);
    CHECK(g.size() == 1 && g[0].scan == 2048 && g[0].bytes == 1024);
    g = png_groups(host, true, 256);
    CHECK(g.size() == 4 && g[0].bytes == 256 && g[1].bytes == 512 && g[2].bytes == 256 && g[3].bytes == 0);
    g = png_groups(host, false, (size_t)1 << 30);
    CHECK(g.size() == 1 && g[0].bytes == 0);
    CHECK(breaks_are(png_groups(host, true, 256 + 256 + 512 + 512), {{0, 2}, {2, 4}})); // (files 0 and 1 with their bytes: exactly the limit; so are 2 and 3)
    CHECK(breaks_are(png_groups(host, true, 256 + 256 + 512 + 512 - 1), {{0, 1}, {1, 2}, {2, 3}, {3, 4}}));
    // a share on file 1 alone moves the first break
    std::vector<TierFile> shared = tier_of({256, 512, 256, 1024});
    shared[1].share = 4096;
    const size_t joins = 256 + 512 + 4096; // files 0 and 1 and file 1's share: the least limit at which file 1 joins file 0
    CHECK(breaks_are(png_groups(t, false, 1024), {{0, 3}, {3, 4}}) && png_groups(shared, false, 1024)[0].g1 == 1);
    CHECK(png_groups(shared, false, joins)[0].g1 == 2 && png_groups(shared, false, joins - 1)[0].g1 == 1);
    CHECK(png_groups(shared, false, joins + 256)[0].g1 == 3 && png_groups(t, false, joins)[0].g1 == 4);
    g = png_groups(shared, false, joins);
    CHECK(g[0].scan == 768 && g[0].bytes == 0); // (the share is counted, not kept: it is the plan's, behind the scanlines)
    // an empty list
    CHECK(png_groups(std::vector<TierFile>(), false, 1024).empty() && png_groups(std::vector<TierFile>(), true, 1).empty());
    // a sweep: lists of up to 12 files, against the restated rule
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](uint32_t n) { return seed = seed * 6364136223846793005ull + 1442695040888963407ull, (uint32_t)((seed >> 33) % n); };
    for (int round = 0; round < 400; round++) {
        std::vector<TierFile> r(rnd(13));
        for (TierFile &q : r) q = TierFile(), q.scan_bytes = rnd(4) ? rnd(3000) : rnd(4) * 256, q.size = rnd(2000), q.share = rnd(3) ? 0 : (size_t)rnd(20) * 256;
        const bool upload = rnd(2);
        const size_t limit = 1 + rnd(rnd(2) ? 3000 : 20000);
        const std::vector<TierGroup> got = png_groups(r, upload, limit);
        if (!breaks_are(got, restated(r, upload, limit))) printf("sweep round %d: other groups than the restated rule's\n", round), bad = 1;
        for (const TierGroup &x : got) {
            size_t scan = 0, bytes = 0;
            for (size_t k = x.g0; k < x.g1; k++) scan += r256(r[k].scan_bytes), bytes += upload ? r256(r[k].size) : 0;
            if (x.scan != scan || x.bytes != bytes || x.g0 >= x.g1) printf("sweep round %d: a group's sums\n", round), bad = 1;
        }
    }
}

static void layout()
{
    // the png calls need align256(m * 64) + align256(m * 32) + bytes + scan; the views calls put align256(m * 32) of boxes in front of the bytes
    const size_t ms[4] = {1, 4, 5, 9}, png_end[4] = {512, 512, 768, 1280}, views_end[4] = {768, 768, 1024, 1792};
    const size_t states_at[4] = {256, 256, 512, 768}, boxes_at[4] = {512, 512, 768, 1280};
    const TierGroup sums[2] = {{0, 0, 0, 0}, {0, 0, 1024, 512}};
    for (int i = 0; i < 4; i++)
        for (const TierGroup &g : sums)
            for (int with_boxes = 0; with_boxes < 2; with_boxes++) {
                const size_t m = ms[i];
                const TierLayout at = png_group_layout(m, g, with_boxes);
                CHECK(at.end == (with_boxes ? views_end[i] : png_end[i]) + g.bytes + g.scan);
                CHECK(at.recs == 0 && at.states == states_at[i] && at.boxes == boxes_at[i] && at.bytes == (with_boxes ? views_end[i] : png_end[i]));
                CHECK(at.scan == at.bytes + g.bytes && at.end == at.scan + g.scan);
                for (size_t o : {at.recs, at.states, at.boxes, at.bytes, at.scan, at.end}) CHECK(o % 256 == 0);
                // in this order, and no piece reaches the next
                CHECK(at.recs + m * sizeof(pngi::File) <= at.states && at.states + m * sizeof(pngi::State) <= at.boxes);
                CHECK(at.boxes + (with_boxes ? m * sizeof(pngi::Box) : 0) <= at.bytes && at.bytes <= at.scan && at.scan <= at.end);
            }
}

// three files, placed and filled; the scratch is a heap block of exactly at.end bytes
static void records(bool upload, uint32_t dst_c)
{
    static uint8_t file_a[300], file_b[1], file_c[256], pixels[3][16];
    std::vector<TierFile> t(3);
    const uint32_t w[3] = {7, 300, 16}, h[3] = {5, 3, 16}, bpp[3] = {3, 1, 4}, color[3] = {2, 3, 6}, kept_rows[3] = {5, 2, 9};
    const void *data[3] = {file_a, file_b, file_c};
    const uint32_t size[3] = {300, 1, 256};
    for (int k = 0; k < 3; k++) {
        t[k].file = 10 + k, t[k].w = w[k], t[k].h = h[k], t[k].bpp = bpp[k], t[k].color = color[k], t[k].data = data[k], t[k].size = size[k], t[k].out = pixels[k];
        t[k].scan_bytes = (uint64_t)(dst_c ? h[k] : kept_rows[k]) * (1 + w[k] * bpp[k]);
    }
    const std::vector<TierGroup> g = png_groups(t, upload, (size_t)1 << 30);
    CHECK(g.size() == 1 && g[0].bytes == (upload ? 512u + 256u + 256u : 0u));
    const TierLayout at = png_group_layout(3, g[0], !dst_c);
    uint8_t *base = (uint8_t *)malloc(at.end);
    std::vector<pngi::File> recs(3);
    std::vector<TierCopy> copies(7); // (whatever it held is gone)
    fill_records(t.data(), 3, at, base, upload, dst_c, recs.data(), copies);
    CHECK(copies.size() == (upload ? 3u : 0u));
    size_t at_bytes = at.bytes, at_scan = at.scan;
    for (int k = 0; k < 3; k++) {
        const pngi::File &r = recs[k];
        CHECK(r.w == w[k] && r.h == h[k] && r.bpp == bpp[k] && r.color == color[k] && r.size == size[k] && r.scan_bytes == t[k].scan_bytes && r.dst_c == dst_c);
        CHECK(r.out == (dst_c ? pixels[k] : nullptr) && r.need_bytes == (dst_c ? 0u : (uint64_t)h[k] * (1 + w[k] * bpp[k])));
        CHECK(r.scan == base + at_scan && at_scan + r.scan_bytes <= at.end);
        r.scan[0] = 1, r.scan[r.scan_bytes - 1] = 2; // (the kernels' writes: first and last byte)
        at_scan += r256(r.scan_bytes);
        if (upload) {
            CHECK(copies[k].src == data[k] && copies[k].size == size[k] && copies[k].ofs == at_bytes && r.data == base + at_bytes && at_bytes + size[k] <= at.scan);
            memcpy(base + copies[k].ofs, copies[k].src, copies[k].size); // (the caller's copy)
            CHECK(r.data[0] == 0 && r.data[r.size - 1] == 0);
            at_bytes += r256(size[k]);
        } else
            CHECK(r.data == data[k]);
    }
    CHECK(at_bytes == at.scan && at_scan == at.end);
    base[at.end - 1] = 3;
    free(base);
}

static void be(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v; }

static void marker()
{
    uint8_t good[kPngHead] = {137, 80, 78, 71, 13, 10, 26, 10};
    be(good + 8, 13), memcpy(good + 12, "IHDR", 4), be(good + 16, 130), be(good + 20, 65), good[24] = 8, good[25] = 2;
    be(good + 33, 5), memcpy(good + 37, "fdEC", 4);
    CHECK(looks_fpng(good, 58) && looks_fpng(good, 4000) && !looks_fpng(good, 57) && !looks_fpng(good, 0));
    for (uint32_t c = 0; c < 8; c++) {
        uint8_t x[kPngHead];
        memcpy(x, good, sizeof x), x[25] = (uint8_t)c;
        CHECK(looks_fpng(x, 4000) == (c == 2 || c == 6));
    }
    uint8_t x[kPngHead];
    memcpy(x, good, sizeof x), x[24] = 16;
    CHECK(!looks_fpng(x, 4000));
    memcpy(x, good, sizeof x), x[24] = 4;
    CHECK(!looks_fpng(x, 4000));
    memcpy(x, good, sizeof x), be(x + 33, 4);
    CHECK(!looks_fpng(x, 4000));
    memcpy(x, good, sizeof x), be(x + 33, 6);
    CHECK(!looks_fpng(x, 4000));
    memcpy(x, good, sizeof x), x[40] = 'c';
    CHECK(!looks_fpng(x, 4000));
    memcpy(x, good, sizeof x), memcpy(x + 37, "IDAT", 4);
    CHECK(!looks_fpng(x, 4000));
    memcpy(x, good, sizeof x), x[0] = 0;
    CHECK(!looks_fpng(x, 4000));
    memcpy(x, good, sizeof x), be(x + 8, 12);
    CHECK(!looks_fpng(x, 4000));
}

static void fold()
{
    const uint32_t statuses[8] = {pngi::kOk, pngi::kNotPng, pngi::kHeaderCrc, pngi::kBadDims, pngi::kDimsTooLarge, pngi::kBadChunk, pngi::kBadIdat, pngi::kUnsupported};
    for (uint32_t st : statuses)
        for (uint32_t color : {0u, 2u, 3u, 4u, 6u})
            for (uint32_t trns : {0u, 1u, 200u}) {
                TierFile q = TierFile();
                q.color = color;
                pngi::State s = pngi::State();
                s.status = st, s.trns_len = trns;
                fpng_amd_decode_result r = fpng_amd_decode_result();
                r.channels_in_file = 3, r.w = 5, r.h = 6, r.status = 99;
                fold_state(r, q, s);
                const bool four = color == 3 && trns && st != pngi::kBadChunk && st != pngi::kUnsupported;
                CHECK(r.status == (int32_t)st && r.channels_in_file == (four ? 4u : 3u) && r.w == 5 && r.h == 6);
            }
}

int main()
{
    grouping();
    layout();
    records(false, 3), records(true, 4), records(false, 0), records(true, 0);
    marker();
    fold();
    if (!bad) printf("ok\n");
    return bad;
}
