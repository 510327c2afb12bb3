// decode_api.cpp -- host side of the GPU batch decoder (decode.hip): what the reference's fpng_decode_memory does in front of
// its pixel loops (reference src/fpng.cpp:2904-3222: container walk, IDAT checks, block type, dynamic header), then uploads (or,
// for files that already live in device memory, fetches the few hundred bytes it has to read) and launches.  The parsing code
// is the CPU decoder's own (png_parse.h), so the status codes of damaged containers are the same.
#include "decode.h"
#include "decode_core.h"
#include "encoder.h"
#include "host_workers.h"
#include "png_parse.h"
#include "png_tier_plan.h"
#include "resize.h"
#include "resize_color.h"
#include "resize_hwc.h"
#include "view_plan.h"
#include "view_post.h"
#include "view_request.h"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <unordered_map>
#include <vector>

using namespace fpng_amd;

namespace {

constexpr uint32_t kMaxGroups = 4;    // groups of files whose upload and decode overlap (8 measured: 5-15 % slower, a dozen launches per group)
constexpr uint32_t kBorderRounds = 2; // synchronisation rounds across workgroup borders launched without asking whether they are needed
constexpr uint32_t kMaxRounds = 64;   // ... and the most a file gets before it is left to the CPU decoder
constexpr uint32_t kHeadBytes = 1024, kTailBytes = 64; // what is copied back of a device-resident file before anything else

struct Parsed {
    uint32_t w = 0, h = 0, c = 0, idat_ofs = 0, idat_len = 0;
    int status = 0;       // fpng::FPNG_DECODE_*
    uint32_t mode = 0;    // 0 dynamic, 1 stored
    uint64_t first_bit = 0;
    int lut = -1;         // index into the unique lookup tables
};

// The stored-block layout the reference accepts (src/fpng.cpp:2107-2207): block headers, sizes, filter bytes 0, exact end.
// 0 = the encoder's own layout (full 65535-byte blocks, then the rest: what dec_stored_kernel copies), 1 = not acceptable,
// 2 = acceptable to the reference but cut into other block sizes (or with the one zero byte behind the image that the reference
// lets pass): left to the CPU decoder.
int check_stored(const uint8_t *z, uint32_t avail, uint32_t zlib_len, uint32_t w, uint32_t h, uint32_t c)
{
    const uint64_t stride = (uint64_t)w * c + 1, total = stride * h;
    uint64_t src = 2, got = 0;
    bool usual = true;
    for (;;) {
        if (src + 5 > avail) return 1;
        const bool final_block = z[src] & 1;
        if (((z[src] >> 1) & 3) != 0) return 1;
        const uint32_t len = z[src + 1] | (z[src + 2] << 8), nlen = z[src + 3] | (z[src + 4] << 8);
        src += 5;
        if (len != (~nlen & 0xFFFF) || src + len > avail) return 1;
        if (!final_block && len != 65535) usual = false;
        for (uint64_t r = (got + stride - 1) / stride * stride; r < got + len; r += stride) // filter bytes inside this block
            if (z[src + (r - got)] != 0) return 1;
        got += len;
        src += len;
        if (final_block) break;
    }
    if (src + 4 != zlib_len) return 1;
    // (the reference reads ONE byte more than the image holds if it is 0: it takes it for the filter byte of a row that never
    //  comes -- :2158-2166 look at a row's first byte before they ask whether there is room; the loop above has checked it)
    if (got == total + 1) return 2;
    if (got != total) return 1;
    return usual ? 0 : 2;
}

// The kernels' lookup table (decode_core.h) from the host parser's (symbol | code length << 9 per 12-bit index) and the code lengths:
// up to three literals per entry, length symbols 257..285 with their base length and extra bit count (RFC 1951 3.2.5; 286 / 287
// never occur in a valid stream), then the literals' code lengths.
void build_multi_lut(const uint32_t *table, const uint8_t sizes[288], uint32_t *lut)
{
    static const uint16_t len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const uint32_t bits = fpng::parse::kTableBits;
    for (uint32_t k = 0; k < (1u << bits); k++) {
        const uint32_t e1 = table[k], l1 = (e1 >> 9) & 15u, s1 = e1 & 511u;
        uint32_t ent = 0;
        if (!l1 || s1 > 285)
            ent = 0;
        else if (s1 == 256)
            ent = dec::kEntEob | l1 << 12;
        else if (s1 > 256)
            ent = len_extra[s1 - 257] ? dec::kEntMatch | l1 << 12 | (uint32_t)len_extra[s1 - 257] << 9 | len_base[s1 - 257] : (l1 + 1) << 28 | dec::kEntMatch | len_base[s1 - 257];
        else {
            uint32_t L = l1, n = 1, lits = s1;
            while (n < 3) { // the next code is whole if its length fits into the index bits that are left
                const uint32_t e2 = table[k >> L], l2 = (e2 >> 9) & 15u, s2 = e2 & 511u;
                if (!l2 || s2 >= 256 || L + l2 > bits) break;
                lits |= s2 << (8 * n);
                n++, L += l2;
            }
            ent = L << 28 | n << 26 | lits;
        }
        lut[k] = ent;
    }
    uint8_t *lenof = (uint8_t *)(lut + dec::kLutEntries);
    std::memcpy(lenof, sizes, 256);
}

// What the host settles about one file's zlib stream before the GPU sees it (the container was parsed: p.w .. p.idat_len): stored
// blocks (checked here) or one final dynamic block (header read: `table` = the host parser's lookup table, `sizes` = the literal /
// length code lengths, p.first_bit = the first row token).  z / avail: the stream's bytes in host memory, `complete`: all of them
// (else only a head of the file: fpng::parse::kParseNeedMore asks for the rest).  Returns the reference's status code (0 or
// FPNG_DECODE_NOT_FPNG) or FPNG_AMD_DECODE_UNDECIDED (a stored layout only the CPU decoder takes).
// (memo: the last dynamic header read -- the files of a 1-pass batch all begin with the same one, and reading it costs 4 us a
//  file; a header that is bit for bit the memo's is not read again.  `table` may be nullptr: the code is then only checked)
struct HeaderMemo {
    uint32_t bits = 0, chans = 0; // bits: the header's end = the first row token, from the stream's first byte (0: no memo)
    uint8_t bytes[320];
    uint8_t sizes[288];
};
int plan_stream(const uint8_t *z, uint32_t avail, bool complete, Parsed &p, uint32_t *table, uint8_t sizes[288], HeaderMemo *memo = nullptr)
{
    using namespace fpng::parse;
    if (avail < 3) return complete ? (int)fpng::FPNG_DECODE_NOT_FPNG : kParseNeedMore;
    if (p.idat_len < 7 || z[0] != 0x78 || z[1] != 0x01) return fpng::FPNG_DECODE_NOT_FPNG;
    const uint64_t total = ((uint64_t)p.w * p.c + 1) * p.h;
    if ((z[2] & 6) == 0) {
        if (total > p.idat_len) return fpng::FPNG_DECODE_NOT_FPNG; // (stored blocks cannot hold the image)
        if (!complete) {
            // only a head of the file is here (it lies in device memory): with the size the USUAL layout has -- blocks of 65535
            // bytes and a last one -- dec_stored_kernel checks the block headers and the filter bytes where they are and reports
            // anything else (kDecStoredOdd: the file is then looked at on the host after all)
            const uint64_t nblk = (total + 65534) / 65535;
            if (p.idat_len != 2 + 5 * nblk + total + 4) return kParseNeedMore;
            p.mode = 1;
            return 0;
        }
        const int r = check_stored(z, avail, p.idat_len, p.w, p.h, p.c);
        if (r == 1) return fpng::FPNG_DECODE_NOT_FPNG;
        p.mode = 1;
        return r ? FPNG_AMD_DECODE_UNDECIDED : 0;
    }
    Bits in = {z, avail, 2, 0, 0, false};
    if (in.get(1) != 1 || in.get(2) != 2) return fpng::FPNG_DECODE_NOT_FPNG; // one final dynamic block
    bool known = false;
    if (memo && memo->bits && memo->chans == p.c) {
        const uint32_t nb = memo->bits >> 3, rb = memo->bits & 7;
        known = avail >= nb + 9 && !std::memcmp(z, memo->bytes, nb) && !((z[nb] ^ memo->bytes[nb]) & ((1u << rb) - 1u));
    }
    if (known) {
        std::memcpy(sizes, memo->sizes, 288);
        p.first_bit = memo->bits;
    } else {
        if (memo) memo->bits = 0;
        const bool ok = read_dynamic_header(in, p.c, table, sizes);
        if (!complete && in.byte + 8 > avail) return kParseNeedMore; // (the header reader may have run off the head)
        if (!ok) return fpng::FPNG_DECODE_NOT_FPNG;
        // a table with codes for the reserved length symbols 286 / 287: the reference's 4-channel decoder gives them a meaning of its
        // own (fpng_decode.cpp: inflate_rows) -- no fpng encoder writes such a table; the CPU decoder's
        if (sizes[286] | sizes[287]) return FPNG_AMD_DECODE_UNDECIDED;
        p.first_bit = in.bitpos();
        if (memo && (p.first_bit >> 3) < sizeof memo->bytes && (p.first_bit >> 3) < avail) {
            memo->bits = (uint32_t)p.first_bit, memo->chans = p.c;
            std::memcpy(memo->bytes, z, (size_t)(p.first_bit >> 3) + 1);
            std::memcpy(memo->sizes, sizes, 288);
        }
    }
    if (p.first_bit >= (uint64_t)(p.idat_len - 4) * 8) return fpng::FPNG_DECODE_NOT_FPNG;
    // a token has at least 2 bits and stands for at most 258 bytes: an IDAT this short cannot hold the image (checked before any
    // device memory is sized by the header's dimensions)
    if (total > (uint64_t)p.idat_len * 1032 + 258) return fpng::FPNG_DECODE_NOT_FPNG;
    return 0;
}

// parse one file that is wholly in host memory
int parse_host(const uint8_t *png, uint32_t size, Parsed &p, uint32_t *table, uint8_t sizes[288], HeaderMemo *memo = nullptr)
{
    p.status = fpng::parse::parse_container(png, size, p.w, p.h, p.c, p.idat_ofs, p.idat_len);
    if (p.status) return p.status;
    return plan_stream(png + p.idat_ofs + 8, size - (p.idat_ofs + 8), true, p, table, sizes, memo);
}

// A new epoch for dec_unfilter_kernel's look-back granules (never cleared: the epoch tells launches apart).  0 is skipped: it is the
// tag of granules that were zeroed and never written.
uint32_t next_epoch(fpng_amd_encoder *e)
{
    if (!(++e->dec_epoch & 0x3FFFFFFFu)) ++e->dec_epoch;
    return e->dec_epoch & 0x3FFFFFFFu;
}

bool tracing() { static const bool t = getenv("FPNG_AMD_TRACE") != nullptr; return t; }

// persistent workgroups of dec_sync_kernel's border rounds: their LDS lets three share a compute unit
int resident_workgroups(fpng_amd_encoder *e, uint32_t &resident)
{
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
    resident = (uint32_t)std::max(cus, 1) * 3;
    return FPNG_AMD_OK;
}

// FPNG_AMD_SRC_* as a DESTINATION (fpng_amd_decode_batch_ex): bytes per pixel, and the v_perm_b32 selector that turns a pixel dword
// in R,G,B,A order (A = 0xFF for 3-channel files) into the format's bytes (byte k of the selector = the R,G,B,A byte of destination
// byte k; 0x0d = a 0xFF byte: the X of the *X formats, and what a 3-byte format's fourth selector byte is never used for)
struct DstFormat {
    uint32_t bytes, sel;
};
constexpr DstFormat kDstFormats[FPNG_AMD_SRC_COUNT] = {
    {3, kDecSelRGB}, {3, 0x0d000102u},                                               // RGB BGR
    {4, 0x03020100u}, {4, 0x03000102u}, {4, 0x02010003u}, {4, 0x00010203u},          // RGBA BGRA ARGB ABGR
    {4, 0x0d020100u}, {4, 0x0d000102u}, {4, 0x0201000du}, {4, 0x0001020du}};         // RGBX BGRX XRGB XBGR
static_assert(sizeof(fpng_amd_png_ex) == 40 && offsetof(fpng_amd_png_ex, d_pixels) == 16 && offsetof(fpng_amd_png_ex, pixels_cap) == 32, "fpng_amd_png_ex layout");

// A parsed file's status: the container's (geometry may be half known), the pixels' size, then the parser's st (reference :3131-3136)
int file_status(const Parsed &p, int st, uint64_t need) { return !p.status && need > UINT32_MAX ? (int)fpng::FPNG_DECODE_FAILED_DIMENSIONS_TOO_LARGE : st; }

// A dynamic file's result from its device status word (stored files: kDecStoredOdd, collect_results())
int dec_result(uint32_t st)
{
    // (nothing else is known then: "invalid" may be a speculative decode's; a match at a row's first pixel is the CPU decoder's)
    if (st & (kDecNotConverged | kDecStalled | kDecTileLeaveToCpu | kDecTileStalled)) return FPNG_AMD_DECODE_UNDECIDED;
    return ((st & (kDecBadStream | kDecTileBadStream | kDecBadFilter)) || !(st & kDecSawEob)) ? fpng::FPNG_DECODE_NOT_FPNG : 0; // (no kDecSawEob: the stream never ended)
}

// ... and what the optional check of the checksums adds (fpng_amd_encoder_set_decode_verify): only a file that would have returned
// 0 can return FPNG_AMD_DECODE_BAD_CRC32 or _BAD_ADLER32, the CRC first
int verify_result(int st, uint32_t device_status)
{
    if (st) return st;
    return device_status & kDecBadCrc ? FPNG_AMD_DECODE_BAD_CRC32 : (device_status & kDecBadAdler ? FPNG_AMD_DECODE_BAD_ADLER32 : 0);
}
static_assert(sizeof(unsigned long long) == 8, "the Adler accumulators");

// The job record of a parsed file; its pointers are the caller's to set
DecJob make_job(const Parsed &p, uint32_t desired)
{
    DecJob j = {};
    j.w = p.w, j.h = p.h, j.src_c = p.c, j.dst_c = desired, j.bpl = p.w * p.c;
    j.z_bytes = p.idat_len, j.first_bit = p.first_bit, j.end_limit_bit = (uint64_t)(p.idat_len - 4) * 8, j.mode = p.mode;
    if (!p.mode) j.n_sub = (uint32_t)((j.end_limit_bit - j.first_bit + kSubBits - 1) / kSubBits), j.nseg = (p.h + kDecUnfRows - 1) / kDecUnfRows;
    return j;
}

struct DecArrays { // the device arrays both decode paths work on (seg: dec_unfilter_kernel's look-back granules, a buffer of their own)
    uint8_t *z;
    uint32_t *win;
    DecSubArrays sub;
    DecBlockRec *recs;
    uint64_t *block_off;
    unsigned long long *seg;
};

// The encoder's device scratch (d_decode, kept between calls), carved into 256-byte aligned pieces: offsets first, pointers once the
// buffer is big enough.  The arrays both paths need come first (z_bytes: the streams and what the kernels read behind them; subs:
// subsequences in whole workgroups); each path carves its own tail behind them, then calls place().
struct Scratch {
    size_t need = 0, z, win, info, bytes, rel, last, eob, tok, recs, boff, win_words, gran_words;
    size_t carve(size_t n) { const size_t o = need; need += align256(n); return o; }
    Scratch(size_t z_bytes, size_t win_words_, size_t subs, size_t gran_words_)
    {
        subs = std::max<size_t>(subs, 1), win_words = std::max<size_t>(win_words_, 1), gran_words = std::max<size_t>(gran_words_, 1);
        const size_t blocks = (subs + kDecSubBlock - 1) / kDecSubBlock;
        z = carve(z_bytes), win = carve(win_words * 4);
        info = carve(subs * 4), bytes = carve(subs * 4), rel = carve(subs * 4), last = carve(subs * 4), eob = carve(subs * 4);
        // (the token records: dec::kRecRows rows of 64 8-byte entries per 64 subsequences -- 16 x the files' bytes, of which a gradient touches a fifth)
        tok = carve((subs * (size_t)dec::kRecRows + 32 * dec::kRecLane) * 8);
        recs = carve(blocks * sizeof(DecBlockRec)), boff = carve(blocks * 8);
    }
    int place(fpng_amd_encoder *e, DecArrays &d) const
    {
        // (the look-back granules of dec_unfilter_kernel: never cleared between calls -- every launch has its own epoch, and memory
        //  that was just allocated, any bit pattern, is zeroed once)
        int rc;
        if ((rc = e->d_decode.ensure(need)) || (rc = e->d_dec_gran.ensure(gran_words))) return rc;
        if (e->d_dec_gran.fresh) {
            HIP_TRY(hipMemsetAsync(e->d_dec_gran.p, 0, e->d_dec_gran.cap * 8, e->stream));
            e->d_dec_gran.fresh = false;
        }
        uint8_t *base = e->d_decode.p;
        d.z = base + z, d.win = (uint32_t *)(base + win), d.sub.info = (uint32_t *)(base + info), d.sub.bytes = (uint32_t *)(base + bytes);
        d.sub.rel = (uint32_t *)(base + rel), d.sub.lastpx = (uint32_t *)(base + last), d.sub.eob = (uint32_t *)(base + eob), d.sub.tok = (uint64_t *)(base + tok);
        d.recs = (DecBlockRec *)(base + recs), d.block_off = (uint64_t *)(base + boff), d.seg = e->d_dec_gran.p;
        // the windows' index: "no subsequence" until dec_subscan_kernel says otherwise (a stream that covers less than the image leaves holes)
        HIP_TRY(hipMemsetAsync(d.win, 0xFF, win_words * 4, e->stream));
        return FPNG_AMD_OK;
    }
};

// The code lengths (288 each) of a batch's distinct lookup tables (1-pass files share two): ONE upload, the tables themselves are
// built on the GPU (dec_build_lut_kernel)
struct LutKeys {
    std::vector<uint8_t> keys;
    std::unordered_multimap<uint64_t, uint32_t> index; // ... found by their hash
    int prev = -1;                                     // the table of the last file
    uint32_t count() const { return (uint32_t)(keys.size() / 288); }
    const uint8_t *key(uint32_t q) const { return keys.data() + (size_t)q * 288; }
    int find_or_add(const uint8_t sizes[288])
    {
        // (the table of the file in front -- every file of a 1-pass batch -- is found by one comparison; else by a hash over the code
        //  lengths, eight bytes a step: a byte a step was 0.25 us a file, most of what the host spent on a 1-pass file)
        if (prev >= 0 && !std::memcmp(key(prev), sizes, 288)) return prev;
        uint64_t hsh = 1469598103934665603ull; // (FNV-1a style: a batch of 2-pass files has a table per file)
        for (int q = 0; q < 288; q += 8) {
            uint64_t v;
            std::memcpy(&v, sizes + q, 8);
            hsh = (hsh ^ v) * 1099511628211ull;
            hsh ^= hsh >> 29;
        }
        for (auto [it, end] = index.equal_range(hsh); it != end; ++it)
            if (!std::memcmp(key(it->second), sizes, 288)) return prev = (int)it->second;
        prev = (int)count();
        index.emplace(hsh, (uint32_t)prev);
        keys.insert(keys.end(), sizes, sizes + 288);
        return prev;
    }
};

struct Group { // files whose upload and decode overlap with the other groups'
    uint32_t j0, j1, blk0, blk1;
    DecUnfPlan plan; // (device pointers)
};

// One call of fpng_amd_decode_batch(_device): what its stages (parse, place, plan, enqueue, settle, collect) hand on to each other
struct Batch {
    fpng_amd_encoder *e;
    const fpng_amd_png *files;
    const fpng_amd_png_ex *ex; // fpng_amd_decode_batch(_device)_ex: the files' layouts (files[] then holds their data and size), else NULL
    uint32_t n, desired;
    fpng_amd_decode_result *results;
    bool device_data;
    hipStream_t s;
    uint32_t resident = 0, max_rounds = kMaxRounds;
    const fpng_amd_png_planar *planar = nullptr; // fpng_amd_decode_batch(_device)_planar: the same for planar destinations
    std::vector<int64_t> plane_pitch;            // (planar) a word per job, uploaded with the job records
    int64_t *d_plane_pitch = nullptr;
    const DecFloat *flt = nullptr; // fpng_amd_decode_batch(_device)_planar_float: the planes' element type and constants (else NULL) ...
    uint32_t elem = 1;             // ... and an element's bytes: a row of a plane is w * elem bytes
    const fpng_amd_crop *crops = nullptr; // fpng_amd_decode_batch(_device)_planar_crop: the planar files' crops (else NULL) ...
    std::vector<DecCrop> crop;            // ... a record per job, uploaded with the job records
    DecCrop *d_crops = nullptr;
    std::vector<uint32_t> col_blocks;     // per job: the column blocks its tiles are numbered over (a crop's: dec_crop_tiles)
    ViewPlan views; // the views of the resize, resize_view and views calls (view_plan.h); empty for every other call
    const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    std::vector<Parsed> ps;
    std::vector<DecJob> jobs;                // (their pointers into the scratch are offsets until place_files())
    std::vector<uint32_t> job_file, status;  // (status: the jobs' device status words, settle_groups())
    LutKeys luts;
    size_t z_total = 0, win_total = 0, seg_total = 0;
    uint32_t sub_total = 0;
    // the optional check of the checksums: FPNG_AMD_VERIFY_*, the most CRC ranges a file has and the most stored blocks, the files'
    // Adler accumulators (two words each) and CRC partials (max_ranges words each) in the scratch
    uint32_t verify = 0, max_ranges = 1, stored_blocks = 1;
    unsigned long long *d_adler_acc = nullptr;
    uint32_t *d_crc_part = nullptr;
    std::vector<uint8_t> whole; // a device-resident file the head and tail were not enough for
    DecArrays d;
    uint32_t *d_luts, *d_status, *d_changed, *d_eob, *d_multi;
    uint8_t *d_keys, *d_plan;
    DecJob *d_jobs;
    size_t setup_ofs = 0, setup_len = 0, setup_plan = 0; // job records, un-filter plans and the (zero) status words: adjacent in the scratch, ONE upload
    bool few_luts = false, luts_cached = false, prof = false;
    std::vector<Group> groups;
    std::mutex mu; // (the uploader thread: groups whose copies are enqueued and whose event is recorded)
    std::condition_variable cv;
    uint32_t issued = 0;
    hipError_t up_err = hipSuccess;
    Worker *uploader = nullptr;
    ~Batch() { if (uploader) uploader->wait(); } // (every way out waits for the uploader first: it works on this struct)
    uint32_t nj() const { return (uint32_t)jobs.size(); }
    double since() const { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_begin).count(); }
};

// ---- parse: every file's container and stream header (device-resident ones: from their heads and tails), job record, table key ----
int parse_files(Batch &b)
{
    using namespace fpng::parse;
    fpng_amd_encoder *e = b.e;
    if (b.device_data) { // their first and last bytes come back first (one round trip for the batch)
        const size_t per = kHeadBytes + kTailBytes, refs = align256((size_t)b.n * sizeof(DecFileRef));
        int rc;
        if ((rc = e->h_dec_fetch.ensure((size_t)b.n * per + refs)) || (rc = e->d_decode.ensure((size_t)b.n * per + refs))) return rc;
        DecFileRef *h_refs = (DecFileRef *)(e->h_dec_fetch.p + (size_t)b.n * per);
        for (uint32_t i = 0; i < b.n; i++) h_refs[i] = {(const uint8_t *)b.files[i].data, b.files[i].size, 0};
        // (one small upload, one gather kernel, one download: two copies per file cost ~10 us each)
        HIP_TRY(hipMemcpyAsync(e->d_decode.p + (size_t)b.n * per, h_refs, (size_t)b.n * sizeof(DecFileRef), hipMemcpyHostToDevice, b.s));
        launch_dec_fetch(b.s, (const DecFileRef *)(e->d_decode.p + (size_t)b.n * per), b.n, kHeadBytes, kTailBytes, e->d_decode.p);
        HIP_TRY(hipMemcpyAsync(e->h_dec_fetch.p, e->d_decode.p, (size_t)b.n * per, hipMemcpyDeviceToHost, b.s));
        HIP_TRY(hipStreamSynchronize(b.s));
        if (tracing()) fprintf(stderr, "[decode] +%.0f us: heads and tails of %u files are here\n", b.since(), b.n);
    }
    uint32_t *const table = nullptr; // (no host-side lookup table: the header reader only checks the code)
    HeaderMemo memo;
    b.ps.resize(b.n);
    for (uint32_t i = 0; i < b.n; i++) {
        const fpng_amd_png &f = b.files[i];
        Parsed &p = b.ps[i];
        fpng_amd_decode_result &r = b.results[i];
        if (!f.data || !f.size) {
            r.status = fpng::FPNG_DECODE_INVALID_ARG;
            continue;
        }
        uint8_t sizes[288];
        int st;
        if (!b.device_data)
            st = parse_host((const uint8_t *)f.data, f.size, p, table, sizes, &memo);
        else {
            const uint8_t *buf = e->h_dec_fetch.p + (size_t)i * (kHeadBytes + kTailBytes);
            const uint32_t size = f.size, hl = std::min(size, kHeadBytes), tl = size > hl ? std::min(size - hl, kTailBytes) : 0u;
            const View v = {buf, hl, tl ? buf + kHeadBytes : nullptr, size - tl, size};
            st = p.status = parse_container_view(v, p.w, p.h, p.c, p.idat_ofs, p.idat_len);
            if (!st) st = (p.idat_ofs + 8 < hl) ? plan_stream(buf + p.idat_ofs + 8, hl - (p.idat_ofs + 8), hl == size, p, table, sizes, &memo) : kParseNeedMore;
            if (st == kParseNeedMore) { // unusual chunks, a stored file, ...: the whole file comes back
                b.whole.resize(size);
                HIP_TRY(hipMemcpy(b.whole.data(), f.data, size, hipMemcpyDeviceToHost));
                p = Parsed();
                st = parse_host(b.whole.data(), size, p, table, sizes, &memo);
            }
        }
        r.w = p.w, r.h = p.h, r.channels_in_file = p.c;
        const uint32_t desired = b.planar ? b.planar[i].num_chans : b.ex ? kDstFormats[b.ex[i].format].bytes : b.desired;
        const uint64_t need = (uint64_t)p.w * p.h * desired;
        if ((r.status = file_status(p, st, need))) continue;
        // (what the job decodes: the destination's planes; with an alpha view of a 4-channel file all four of them)
        const uint32_t job_planes = b.views.active() ? b.views.job_planes(i, p.c, desired) : desired;
        // (a crop that leaves the image: the file's own outcome -- it is not decoded and needs no room)
        DecCrop crop = {0, 0, p.w, p.h};
        uint32_t crop_nseg = 0, crop_cb0 = 0, crop_ncb = 0;
        const uint32_t v0 = b.views.first_view(i), nv = b.views.views_of(i); // (the file's records of the crops)
        if (b.crops) {
            bool inside = true; // (every one of the file's crops)
            for (uint32_t v = v0; v < v0 + nv && inside; v++) {
                crop = {b.crops[v].x, b.crops[v].y, b.crops[v].w, b.crops[v].h};
                inside = dec_crop_tiles(p.w, p.h, crop, &crop_nseg, &crop_cb0, &crop_ncb);
            }
            if (!inside) {
                r.status = FPNG_AMD_DECODE_CROP_OUTSIDE;
                continue;
            }
        }
        // (views: judged on the caller's crops above; what the crop stage decodes, and the tiles that run, are those of the ONE box
        //  that holds the boxes of all of the file's views)
        if (b.views.active()) {
            crop = b.views.file_box(i);
            dec_crop_tiles(p.w, p.h, crop, &crop_nseg, &crop_cb0, &crop_ncb); // (inside the caller's crops: never outside)
        }
        // (only files that will be written need room)
        int64_t pitch = 0, plane_pitch = 0;
        if (b.planar && !b.views.active()) { // a destination of the crop's w x h elements per plane: its pitches, its room
            const fpng_amd_png_planar &x = b.planar[i];
            const DestPitches d = judge_planar_dest((const uint8_t *)f.d_pixels, x.row_pitch, x.plane_pitch, f.pixels_cap, crop.w, crop.h, desired, b.elem);
            if (d.refused) return fail(d.refused.code, d.refused.why);
            pitch = d.pitch, plane_pitch = d.plane_pitch;
        } else if (b.planar) {
            if (const Refusal no = b.views.file_records(i, f, b.planar[i], desired, crop, p.c)) return fail(no.code, no.why);
        } else if (b.ex) {
            const uint64_t row = (uint64_t)p.w * desired;
            pitch = b.ex[i].row_pitch ? b.ex[i].row_pitch : (int64_t)row;
            const uint64_t step = (uint64_t)(pitch < 0 ? -pitch : pitch);
            if (step < row) return fail(FPNG_AMD_ERR_INVALID_ARG, "|row_pitch| < w * format bytes");
            if (!f.d_pixels || f.pixels_cap < (uint64_t)(p.h - 1) * step + row) return fail(FPNG_AMD_ERR_BUFFER_TOO_SMALL, "d_pixels / pixels_cap < (h - 1) * |row_pitch| + w * format bytes");
        } else if (!f.d_pixels || f.pixels_cap < need)
            return fail(FPNG_AMD_ERR_BUFFER_TOO_SMALL, "d_pixels / pixels_cap < w * h * desired_chans");
        if (!p.mode && !b.max_rounds) {
            r.status = FPNG_AMD_DECODE_UNDECIDED;
            continue;
        }
        if (!p.mode) p.lut = b.luts.find_or_add(sizes);
        DecJob j = make_job(p, job_planes);
        j.out = f.d_pixels, j.sub_base = b.sub_total;
        if (b.ex) j.sel = kDstFormats[b.ex[i].format].sel, j.pitch = (int32_t)pitch; // (|pitch| < 2^31: decode_files)
        if (b.views.active()) { // (the job writes its box's planes into the scratch: an offset until place_files())
            j.out = (uint8_t *)(uintptr_t)b.views.add_job(i, desired, crop, job_planes);
            pitch = (int64_t)crop.w, plane_pitch = (int64_t)((uint64_t)crop.w * crop.h);
        }
        if (b.planar) j.pitch = (int32_t)pitch, b.plane_pitch.push_back(plane_pitch); // (|pitch| < 2^31: decode_files_planar)
        // (the tiles a crop needs: DecJob::nseg is read by the un-filter kernels, by the plan and by the granules' sizing only, so
        //  a crop's job carries the segments it needs and the plan its column blocks; with the Adler-32 check every tile runs)
        uint32_t ncb = dec_col_blocks(j.w, j.src_c, j.dst_c);
        if (b.crops) {
            if (!p.mode && !(b.verify & FPNG_AMD_VERIFY_ADLER32)) j.nseg = crop_nseg, ncb = crop_ncb;
            b.crop.push_back(crop);
        }
        b.col_blocks.push_back(ncb);
        if (!p.mode) {
            b.sub_total += (j.n_sub + kDecSubBlock - 1) / kDecSubBlock * kDecSubBlock; // whole workgroups per file
            // offsets into the shared scratch (pointers are patched once the buffers exist)
            j.win = (uint32_t *)(uintptr_t)b.win_total; // (words)
            b.win_total += (size_t)j.h * dec_col_blocks(j.w, j.src_c, j.dst_c) * dec::kWinWords;
            j.segsum = (uint32_t *)(uintptr_t)b.seg_total;
            b.seg_total += (size_t)j.nseg * ((j.bpl + 3) / 4);
        }
        if (b.verify) {
            // (the streams of host-resident files start on 16-byte boundaries of the scratch)
            b.max_ranges = std::max(b.max_ranges, dec_crc_ranges(b.device_data ? (uintptr_t)f.data + p.idat_ofs + 8 : 0, p.idat_len));
            if (p.mode) b.stored_blocks = std::max(b.stored_blocks, (uint32_t)((((uint64_t)j.bpl + 1) * j.h + 65534) / 65535));
        }
        if (b.device_data) {
            const uintptr_t zr = (uintptr_t)f.data + p.idat_ofs + 8;
            j.z = (const uint8_t *)(zr & ~(uintptr_t)3), j.z_shift = (uint32_t)(zr & 3);
            j.z_bytes += j.z_shift, j.first_bit += 8 * j.z_shift, j.end_limit_bit += 8 * j.z_shift;
        } else {
            j.z = (const uint8_t *)(uintptr_t)b.z_total;
            b.z_total += ((size_t)p.idat_len + 16 + 15) & ~(size_t)15; // (a token's window reaches up to 8 bytes ahead)
        }
        b.jobs.push_back(j);
        b.job_file.push_back(i);
    }
    b.views.close();
    if (tracing()) fprintf(stderr, "[decode] +%.0f us: %u files parsed, %u lookup tables wanted\n", b.since(), b.n, b.luts.count());
    return FPNG_AMD_OK;
}

// ---- place: the device scratch, where the lookup tables come from, the job records' pointers ----
int place_files(Batch &b)
{
    fpng_amd_encoder *e = b.e;
    const uint32_t nj = b.nj(), n_luts = b.luts.count();
    const size_t n_status = 2 * (size_t)nj + 1 + 2 * kMaxGroups; // status and eob index per file, changed and multi per group
    Scratch sc(b.z_total + 64, b.win_total, b.sub_total, b.seg_total);
    const size_t o_luts = sc.carve(std::max<size_t>(n_luts, 1) * dec::kLutDwords * 4), o_keys = sc.carve(std::max<size_t>(b.luts.keys.size(), 288));
    // the set-up block: job records, plane pitches, crops, the views' records, un-filter plans, status words
    const size_t o_jobs = sc.carve(nj * sizeof(DecJob)), o_pp = sc.carve(b.planar ? nj * sizeof(int64_t) : 0), o_crop = sc.carve(b.crops ? nj * sizeof(DecCrop) : 0);
    b.views.carve_records(sc);
    const size_t o_plan = sc.carve(((size_t)nj + kMaxGroups) * (sizeof(DecUnfPiece) + 8)), o_status = sc.carve(n_status * 4);
    // (behind the block, which is uploaded: what is only written on the device.  Nothing more than without the check unless it is asked for)
    b.views.carve_scratch(sc);
    const size_t o_acc = b.verify & FPNG_AMD_VERIFY_ADLER32 ? sc.carve((size_t)nj * 16) : 0, o_part = b.verify & FPNG_AMD_VERIFY_CRC32 ? sc.carve((size_t)nj * b.max_ranges * 4) : 0;
    int rc;
    if ((rc = sc.place(e, b.d))) return rc;
    uint8_t *base = e->d_decode.p;
    if (b.verify & FPNG_AMD_VERIFY_ADLER32) b.d_adler_acc = (unsigned long long *)(base + o_acc);
    if (b.verify & FPNG_AMD_VERIFY_CRC32) b.d_crc_part = (uint32_t *)(base + o_part);
    b.d_luts = (uint32_t *)(base + o_luts), b.d_keys = base + o_keys, b.d_jobs = (DecJob *)(base + o_jobs), b.d_plan = base + o_plan, b.d_status = (uint32_t *)(base + o_status);
    b.d_plane_pitch = b.planar ? (int64_t *)(base + o_pp) : nullptr;
    b.d_crops = b.crops ? (DecCrop *)(base + o_crop) : nullptr;
    b.views.place(base);
    b.d_changed = b.d_status + nj, b.d_eob = b.d_changed + kMaxGroups, b.d_multi = b.d_eob + nj + 1; // (changed, multi: a word per group -- launch_dec_sync)
    b.setup_ofs = o_jobs, b.setup_plan = o_plan - o_jobs, b.setup_len = o_status + n_status * 4 - o_jobs;
    // the tables: from the encoder's cache when every one of this batch's is there; a batch of few distinct tables that are not
    // refills the cache (its tables are built in place); a batch of many (2-pass files: one each) builds them in the call's scratch
    std::vector<uint32_t> lut_slot(n_luts, 0);
    b.few_luts = n_luts && n_luts <= fpng_amd_encoder::kDecLutCache;
    if (b.few_luts) {
        if ((rc = e->d_lut_cache.ensure((size_t)fpng_amd_encoder::kDecLutCache * dec::kLutDwords))) return rc;
        if (e->d_lut_cache.fresh) e->lut_cache_n = 0, e->d_lut_cache.fresh = false;
        b.luts_cached = true;
        for (uint32_t q = 0; q < n_luts && b.luts_cached; q++) {
            bool hit = false;
            for (uint32_t c = 0; c < e->lut_cache_n && !hit; c++)
                if (!std::memcmp(e->lut_cache_keys[c], b.luts.key(q), 288)) lut_slot[q] = c, hit = true;
            b.luts_cached = hit;
        }
        if (!b.luts_cached) { // (re)fill: this batch's tables become the cache
            // The cache holds NOTHING until launch_dec_build_luts has been enqueued (enqueue_groups()): every error return between here
            // and there leaves it empty instead of naming tables that were never built.
            e->lut_cache_n = 0;
            for (uint32_t q = 0; q < n_luts; q++) std::memcpy(e->lut_cache_keys[q], b.luts.key(q), 288), lut_slot[q] = q;
            b.d_luts = e->d_lut_cache.p; // (built in place)
        }
    }
    for (uint32_t k = 0; k < nj; k++) {
        DecJob &j = b.jobs[k];
        const Parsed &p = b.ps[b.job_file[k]];
        if (!b.device_data) j.z = b.d.z + (size_t)(uintptr_t)j.z;
        if (b.views.active()) j.out = b.views.d_mid + (size_t)(uintptr_t)j.out;
        // (parse_files sized the CRC partials of a host-resident file for a stream that starts on a 16-byte boundary; dec_verify_kernel
        //  counts the ranges from the real address, and one more range than sized would be the next file's slot)
        if (!b.device_data && (b.verify & FPNG_AMD_VERIFY_CRC32) && ((uintptr_t)j.z & 15)) return fail(FPNG_AMD_ERR_UNSUPPORTED, "decode scratch: a file's stream is not 16-byte aligned");
        if (!j.mode) {
            j.win = b.d.win + (size_t)(uintptr_t)j.win;
            j.segsum = (uint32_t *)(b.d.seg + (size_t)(uintptr_t)j.segsum);
            j.lut = (b.few_luts ? e->d_lut_cache.p + (size_t)lut_slot[p.lut] * dec::kLutDwords : b.d_luts + (size_t)p.lut * dec::kLutDwords);
        }
    }
    return FPNG_AMD_OK;
}

// ---- plan: the groups of files -- while one group is decoded the next one's bytes are on their way (its own stream; from pageable
//      memory an "asynchronous" copy keeps its caller busy for most of its duration, so a thread of its own issues them); files that
//      are in device memory already form one group -- and the set-up block: job records, un-filter plans, zero status words ----
int plan_groups(Batch &b)
{
    const uint32_t nj = b.nj();
    const std::vector<DecJob> &jobs = b.jobs;
    // (file k goes to the group its middle byte falls into when the batch's bytes are cut into `want` equal parts)
    // Files in device memory are ONE group.  (Cutting them into 2..4 groups whose kernels alternate between two streams -- one
    // group's un-filter pass, memory-bound, under the next group's synchronisation and emit passes -- was measured in round 5: no
    // gain, 8 x 8K 2.33 -> 2.39 / 2.45 / 2.46 ms, profiles/r05_decode_groups.txt.)
    uint64_t total = 0, run = 0;
    for (uint32_t k = 0; k < nj; k++) total += jobs[k].z_bytes;
    const uint32_t want = (!b.device_data && b.z_total >= (8u << 20) && nj > 1) ? std::min<uint32_t>(kMaxGroups, nj) : 1u;
    auto close = [&](uint32_t j0, uint32_t j1) {
        b.groups.push_back({j0, j1, jobs[j0].sub_base / kDecSubBlock, (j1 < nj ? jobs[j1].sub_base : b.sub_total) / kDecSubBlock, {}});
    };
    uint32_t j0 = 0, cur = 0;
    for (uint32_t k = 0; k < nj; k++) {
        const uint32_t gi = (uint32_t)std::min<uint64_t>(want - 1, (run + jobs[k].z_bytes / 2) * want / std::max<uint64_t>(total, 1));
        if (k > j0 && gi != cur) close(j0, k), j0 = k;
        cur = gi;
        run += jobs[k].z_bytes;
    }
    close(j0, nj);
    // (four small uploads -- job records, plan pieces, plan words, cleared status words -- were four blit kernels with their dispatch
    //  gaps in front of the first decode kernel, ~7 us each: they go up as one block from pinned memory)
    if (int rc = b.e->h_dec_fetch.ensure(b.setup_len)) return rc;
    uint8_t *const h_setup = b.e->h_dec_fetch.p; // (the fetched heads and tails that lived here have been parsed)
    std::memset(h_setup, 0, b.setup_len);
    // dec_unfilter_kernel's work items per group of files, numbered segment by segment (decode.h: DecUnfPlan)
    DecUnfPiece *d_pieces = (DecUnfPiece *)b.d_plan;
    uint32_t *d_words = (uint32_t *)(d_pieces + nj + kMaxGroups);
    std::vector<DecUnfPiece> pieces;
    std::vector<uint32_t> words; // per group: cbpre (files + 1), then order (files)
    for (Group &g : b.groups) {
        std::vector<uint32_t> order;
        for (uint32_t q = g.j0; q < g.j1; q++)
            if (!jobs[q].mode) order.push_back(q - g.j0);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t c) { return jobs[g.j0 + a].nseg > jobs[g.j0 + c].nseg; });
        const uint32_t m = (uint32_t)order.size();
        const size_t w0 = words.size(), p0 = pieces.size();
        words.push_back(0);
        for (uint32_t k = 0; k < m; k++) words.push_back(words.back() + b.col_blocks[g.j0 + order[k]]);
        words.insert(words.end(), order.begin(), order.end());
        uint32_t seg = 0, item = 0;
        for (uint32_t alive = m; alive >= 1; alive--) { // the alive-th file of the order is the next one to run out of rows
            const uint32_t end = jobs[g.j0 + order[alive - 1]].nseg;
            if (end > seg) {
                pieces.push_back({item, seg, alive, 0});
                item += (end - seg) * words[w0 + alive];
                seg = end;
            }
        }
        g.plan.pieces = d_pieces + p0, g.plan.n_pieces = (uint32_t)(pieces.size() - p0), g.plan.total_items = item;
        g.plan.cbpre = d_words + w0, g.plan.order = d_words + w0 + m + 1, g.plan.n_files = m, g.plan.pad_ = 0;
    }
    if (!pieces.empty()) std::memcpy(h_setup + b.setup_plan, pieces.data(), pieces.size() * sizeof(DecUnfPiece));
    if (!words.empty()) std::memcpy(h_setup + b.setup_plan + ((size_t)nj + kMaxGroups) * sizeof(DecUnfPiece), words.data(), words.size() * 4);
    std::memcpy(h_setup, jobs.data(), nj * sizeof(DecJob));
    if (b.planar) std::memcpy(h_setup + ((uint8_t *)b.d_plane_pitch - (uint8_t *)b.d_jobs), b.plane_pitch.data(), nj * sizeof(int64_t));
    if (b.crops) std::memcpy(h_setup + ((uint8_t *)b.d_crops - (uint8_t *)b.d_jobs), b.crop.data(), nj * sizeof(DecCrop));
    b.views.write_setup(h_setup, b.setup_ofs);
    return FPNG_AMD_OK;
}

// the bytes of group g's files, host to device on stream st
hipError_t upload_group(const Batch &b, const Group &g, hipStream_t st)
{
    for (uint32_t k = g.j0; k < g.j1; k++) {
        const Parsed &p = b.ps[b.job_file[k]];
        // (with the CRC check the chunk's CRC word, the four bytes behind the payload, comes along: the container walk has seen that they are there)
        const size_t len = (size_t)p.idat_len + (b.verify & FPNG_AMD_VERIFY_CRC32 ? 4 : 0);
        if (hipError_t err = hipMemcpyAsync((void *)b.jobs[k].z, (const uint8_t *)b.files[b.job_file[k]].data + p.idat_ofs + 8, len, hipMemcpyHostToDevice, st)) return err;
    }
    return hipSuccess;
}

// profiling (fpng_amd_encoder_set_profiling): events around the kernels of the first group of files
hipError_t stamp(const Batch &b, uint32_t gi, int k) { return (b.prof && gi == 0) ? hipEventRecord(b.e->dec_prof_ev[k], b.s) : hipSuccess; }

} // namespace

// The resize of the records of jobs j0 .. j1 - 1: behind the group's pixel pass and stored copy on the same stream, on whatever the
// scratch then holds -- it writes the spans of the destination and nothing else, whatever a file's status turns out to be
int fpng_amd::ViewPlan::enqueue(hipStream_t s, uint32_t j0, uint32_t j1, const DecFloat *flt) const
{
    if (!active()) return FPNG_AMD_OK;
    const uint32_t r0 = job_rec[j0], r1 = job_rec[j1]; // (the records of the group's jobs)
    bool ok;
    if (rq.posts) {
        // the group's direct views as the colour call launches them; its post views' windows into the scratch -- uint8, planar,
        // un-mirrored -- and the post stage out of those into the destinations
        const DecResizeColor *recs = (const DecResizeColor *)d_recs;
        const uint32_t p0 = job_post[j0], p1 = job_post[j1], d0 = r0 - p0, d1 = r1 - p1;
        const uint32_t nd = (uint32_t)(resize.size() - post_recs.size());
        uint32_t most_lds[2] = {0, 0};
        uint32_t any_filter[2] = {0, 0}; // (resize_launch_kind: the most of the launch's records)
        bool any_alpha[2] = {false, false};
        for (uint32_t q = r0; q < r1; q++) {
            const int kind = post_of[q] >= 0;
            most_lds[kind] = std::max(most_lds[kind], lds[q]), any_filter[kind] = std::max(any_filter[kind], resize_launch_kind(resize[q].filter)), any_alpha[kind] |= resize_alpha_op(resize[q].flags) != 0;
        }
        ok = launch_dec_resize_color(s, recs + d0, d_pre + d0, dir_pre.data() + d0, d1 - d0, most_lds[0], flt, any_filter[0], hwc(), any_alpha[0]) &&
             launch_dec_resize_color(s, recs + nd + p0, d_pre + nd + 1 + p0, post_pre.data() + p0, p1 - p0, most_lds[1], nullptr, any_filter[1], false, any_alpha[1]);
        // (the group's tone views: their histograms zeroed every time -- a group that needed more rounds comes here again -- and
        //  counted out of the windows just written, then their tables; the post stage looks them up)
        const uint32_t t0 = d_tone ? job_tone[j0] : 0, t1 = d_tone ? job_tone[j1] : 0;
        if (ok && t1 > t0) {
            HIP_TRY(hipMemsetAsync(d_tone + (size_t)t0 * kToneBytes, 0, (size_t)(t1 - t0) * kToneBytes, s));
            ok = launch_dec_view_tone(s, d_post, d_tone_refs + t0, tone_refs.data() + t0, t1 - t0);
        }
        ok = ok && launch_dec_view_post(s, d_post + p0, d_pre + nd + 1 + p0, post_pre.data() + p0, p1 - p0, flt, hwc(), rq.enhances ? 3 : rq.tones ? 2 : rq.warps ? 1 : 0);
    } else {
        const uint32_t most_tiles = *std::max_element(tiles.begin() + r0, tiles.begin() + r1), most_lds = *std::max_element(lds.begin() + r0, lds.begin() + r1);
        // (a group of bilinear views -- the plain resize call's always are -- runs the instantiation without the second filter)
        // (and one with a RESAMPLE filter -- the _resample calls' alone -- the instantiation that takes every filter as a value)
        uint32_t any_filter = 0;
        for (uint32_t q = r0; q < r1; q++) any_filter = std::max(any_filter, resize_launch_kind(resize[q].filter));
        // (the views call mixes sizes and plane counts in one launch: a grid of exactly its records' workgroups; the calls with one
        //  output per file keep the grid of the largest record)
        // (and a group without an alpha op -- every call but the _alpha ones, and those without one -- the instantiations without the stage)
        const bool any_alpha = std::any_of(resize.begin() + r0, resize.begin() + r1, [](const DecResize &r) { return resize_alpha_op(r.flags) != 0; });
        // (the per-plane kernels have no PREMULTIPLIED store: normalise_views sends such a request to the colour kernel)
        if (!per_tile() && std::any_of(resize.begin() + r0, resize.begin() + r1, [](const DecResize &r) { return resize_alpha_op(r.flags) == kAlphaPremultiplied; }))
            return fail(FPNG_AMD_ERR_UNSUPPORTED, "a premultiplied view in a per-plane resize launch");
        ok = rq.colors ? launch_dec_resize_color(s, (const DecResizeColor *)d_recs + r0, d_pre + r0, tile_pre.data() + r0, r1 - r0, most_lds, flt, any_filter, hwc(), any_alpha)
             : hwc()   ? launch_dec_resize_hwc(s, (const DecResizeHwc *)d_recs + r0, d_pre + r0, tile_pre.data() + r0, r1 - r0, most_lds, flt, any_filter, any_alpha)
             : multi() ? launch_dec_resize_exact(s, (const DecResize *)d_recs + r0, d_pre + r0, plane_pre.data() + r0, r1 - r0, most_lds, flt, any_filter, any_alpha)
                       : launch_dec_resize(s, (const DecResize *)d_recs + r0, r1 - r0, most_tiles, most_lds, flt, any_filter != 0);
        // (a YUV call: the planes just written into the scratch become the caller's surfaces)
        if (ok && rq.yuv) {
            YuvMatrix f;
            std::memcpy(f.m, rq.yuv_fmt->m, sizeof f.m);
            ok = launch_dec_yuv_store(s, d_yuv + r0, d_yuv_pre + r0, yuv_pre.data() + r0, r1 - r0, rq.yuv_fmt->surface, f, yuv_depth(rq.yuv_fmt->surface, rq.yuv_depth));
        }
    }
    return ok ? FPNG_AMD_OK : fail(FPNG_AMD_ERR_UNSUPPORTED, "resize launch: tiles or LDS out of range");
}

namespace {

// everything behind group gi's synchronisation (every step of it is idempotent)
int finish_group(Batch &b, uint32_t gi)
{
    const Group &g = b.groups[gi];
    const uint32_t nblk = g.blk1 - g.blk0;
    HIP_TRY(stamp(b, gi, 1));
    if (nblk) launch_dec_offsets(b.s, b.d_jobs, b.nj(), g.blk0, nblk, b.sub_total, b.d_jobs + g.j0, g.j1 - g.j0, b.d.sub, b.d.recs, b.d.block_off, b.d_status, b.d_eob);
    HIP_TRY(stamp(b, gi, 2));
    HIP_TRY(stamp(b, gi, 3));
    const bool any_stored = std::any_of(b.jobs.begin() + g.j0, b.jobs.begin() + g.j1, [](const DecJob &j) { return j.mode != 0; });
    // (all groups run on one stream: two un-filter kernels never run at once -- each one's workgroups wait for lower-numbered ones
    //  of their own launch, and two sets of waiting workgroups could keep each other's predecessors off the compute units)
    const DecPlaced placed = {b.d.sub, b.d.block_off, b.d_eob + g.j0, 0xFFFFFFFFu};
    DecVerify verify = {b.verify, b.max_ranges, b.stored_blocks, 0, nullptr, nullptr, device_crc_tables(b.e->device)};
    if (b.verify & FPNG_AMD_VERIFY_ADLER32) { // (zero every time: a group that needed more rounds comes here again)
        verify.adler_acc = b.d_adler_acc + 2 * (size_t)g.j0;
        HIP_TRY(hipMemsetAsync(verify.adler_acc, 0, (size_t)(g.j1 - g.j0) * 16, b.s));
    }
    if (b.verify & FPNG_AMD_VERIFY_CRC32) verify.crc_partials = b.d_crc_part + (size_t)g.j0 * b.max_ranges;
    launch_dec_finish(b.s, b.d_jobs + g.j0, g.j1 - g.j0, g.plan, placed, b.d_status + g.j0, next_epoch(b.e), any_stored, b.ex != nullptr,
                      b.planar ? b.d_plane_pitch + g.j0 : nullptr, b.verify ? &verify : nullptr, b.views.active() ? nullptr : b.flt, b.crops ? b.d_crops + g.j0 : nullptr);
    if (int rc = b.views.enqueue(b.s, g.j0, g.j1, b.flt)) return rc;
    HIP_TRY(stamp(b, gi, 4));
    if (b.prof && gi == 0) b.e->dec_prof_recorded = true;
    return FPNG_AMD_OK;
}

// ---- enqueue: the uploads, the lookup tables, the set-up block, then per group its synchronisation and what follows it ----
int enqueue_groups(Batch &b)
{
    fpng_amd_encoder *e = b.e;
    const uint32_t ng = (uint32_t)b.groups.size();
    const bool uploads = !b.device_data && ng > 1; // groups of host-resident files: their bytes go up on a stream of their own
    if (uploads) {
        if (!e->dec_up) HIP_TRY(create_copy_stream(&e->dec_up));
        for (uint32_t g = 0; g < ng; g++)
            if (!e->dec_ev[g]) HIP_TRY(hipEventCreateWithFlags(&e->dec_ev[g], hipEventDisableTiming));
        if (!e->workers) e->workers = new HostWorkers(); // (the encoder's copy threads, made once: host_workers.h)
        b.uploader = &e->workers->up;
        b.uploader->start([&b, ng] {
            hipError_t err = hipSetDevice(b.e->device);
            for (uint32_t g = 0; g < ng; g++) {
                if (err == hipSuccess) err = upload_group(b, b.groups[g], b.e->dec_up);
                if (err == hipSuccess) err = hipEventRecord(b.e->dec_ev[g], b.e->dec_up);
                if (tracing()) fprintf(stderr, "[decode] +%.0f us: uploads of group %u issued\n", b.since(), g);
                std::lock_guard<std::mutex> lk(b.mu);
                if (err != hipSuccess) b.up_err = err;
                b.issued = g + 1;
                b.cv.notify_all();
            }
        });
    }
    if (!b.luts.keys.empty() && !b.luts_cached) {
        HIP_TRY(hipMemcpyAsync(b.d_keys, b.luts.keys.data(), b.luts.keys.size(), hipMemcpyHostToDevice, b.s));
        launch_dec_build_luts(b.s, b.d_keys, b.luts.count(), b.d_luts);
        if (b.few_luts) e->lut_cache_n = b.luts.count(); // (the build is in the stream, in front of everything that will read the tables: now the cache names them)
    }
    HIP_TRY(hipMemcpyAsync(e->d_decode.p + b.setup_ofs, e->h_dec_fetch.p, b.setup_len, hipMemcpyHostToDevice, b.s));
    b.prof = e->profiling, e->dec_prof_recorded = false;
    if (b.prof)
        for (hipEvent_t &ev : e->dec_prof_ev)
            if (!ev) HIP_TRY(hipEventCreate(&ev));
    for (uint32_t gi = 0; gi < ng; gi++) {
        const Group &g = b.groups[gi];
        if (ng == 1) {
            if (!b.device_data) HIP_TRY(upload_group(b, g, b.s));
        } else if (uploads) {
            std::unique_lock<std::mutex> lk(b.mu);
            b.cv.wait(lk, [&] { return b.issued > gi; });
            if (b.up_err != hipSuccess) return fail(FPNG_AMD_ERR_HIP, "upload of the files", b.up_err);
            lk.unlock();
            HIP_TRY(hipStreamWaitEvent(b.s, e->dec_ev[gi], 0));
        }
        if (tracing()) fprintf(stderr, "[decode] +%.0f us: group %u (files %u..%u, %u workgroups) starts\n", b.since(), gi, g.j0, g.j1, g.blk1 - g.blk0);
        // The CRC pass needs the group's bytes and job records and nothing else: on a lane's stream (the lanes are drained), so that it
        // can run next to the synchronisation, which is bound by issue and latency while this streams through the files once.
        hipStream_t s_crc = e->lane_stream[0] ? e->lane_stream[0] : b.s;
        // (a failure between the launch and the main stream's wait for it must not return while the kernel may still read the
        //  scratch, which the next call reuses)
        struct CrcInFlight {
            hipStream_t s = nullptr;
            ~CrcInFlight() { if (s) (void)hipStreamSynchronize(s); }
        } crc_in_flight;
        if (b.verify & FPNG_AMD_VERIFY_CRC32) {
            for (hipEvent_t *ev : {&e->dec_crc_ev[2 * gi], &e->dec_crc_ev[2 * gi + 1]})
                if (!*ev) HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
            if (s_crc != b.s) {
                HIP_TRY(hipEventRecord(e->dec_crc_ev[2 * gi], b.s));
                HIP_TRY(hipStreamWaitEvent(s_crc, e->dec_crc_ev[2 * gi], 0));
            }
            launch_dec_crc(s_crc, b.d_jobs + g.j0, g.j1 - g.j0, b.max_ranges, device_crc_tables(e->device), b.d_crc_part + (size_t)g.j0 * b.max_ranges);
            if (s_crc != b.s) crc_in_flight.s = s_crc;
            if (s_crc != b.s) HIP_TRY(hipEventRecord(e->dec_crc_ev[2 * gi + 1], s_crc));
        }
        HIP_TRY(stamp(b, gi, 0));
        // round 0 settles every workgroup in itself; the borders between workgroups get kBorderRounds rounds launched blind (a
        // workgroup whose border holds leaves at once), and the chain check of dec_offsets_kernel says whether that was enough
        for (uint32_t r = 0; g.blk1 > g.blk0 && r <= std::min(kBorderRounds, b.max_rounds - 1); r++)
            launch_dec_sync(b.s, b.resident, b.d_jobs, b.nj(), g.blk0, g.blk1 - g.blk0, b.sub_total, r, b.d.sub, b.d.recs, b.d_changed + gi, b.d_multi + gi);
        if ((b.verify & FPNG_AMD_VERIFY_CRC32) && s_crc != b.s) HIP_TRY(hipStreamWaitEvent(b.s, e->dec_crc_ev[2 * gi + 1], 0));
        crc_in_flight.s = nullptr; // (from here on the main stream is behind it)
        if (int rc = finish_group(b, gi)) return rc;
        if (tracing()) fprintf(stderr, "[decode] +%.0f us: group %u enqueued\n", b.since(), gi);
    }
    return FPNG_AMD_OK;
}

// ---- settle: groups with a file whose chain does not hold across some border yet (nothing of such a file was written) get more
//      rounds, in fours, until one changes nothing -- a stream whose decoders stay out of step over whole workgroups (periodic
//      content) needs a round per border and is left to the CPU decoder beyond max_rounds -- then the rest of the pipeline again ----
int settle_groups(Batch &b)
{
    b.status.resize(b.nj());
    auto read_status = [&b]() -> int {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(b.status.data(), b.d_status, b.nj() * 4, hipMemcpyDeviceToHost, b.s));
        HIP_TRY(hipStreamSynchronize(b.s));
        return FPNG_AMD_OK;
    };
    if (int rc = read_status()) return rc;
    bool again = false;
    for (uint32_t gi = 0; gi < (uint32_t)b.groups.size(); gi++) {
        const Group &g = b.groups[gi];
        const bool open = std::any_of(b.status.begin() + g.j0, b.status.begin() + g.j1, [](uint32_t st) { return (st & kDecNotConverged) != 0; });
        if (!open || g.blk1 == g.blk0) continue;
        again = true;
        uint32_t r = std::min(kBorderRounds, b.max_rounds - 1);
        for (bool settled = false; !settled && r + 1 < b.max_rounds;) {
            uint32_t changed = 0;
            for (int k = 0; k < 4; k++) {
                r++;
                if (k == 3) HIP_TRY(hipMemsetAsync(b.d_changed + gi, 0, 4, b.s)); // (only the last of the four is asked)
                launch_dec_sync(b.s, b.resident, b.d_jobs, b.nj(), g.blk0, g.blk1 - g.blk0, b.sub_total, r, b.d.sub, b.d.recs, b.d_changed + gi, b.d_multi + gi);
            }
            HIP_TRY(hipMemcpyAsync(&changed, b.d_changed + gi, 4, hipMemcpyDeviceToHost, b.s));
            HIP_TRY(hipStreamSynchronize(b.s));
            settled = !changed;
        }
        if (tracing()) fprintf(stderr, "[decode] +%.0f us: group %u needed %u rounds\n", b.since(), gi, r + 1);
        HIP_TRY(hipMemsetAsync(b.d_status + g.j0, 0, (g.j1 - g.j0) * 4, b.s));
        if (int rc = finish_group(b, gi)) return rc;
    }
    return again ? read_status() : FPNG_AMD_OK;
}

// ---- collect: the status words become the files' results ----
int collect_results(Batch &b)
{
    if (tracing()) fprintf(stderr, "[decode] +%.0f us: done\n", b.since());
#ifdef FPNG_DEC_TILE_TIMING
    if (const char *tp = getenv("FPNG_AMD_TILE_TIMES")) dec_dump_tile_times(tp, b.groups[0].plan.total_items);
#endif
#ifdef FPNG_DEC_SYNC_TIMING
    if (const char *tp = getenv("FPNG_AMD_SYNC_TIMES")) dec_dump_sync_times(tp, b.groups[0].blk1 - b.groups[0].blk0);
#endif
    for (uint32_t k = 0; k < b.nj(); k++) {
        const DecJob &j = b.jobs[k];
        const uint32_t status = b.status[k];
        if (tracing())
            fprintf(stderr, "[decode] file %u: %ux%ux%u mode %u, %u subsequences, first bit %llu, device status 0x%x\n", b.job_file[k], j.w, j.h, j.src_c, j.mode, j.n_sub, (unsigned long long)j.first_bit, status);
        int32_t &st = b.results[b.job_file[k]].status;
        if (!j.mode) st = verify_result(dec_result(status), status);
        else if (!(status & kDecStoredOdd)) st = verify_result(0, status);
        else { // not the usual stored layout after all: the whole file, on the host (check_stored() is the rule)
            st = FPNG_AMD_DECODE_UNDECIDED;
            if (b.device_data) {
                const Parsed &p = b.ps[b.job_file[k]];
                b.whole.resize(p.idat_len);
                HIP_TRY(hipMemcpy(b.whole.data(), (const uint8_t *)b.files[b.job_file[k]].data + p.idat_ofs + 8, p.idat_len, hipMemcpyDeviceToHost));
                if (check_stored(b.whole.data(), p.idat_len, p.idat_len, p.w, p.h, p.c) == 1) st = fpng::FPNG_DECODE_NOT_FPNG;
            }
        }
    }
    return FPNG_AMD_OK;
}

// ex / planar: fpng_amd_decode_batch(_device)_ex's / _planar's files (files = their data and size; desired is not used); flt: the
// planar files are fpng_amd_decode_batch(_device)_planar_float's; rq: what else a planar-family call carries -- the crop call's
// crops, the resize calls' views, the views calls' records, judged and normalised (decode_files_views)
int decode_files(fpng_amd_encoder *e, const fpng_amd_png *files, uint32_t n, uint32_t desired, fpng_amd_decode_result *results, bool device_data,
                 const fpng_amd_png_ex *ex = nullptr, const fpng_amd_png_planar *planar = nullptr, const DecFloat *flt = nullptr, const ViewRequest &rq = ViewRequest())
{
    if (!e || !files || !n || !results) return fail(FPNG_AMD_ERR_INVALID_ARG, "null/empty batch");
    if (!ex && !planar && desired != 3 && desired != 4) return fail(FPNG_AMD_ERR_INVALID_ARG, "desired_chans must be 3 or 4");
    std::memset(results, 0, (size_t)n * sizeof *results); // (every entry is defined on every way out)
    HIP_TRY(hipSetDevice(e->device));
    int rc = drain(e);
    if (rc) return rc;
    Batch b{e, files, ex, n, desired, results, device_data, e->stream};
    b.planar = planar, b.crops = rq.crops, b.verify = e->dec_verify;
    if (flt) b.flt = flt, b.elem = dec_float_bytes(flt->dtype);
    b.views.begin(rq, n, b.elem);
    if ((rc =resident_workgroups(e, b.resident))) return rc;
    if (const char *mr = getenv("FPNG_AMD_DECODE_MAX_ROUNDS")) b.max_rounds = (uint32_t)std::max(0, atoi(mr)); // (0: every dynamic file is left to the CPU decoder -- tests)
    if ((rc = parse_files(b)) || !b.nj()) return rc;
    if ((rc = place_files(b)) || (rc = plan_groups(b)) || (rc = enqueue_groups(b)) || (rc = settle_groups(b))) return rc;
    return collect_results(b);
}

// fpng_amd_decode_host for a LARGE compressed file, streamed: the IDAT goes up in pieces (the encoder's uploader thread), every
// piece is synchronised, placed (dec_offsets_range_kernel carries the byte count from piece to piece) and decoded as soon as it has
// arrived, the rows that are complete get their Up filter undone and go down (the downloader thread) while later pieces are still
// on their way up: upload, decode and download overlap instead of following one another (8K RGBA: 58 MB up + 133 MB down).
// `out`: the caller's w * h * desired bytes.  *redo: the file's token boundaries did not settle in the rounds launched here --
// the caller goes through fpng_amd_decode_batch, which adds rounds.
int decode_host_streamed(fpng_amd_encoder *e, const uint8_t *png, const Parsed &p, const uint32_t *table, const uint8_t *sizes, uint32_t desired, uint8_t *out,
                         fpng_amd_decode_result *result, bool *redo)
{
    *redo = false;
    int rc;
    if ((rc = ensure_copy_streams(e))) return rc;
    hipStream_t s = e->stream, s_up = e->host.up, s_down = e->host.down;
    // The Up filter's undoing of a piece's rows runs on a stream of its own (a lane's: the lanes are drained), next to the following
    // piece's synchronisation and decode instead of behind them: the rows go down one piece earlier.
    hipStream_t s_unf = e->lane_stream[0] ? e->lane_stream[0] : s;
    uint32_t resident = 0;
    if ((rc = resident_workgroups(e, resident))) return rc;
    std::vector<uint32_t> lut(dec::kLutDwords);
    build_multi_lut(table, sizes, lut.data());
    DecJob j = make_job(p, desired);
    const uint32_t n_blocks = (j.n_sub + kDecSubBlock - 1) / kDecSubBlock, sub_total = n_blocks * kDecSubBlock;
    const size_t col_blocks = dec_col_blocks(j.w, j.src_c, j.dst_c), os = (size_t)p.w * desired;
    // ---- scratch: the shared arrays, then the table, the job record and the few words the kernels start from ----
    Scratch sc((size_t)p.idat_len + 80, (size_t)j.h * col_blocks * dec::kWinWords, sub_total, (size_t)j.nseg * ((j.bpl + 3) / 4));
    const size_t o_lut = sc.carve(dec::kLutDwords * 4), o_job = sc.carve(sizeof(DecJob)), o_small = sc.carve(256);
    DecArrays d;
    if ((rc = sc.place(e, d))) return rc;
    uint8_t *const base = e->d_decode.p, *const sm = base + o_small; // status, eob index | carry | unfilter piece | cbpre[2], order[1]
    uint32_t *d_lut = (uint32_t *)(base + o_lut), *d_status = (uint32_t *)sm, *d_eob = d_status + 1, *d_words = (uint32_t *)(sm + 48);
    DecJob *d_job = (DecJob *)(base + o_job);
    DecCarry *d_carry = (DecCarry *)(sm + 16);
    j.z = d.z, j.win = d.win, j.lut = d_lut, j.out = e->d_stage_in.p, j.segsum = (uint32_t *)d.seg;
    struct Small { // (one upload for the few words the kernels start from)
        uint32_t status, eob;
        uint32_t pad0[2];
        DecCarry carry;
        DecUnfPiece piece;
        uint32_t cbpre[2], order[1];
    } small = {0, j.n_sub, {0, 0}, {0, 0, 0}, {0, 0, 1, 0}, {0, (uint32_t)col_blocks}, {0}};
    static_assert(sizeof(Small) <= 256 && offsetof(Small, carry) == 16 && offsetof(Small, piece) == 32 && offsetof(Small, cbpre) == 48, "layout of the small words");
    HIP_TRY(hipMemcpyAsync(d_status, &small, sizeof small, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_lut, lut.data(), dec::kLutDwords * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_job, &j, sizeof j, hipMemcpyHostToDevice, s));
    DecUnfPlan plan;
    plan.pieces = (DecUnfPiece *)(sm + 32), plan.cbpre = d_words, plan.order = d_words + 2, plan.n_pieces = 1, plan.total_items = j.nseg * (uint32_t)col_blocks, plan.n_files = 1, plan.pad_ = 0;
    const uint32_t epoch = next_epoch(e); // (one epoch for all of this file's unfilter launches: later segments look back at earlier launches' sums)
    // ---- pieces: whole blocks of subsequences; a piece's kernels read up to 64 bytes behind its last block (a token's window, the pad) ----
    constexpr uint32_t kMaxPieces = 16;
    // (a piece costs ~100 us of launches and a host round trip: pieces of 6 MiB, but at least four of them -- measured on one box,
    //  2 / 3 / 4 / 6 MiB pieces: 8K RGBA 3.06 / 3.05 / 3.01 / 2.99 ms, an 11 MP photograph 2.46 / 1.90 / 1.53 / 1.38, 4K RGBA 1.03 / 0.95 / 1.02 / 1.06)
    const uint32_t np_want = std::max(4u, p.idat_len / (6u << 20));
    const uint32_t np = std::max(1u, std::min<uint32_t>({kMaxPieces, n_blocks, np_want}));
    // The first pieces are small -- a quarter, then half a share: the first rows are on their way down after 1 MiB instead of 4,
    // and the download, which takes longer than everything else together, starts that much earlier.
    uint32_t blk_end[kMaxPieces], byte_end[kMaxPieces];
    for (uint32_t k = 0; k < np; k++) {
        // shares: 1/4, 1/2, 1, 1, ... of (np - 1.25) equal ones
        const double done = np >= 4 ? (k == 0 ? 0.25 : (k == 1 ? 0.75 : (double)k - 0.25)) / ((double)np - 1.25) : (double)(k + 1) / np;
        blk_end[k] = k + 1 == np ? n_blocks : std::min<uint32_t>(n_blocks, std::max<uint32_t>(k + 1, (uint32_t)(n_blocks * done)));
        const uint64_t end_bit = j.first_bit + (uint64_t)blk_end[k] * kDecSubBlock * kSubBits;
        byte_end[k] = k + 1 == np ? p.idat_len : (uint32_t)std::min<uint64_t>(p.idat_len, (end_bit >> 3) + 64);
    }
    hipEvent_t *const ev_up = e->dec_ev, *const ev_carry = e->dec_ev2, *const ev_rows = e->dec_ev3;
    for (uint32_t k = 0; k < np; k++)
        for (hipEvent_t *ev : {ev_up, ev_carry, ev_rows})
            if (!ev[k]) HIP_TRY(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
    if ((rc = e->h_dec_fetch.ensure(kMaxPieces * sizeof(DecCarry) + 64))) return rc;
    DecCarry *h_carry = (DecCarry *)e->h_dec_fetch.p;
    uint32_t *h_status = (uint32_t *)(h_carry + kMaxPieces);
    if (!e->workers) e->workers = new HostWorkers();
    std::mutex mu;
    std::condition_variable cv;
    uint32_t issued = 0, rows_ready = 0; // pieces whose upload is enqueued; pieces whose finished rows may go down
    uint32_t row_end[kMaxPieces] = {};   // rows [row_end[k - 1], row_end[k]) are complete behind piece k's unfilter launch
    hipError_t copy_err = hipSuccess;
    bool stop = false;
    const uint8_t *zsrc = png + p.idat_ofs + 8;
    struct Joiner { // (every way out waits for the copy threads: they work on this frame's variables)
        Worker &a, &b;
        std::mutex &mu;
        std::condition_variable &cv;
        bool &stop;
        ~Joiner()
        {
            {
                std::lock_guard<std::mutex> lk(mu);
                stop = true;
            }
            cv.notify_all();
            a.wait(), b.wait();
        }
    } joiner{e->workers->up, e->workers->down, mu, cv, stop};
    e->workers->up.start([&] {
        hipError_t err = hipSetDevice(e->device);
        for (uint32_t k = 0; k < np; k++) {
            const uint32_t from = k ? byte_end[k - 1] : 0;
            if (err == hipSuccess && byte_end[k] > from) err = hipMemcpyAsync(d.z + from, zsrc + from, byte_end[k] - from, hipMemcpyHostToDevice, s_up);
            if (err == hipSuccess) err = hipEventRecord(ev_up[k], s_up);
            std::lock_guard<std::mutex> lk(mu);
            if (err != hipSuccess) copy_err = err;
            issued = k + 1;
            cv.notify_all();
        }
    });
    e->workers->down.start([&] {
        hipError_t err = hipSetDevice(e->device);
        for (uint32_t k = 0; k < np; k++) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return rows_ready > k || stop; });
                if (rows_ready <= k) return;
            }
            const uint32_t r0 = k ? row_end[k - 1] : 0, r1 = row_end[k];
            if (err == hipSuccess && r1 > r0) {
                err = hipStreamWaitEvent(s_down, ev_rows[k], 0);
                if (err == hipSuccess) err = hipMemcpyAsync(out + (size_t)r0 * os, e->d_stage_in.p + (size_t)r0 * os, (size_t)(r1 - r0) * os, hipMemcpyDeviceToHost, s_down);
            }
            if (err != hipSuccess) {
                std::lock_guard<std::mutex> lk(mu);
                copy_err = err;
            }
        }
        if (err == hipSuccess) err = hipStreamSynchronize(s_down);
        if (err != hipSuccess) {
            std::lock_guard<std::mutex> lk(mu);
            copy_err = err;
        }
    });
    // ---- the calling thread: piece k's kernels are enqueued, then piece k - 1 is closed (its byte count read, the rows it completed
    //      sent through the Up filter's undoing and handed to the downloader): the GPU always has the next piece's kernels queued ----
    uint32_t segs_done = 0;
    for (uint32_t k = 0; k <= np; k++) {
        if (k < np) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return issued > k; });
                if (copy_err != hipSuccess) return fail(FPNG_AMD_ERR_HIP, "upload of the file", copy_err);
            }
            HIP_TRY(hipStreamWaitEvent(s, ev_up[k], 0));
            const uint32_t a = k ? blk_end[k - 1] : 0, b = blk_end[k];
            if (b > a) {
                for (uint32_t r = 0; r <= kBorderRounds; r++) launch_dec_sync(s, resident, d_job, 1, a, b - a, sub_total, r, d.sub, d.recs, d_status + 2, d_status + 3);
                launch_dec_offsets_range(s, d_job, 0, a, b, k + 1 == np, sub_total, d.sub, d.recs, d.block_off, d_status, d_eob, d_carry);
            }
            HIP_TRY(hipMemcpyAsync(&h_carry[k], d_carry, sizeof(DecCarry), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipEventRecord(ev_carry[k], s));
        }
        if (k >= 1) {
            const uint32_t q = k - 1;
            HIP_TRY(hipEventSynchronize(ev_carry[q]));
            const uint64_t bytes = h_carry[q].bytes;
            uint32_t rows = (uint32_t)std::min<uint64_t>(bytes / ((uint64_t)j.bpl + 1), p.h);
            uint32_t segs = rows / kDecUnfRows; // whole segments only -- or, behind the last piece, everything
            if (q + 1 == np) segs = j.nseg, rows = p.h;
            else rows = segs * kDecUnfRows;
            if (s_unf != s) HIP_TRY(hipStreamWaitEvent(s_unf, ev_carry[q], 0)); // (piece q's rows are in the records of the subsequences placed so far; the small words went up in front of piece 0)
            // (the rows of these segments lie in the output of the subsequences placed so far: the tiles' walks stop there -- what the
            //  next piece's kernels are writing behind it meanwhile is not theirs to read)
            const DecPlaced placed = {d.sub, d.block_off, d_eob, blk_end[q] * kDecSubBlock};
            if (segs > segs_done) launch_dec_unfilter(s_unf, d_job, plan, placed, segs_done * (uint32_t)col_blocks, (segs - segs_done) * (uint32_t)col_blocks, d_status, epoch, s_unf != s);
            segs_done = std::max(segs_done, segs);
            HIP_TRY(hipEventRecord(ev_rows[q], s_unf));
            {
                std::lock_guard<std::mutex> lk(mu);
                row_end[q] = std::max(rows, q ? row_end[q - 1] : 0u);
                rows_ready = q + 1;
            }
            cv.notify_all();
        }
    }
    HIP_TRY(hipGetLastError());
    if (s_unf != s) HIP_TRY(hipStreamWaitEvent(s, ev_rows[np - 1], 0)); // (the last rows' filter literals are part of the status)
    HIP_TRY(hipMemcpyAsync(h_status, d_status, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    e->workers->down.wait();
    if (copy_err != hipSuccess) return fail(FPNG_AMD_ERR_HIP, "copies of the streamed decode", copy_err);
    const int st = dec_result(*h_status);
    *redo = st == FPNG_AMD_DECODE_UNDECIDED; // (fpng_amd_decode_batch adds rounds)
    if (!*redo) result->status = st;
    return FPNG_AMD_OK;
}

} // namespace

extern "C" int fpng_amd_encoder_set_decode_verify(fpng_amd_encoder *e, uint32_t flags)
{
    if (!e) return fail(FPNG_AMD_ERR_INVALID_ARG, "null encoder");
    if (flags & ~(uint32_t)(FPNG_AMD_VERIFY_CRC32 | FPNG_AMD_VERIFY_ADLER32)) return fail(FPNG_AMD_ERR_INVALID_ARG, "unknown FPNG_AMD_VERIFY_* bits");
    e->dec_verify = flags;
    return FPNG_AMD_OK;
}

extern "C" uint32_t fpng_amd_encoder_decode_verify(const fpng_amd_encoder *e) { return e ? e->dec_verify : 0u; }

extern "C" int fpng_amd_decode_last_phase_ms(fpng_amd_encoder *e, float ms[FPNG_AMD_NUM_DECODE_PHASES])
{
    if (!e || !ms) return fail(FPNG_AMD_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < FPNG_AMD_NUM_DECODE_PHASES; i++) ms[i] = 0.f;
    if (!e->dec_prof_recorded) return FPNG_AMD_OK;
    HIP_TRY(hipEventSynchronize(e->dec_prof_ev[4]));
    for (int i = 0; i < FPNG_AMD_NUM_DECODE_PHASES; i++) HIP_TRY(hipEventElapsedTime(&ms[i], e->dec_prof_ev[i], e->dec_prof_ev[i + 1]));
    return FPNG_AMD_OK;
}

extern "C" int fpng_amd_decode_batch(fpng_amd_encoder *e, const fpng_amd_png *files, uint32_t n, uint32_t desired, fpng_amd_decode_result *results)
{
    return decode_files(e, files, n, desired, results, false);
}

extern "C" int fpng_amd_decode_batch_device(fpng_amd_encoder *e, const fpng_amd_png *files, uint32_t n, uint32_t desired, fpng_amd_decode_result *results)
{
    return decode_files(e, files, n, desired, results, true);
}

namespace {
// fpng_amd_decode_batch(_device)_ex: the rules that need no file are checked here, for every file, before anything is done; the
// pitch's and the room's once a file's header is known (parse_files)
int decode_files_ex(fpng_amd_encoder *e, const fpng_amd_png_ex *files, uint32_t n, fpng_amd_decode_result *results, bool device_data)
{
    if (!e || !files || !n || !results) return fail(FPNG_AMD_ERR_INVALID_ARG, "null/empty batch");
    std::vector<fpng_amd_png> plain(n);
    for (uint32_t i = 0; i < n; i++) {
        const fpng_amd_png_ex &x = files[i];
        if (x.format >= FPNG_AMD_SRC_COUNT) return fail(FPNG_AMD_ERR_INVALID_ARG, "unknown destination format");
        if (kDstFormats[x.format].bytes == 4 && (((uintptr_t)x.d_pixels & 3) || (x.row_pitch & 3)))
            return fail(FPNG_AMD_ERR_INVALID_ARG, "4-byte destination pixels need d_pixels and row_pitch to be multiples of 4");
        if (x.row_pitch <= -(int64_t)0x80000000ll || x.row_pitch >= (int64_t)0x80000000ll) return fail(FPNG_AMD_ERR_INVALID_ARG, "|row_pitch| >= 2^31");
        plain[i].data = x.data, plain[i].size = x.size, plain[i].reserved = 0, plain[i].d_pixels = x.d_pixels, plain[i].pixels_cap = x.pixels_cap;
    }
    return decode_files(e, plain.data(), n, 0, results, device_data, files);
}
} // namespace

namespace {
static_assert(sizeof(fpng_amd_png_planar) == 48 && offsetof(fpng_amd_png_planar, d_pixels) == 16 && offsetof(fpng_amd_png_planar, pixels_cap) == 40, "fpng_amd_png_planar layout");
// fpng_amd_decode_batch(_device)_planar: as decode_files_ex -- the rules that need no file here, the pitches' and the room's in parse_files
// fmt: fpng_amd_decode_batch(_device)_planar_float's format (its planes hold elements of fmt->dtype, the pitches stay bytes), else NULL
static_assert(sizeof(fpng_amd_float_format) == 40 && sizeof(DecFloat) == 40 && offsetof(DecFloat, scale) == offsetof(fpng_amd_float_format, scale) &&
                  offsetof(DecFloat, bias) == offsetof(fpng_amd_float_format, bias), "fpng_amd_float_format layout");
static_assert(FPNG_AMD_F32 == 0 && FPNG_AMD_F16 == 1 && FPNG_AMD_BF16 == 2 && kDecFloatTypes == 3, "the kernels' element types");
// crops: fpng_amd_decode_batch(_device)_planar_crop's, a crop per file (the destinations are then the crops' sizes), else NULL
static_assert(sizeof(fpng_amd_crop) == 16 && sizeof(DecCrop) == 16 && offsetof(fpng_amd_crop, w) == offsetof(DecCrop, w), "fpng_amd_crop layout");
static_assert(sizeof(fpng_amd_resize) == 16 && offsetof(fpng_amd_resize, flags) == 8 && FPNG_AMD_RESIZE_MIRROR == kResizeMirror, "fpng_amd_resize layout");
// sizes: fpng_amd_decode_batch(_device)_planar_resize's, an output size per file (with crops; the destinations are then those sizes).
// The records' own rules, which need no file, no encoder and no device
int check_resize_records(const fpng_amd_crop *crops, const fpng_amd_resize *sizes, uint32_t n)
{
    for (uint32_t i = 0; crops && sizes && i < n; i++) {
        const fpng_amd_resize &z = sizes[i];
        if (!crops[i].w || !crops[i].h) return fail(FPNG_AMD_ERR_INVALID_ARG, "an empty crop (w or h is 0)");
        if (!z.out_w || !z.out_h) return fail(FPNG_AMD_ERR_INVALID_ARG, "an empty output size (out_w or out_h is 0)");
        if (z.reserved) return fail(FPNG_AMD_ERR_INVALID_ARG, "fpng_amd_resize::reserved must be 0");
        if (z.flags & ~(uint32_t)FPNG_AMD_RESIZE_MIRROR) return fail(FPNG_AMD_ERR_INVALID_ARG, "unknown fpng_amd_resize::flags bits");
        if (!resize_scale_ok(crops[i].w, z.out_w) || !resize_scale_ok(crops[i].h, z.out_h))
            return fail(FPNG_AMD_ERR_INVALID_ARG, "a crop of more than 32 x its output size (w <= 32 * out_w and h <= 32 * out_h)");
    }
    return FPNG_AMD_OK;
}
static_assert(sizeof(fpng_amd_resize_view) == 32 && offsetof(fpng_amd_resize_view, x) == 8 && offsetof(fpng_amd_resize_view, flags) == 24 && offsetof(fpng_amd_resize_view, filter) == 28,
              "fpng_amd_resize_view layout");
static_assert(FPNG_AMD_FILTER_BILINEAR == kResizeBilinear && FPNG_AMD_FILTER_BICUBIC == kResizeBicubic, "the kernel's filters");
// views: fpng_amd_decode_batch(_device)_planar_resize_view's, a view per file (with crops; the destinations are then the views'
// windows).  As check_resize_records: no file, no encoder, no device
// resamples (or NULL): the views' RESAMPLE records, which have been judged -- the scale limit is the effective filter's
int check_view_records(const fpng_amd_crop *crops, const fpng_amd_resize_view *views, uint32_t n, const fpng_amd_view_resample *resamples = nullptr)
{
    for (uint32_t i = 0; crops && views && i < n; i++) {
        const fpng_amd_resize_view &z = views[i];
        if (!crops[i].w || !crops[i].h) return fail(FPNG_AMD_ERR_INVALID_ARG, "an empty crop (w or h is 0)");
        if (!z.full_w || !z.full_h) return fail(FPNG_AMD_ERR_INVALID_ARG, "an empty full size (full_w or full_h is 0)");
        if (!z.w || !z.h) return fail(FPNG_AMD_ERR_INVALID_ARG, "an empty window (w or h is 0)");
        if ((uint64_t)z.x + z.w > z.full_w || (uint64_t)z.y + z.h > z.full_h) return fail(FPNG_AMD_ERR_INVALID_ARG, "a window that leaves the full size (x + w <= full_w and y + h <= full_h)");
        if (z.flags & ~(uint32_t)FPNG_AMD_RESIZE_MIRROR) return fail(FPNG_AMD_ERR_INVALID_ARG, "unknown fpng_amd_resize_view::flags bits");
        if (z.filter >= kResizeFilters) return fail(FPNG_AMD_ERR_INVALID_ARG, "unknown filter (FPNG_AMD_FILTER_BILINEAR, _BICUBIC)");
        const uint32_t filter = view_filter(z, resamples ? resamples + i : nullptr);
        if (filter >= kResizeFilters && (!resize_scale_ok(crops[i].w, z.full_w, filter) || !resize_scale_ok(crops[i].h, z.full_h, filter)))
            return fail(FPNG_AMD_ERR_INVALID_ARG, filter == kResizeLanczos ? "a crop past the Lanczos limit (3 * w <= 32 * full_w and 3 * h <= 32 * full_h)"
                                                                            : "a crop of more than 32 x its full size (nearest, box, Hamming: w <= 32 * full_w and h <= 32 * full_h)");
        if (filter < kResizeFilters && (!resize_scale_ok(crops[i].w, z.full_w, z.filter) || !resize_scale_ok(crops[i].h, z.full_h, z.filter)))
            return fail(FPNG_AMD_ERR_INVALID_ARG, z.filter == kResizeBicubic ? "a crop of more than 16 x its full size (bicubic: w <= 16 * full_w and h <= 16 * full_h)"
                                                                              : "a crop of more than 32 x its full size (bilinear: w <= 32 * full_w and h <= 32 * full_h)");
    }
    return FPNG_AMD_OK;
}
// rq: what the call carries besides its files (ViewRequest: nothing, the float format, crops, one view per file, or the views calls'
// records, which decode_files_views has judged and normalised: crops and views then hold a record per view, and the destinations,
// which `files` leave empty, are dests' or hwc's)
int decode_files_planar(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, fpng_amd_decode_result *results, bool device_data, const ViewRequest &rq)
{
    if (!e || !files || !n || !results) return fail(FPNG_AMD_ERR_INVALID_ARG, "null/empty batch");
    for (uint32_t i = 0; rq.crops && !rq.view_count && i < n; i++)
        if (!rq.crops[i].w || !rq.crops[i].h) return fail(FPNG_AMD_ERR_INVALID_ARG, "an empty crop (w or h is 0)");
    DecFloat flt; // (views: their entry points have judged them -- check_resize_records / check_view_records)
    uint32_t elem;
    if (int rc = check_float_format(rq.fmt, flt, elem)) return rc;
    std::vector<fpng_amd_png> plain(n);
    for (uint32_t i = 0; i < n; i++) {
        const fpng_amd_png_planar &x = files[i];
        if (x.num_chans != 3 && x.num_chans != 4) return fail(FPNG_AMD_ERR_INVALID_ARG, "num_chans must be 3 or 4");
        if (((uintptr_t)x.d_pixels | (uint64_t)x.row_pitch | (uint64_t)x.plane_pitch) & (elem - 1))
            return fail(FPNG_AMD_ERR_INVALID_ARG, "d_pixels, row_pitch and plane_pitch must be multiples of the element size");
        if (x.row_pitch <= -(int64_t)0x80000000ll || x.row_pitch >= (int64_t)0x80000000ll) return fail(FPNG_AMD_ERR_INVALID_ARG, "|row_pitch| >= 2^31");
        plain[i].data = x.data, plain[i].size = x.size, plain[i].reserved = 0, plain[i].d_pixels = x.d_pixels, plain[i].pixels_cap = x.pixels_cap;
    }
    uint64_t n_views = 0;
    for (uint32_t i = 0; rq.view_count && i < n; i++) n_views += rq.view_count[i];
    if (int rc = check_view_dests(rq, n_views, elem)) return rc;
    return decode_files(e, plain.data(), n, 0, results, device_data, nullptr, files, rq.fmt ? &flt : nullptr, rq);
}
// fpng_amd_decode_batch(_device)_planar_views: what needs no file, no encoder and no device is judged first, as in the view call
static_assert(sizeof(fpng_amd_view_dest) == 32 && offsetof(fpng_amd_view_dest, row_pitch) == 8 && offsetof(fpng_amd_view_dest, pixels_cap) == 24, "fpng_amd_view_dest layout");
// hwc in the place of dests: fpng_amd_decode_batch(_device)_hwc_views's destinations, whose own rules -- pixel_elems, flags -- are judged here too
static_assert(sizeof(fpng_amd_view_dest_hwc) == 32 && offsetof(fpng_amd_view_dest_hwc, row_pitch) == 8 && offsetof(fpng_amd_view_dest_hwc, pixel_elems) == 16 &&
                  offsetof(fpng_amd_view_dest_hwc, flags) == 20 && offsetof(fpng_amd_view_dest_hwc, pixels_cap) == 24 && FPNG_AMD_HWC_REVERSED == kHwcReversed,
              "fpng_amd_view_dest_hwc layout");
// fpng_amd_decode_batch(_device)_planar_views_color / _hwc_views_color: the matrices are judged first -- a record per view, the sum of
// the counts (those the views call refuses: its own message, below) -- then everything the views call judges
static_assert(sizeof(fpng_amd_view_color) == 64 && offsetof(fpng_amd_view_color, flags) == 48 && offsetof(fpng_amd_view_color, reserved) == 52, "fpng_amd_view_color layout");
int check_color_records(const fpng_amd_view_color *colors, uint64_t total)
{
    for (uint64_t v = 0; v < total; v++) {
        const fpng_amd_view_color &c = colors[v];
        for (int k = 0; k < 12; k++)
            if (!std::isfinite(c.m[k / 4][k % 4]) || std::fabs(c.m[k / 4][k % 4]) > kColorMaxEntry)
                return fail(FPNG_AMD_ERR_INVALID_ARG, "fpng_amd_view_color::m: every entry must be finite and at most 65536 in magnitude");
        if (c.flags) return fail(FPNG_AMD_ERR_INVALID_ARG, "unknown fpng_amd_view_color::flags bits (must be 0)");
        if (c.reserved[0] | c.reserved[1] | c.reserved[2]) return fail(FPNG_AMD_ERR_INVALID_ARG, "fpng_amd_view_color::reserved must be 0");
    }
    return FPNG_AMD_OK;
}
// fpng_amd_decode_batch(_device)_planar_views_post / _hwc_views_post: the post records are judged first, then the matrices (NULL: the
// identity for every view), then everything the views call judges.  w, h: the view's window, where it is known (else 0: not judged)
const char *check_post_record(const fpng_amd_view_post &p, uint32_t w, uint32_t h)
{
    if (p.flags & ~(uint32_t)(kPostBlur | kPostSolarize | kPostPosterize)) return "unknown fpng_amd_view_post::flags bits (FPNG_AMD_POST_BLUR, _SOLARIZE, _POSTERIZE)";
    if (p.reserved[0] | p.reserved[1]) return "fpng_amd_view_post::reserved must be 0";
    if (p.flags & kPostBlur) {
        if (!p.blur_radius || p.blur_radius > kPostMaxRadius) return "fpng_amd_view_post::blur_radius must be 1 .. 16 with FPNG_AMD_POST_BLUR";
        if (!std::isfinite(p.blur_sigma) || !(p.blur_sigma > 0.0)) return "fpng_amd_view_post::blur_sigma must be finite and > 0 with FPNG_AMD_POST_BLUR";
        if (w && h && p.blur_radius >= std::min(w, h)) return "fpng_amd_view_post::blur_radius must be below the window's w and h (one reflection at the border)";
    } else if (p.blur_radius || p.blur_sigma != 0.0) // (a NaN is not 0)
        return "fpng_amd_view_post::blur_radius and blur_sigma must be 0 without FPNG_AMD_POST_BLUR";
    if (p.solarize_threshold > 255u) return "fpng_amd_view_post::solarize_threshold must be 0 .. 255";
    if (p.posterize_bits > 8u) return "fpng_amd_view_post::posterize_bits must be 0 .. 8";
    if (p.solarize_threshold && !(p.flags & kPostSolarize)) return "fpng_amd_view_post::solarize_threshold must be 0 without FPNG_AMD_POST_SOLARIZE";
    if (p.posterize_bits && !(p.flags & kPostPosterize)) return "fpng_amd_view_post::posterize_bits must be 0 without FPNG_AMD_POST_POSTERIZE";
    return nullptr;
}
static_assert(sizeof(fpng_amd_view_post) == 32 && offsetof(fpng_amd_view_post, blur_sigma) == 8 && offsetof(fpng_amd_view_post, solarize_threshold) == 16 &&
                  offsetof(fpng_amd_view_post, reserved) == 24 && FPNG_AMD_POST_BLUR == kPostBlur && FPNG_AMD_POST_SOLARIZE == kPostSolarize &&
                  FPNG_AMD_POST_POSTERIZE == kPostPosterize && FPNG_AMD_BLUR_MAX_RADIUS == kPostMaxRadius,
              "fpng_amd_view_post layout");
// The views calls (fpng_amd_decode_batch(_device)_{planar,hwc}_views and their _color, _post, _warp, _tone, _enhance siblings): what
// needs no file, no encoder and no device is judged first, in this order -- the record array that names the family (the arrays in
// front of it may be NULL: the identity, no flags, no warp, no op), the destinations, every stage's records from the last stage to
// the first, then what the plain views call judges: the arrays, the counts, the views, the files' empty destination fields and the
// channels-last destinations' own rules.  used: which stages some view really uses (normalise_views)
// the RESAMPLE record's own rules
const char *check_resample_record(const fpng_amd_view_resample &r)
{
    if (r.filter > FPNG_AMD_RESAMPLE_LANCZOS) return "unknown fpng_amd_view_resample::filter (FPNG_AMD_RESAMPLE_NEAREST, _BOX, _HAMMING, _LANCZOS; 0: the view's own)";
    if (r.flags) return "fpng_amd_view_resample::flags must be 0";
    if (r.reserved[0] | r.reserved[1]) return "fpng_amd_view_resample::reserved must be 0";
    return nullptr;
}
static_assert(sizeof(fpng_amd_view_resample) == 16 && offsetof(fpng_amd_view_resample, flags) == 4 && offsetof(fpng_amd_view_resample, reserved) == 8, "fpng_amd_view_resample layout");
// (StagesUsed, ViewDefaults and the functions below: declared in view_request.h, which png_views_api.cpp judges its request through)
} // namespace

int fpng_amd::check_float_format(const fpng_amd_float_format *fmt, DecFloat &flt, uint32_t &elem)
{
    flt = {}, elem = 1;
    if (!fmt) return FPNG_AMD_OK;
    if (fmt->dtype >= kDecFloatTypes) return fail(FPNG_AMD_ERR_INVALID_ARG, "unknown element type (FPNG_AMD_F32, _F16, _BF16)");
    if (fmt->reserved) return fail(FPNG_AMD_ERR_INVALID_ARG, "fpng_amd_float_format::reserved must be 0");
    for (int c = 0; c < 4; c++)
        if (!std::isfinite(fmt->scale[c]) || !std::isfinite(fmt->bias[c])) return fail(FPNG_AMD_ERR_INVALID_ARG, "scale and bias must be finite");
    flt.dtype = fmt->dtype, elem = dec_float_bytes(fmt->dtype);
    std::memcpy(flt.scale, fmt->scale, sizeof flt.scale), std::memcpy(flt.bias, fmt->bias, sizeof flt.bias);
    return FPNG_AMD_OK;
}
int fpng_amd::check_view_dests(const ViewRequest &rq, uint64_t n_views, uint32_t elem)
{
    for (uint64_t v = 0; rq.hwc && v < n_views; v++) { // (a channels-last destination's twins of the two rules below)
        const fpng_amd_view_dest_hwc &x = rq.hwc[v];
        if (((uintptr_t)x.d_pixels | (uint64_t)x.row_pitch) & (elem - 1)) return fail(FPNG_AMD_ERR_INVALID_ARG, "d_pixels and row_pitch must be multiples of the element size");
        if (x.row_pitch <= -(int64_t)0x80000000ll || x.row_pitch >= (int64_t)0x80000000ll) return fail(FPNG_AMD_ERR_INVALID_ARG, "|row_pitch| >= 2^31");
    }
    for (uint64_t v = 0; rq.dests && v < n_views; v++) { // (a file's own destination words, for every view's destination: decode_files_planar)
        const fpng_amd_view_dest &x = rq.dests[v];
        if (((uintptr_t)x.d_pixels | (uint64_t)x.row_pitch | (uint64_t)x.plane_pitch) & (elem - 1))
            return fail(FPNG_AMD_ERR_INVALID_ARG, "d_pixels, row_pitch and plane_pitch must be multiples of the element size");
        if (x.row_pitch <= -(int64_t)0x80000000ll || x.row_pitch >= (int64_t)0x80000000ll) return fail(FPNG_AMD_ERR_INVALID_ARG, "|row_pitch| >= 2^31");
    }
    return FPNG_AMD_OK;
}
int fpng_amd::check_views_request(const fpng_amd_png_planar *files, uint32_t n, const ViewRequest &rq, const fpng_amd_decode_result *results, StagesUsed &used)
{
    const char *const null_array = "null files, view_count, crops, views, dests or results";
    switch (rq.family) {
    case ViewFamily::Resample: if (!rq.resamples) return fail(FPNG_AMD_ERR_INVALID_ARG, "null resamples"); break;
    case ViewFamily::Alpha: if (!rq.alphas) return fail(FPNG_AMD_ERR_INVALID_ARG, "null alphas"); break;
    case ViewFamily::Enhance: if (!rq.enhances) return fail(FPNG_AMD_ERR_INVALID_ARG, "null enhances"); break;
    case ViewFamily::Tone: if (!rq.tones) return fail(FPNG_AMD_ERR_INVALID_ARG, "null tones"); break;
    case ViewFamily::Warp: if (!rq.warps) return fail(FPNG_AMD_ERR_INVALID_ARG, "null warps"); break;
    case ViewFamily::Post: if (!rq.posts) return fail(FPNG_AMD_ERR_INVALID_ARG, "null posts"); break;
    case ViewFamily::Color: if (!rq.colors) return fail(FPNG_AMD_ERR_INVALID_ARG, "null colors"); break;
    case ViewFamily::Plain: break;
    }
    if (rq.family != ViewFamily::Plain && !rq.dests && !rq.hwc) return fail(FPNG_AMD_ERR_INVALID_ARG, null_array);
    const uint32_t *const view_count = rq.view_count;
    const fpng_amd_resize_view *const views = rq.views;
    uint64_t total = 0;
    bool counts_ok = view_count != nullptr; // (else the counts are refused below, and no stage's record is read)
    for (uint32_t i = 0; counts_ok && i < n; i++) counts_ok = view_count[i] && (total += view_count[i]) <= UINT32_MAX;
    used.total = counts_ok ? total : 0;
    for (uint64_t v = 0; rq.resamples && v < used.total; v++)
        if (const char *why = check_resample_record(rq.resamples[v])) return fail(FPNG_AMD_ERR_INVALID_ARG, why);
    for (uint64_t v = 0; rq.alphas && v < used.total; v++) {
        if (const char *why = check_alpha_record(rq.alphas[v])) return fail(FPNG_AMD_ERR_INVALID_ARG, why);
        if (rq.resamples && rq.resamples[v].filter == FPNG_AMD_RESAMPLE_NEAREST && rq.alphas[v].op == kAlphaPremultiplied)
            return fail(FPNG_AMD_ERR_INVALID_ARG, "a PREMULTIPLIED alpha record on a view whose RESAMPLE filter is NEAREST (Pillow does not premultiply for nearest: the view without an alpha op is its result)");
    }
    for (uint32_t i = 0, v = 0; rq.enhances && counts_ok && i < n; i++) // (the planes of a view's destination: its file's num_chans)
        for (const uint32_t end = v + view_count[i]; v < end; v++) {
            if (const char *why = check_enhance_record(rq.enhances[v], files ? files[i].num_chans : 0u)) return fail(FPNG_AMD_ERR_INVALID_ARG, why);
            used.enhance |= rq.enhances[v].op != 0;
        }
    for (uint64_t v = 0; rq.tones && v < used.total; v++) { // (w, h: the view's window, where it is known -- else 0: not judged)
        if (const char *why = check_tone_record(rq.tones[v], views ? views[v].w : 0u, views ? views[v].h : 0u)) return fail(FPNG_AMD_ERR_INVALID_ARG, why);
        used.tone |= rq.tones[v].op != 0;
    }
    for (uint64_t v = 0; rq.warps && v < used.total; v++) {
        if (const char *why = check_warp_record(rq.warps[v], views ? views[v].w : 0u, views ? views[v].h : 0u)) return fail(FPNG_AMD_ERR_INVALID_ARG, why);
        used.warp |= warp_moves(rq.warps[v]);
    }
    for (uint64_t v = 0; rq.posts && v < used.total; v++) {
        if (const char *why = check_post_record(rq.posts[v], views ? views[v].w : 0u, views ? views[v].h : 0u)) return fail(FPNG_AMD_ERR_INVALID_ARG, why);
        used.post |= rq.posts[v].flags != 0;
    }
    if (rq.colors)
        if (int rc = check_color_records(rq.colors, used.total)) return rc;
    if (!files || !view_count || !rq.crops || !views || !(rq.dests || rq.hwc || rq.yuv) || !results) return fail(FPNG_AMD_ERR_INVALID_ARG, null_array);
    total = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!view_count[i]) return fail(FPNG_AMD_ERR_INVALID_ARG, "a view_count of 0 (every file has at least one view)");
        if ((total += view_count[i]) > UINT32_MAX) return fail(FPNG_AMD_ERR_INVALID_ARG, "the sum of view_count does not fit 32 bits");
    }
    if (int rc = check_view_records(rq.crops, views, (uint32_t)total, rq.resamples)) return rc;
    for (uint32_t i = 0; i < n; i++)
        if (files[i].d_pixels || files[i].row_pitch || files[i].plane_pitch || files[i].pixels_cap)
            return fail(FPNG_AMD_ERR_INVALID_ARG, "fpng_amd_png_planar::d_pixels, row_pitch, plane_pitch and pixels_cap must be NULL / 0: the destinations are the fpng_amd_view_dest records");
    for (uint32_t i = 0, v = 0; rq.hwc && i < n; i++)
        for (const uint32_t end = v + view_count[i]; v < end; v++) {
            const uint32_t px = rq.hwc[v].pixel_elems, c = files[i].num_chans;
            if (px && px != c && !(px == 4 && c == 3)) return fail(FPNG_AMD_ERR_INVALID_ARG, "fpng_amd_view_dest_hwc::pixel_elems must be 0, num_chans, or 4 with num_chans = 3");
            if (rq.hwc[v].flags & ~(uint32_t)FPNG_AMD_HWC_REVERSED) return fail(FPNG_AMD_ERR_INVALID_ARG, "unknown fpng_amd_view_dest_hwc::flags bits");
        }
    return FPNG_AMD_OK;
}

// THE normalisation rule of the views calls.  No view with a post flag, a warp that moves, a tone or an enhance op: the request is
// the colour call's (with matrices) or the plain call's (without), which enqueue what they always do.  Otherwise the request is a
// post call's: matrices for every view (the identity where none were given), post records for every view (without flags where none
// were given), and of warps, tones and enhances only the stages that some view uses.  The alpha records are no post stage: they
// travel inside the resize records of whichever call the request becomes, and a request in which no record has an op drops them.
// One op chooses the kernel: a PREMULTIPLIED view divides its colour planes by its alpha plane's result at the store, which a
// kernel with all of a sample's planes in one thread can do and the per-plane kernel of the plain planar call cannot, so a planar
// request with such a view and without matrices becomes the colour call's under identity matrices -- bit for bit the plain call's
// elements, at the plain call's speed (profiles/views_color_timing.txt).  `made` keeps what is supplied here alive
ViewRequest fpng_amd::normalise_views(ViewRequest rq, const StagesUsed &used, ViewDefaults &made)
{
    const auto identity_colors = [&] {
        fpng_amd_view_color one = {};
        one.m[0][0] = one.m[1][1] = one.m[2][2] = 1.0f;
        made.colors.assign((size_t)used.total, one), rq.colors = made.colors.data();
    };
    // (RESAMPLE records without a filter: the request is the alpha call's)
    if (rq.resamples && std::none_of(rq.resamples, rq.resamples + used.total, [](const fpng_amd_view_resample &r) { return r.filter != 0; })) rq.resamples = nullptr;
    if (rq.alphas && std::none_of(rq.alphas, rq.alphas + used.total, [](const fpng_amd_view_alpha &a) { return a.op != 0; })) rq.alphas = nullptr;
    if (rq.alphas && !rq.colors && !rq.hwc && std::any_of(rq.alphas, rq.alphas + used.total, [](const fpng_amd_view_alpha &a) { return a.op == kAlphaPremultiplied; }))
        identity_colors();
    if (!used.post && !used.warp && !used.tone && !used.enhance) {
        rq.posts = nullptr, rq.warps = nullptr, rq.tones = nullptr, rq.enhances = nullptr;
        return rq;
    }
    if (!rq.posts) made.posts.assign((size_t)used.total, fpng_amd_view_post{}), rq.posts = made.posts.data();
    if (!rq.colors) identity_colors();
    if (!used.warp) rq.warps = nullptr;
    if (!used.tone) rq.tones = nullptr;
    if (!used.enhance) rq.enhances = nullptr;
    return rq;
}

int fpng_amd::decode_files_views(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, fpng_amd_decode_result *results, bool device_data, const ViewRequest &asked)
{
    StagesUsed used;
    if (int rc = check_views_request(files, n, asked, results, used)) return rc;
    ViewDefaults made;
    return decode_files_planar(e, files, n, results, device_data, normalise_views(asked, used, made));
}
namespace {

// ---- fpng_amd_decode_batch(_device)_yuv_views (the rule: yuv_store.h) ----
static_assert(sizeof(fpng_amd_yuv_dest) == 40 && offsetof(fpng_amd_yuv_dest, chroma_offset) == 16 && offsetof(fpng_amd_yuv_dest, reserved) == 32 &&
                  sizeof(fpng_amd_yuv_store_format) == 56 && offsetof(fpng_amd_yuv_store_format, m) == 8,
              "fpng_amd_yuv_dest / fpng_amd_yuv_store_format layout");
// fmt of the YUV views call and of its host twin: its depth (the surface's own for 0) into *depth
int check_yuv_store_format(const fpng_amd_yuv_store_format *fmt, uint32_t *depth)
{
    if (fmt->surface >= FPNG_AMD_YUV_SURFACES) return fail(FPNG_AMD_ERR_INVALID_ARG, "unknown surface (FPNG_AMD_YUV_*)");
    if (!(*depth = yuv_store_depth(fmt->surface, fmt->depth)))
        return fail(FPNG_AMD_ERR_INVALID_ARG, "a depth the surface does not have (8-bit surfaces: 0 or 8; 16-bit surfaces: 0, 10, 12 or 16)");
    for (int k = 0; k < 12; k++)
        if (!std::isfinite(fmt->m[k / 4][k % 4]) || std::fabs(fmt->m[k / 4][k % 4]) > kColorMaxEntry)
            return fail(FPNG_AMD_ERR_INVALID_ARG, "fpng_amd_yuv_store_format::m: every entry must be finite and at most 65536 in magnitude");
    return FPNG_AMD_OK;
}
// What needs no file, no encoder and no device is judged first: the format, then what the views call judges, then every surface's
// own words against its view's size; the room (d_luma, surface_cap) is judged per file whose header is accepted (ViewPlan::file_records)
int decode_files_yuv(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops, const fpng_amd_resize_view *views,
                     const fpng_amd_yuv_dest *dests, const fpng_amd_yuv_store_format *fmt, fpng_amd_decode_result *results, bool device_data)
{
    if (!fmt || !dests) return fail(FPNG_AMD_ERR_INVALID_ARG, fmt ? "null dests" : "null fmt");
    ViewRequest rq;
    rq.family = ViewFamily::Plain, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.yuv = dests, rq.yuv_fmt = fmt;
    if (int rc = check_yuv_store_format(fmt, &rq.yuv_depth)) return rc;
    StagesUsed used;
    if (int rc = check_views_request(files, n, rq, results, used)) return rc;
    for (uint32_t i = 0; i < n; i++)
        if (files[i].num_chans != 3) return fail(FPNG_AMD_ERR_INVALID_ARG, "num_chans must be 3 (a 4-channel file's alpha is dropped)");
    for (uint64_t v = 0; v < used.total; v++)
        if (const Refusal no = judge_yuv_dest(dests[v], fmt->surface, views[v].w, views[v].h, false)) return fail(no.code, no.why);
    return decode_files_planar(e, files, n, results, device_data, rq);
}

// the plain resize call's records as views: the whole of the resized crop, bilinear
std::vector<fpng_amd_resize_view> whole_views(const fpng_amd_resize *sizes, uint32_t n)
{
    std::vector<fpng_amd_resize_view> v(n);
    for (uint32_t i = 0; i < n; i++) v[i] = {sizes[i].out_w, sizes[i].out_h, 0, 0, sizes[i].out_w, sizes[i].out_h, sizes[i].flags, FPNG_AMD_FILTER_BILINEAR};
    return v;
}
} // namespace

extern "C" int fpng_amd_decode_batch_planar_float(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    if (!fmt) return fail(FPNG_AMD_ERR_INVALID_ARG, "null format");
    ViewRequest rq;
    rq.fmt = fmt;
    return decode_files_planar(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_planar_float(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    if (!fmt) return fail(FPNG_AMD_ERR_INVALID_ARG, "null format");
    ViewRequest rq;
    rq.fmt = fmt;
    return decode_files_planar(e, files, n, results, true, rq);
}

extern "C" int fpng_amd_decode_batch_planar(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, fpng_amd_decode_result *results)
{
    return decode_files_planar(e, files, n, results, false, ViewRequest());
}

extern "C" int fpng_amd_decode_batch_device_planar(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, fpng_amd_decode_result *results)
{
    return decode_files_planar(e, files, n, results, true, ViewRequest());
}

extern "C" int fpng_amd_decode_batch_planar_crop(fpng_amd_encoder *e, const fpng_amd_png_planar *files, const fpng_amd_crop *crops, uint32_t n, const fpng_amd_float_format *fmt,
                                                 fpng_amd_decode_result *results)
{
    if (!crops) return fail(FPNG_AMD_ERR_INVALID_ARG, "null crops");
    ViewRequest rq;
    rq.fmt = fmt, rq.crops = crops;
    return decode_files_planar(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_planar_crop(fpng_amd_encoder *e, const fpng_amd_png_planar *files, const fpng_amd_crop *crops, uint32_t n, const fpng_amd_float_format *fmt,
                                                        fpng_amd_decode_result *results)
{
    if (!crops) return fail(FPNG_AMD_ERR_INVALID_ARG, "null crops");
    ViewRequest rq;
    rq.fmt = fmt, rq.crops = crops;
    return decode_files_planar(e, files, n, results, true, rq);
}

// (the records are judged first: their refusals need neither an encoder nor a device)
extern "C" int fpng_amd_decode_batch_planar_resize(fpng_amd_encoder *e, const fpng_amd_png_planar *files, const fpng_amd_crop *crops, const fpng_amd_resize *sizes, uint32_t n,
                                                   const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    if (!crops || !sizes) return fail(FPNG_AMD_ERR_INVALID_ARG, crops ? "null sizes" : "null crops");
    if (int rc = check_resize_records(crops, sizes, n)) return rc;
    const std::vector<fpng_amd_resize_view> views = whole_views(sizes, n);
    ViewRequest rq;
    rq.fmt = fmt, rq.crops = crops, rq.views = views.data();
    return decode_files_planar(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_planar_resize(fpng_amd_encoder *e, const fpng_amd_png_planar *files, const fpng_amd_crop *crops, const fpng_amd_resize *sizes, uint32_t n,
                                                          const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    if (!crops || !sizes) return fail(FPNG_AMD_ERR_INVALID_ARG, crops ? "null sizes" : "null crops");
    if (int rc = check_resize_records(crops, sizes, n)) return rc;
    const std::vector<fpng_amd_resize_view> views = whole_views(sizes, n);
    ViewRequest rq;
    rq.fmt = fmt, rq.crops = crops, rq.views = views.data();
    return decode_files_planar(e, files, n, results, true, rq);
}

extern "C" int fpng_amd_decode_batch_planar_resize_view(fpng_amd_encoder *e, const fpng_amd_png_planar *files, const fpng_amd_crop *crops, const fpng_amd_resize_view *views, uint32_t n,
                                                        const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    if (!crops || !views) return fail(FPNG_AMD_ERR_INVALID_ARG, crops ? "null views" : "null crops");
    if (int rc = check_view_records(crops, views, n)) return rc;
    ViewRequest rq;
    rq.fmt = fmt, rq.crops = crops, rq.views = views;
    return decode_files_planar(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_planar_resize_view(fpng_amd_encoder *e, const fpng_amd_png_planar *files, const fpng_amd_crop *crops, const fpng_amd_resize_view *views,
                                                               uint32_t n, const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    if (!crops || !views) return fail(FPNG_AMD_ERR_INVALID_ARG, crops ? "null views" : "null crops");
    if (int rc = check_view_records(crops, views, n)) return rc;
    ViewRequest rq;
    rq.fmt = fmt, rq.crops = crops, rq.views = views;
    return decode_files_planar(e, files, n, results, true, rq);
}

// ---- the views calls: each fills its request by name -- the family, the destinations' layout (dests: planar, hwc: channels-last)
//      and the record arrays its signature takes -- and decode_files_views does the rest ----
extern "C" int fpng_amd_decode_batch_planar_views(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                  const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests, const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Plain, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_planar_views(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                         const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests, const fpng_amd_float_format *fmt,
                                                         fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Plain, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests;
    return decode_files_views(e, files, n, results, true, rq);
}

extern "C" int fpng_amd_decode_batch_yuv_views(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                               const fpng_amd_resize_view *views, const fpng_amd_yuv_dest *dests, const fpng_amd_yuv_store_format *fmt, fpng_amd_decode_result *results)
{
    return decode_files_yuv(e, files, n, view_count, crops, views, dests, fmt, results, false);
}

extern "C" int fpng_amd_decode_batch_device_yuv_views(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                      const fpng_amd_resize_view *views, const fpng_amd_yuv_dest *dests, const fpng_amd_yuv_store_format *fmt,
                                                      fpng_amd_decode_result *results)
{
    return decode_files_yuv(e, files, n, view_count, crops, views, dests, fmt, results, true);
}

// the host twin: yuv_store.h's walk over tight R,G,B bytes into a surface in HOST memory, the format and the record judged as by the call
extern "C" int fpng_amd_yuv_surface(const uint8_t *rgb, uint32_t w, uint32_t h, const fpng_amd_yuv_store_format *fmt, const fpng_amd_yuv_dest *host_dest)
{
    if (!fmt || !host_dest) return fail(FPNG_AMD_ERR_INVALID_ARG, fmt ? "null host_dest" : "null fmt");
    if (!rgb || !w || !h) return fail(FPNG_AMD_ERR_INVALID_ARG, "null rgb or an empty size (w or h is 0)");
    uint32_t depth = 0;
    if (int rc = check_yuv_store_format(fmt, &depth)) return rc;
    int64_t pitch = 0;
    if (const Refusal no = judge_yuv_dest(*host_dest, fmt->surface, w, h, true, &pitch)) return fail(no.code, no.why);
    YuvMatrix f;
    std::memcpy(f.m, fmt->m, sizeof f.m);
    const YuvDepth dp = yuv_depth(fmt->surface, depth);
    uint8_t *const luma = (uint8_t *)host_dest->d_luma;
    switch (fmt->surface) {
    case FPNG_AMD_YUV_NV12: yuv_store_surface<kYuvNV12>(rgb, w, h, f, dp, luma, pitch, host_dest->chroma_offset); break;
    case FPNG_AMD_YUV_P016: yuv_store_surface<kYuvP016>(rgb, w, h, f, dp, luma, pitch, host_dest->chroma_offset); break;
    case FPNG_AMD_YUV_444: yuv_store_surface<kYuv444>(rgb, w, h, f, dp, luma, pitch, host_dest->chroma_offset); break;
    default: yuv_store_surface<kYuv444_16>(rgb, w, h, f, dp, luma, pitch, host_dest->chroma_offset); break;
    }
    return FPNG_AMD_OK;
}

extern "C" int fpng_amd_decode_batch_hwc_views(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                               const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests, const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Plain, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_hwc_views(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                      const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests, const fpng_amd_float_format *fmt,
                                                      fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Plain, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests;
    return decode_files_views(e, files, n, results, true, rq);
}

extern "C" int fpng_amd_decode_batch_planar_views_color(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                        const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests, const fpng_amd_view_color *colors,
                                                        const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Color, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests, rq.colors = colors;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_planar_views_color(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                               const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests, const fpng_amd_view_color *colors,
                                                               const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Color, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests, rq.colors = colors;
    return decode_files_views(e, files, n, results, true, rq);
}

extern "C" int fpng_amd_decode_batch_hwc_views_color(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                     const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests, const fpng_amd_view_color *colors,
                                                     const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Color, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests, rq.colors = colors;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_hwc_views_color(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                            const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests, const fpng_amd_view_color *colors,
                                                            const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Color, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests, rq.colors = colors;
    return decode_files_views(e, files, n, results, true, rq);
}

extern "C" int fpng_amd_decode_batch_planar_views_post(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                       const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests, const fpng_amd_view_color *colors,
                                                       const fpng_amd_view_post *posts, const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Post, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests, rq.colors = colors, rq.posts = posts;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_planar_views_post(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                              const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests, const fpng_amd_view_color *colors,
                                                              const fpng_amd_view_post *posts, const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Post, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests, rq.colors = colors, rq.posts = posts;
    return decode_files_views(e, files, n, results, true, rq);
}

extern "C" int fpng_amd_decode_batch_hwc_views_post(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                    const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests, const fpng_amd_view_color *colors,
                                                    const fpng_amd_view_post *posts, const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Post, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests, rq.colors = colors, rq.posts = posts;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_hwc_views_post(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                           const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests, const fpng_amd_view_color *colors,
                                                           const fpng_amd_view_post *posts, const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Post, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests, rq.colors = colors, rq.posts = posts;
    return decode_files_views(e, files, n, results, true, rq);
}

extern "C" int fpng_amd_decode_batch_planar_views_warp(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                       const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests, const fpng_amd_view_color *colors,
                                                       const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps, const fpng_amd_float_format *fmt,
                                                       fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Warp, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_planar_views_warp(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                              const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests, const fpng_amd_view_color *colors,
                                                              const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps, const fpng_amd_float_format *fmt,
                                                              fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Warp, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps;
    return decode_files_views(e, files, n, results, true, rq);
}

extern "C" int fpng_amd_decode_batch_hwc_views_warp(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                    const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests, const fpng_amd_view_color *colors,
                                                    const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps, const fpng_amd_float_format *fmt,
                                                    fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Warp, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_hwc_views_warp(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                           const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests, const fpng_amd_view_color *colors,
                                                           const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps, const fpng_amd_float_format *fmt,
                                                           fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Warp, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps;
    return decode_files_views(e, files, n, results, true, rq);
}

extern "C" int fpng_amd_decode_batch_planar_views_tone(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                       const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests, const fpng_amd_view_color *colors,
                                                       const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps, const fpng_amd_view_tone *tones,
                                                       const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Tone, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_planar_views_tone(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                              const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests, const fpng_amd_view_color *colors,
                                                              const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps, const fpng_amd_view_tone *tones,
                                                              const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Tone, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones;
    return decode_files_views(e, files, n, results, true, rq);
}

extern "C" int fpng_amd_decode_batch_hwc_views_tone(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                    const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests, const fpng_amd_view_color *colors,
                                                    const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps, const fpng_amd_view_tone *tones,
                                                    const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Tone, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_hwc_views_tone(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                           const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests, const fpng_amd_view_color *colors,
                                                           const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps, const fpng_amd_view_tone *tones,
                                                           const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Tone, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones;
    return decode_files_views(e, files, n, results, true, rq);
}

extern "C" int fpng_amd_decode_batch_planar_views_enhance(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                          const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests, const fpng_amd_view_color *colors,
                                                          const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps, const fpng_amd_view_tone *tones,
                                                          const fpng_amd_view_enhance *enhances, const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Enhance, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones, rq.enhances = enhances;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_planar_views_enhance(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count,
                                                                 const fpng_amd_crop *crops, const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests,
                                                                 const fpng_amd_view_color *colors, const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps,
                                                                 const fpng_amd_view_tone *tones, const fpng_amd_view_enhance *enhances, const fpng_amd_float_format *fmt,
                                                                 fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Enhance, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones, rq.enhances = enhances;
    return decode_files_views(e, files, n, results, true, rq);
}

extern "C" int fpng_amd_decode_batch_hwc_views_enhance(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                       const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests, const fpng_amd_view_color *colors,
                                                       const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps, const fpng_amd_view_tone *tones,
                                                       const fpng_amd_view_enhance *enhances, const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Enhance, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones, rq.enhances = enhances;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_hwc_views_enhance(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count,
                                                              const fpng_amd_crop *crops, const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests,
                                                              const fpng_amd_view_color *colors, const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps,
                                                              const fpng_amd_view_tone *tones, const fpng_amd_view_enhance *enhances, const fpng_amd_float_format *fmt,
                                                              fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Enhance, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones, rq.enhances = enhances;
    return decode_files_views(e, files, n, results, true, rq);
}

static_assert(sizeof(fpng_amd_view_alpha) == 16 && offsetof(fpng_amd_view_alpha, background) == 4 && offsetof(fpng_amd_view_alpha, reserved) == 8 &&
                  FPNG_AMD_ALPHA_COMPOSITE == kAlphaComposite && FPNG_AMD_ALPHA_PREMULTIPLIED == kAlphaPremultiplied,
              "fpng_amd_view_alpha layout");
extern "C" int fpng_amd_decode_batch_planar_views_alpha(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                        const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests, const fpng_amd_view_color *colors,
                                                        const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps, const fpng_amd_view_tone *tones,
                                                        const fpng_amd_view_enhance *enhances, const fpng_amd_view_alpha *alphas, const fpng_amd_float_format *fmt,
                                                        fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Alpha, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones, rq.enhances = enhances, rq.alphas = alphas;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_planar_views_alpha(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count,
                                                               const fpng_amd_crop *crops, const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests,
                                                               const fpng_amd_view_color *colors, const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps,
                                                               const fpng_amd_view_tone *tones, const fpng_amd_view_enhance *enhances, const fpng_amd_view_alpha *alphas,
                                                               const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Alpha, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones, rq.enhances = enhances, rq.alphas = alphas;
    return decode_files_views(e, files, n, results, true, rq);
}

extern "C" int fpng_amd_decode_batch_hwc_views_alpha(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                     const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests, const fpng_amd_view_color *colors,
                                                     const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps, const fpng_amd_view_tone *tones,
                                                     const fpng_amd_view_enhance *enhances, const fpng_amd_view_alpha *alphas, const fpng_amd_float_format *fmt,
                                                     fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Alpha, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones, rq.enhances = enhances, rq.alphas = alphas;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_hwc_views_alpha(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count,
                                                            const fpng_amd_crop *crops, const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests,
                                                            const fpng_amd_view_color *colors, const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps,
                                                            const fpng_amd_view_tone *tones, const fpng_amd_view_enhance *enhances, const fpng_amd_view_alpha *alphas,
                                                            const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Alpha, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones, rq.enhances = enhances, rq.alphas = alphas;
    return decode_files_views(e, files, n, results, true, rq);
}

// the alpha calls with a RESAMPLE record per view (fpng_amd_view_resample): the resize's filter
extern "C" int fpng_amd_decode_batch_planar_views_resample(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                        const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests, const fpng_amd_view_color *colors,
                                                        const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps, const fpng_amd_view_tone *tones,
                                                        const fpng_amd_view_enhance *enhances, const fpng_amd_view_alpha *alphas, const fpng_amd_view_resample *resamples, const fpng_amd_float_format *fmt,
                                                        fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Resample, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones, rq.enhances = enhances, rq.alphas = alphas, rq.resamples = resamples;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_planar_views_resample(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count,
                                                               const fpng_amd_crop *crops, const fpng_amd_resize_view *views, const fpng_amd_view_dest *dests,
                                                               const fpng_amd_view_color *colors, const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps,
                                                               const fpng_amd_view_tone *tones, const fpng_amd_view_enhance *enhances, const fpng_amd_view_alpha *alphas, const fpng_amd_view_resample *resamples,
                                                               const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Resample, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.dests = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones, rq.enhances = enhances, rq.alphas = alphas, rq.resamples = resamples;
    return decode_files_views(e, files, n, results, true, rq);
}

extern "C" int fpng_amd_decode_batch_hwc_views_resample(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count, const fpng_amd_crop *crops,
                                                     const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests, const fpng_amd_view_color *colors,
                                                     const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps, const fpng_amd_view_tone *tones,
                                                     const fpng_amd_view_enhance *enhances, const fpng_amd_view_alpha *alphas, const fpng_amd_view_resample *resamples, const fpng_amd_float_format *fmt,
                                                     fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Resample, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones, rq.enhances = enhances, rq.alphas = alphas, rq.resamples = resamples;
    return decode_files_views(e, files, n, results, false, rq);
}

extern "C" int fpng_amd_decode_batch_device_hwc_views_resample(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, const uint32_t *view_count,
                                                            const fpng_amd_crop *crops, const fpng_amd_resize_view *views, const fpng_amd_view_dest_hwc *dests,
                                                            const fpng_amd_view_color *colors, const fpng_amd_view_post *posts, const fpng_amd_view_warp *warps,
                                                            const fpng_amd_view_tone *tones, const fpng_amd_view_enhance *enhances, const fpng_amd_view_alpha *alphas, const fpng_amd_view_resample *resamples,
                                                            const fpng_amd_float_format *fmt, fpng_amd_decode_result *results)
{
    ViewRequest rq;
    rq.family = ViewFamily::Resample, rq.fmt = fmt, rq.view_count = view_count, rq.crops = crops, rq.views = views, rq.hwc = dests, rq.colors = colors, rq.posts = posts, rq.warps = warps, rq.tones = tones, rq.enhances = enhances, rq.alphas = alphas, rq.resamples = resamples;
    return decode_files_views(e, files, n, results, true, rq);
}

// the alpha rule on the host: the texts of view_alpha.h, which the resize kernels run in their load (source) and store (result)
extern "C" int fpng_amd_view_alpha_source(const fpng_amd_view_alpha *alpha, uint32_t w, uint32_t h, const uint8_t *in, uint8_t *out)
{
    const char *why = nullptr;
    const int rc = alpha_twin_checked(alpha, w, h, in, out, false, &why);
    return rc ? fail(rc, why) : FPNG_AMD_OK;
}

extern "C" int fpng_amd_view_alpha_result(const fpng_amd_view_alpha *alpha, uint32_t w, uint32_t h, const uint8_t *in, uint8_t *out)
{
    const char *why = nullptr;
    const int rc = alpha_twin_checked(alpha, w, h, in, out, true, &why);
    return rc ? fail(rc, why) : FPNG_AMD_OK;
}

// the enhance rule on the host: the texts of view_enhance.h, which dec_view_post_kernel runs
extern "C" int fpng_amd_view_enhance_apply(const fpng_amd_view_enhance *enhance, uint32_t w, uint32_t h, const uint8_t *in, uint8_t *out)
{
    const char *why = nullptr;
    const int rc = enhance_apply_checked(enhance, w, h, in, out, &why);
    return rc ? fail(rc, why) : FPNG_AMD_OK;
}

// the tone rule on the host: the texts of view_tone.h, which dec_view_tone_lut_kernel runs
extern "C" int fpng_amd_view_tone_lut(const fpng_amd_view_tone *tone, const uint32_t *hist, uint8_t *lut)
{
    const char *why = nullptr;
    const int rc = tone_lut_checked(tone, hist, lut, &why);
    return rc ? fail(rc, why) : FPNG_AMD_OK;
}

extern "C" int fpng_amd_view_tone_apply(const fpng_amd_view_tone *tone, uint32_t w, uint32_t h, const uint8_t *in, uint8_t *out)
{
    const char *why = nullptr;
    const int rc = tone_apply_checked(tone, w, h, in, out, &why);
    return rc ? fail(rc, why) : FPNG_AMD_OK;
}

// step 1a of the warp rule for one w x h plane of bytes, on the host: the texts of view_warp.h, which dec_view_post_kernel runs
extern "C" int fpng_amd_view_warp_apply(const fpng_amd_view_warp *warp, uint32_t w, uint32_t h, uint32_t mirror, const uint8_t *in, uint8_t *out, uint8_t fill_value)
{
    const char *why = nullptr;
    const int rc = warp_apply_checked(warp, w, h, mirror, in, out, fill_value, &why);
    return rc ? fail(rc, why) : FPNG_AMD_OK;
}

// the blur's weights on the host: post_blur_weights (view_post.h), what the post calls hand to dec_view_post_kernel
extern "C" int fpng_amd_blur_weights(uint32_t radius, double sigma, int32_t k[17])
{
    if (!k) return fail(FPNG_AMD_ERR_INVALID_ARG, "null k");
    if (!radius || radius > kPostMaxRadius) return fail(FPNG_AMD_ERR_INVALID_ARG, "fpng_amd_view_post::blur_radius must be 1 .. 16 with FPNG_AMD_POST_BLUR");
    if (!std::isfinite(sigma) || !(sigma > 0.0)) return fail(FPNG_AMD_ERR_INVALID_ARG, "fpng_amd_view_post::blur_sigma must be finite and > 0 with FPNG_AMD_POST_BLUR");
    post_blur_weights(radius, sigma, k);
    return FPNG_AMD_OK;
}

// steps 2 to 4 of the post rule for one w x h plane of bytes, on the host: the texts of view_post.h, which dec_view_post_kernel runs
extern "C" int fpng_amd_view_post_apply(const fpng_amd_view_post *post, uint32_t w, uint32_t h, const uint8_t *in, uint8_t *out)
{
    if (!post || !in || !out || !w || !h) return fail(FPNG_AMD_ERR_INVALID_ARG, "null post, in or out, or an empty plane");
    if (const char *why = check_post_record(*post, w, h)) return fail(FPNG_AMD_ERR_INVALID_ARG, why);
    const size_t count = (size_t)w * h;
    std::vector<uint8_t> g(in, in + count);
    if (post->flags & kPostBlur) {
        const int32_t R = (int32_t)post->blur_radius;
        int32_t k[kPostMaxRadius + 1];
        post_blur_weights(post->blur_radius, post->blur_sigma, k);
        std::vector<uint8_t> hp(count);
        for (uint32_t q = 0; q < h; q++)
            for (uint32_t i = 0; i < w; i++) {
                int32_t sum = 1 << (kResizeBits - 1);
                for (int32_t t = -R; t <= R; t++) sum += (int32_t)in[(size_t)q * w + post_refl((int32_t)i + t, w)] * k[t < 0 ? -t : t];
                hp[(size_t)q * w + i] = (uint8_t)resize_clip8(sum);
            }
        for (uint32_t q = 0; q < h; q++)
            for (uint32_t i = 0; i < w; i++) {
                int32_t sum = 1 << (kResizeBits - 1);
                for (int32_t t = -R; t <= R; t++) sum += (int32_t)hp[(size_t)post_refl((int32_t)q + t, h) * w + i] * k[t < 0 ? -t : t];
                g[(size_t)q * w + i] = (uint8_t)resize_clip8(sum);
            }
    }
    for (size_t q = 0; q < count; q++) out[q] = (uint8_t)post_point(g[q], post->flags, post->solarize_threshold, post->posterize_bits);
    return FPNG_AMD_OK;
}

// u_c of the colour rule for one pixel, on the host: color_apply (resize_color.h), the text dec_resize_color_kernel runs
extern "C" void fpng_amd_color_apply(const fpng_amd_view_color *color, const uint8_t rgb[3], float u[3])
{
    for (int c = 0; c < 3; c++) u[c] = color_apply(color->m[c][0], color->m[c][1], color->m[c][2], color->m[c][3], (float)rgb[0], (float)rgb[1], (float)rgb[2]);
}

// the ONE box that a file with these views decodes: the bounding rectangle of the boxes below
extern "C" int fpng_amd_views_source(const fpng_amd_crop *crops, const fpng_amd_resize_view *views, uint32_t count, fpng_amd_crop *box)
{
    if (!crops || !views || !box) return fail(FPNG_AMD_ERR_INVALID_ARG, "null argument");
    if (!count) return fail(FPNG_AMD_ERR_INVALID_ARG, "a count of 0");
    if (int rc = check_view_records(crops, views, count)) return rc;
    const DecCrop b = views_box(crops, views, count);
    box->x = b.x, box->y = b.y, box->w = b.w, box->h = b.h;
    return FPNG_AMD_OK;
}

// the source pixels, in the file's coordinates, that the taps of a view of a crop reach: what the crop stage decodes
extern "C" int fpng_amd_resize_view_source(const fpng_amd_crop *crop, const fpng_amd_resize_view *view, fpng_amd_crop *box)
{
    if (!crop || !view || !box) return fail(FPNG_AMD_ERR_INVALID_ARG, "null argument");
    if (int rc = check_view_records(crop, view, 1)) return rc;
    const DecCrop b = view_box({crop->x, crop->y, crop->w, crop->h}, *view);
    box->x = b.x, box->y = b.y, box->w = b.w, box->h = b.h;
    return FPNG_AMD_OK;
}

// out_size rows of kResizeMaxTaps weights (those behind a row's count: 0), first and count per output sample: resize_weights_of,
// the text dec_resize_kernel runs
extern "C" int fpng_amd_resize_weights(uint32_t in_size, uint32_t out_size, uint32_t *first, uint32_t *count, int32_t *weights)
{
    if (!first || !count || !weights) return fail(FPNG_AMD_ERR_INVALID_ARG, "null argument");
    if (!resize_scale_ok(in_size, out_size)) return fail(FPNG_AMD_ERR_INVALID_ARG, "in_size and out_size are at least 1, and in_size <= 32 * out_size");
    for (uint32_t o = 0; o < out_size; o++) {
        int32_t *K = weights + (size_t)o * kResizeMaxTaps;
        std::fill(K, K + kResizeMaxTaps, 0);
        count[o] = resize_weights_of<kResizeBilinear>(in_size, out_size, o, &first[o], K, 1);
    }
    return FPNG_AMD_OK;
}

extern "C" int fpng_amd_resize_weights_filter(uint32_t in_size, uint32_t out_size, uint32_t filter, uint32_t *first, uint32_t *count, int32_t *weights)
{
    if (!first || !count || !weights) return fail(FPNG_AMD_ERR_INVALID_ARG, "null argument");
    if (filter >= kResizeFilters) return fail(FPNG_AMD_ERR_INVALID_ARG, "unknown filter (FPNG_AMD_FILTER_BILINEAR, _BICUBIC)");
    if (!resize_scale_ok(in_size, out_size, filter))
        return fail(FPNG_AMD_ERR_INVALID_ARG, filter == kResizeBicubic ? "in_size and out_size are at least 1, and in_size <= 16 * out_size (bicubic)"
                                                                       : "in_size and out_size are at least 1, and in_size <= 32 * out_size (bilinear)");
    for (uint32_t o = 0; o < out_size; o++) {
        int32_t *K = weights + (size_t)o * kResizeMaxTaps;
        std::fill(K, K + kResizeMaxTaps, 0);
        count[o] = resize_weights_of(filter, in_size, out_size, o, &first[o], K, 1);
    }
    return FPNG_AMD_OK;
}

// fpng_amd_resize_weights_filter for the RESAMPLE filters: resample_weights_of, the text the kernels' resample instantiations run;
// NEAREST: resize_nearest_indices, the text the host fills a view's indices with
extern "C" int fpng_amd_resample_weights(uint32_t in_size, uint32_t out_size, uint32_t resample_filter, uint32_t *first, uint32_t *count, int32_t *weights)
{
    if (!first || !count || !weights) return fail(FPNG_AMD_ERR_INVALID_ARG, "null argument");
    if (resample_filter < FPNG_AMD_RESAMPLE_NEAREST || resample_filter > FPNG_AMD_RESAMPLE_LANCZOS)
        return fail(FPNG_AMD_ERR_INVALID_ARG, "unknown filter (FPNG_AMD_RESAMPLE_NEAREST, _BOX, _HAMMING, _LANCZOS)");
    const uint32_t filter = resample_filter + (kResizeNearest - FPNG_AMD_RESAMPLE_NEAREST);
    if (!resize_scale_ok(in_size, out_size, filter))
        return fail(FPNG_AMD_ERR_INVALID_ARG, filter == kResizeLanczos ? "in_size and out_size are at least 1, and 3 * in_size <= 32 * out_size (Lanczos)"
                                                                       : "in_size and out_size are at least 1, and in_size <= 32 * out_size (nearest, box, Hamming)");
    if (filter == kResizeNearest && !resize_nearest_indices(in_size, out_size, 0, out_size, first)) return fail(FPNG_AMD_ERR_UNSUPPORTED, "a NEAREST index outside the input");
    for (uint32_t o = 0; o < out_size; o++) {
        int32_t *K = weights + (size_t)o * kResizeMaxTaps;
        std::fill(K, K + kResizeMaxTaps, 0);
        if (filter == kResizeNearest) count[o] = 1, K[0] = 1 << kResizeBits;
        else count[o] = resample_weights_of(filter, in_size, out_size, o, &first[o], K, 1);
    }
    return FPNG_AMD_OK;
}

extern "C" int fpng_amd_resample_view_source(const fpng_amd_crop *crop, const fpng_amd_resize_view *view, const fpng_amd_view_resample *resample, fpng_amd_crop *box)
{
    if (!crop || !view || !resample || !box) return fail(FPNG_AMD_ERR_INVALID_ARG, "null argument");
    if (const char *why = check_resample_record(*resample)) return fail(FPNG_AMD_ERR_INVALID_ARG, why);
    if (int rc = check_view_records(crop, view, 1, resample)) return rc;
    const DecCrop b = view_box({crop->x, crop->y, crop->w, crop->h}, *view, resample);
    box->x = b.x, box->y = b.y, box->w = b.w, box->h = b.h;
    return FPNG_AMD_OK;
}

extern "C" int fpng_amd_decode_crop_tiles(uint32_t file_w, uint32_t file_h, const fpng_amd_crop *crop, uint32_t *n_segments, uint32_t *first_col_block, uint32_t *n_col_blocks)
{
    if (!crop || !n_segments || !first_col_block || !n_col_blocks) return fail(FPNG_AMD_ERR_INVALID_ARG, "null argument");
    if (!dec_crop_tiles(file_w, file_h, {crop->x, crop->y, crop->w, crop->h}, n_segments, first_col_block, n_col_blocks))
        return fail(FPNG_AMD_ERR_INVALID_ARG, "the crop is empty or leaves the image");
    return FPNG_AMD_OK;
}

extern "C" int fpng_amd_decode_batch_ex(fpng_amd_encoder *e, const fpng_amd_png_ex *files, uint32_t n, fpng_amd_decode_result *results)
{
    return decode_files_ex(e, files, n, results, false);
}

extern "C" int fpng_amd_decode_batch_device_ex(fpng_amd_encoder *e, const fpng_amd_png_ex *files, uint32_t n, fpng_amd_decode_result *results)
{
    return decode_files_ex(e, files, n, results, true);
}

// One host-resident file to host pixels: what fpng::fpng_decode_memory() does for large images (fpng_decode.cpp).  The pixels land in
// the encoder's staging buffer and go down in one copy into memory obtained from `reserve` (asked once the file is known to decode).
extern "C" int fpng_amd_decode_host(fpng_amd_encoder *e, const void *png, uint32_t size, uint32_t desired, fpng_amd_reserve_fn reserve, void *user,
                                    fpng_amd_decode_result *result)
{
    if (!e || !result || !reserve) return fail(FPNG_AMD_ERR_INVALID_ARG, "null argument");
    if (desired != 3 && desired != 4) return fail(FPNG_AMD_ERR_INVALID_ARG, "desired_chans must be 3 or 4");
    std::memset(result, 0, sizeof *result);
    if (!png || !size) {
        result->status = fpng::FPNG_DECODE_INVALID_ARG;
        return FPNG_AMD_OK;
    }
    // the container, then the stream's shape: a header that promises more pixels than the IDAT can hold must not size any device memory
    Parsed sp;
    static thread_local uint32_t stable[1u << fpng::parse::kTableBits];
    uint8_t ssizes[288];
    const int ss = parse_host((const uint8_t *)png, size, sp, stable, ssizes);
    result->w = sp.w, result->h = sp.h, result->channels_in_file = sp.c;
    const uint64_t need = (uint64_t)sp.w * sp.h * desired;
    if ((result->status = file_status(sp, ss, need))) return FPNG_AMD_OK;
    HIP_TRY(hipSetDevice(e->device));
    int rc = drain(e);
    if (rc) return rc;
    if ((rc = e->d_stage_in.ensure((size_t)need + 16))) return rc;
    // large compressed files: upload, decode and download overlapped (FPNG_AMD_DECODE_STREAM=0: one after the other)
    static const bool stream_ok = [] {
        const char *v = getenv("FPNG_AMD_DECODE_STREAM");
        return !(v && v[0] == '0');
    }();
    // (with the checksums' check on, the serial form below: fpng_amd_encoder_set_decode_verify in fpng_amd.h)
    if (stream_ok && !e->dec_verify && sp.mode == 0 && sp.idat_len >= (8u << 20) && getenv("FPNG_AMD_DECODE_MAX_ROUNDS") == nullptr) {
        uint8_t *out = reserve(user, (size_t)need);
        if (!out) return fail(FPNG_AMD_ERR_BUFFER_TOO_SMALL, "no room for the pixels");
        bool redo = false;
        if ((rc = decode_host_streamed(e, (const uint8_t *)png, sp, stable, ssizes, desired, out, result, &redo))) return rc;
        if (!redo) return FPNG_AMD_OK;
    }
    fpng_amd_png f;
    std::memset(&f, 0, sizeof f);
    f.data = png, f.size = size, f.d_pixels = e->d_stage_in.p, f.pixels_cap = e->d_stage_in.cap;
    if ((rc = fpng_amd_decode_batch(e, &f, 1, desired, result))) return rc;
    if (result->status) return FPNG_AMD_OK;
    uint8_t *out = reserve(user, (size_t)need); // (the same memory again if the streamed attempt above asked already)
    if (!out) return fail(FPNG_AMD_ERR_BUFFER_TOO_SMALL, "no room for the pixels");
    HIP_TRY(hipMemcpy(out, e->d_stage_in.p, (size_t)need, hipMemcpyDeviceToHost));
    return FPNG_AMD_OK;
}

// What fpng_amd_decode_batch() prepares on the host for one file, without a GPU (tests hold a model of the kernels against it):
// container status, geometry, stored or dynamic, the token stream's first bit and its limit, the kernels' lookup table.
extern "C" int fpng_amd_decode_plan(const void *png_, uint32_t size, fpng_amd_decode_result *result, uint32_t *mode, uint32_t *idat_ofs, uint32_t *idat_len,
                                    uint64_t *first_bit, uint64_t *end_limit_bit, uint32_t *lut)
{
    if (!png_ || !size || !result || !mode || !idat_ofs || !idat_len || !first_bit || !end_limit_bit || !lut) return fail(FPNG_AMD_ERR_INVALID_ARG, "null argument");
    const uint8_t *png = (const uint8_t *)png_;
    std::memset(result, 0, sizeof *result);
    Parsed p;
    static thread_local uint32_t table[1u << fpng::parse::kTableBits];
    uint8_t sizes[288];
    result->status = parse_host(png, size, p, table, sizes);
    result->w = p.w, result->h = p.h, result->channels_in_file = p.c;
    *mode = 0, *idat_ofs = p.idat_ofs, *idat_len = p.idat_len, *first_bit = 0, *end_limit_bit = 0;
    if (result->status) return FPNG_AMD_OK;
    *mode = p.mode;
    if (!p.mode) {
        *first_bit = p.first_bit, *end_limit_bit = (uint64_t)(p.idat_len - 4) * 8;
        build_multi_lut(table, sizes, lut);
    }
    return FPNG_AMD_OK;
}
