// decode.h -- host/device shared structures of the GPU batch decoder (decode.hip, decode_api.cpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace fpng_amd {

constexpr uint32_t kSubBits = 512;      // token bits per subsequence (one thread each)
constexpr uint32_t kDecSubBlock = 512;  // subsequences per workgroup of the synchronisation (a file's subsequences are padded to whole workgroups)
#ifndef FPNG_DEC_LEADIN // (build variants lead96 / lead64: a shorter lead-in is less work for every thread and more threads to correct)
#define FPNG_DEC_LEADIN 128
#endif
constexpr uint32_t kDecLeadIn = FPNG_DEC_LEADIN; // bits a subsequence's first decode starts early (decode_core.h: sub_first); a multiple of 32
#ifndef FPNG_DEC_UNF_ROWS
#define FPNG_DEC_UNF_ROWS 48
#endif
constexpr uint32_t kDecUnfRows = FPNG_DEC_UNF_ROWS; // rows per segment of the Up filter's undoing (held in registers)
enum : uint32_t { kDecNotConverged = 1u, kDecBadStream = 2u, kDecBadFilter = 8u, kDecStalled = 16u, kDecStoredOdd = 32u, kDecSawEob = 0x100u };
// dec_unfilter_kernel's own findings, bits of their own: a tile's walk met a bad match (kEmitBadStream of decode_core.h) or a match at
// a row's first pixel (kEmitLeaveToCpu), or its look-back gave up waiting for a lower segment.  The host reads them as kDecBadStream,
// kDecStalled, kDecStalled (decode_api.cpp: dec_result).
enum : uint32_t { kDecTileBadStream = 4u, kDecTileLeaveToCpu = 64u, kDecTileStalled = 128u };
// the bits for which dec_unfilter_kernel skips a file's tiles in the batch path: set only by kernels in FRONT of its launch, never
// by the kernel itself, so that every thread of every workgroup reads the same answer (a tile that skips publishes no look-back granule)
constexpr uint32_t kDecUnfSkipMask = kDecNotConverged | kDecBadStream | kDecStalled;
// what the optional check of a file's checksums found (fpng_amd_encoder_set_decode_verify; set by dec_verify_kernel, the last kernel
// of the chain, and read by the host only for files whose other bits say "decoded": decode_api.cpp, verify_result): the IDAT
// chunk's CRC-32 / the zlib stream's Adler-32 is not what the file says
enum : uint32_t { kDecBadCrc = 0x200u, kDecBadAdler = 0x400u };
static_assert(!(kDecUnfSkipMask & (kDecTileBadStream | kDecTileLeaveToCpu | kDecTileStalled | kDecBadFilter | kDecBadCrc | kDecBadAdler)), "dec_unfilter_kernel must not set the bits it skips on");

struct DecJob {
    const uint8_t *z;         // device: the zlib stream (IDAT payload) from the dword its first byte (0x78) lies in; readable up to z_bytes + 16 rounded down to a dword
    uint64_t z_bytes;         // length of the IDAT payload + z_shift
    uint64_t first_bit;       // first row token (behind the dynamic block header)
    uint64_t end_limit_bit;   // (z_bytes - 4) * 8: no token may start here or later
    const uint32_t *lut;      // device: dec::kLutDwords words (decode_core.h)
    uint32_t *win;            // device scratch: h x dec_col_blocks() x dec::kWinWords words: for each window of dec_unfilter_kernel's tiles (decode_core.h:
                              // Window) the file's subsequence (counted from its first one) in whose output it begins, 0xFFFFFFFF: none; and where
                              // that subsequence's walk may begin (decode_core.h: Resume)
    uint8_t *out;             // device: w * h * dst_c pixels (layout jobs: the top row's first destination pixel)
    uint32_t *segsum;         // device scratch: nseg x ceil(bpl / 4) 8-byte granules {tag, column sum} of dec_unfilter_kernel's look-back
    uint32_t w, h, src_c, dst_c, bpl;
    uint32_t n_sub;           // subsequences of the file
    uint32_t sub_base;        // index of its first subsequence (a multiple of kDecSubBlock: one file per workgroup)
    uint32_t mode;            // 0 one dynamic block, 1 stored blocks
    uint32_t nseg;            // segments of kDecUnfRows rows (dec_unfilter_*_kernel)
    // destination layout of fpng_amd_decode_batch_ex jobs (zero elsewhere; read only by the *_ex kernels): row y starts at
    // out + y * pitch, a pixel is dst_c bytes, and v_perm_b32 with selector `sel` turns an R,G,B,A pixel dword into the destination's
    // byte order (0x0d = a 0xFF byte).  These words were padding before: the record stays 112 bytes with z_shift where it was, so
    // the other kernels' code is, instruction for instruction, the same (tools/isa_diff.py)
    uint32_t sel;
    int32_t pitch;            // signed bytes from one row to the next
    uint32_t z_shift;         // bytes between z (rounded down to a dword) and the stream's first byte; the bit positions above count from z
};
static_assert(sizeof(DecJob) == 112 && offsetof(DecJob, sel) == 100 && offsetof(DecJob, z_shift) == 108, "DecJob layout");
// DecJob::sel of the R,G,B order: rows of 3-channel files go out as they are
constexpr uint32_t kDecSelRGB = 0x0d020100u;

// Column blocks of dec_unfilter_kernel for one file: 256 PIXELS of the file's rows each -- 256 dword columns of 4-byte pixels, or
// 4 waves x 48 dword columns of 3-byte ones (see the kernel) -- so that a match, which repeats whole pixels, is whole pixels in
// every block it touches.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t dec_col_blocks(uint32_t w, uint32_t /*src_c*/, uint32_t /*dst_c*/) { return (w + 255u) / 256u; }

// bytes of a row that one column block covers (the first one also holds the row's filter byte: decode_core.h, Window)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t dec_col_block_bytes(uint32_t src_c, uint32_t /*dst_c*/) { return 256u * src_c; }

// what the synchronisation leaves per workgroup of kDecSubBlock subsequences (indices inside the workgroup, kDecSubBlock = none)
struct DecBlockRec {
    uint32_t sum;           // output bytes of its subsequences
    uint32_t first_eob;     // first one that met an end-of-block symbol
    uint32_t first_invalid; // first one whose decode derailed
    uint32_t first_overflow; // first one that needed more records than it has room for (decode_core.h: kRecCap)
    uint32_t entry_rel;     // where its first subsequence starts, in bits behind the workgroup's first nominal bit
    uint32_t exit_rel;      // where its last subsequence ends, in bits behind the next workgroup's first nominal bit
    uint32_t want_rel;      // dec_chain_kernel: where its first subsequence must start (kDecWantUnknown: ask the workgroup in front)
    uint32_t map[3];        // dec::PhaseMap: what the workgroup does to the phases it can be entered in (entry -> exit: one pair unless the
                            // stream is periodic, decode_core.h; no pair at all: round 0 left the workgroup unsettled)
    uint32_t left;          // ... and why (decode.hip: many threads to correct / corrections that do not end)
};
constexpr uint32_t kDecWantUnknown = 0xFFFFFFFFu;

// dec_unfilter_kernel's work items -- (segment of rows, block of 256 dword columns) of a file -- numbered segment by segment over a
// group of files: the files sorted by segment count (most first) in order[]; cbpre[k] = column blocks of the first k of them;
// a piece = a range of segments over which the same `alive` first files of that order still have rows
struct DecUnfPiece {
    uint32_t item0; // number of its first item
    uint32_t seg0;  // its first segment
    uint32_t alive;
    uint32_t pad_;
};
struct DecUnfPlan {
    const DecUnfPiece *pieces;
    const uint32_t *cbpre; // n_files + 1
    const uint32_t *order; // n_files: indices into the group's jobs
    uint32_t n_pieces, total_items;
    uint32_t n_files, pad_; // files of the order (cbpre holds n_files + 1 words)
};

// a device-resident file (dec_fetch_kernel gathers the heads and tails of a batch's files for the host's container walk)
struct DecFileRef {
    const uint8_t *data;
    uint32_t size, pad_;
};
// sizes: n x 288 code lengths (checked by the host) -> luts: n x FPNG_AMD_DECODE_LUT_WORDS
void launch_dec_build_luts(hipStream_t s, const uint8_t *sizes, uint32_t n, uint32_t *luts);
void launch_dec_fetch(hipStream_t s, const DecFileRef *files, uint32_t n, uint32_t head, uint32_t tail, uint8_t *out);

// a file that is decoded piece by piece: what the pieces so far amount to (dec_offsets_range_kernel)
struct DecCarry {
    uint64_t bytes; // output bytes of the blocks so far (up to the end-of-block symbol once it was met)
    uint32_t done;  // the stream's end-of-block symbol was met
    uint32_t pad_;
};

// per-subsequence arrays (index = batch-wide subsequence number)
struct DecSubArrays {
    uint32_t *info;   // dec::pack_info
    uint32_t *bytes;  // output bytes
    uint32_t *rel;    // output offset inside its workgroup (exclusive scan of bytes)
    uint32_t *lastpx; // the four literal bytes in front of it (decode_core.h: lookback_lastpx, over the records)
    uint32_t *eob;    // where its end-of-block symbol ends, in bits behind its nominal first bit (subsequences flagged kSubEob)
    uint64_t *tok;    // its token records, two to an entry (decode_core.h: rec_index)
};

// the kernels work on the workgroups [first_block, first_block + n_blocks) of the batch's subsequences (one group of files);
// jobs / n_jobs: the whole batch
// resident: how many persistent workgroups to launch at most; changed: set by a border round that changed something; multi: set
// once a workgroup's map has more than one pair (zero at the start of the call, never cleared inside it)
void launch_dec_sync(hipStream_t s, uint32_t resident, const DecJob *jobs, uint32_t n_jobs, uint32_t first_block, uint32_t n_blocks, uint32_t total_subs, uint32_t round, DecSubArrays a,
                     DecBlockRec *recs, uint32_t *changed, uint32_t *multi);
// group_jobs: the group's first file; status / eob_index: batch-wide arrays
void launch_dec_offsets(hipStream_t s, const DecJob *jobs, uint32_t n_jobs, uint32_t first_block, uint32_t n_blocks, uint32_t total_subs, const DecJob *group_jobs,
                        uint32_t n_group_jobs, DecSubArrays a, const DecBlockRec *recs, uint64_t *block_off, uint32_t *status, uint32_t *eob_index);
// ONE file (jobs[0], a DEVICE pointer whose sub_base the caller knows: passed as first_block of the other launchers), blocks [blk_a, blk_b)
void launch_dec_offsets_range(hipStream_t s, const DecJob *jobs, uint32_t sub_base_block, uint32_t blk_a, uint32_t blk_b, bool final_piece, uint32_t total_subs, DecSubArrays a,
                              const DecBlockRec *recs, uint64_t *block_off, uint32_t *status, uint32_t *eob_index, DecCarry *carry);
// What the pass that writes the pixels needs of the synchronisation's results: the per-subsequence arrays, the workgroups' output offsets,
// every file's last subsequence (the one with the stream's end-of-block symbol; sub_limit: subsequences of a file that arrives in
// pieces which have been placed so far, else 0xFFFFFFFF)
struct DecPlaced {
    DecSubArrays a;
    const uint64_t *block_off;
    const uint32_t *eob_index; // per file of the launch's `jobs`
    uint32_t sub_limit;
};
// concurrent_status: kernels that may set the file's status bits run next to this launch (no workgroup may then skip its file: dec_unfilter_kernel)
// layout: the jobs are fpng_amd_decode_batch_ex's (DecJob::sel / pitch: the *_ex kernels write them; a launch is all one or the other)
// plane_pitch (device, a word per file of `jobs`, or NULL): the jobs are fpng_amd_decode_batch_planar's -- dst_c planes, DecJob::pitch
// between a plane's rows; the *_planar kernels write them
// adler_acc (device, two 64-bit words per file of `jobs`, or NULL): the verify forms of the kernels run instead -- every tile adds its
// filtered bytes' sum and position-weighted sum (mod 65521) to its file's two words (DecVerify)
// flt (host, or NULL; needs plane_pitch): the jobs are fpng_amd_decode_batch_planar_float's -- the planes hold flt->dtype elements,
// fmaf(value, scale[c], bias[c]) of the file's channel c; DecJob::pitch and plane_pitch stay bytes; the *_float kernels write them
struct DecFloat { // (the words of fpng_amd_float_format)
    uint32_t dtype, pad_; // FPNG_AMD_F32 / F16 / BF16
    float scale[4], bias[4];
};
constexpr uint32_t kDecFloatTypes = 3;
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr uint32_t dec_float_bytes(uint32_t dtype) { return dtype == 0 ? 4u : 2u; }
// crops (device, a record per file of `jobs`, or NULL; needs plane_pitch): the jobs are fpng_amd_decode_batch_planar_crop's -- the
// planes hold the crop's w x h elements (bytes, or flt's), DecJob::out / pitch and plane_pitch describe THAT destination, and
// DecJob::nseg and the plan's column blocks count only the tiles dec_crop_tiles() names (all of them where adler_acc is given: the
// Adler-32 needs every filtered byte); the *_crop kernels write them
struct DecCrop { // (the words of fpng_amd_crop)
    uint32_t x, y, w, h;
};
// The tiles of dec_unfilter_kernel that a crop needs: segments 0 .. n_segments - 1 (a pixel depends on its column in the rows above
// it) of the column blocks first_col_block .. first_col_block + n_col_blocks - 1.  The ONE text: the host's plan, the kernels
// (dec_crop_first_block) and fpng_amd_decode_crop_tiles use it.  false: the crop is empty or leaves the image.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t dec_crop_first_block(uint32_t crop_x) { return crop_x / 256u; }
inline bool dec_crop_tiles(uint32_t file_w, uint32_t file_h, const DecCrop &c, uint32_t *n_segments, uint32_t *first_col_block, uint32_t *n_col_blocks)
{
    if (!c.w || !c.h || (uint64_t)c.x + c.w > file_w || (uint64_t)c.y + c.h > file_h) return false;
    *n_segments = (c.y + c.h + kDecUnfRows - 1) / kDecUnfRows;
    *first_col_block = dec_crop_first_block(c.x);
    *n_col_blocks = (c.x + c.w - 1) / 256u - *first_col_block + 1;
    return true;
}
void launch_dec_unfilter(hipStream_t s, const DecJob *jobs, DecUnfPlan plan, DecPlaced placed, uint32_t item0, uint32_t n_items, uint32_t *status, uint32_t epoch, bool concurrent_status,
                         bool layout = false, const int64_t *plane_pitch = nullptr, unsigned long long *adler_acc = nullptr, const DecFloat *flt = nullptr,
                         const DecCrop *crops = nullptr);
// The optional check of the files' checksums (fpng_amd_encoder_set_decode_verify), per launch of launch_dec_finish: flags =
// FPNG_AMD_VERIFY_*; adler_acc as above, zero when the launch begins; crc_partials: max_ranges words per file that launch_dec_crc
// filled (FPNG_AMD_VERIFY_CRC32).  All pointers are the entries of the launch's first file.
struct CrcDeviceTables;
struct DecVerify {
    uint32_t flags, max_ranges;
    uint32_t stored_blocks, pad_; // the most stored blocks (of 65535 bytes) a stored file of the launch has
    unsigned long long *adler_acc;
    const uint32_t *crc_partials;
    const CrcDeviceTables *tabs;
};
// ranges of kDecCrcRange bytes that launch_dec_crc cuts a payload of idat_len bytes at address z into (they hang off the payload's
// end, rounded up to 16 bytes).  The one place this is computed: the host sizes the partials with it, dec_crc_kernel's grid covers
// it and dec_verify_kernel folds that many.  A file has a 32-bit size and at least 57 bytes that are not IDAT payload (signature,
// IHDR, the IDAT's own 12 bytes, IEND), so payload + 2 * 15 bytes of alignment < 2^32: at most 2^32 / range of them.
// crc_fold_partials (crc_device.h) gives each of its kCrcBlock = 256 threads 2^g partials, g <= 8 (its table of in-group powers
// has 256 entries), and reads CrcDeviceTables::fold[range log2 + g - 12] of 13 rows: both hold while a file has at most 2^16 ranges
// of at most 2^16 bytes.
constexpr uint32_t kDecCrcRangeLog2 = 16;
static_assert(kDecCrcRangeLog2 >= 12 && 32 - kDecCrcRangeLog2 <= 8 + 8 && kDecCrcRangeLog2 + 8 - 12 <= 12,
              "a file's CRC ranges: at most 256 threads x 256 partials, and CrcDeviceTables::fold has rows e = 12 .. 24 (crc_fold_partials)");
#ifdef __HIPCC__
__host__ __device__
#endif
inline uint32_t dec_crc_ranges(uintptr_t z, uint64_t idat_len)
{
    const uint64_t a = z & ~(uintptr_t)15, e = (z + idat_len + 15) & ~(uint64_t)15;
    return (uint32_t)((e - a + (1ull << kDecCrcRangeLog2) - 1) >> kDecCrcRangeLog2);
}
// raw CRC-32 partials of every file's IDAT payload, max_ranges words per file (depends on nothing but the files' bytes and the job records)
void launch_dec_crc(hipStream_t s, const DecJob *jobs, uint32_t n_jobs, uint32_t max_ranges, const CrcDeviceTables *tabs, uint32_t *partials);
void launch_dec_finish(hipStream_t s, const DecJob *jobs, uint32_t n_jobs, DecUnfPlan plan, DecPlaced placed, uint32_t *status, uint32_t epoch, bool any_stored, bool layout = false,
                       const int64_t *plane_pitch = nullptr, const DecVerify *verify = nullptr, const DecFloat *flt = nullptr, const DecCrop *crops = nullptr);
// The second stage of fpng_amd_decode_batch_planar_resize (resize.h, resize.hip): recs (device) -- a record per file of the launch,
// whose boxes' uint8 planes the crop kernels in front of it on the stream wrote; max_tiles / lds_bytes: the most tiles per plane a
// file of the launch has and the most LDS one of its tiles needs (resize_tile_lds); flt (host, or NULL: bytes): the elements.
// false: max_tiles or lds_bytes is out of range, nothing was launched.
struct DecResize;
bool launch_dec_resize(hipStream_t s, const DecResize *recs, uint32_t n, uint32_t max_tiles, uint32_t lds_bytes, const DecFloat *flt, bool any_filter);
// The same for fpng_amd_decode_batch(_device)_planar_views, whose records -- several per file -- mix sizes and plane counts: a grid
// of exactly the records' workgroups.  pre (device) and h_pre (host, the same words): n + 1 entries, the workgroups (planes x tiles)
// of the batch's records in front of each of recs[0 .. n]; split into launches of fewer than 2^24 workgroups.  false: a record
// without or with too many workgroups, or lds_bytes out of range; nothing is launched.  any_alpha: some record of the launch
// carries an alpha op (view_alpha.h) -- the kernel's alpha instantiation, as filters (resize_launch_kind: 0 all bilinear, 1 some bicubic, 2 some RESAMPLE
// filter) chooses among the one with the triangle alone, the one with both filters and the resample instantiation.
bool launch_dec_resize_exact(hipStream_t s, const DecResize *recs, const uint64_t *pre, const uint64_t *h_pre, uint32_t n, uint32_t lds_bytes, const DecFloat *flt, uint32_t filters,
                             bool any_alpha = false);
#ifdef FPNG_DEC_SYNC_TIMING
void dec_dump_sync_times(const char *path, uint32_t n_blocks); // (diagnostic build: dec_sync_kernel<false>'s per-workgroup time stamps of the last launch)
#endif
#ifdef FPNG_DEC_TILE_TIMING
void dec_dump_tile_times(const char *path, uint32_t n_items); // (diagnostic build: dec_unfilter_kernel's per-tile time stamps of the last launch)
#endif

} // namespace fpng_amd
