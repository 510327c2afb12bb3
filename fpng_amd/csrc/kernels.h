// kernels.h -- host/device shared structures and kernel launchers (internal).
#pragma once
#include "fpng_amd.h"
#include "format.h"
#include "pack.h"
#include "crc_geometry.h"

#include <hip/hip_runtime_api.h>

namespace fpng_amd {

// CRC work decomposition: every block owns kCrcRangeBytes of the (16-byte aligned) file span,
// 256 lanes x 16 B = one 4 KiB block row per step.
constexpr uint32_t kCrcRangeBytes = 1u << 16;
constexpr uint32_t kCrcRowBytes = 4096;
static_assert(kCrcRangeBytes == 1u << kCrcRangeLog2Max && kCrcRowBytes == 1u << kCrcRangeLog2Min, "crc_geometry.h: range sizes from one block row to kCrcRangeBytes");

// The form of a job's source pixels: ONE numbering for Job::src_bytes and for the template argument of everything that reads pixels
// (hist_kernel, encode_rows_kernel, stored_kernel and what they call).  kFormEx3 / kFormEx4 are the bytes of an _ex source pixel.
constexpr int kFormPacked = 0; // fpng_amd_encode_submit: R,G,B[,A] bytes, rows bpl apart (the jobs' layout fields stay 0)
constexpr int kFormPlanar = 1; // fpng_amd_encode_submit_planar
constexpr int kFormEx = 2;     // an _ex job of either pixel size, read from the job at run time (never in Job::src_bytes; the row walk has none)
constexpr int kFormEx3 = 3, kFormEx4 = 4; // fpng_amd_encode_submit_ex
constexpr int kFloatLayout = 16; // + dtype (FPNG_AMD_F32 / _F16 / _BF16): fpng_amd_encode_submit_planar_float
constexpr int kYuvLayout = 32;   // + surface (FPNG_AMD_YUV_*): fpng_amd_encode_submit_yuv -- always 3 channels in the file
constexpr int kYuvSurfaces = 4;
constexpr bool is_float_layout(int form) { return form >= kFloatLayout && form < kYuvLayout; }
constexpr bool is_yuv_layout(int form) { return form >= kYuvLayout && form < kYuvLayout + kYuvSurfaces; }
// (YUV surfaces are walked as planar ones: their loads hand the walk a lane's bytes per FILE channel, yuv.h's rule applied)
constexpr bool is_planar_layout(int form) { return form == kFormPlanar || is_float_layout(form) || is_yuv_layout(form); }
// SourceForms::kind of a YUV batch: an internal kind, reached through fpng_amd_encode_submit_yuv only -- the generic entry points
// keep refusing it as an unknown desc_kind, and there is no public FPNG_AMD_DESC_* name for it
constexpr uint32_t kDescYuv = 4;

// One unit of work: a whole image, or a band of rows of one image (multi-GPU).
struct Job {
    const uint8_t *rows;      // first row of the job (row y0 of the image)
    const uint8_t *row_above; // row y0-1, used only when y0 > 0
    uint8_t *out;             // whole_png: start of the .png file; band: start of the band's byte window
    const TokenTable *table;  // device table (1-pass static or per-job dynamic)
    uint64_t out_cap;
    uint64_t start_bit;       // band: absolute zlib bit of the band's first token (ignored if is_first)
    int64_t bit_bias;         // destination bit = zlib bit + bit_bias  (whole_png: 58*8)
    uint32_t w, c, bpl, nrows, y0, h_total, flags;
    uint32_t row_base;        // index of the job's first row in the per-row scratch arrays
    uint32_t one_pass, whole_png, is_first, is_last;
    uint32_t crc_blocks;      // upper bound of CRC ranges for this job
    uint64_t band_zlib_size;  // row bands, placement phase: size of the WHOLE image's zlib stream (bands share the file's geometry)
    // whole images: every row is first encoded into its own dword-aligned stream in scratch ("local stream"),
    // assemble_kernel then shifts the streams into place.  Row r lives at local + local_base + r*local_stride.
    uint64_t local_base;      // dwords
    uint32_t local_stride;    // dwords per row (worst-case token bits of a row + slack)
    uint32_t local_pad;
    // source layout of fpng_amd_encode_submit_ex jobs (zero elsewhere; read only by the kernels of their form): row r of the job starts at
    // rows + r * pitch, a pixel is src_bytes bytes, and v_perm_b32 with selector `sel` turns a source pixel's dword into the PNG's
    // R,G,B[,A] bytes (0x0c = a zero byte).  These words were reserved before: the record stays 224 bytes and png_header where it
    // was, so the other kernels' code is, instruction for instruction, the same (tools/isa_diff.py)
    int64_t pitch;            // signed bytes from one row to the next
    uint32_t src_bytes;       // the job's source form (kForm*, above):kFormEx3 / kFormEx4 = the bytes of a source pixel; kFormPlanar: a byte per pixel
                              // and plane; kFloatLayout + dtype: planes of floats, pitches in bytes of the float source;
                              // kYuvLayout + surface: `rows` = the luma plane's top row, `pitch` = the row pitch of all planes,
                              // `plane_pitch` = the chroma offset (yuv.h)
    uint32_t sel;
    int64_t plane_pitch;      // planar jobs: signed bytes from one channel's plane to the next (R -> G -> B [-> A]); `rows` is the R plane's top row
    uint8_t png_header[60];   // 58 bytes used (reference fpng.cpp:1767-1791), IDAT length patched on device
};
static_assert(sizeof(Job) == 224 && offsetof(Job, pitch) == 136 && offsetof(Job, plane_pitch) == 152 && offsetof(Job, png_header) == 160, "Job layout");

struct RowInfo {
    uint32_t bits; // token bits of the row
    uint32_t s1;   // Adler raw sums of the filtered row mod 65521
    uint32_t s2;
    uint32_t pad;
};

struct JobState {
    uint64_t token_end_bit; // zlib bit position after the last token
    uint64_t zlib_size;     // bytes of the zlib stream incl. Adler
    uint32_t mode;          // 0 compressed, 1 stored
    uint32_t last_unit_bits;
    uint32_t s1, s2;        // Adler raw sums of the job's filtered bytes
    uint32_t adler, crc;
    uint32_t status;        // nonzero = device-side failure, reported in fpng_amd_result.status (kStatus*)
    uint32_t range_log2;    // log2 of the bytes one assemble/crc block covers (12..16; 0 = 16), chosen by scan_kernel
    uint64_t reserved[2];
};

// JobState::status: a stored outcome whose 58 + zlib_size exceeds UINT32_MAX (FPNG_AMD_STATUS_STORED_TOO_LARGE): scan_kernel decides
// it, and assemble / stored_kernel / finalize then write nothing of that file.  (kStatusArenaFull = 2, packed submissions: pack.h)
constexpr uint32_t kStatusStoredTooLarge = 1;
// JobState::zlib_size of a file of a packed submission that is refused (by pack_place_kernel, or by the scan before it).  assemble_kernel has no look at the status on its way to a compressed file's
// rows (before packed submissions only stored files could be refused), but it leaves -- as the stored forms and crc_kernel do -- when
// its range holds nothing of the data [58, 58 + zlib_size - 4): with this value that interval is [58, 0), empty for every range, so
// no workgroup gets as far as Job::out, which such a file does not have.  (Modulo 2^64: 58 + kZlibSizeNoFile - 4 == 0.)
constexpr uint64_t kZlibSizeNoFile = (uint64_t)4 - kPngHeaderBytes;

struct Result {
    uint64_t png_size;
    uint32_t mode;
    uint32_t status;
};

// device-side CRC constants (superset of CrcTables in format.h)
struct CrcDeviceTables {
    uint32_t striped[16][256]; // raw CRC of byte b, followed by (15-k) + (kCrcRowBytes-16) zero bytes
    uint32_t lane_fix[256];    // x^(8*(kCrcRowBytes - 16*tid)): lane stripe -> one row past the range end
    uint32_t pow2[48];         // x^(8*2^i)
    uint32_t inv_pad[16];      // x^(-8*p)
    uint32_t inv_row;          // x^(-8*kCrcRowBytes)
    uint32_t pad[15];
    uint32_t inv_row_pad[16];  // x^(-8*(kCrcRowBytes + p)): inv_row * inv_pad[p]
    uint32_t fold[kCrcFoldRows][kCrcFoldCols]; // fold[e-12][t] = x^(8 * 2^e * t), e = 12..24: thread t's group of partials -> the common end point
    uint32_t pow_byte[6][256]; // pow_byte[k][b] = x^(8 * b * 256^k): x^(8n) is the product of six entries
};
void build_crc_device_tables(CrcDeviceTables *t);

// The sources of one submission, as far as the launchers of the three stages that read pixels (hist, encode_rows, assemble's stored
// files) need them to pick their kernels.  Only those kernels have a form per kind; the rest of the chain is shared as it is.
struct FloatQuant {
    float scale[4], bias[4]; // per file channel R, G, B, A
};
// the 3 x 4 matrix of a YUV submission (yuv.h): file channel c = m[c][0] Y + m[c][1] Cb + m[c][2] Cr + m[c][3]
struct YuvMatrix {
    float m[3][4];
};
struct SourceForms {
    // FPNG_AMD_DESC_* of the batch, or kDescYuv.  _IMAGE: kFormPacked jobs; _EX: jobs with a source layout (Job::pitch / src_bytes / sel);
    // _PLANAR: planar jobs (Job::plane_pitch); _PLANAR_FLOAT: planar jobs whose planes hold elements of `dtype`, which the kernels turn
    // into bytes as they load them (quantize.h) -- fq's constants are the submission's and travel in the kernel arguments: the Job record is full
    uint32_t kind = FPNG_AMD_DESC_IMAGE;
    // kDescYuv: jobs of kYuvLayout + dtype, dtype = the surface; ym's matrix travels as fq does
    uint32_t dtype = 0; // FPNG_AMD_F32 / _F16 / _BF16; kDescYuv: FPNG_AMD_YUV_*
    // one row kernel instantiation per bit.  _EX: bit 0 = 3-byte sources, bit 1 = 4-byte sources with 4 channels, bit 2 = 4-byte sources
    // with 3; every other kind: bit 0 = the batch has 3-channel jobs, bit 1 = 4-channel jobs
    uint32_t mask = 0;
    // _IMAGE, _EX: the 4-channel jobs' pixels lie mostly in rows of kWideRowPixels and more (their walk then runs with seven waves per SIMD instead of eight: kernels.hip)
    bool wide4 = false;
    FloatQuant fq = {};
    YuvMatrix ym = {};
};
constexpr uint32_t kWideRowPixels = 3584; // (same-box A/B: 3840-pixel rows gain with six waves, 3072-pixel rows lose 1 % in 1-pass)
// one plain image or row band of `chans` channels and rows of w pixels
inline SourceForms plain_source(uint32_t chans, uint32_t w) { return {FPNG_AMD_DESC_IMAGE, 0, chans == 3 ? 1u : 2u, w >= kWideRowPixels, {}}; }
// (src defaults to plain images: what the stages that look at no mask need to know of row bands and training sets)
void launch_hist(hipStream_t s, const Job *jobs, uint32_t n_jobs, uint32_t max_rows, uint32_t *hist, SourceForms src = {});
void launch_scan(hipStream_t s, const Job *jobs, uint32_t n_jobs, const RowInfo *rows, uint64_t *row_off, JobState *states);
// fpng_amd_encode_submit_packed: the scan without the heads (the jobs have no `out` yet), then pack_place_kernel -- one workgroup:
// the rule of pack.h over the sizes the scan decided; it patches jobs[i].out / out_cap and refuses (JobState::status =
// kStatusArenaFull, JobState::zlib_size = kZlibSizeNoFile) what finds no room -- and pack_heads_kernel, which writes the heads of
// the placed files.  Three launches.  assemble / stored_kernel / finalize behind them are the ones every submission runs.
struct PackArgs {
    uint8_t *arena;
    uint64_t cap;
    uint32_t align, lead; // align: the effective one (pack_align_of)
    uint64_t *d_table;    // device, 2 * (n + 1) words, or NULL
    uint64_t *h_offsets;  // pinned host memory (device-visible), n + 2 words: the files' offsets, total, files placed
};
void launch_scan_packed(hipStream_t s, Job *jobs, uint32_t n_jobs, const RowInfo *rows, uint64_t *row_off, JobState *states, const PackArgs &pa);
void launch_encode_rows(hipStream_t s, const Job *jobs, uint32_t n_jobs, uint32_t max_rows, RowInfo *rows, JobState *states, uint32_t *local, SourceForms src);
// one job per submission: the record travels in the kernel arguments and is left at d_job for the kernels that follow
void launch_encode_rows_first(hipStream_t s, const Job &job, Job *d_job, RowInfo *rows, JobState *states, uint32_t *local);
void launch_hist_first(hipStream_t s, const Job &job, Job *d_job, uint32_t *hist);
// adler_parts (whole images; two words per CRC range and job, or NULL for row bands): where the workgroups of an image that
// fell back to stored blocks leave their range's share of the Adler-32.  Every kind but _IMAGE: stored_kernel of the kind's form writes
// the stored files first, and assemble_kernel then takes their CRC in place
void launch_assemble(hipStream_t s, const Job *jobs, uint32_t n_jobs, uint32_t max_crc_blocks, JobState *states,
                     const uint64_t *row_off, const uint32_t *local, const CrcDeviceTables *tabs, uint32_t *partials, uint32_t *adler_parts, SourceForms src = {});
void launch_crc(hipStream_t s, const Job *jobs, uint32_t n_jobs, uint32_t max_crc_blocks, const JobState *states,
                const CrcDeviceTables *tabs, uint32_t *partials);
void launch_finalize(hipStream_t s, const Job *jobs, uint32_t n_jobs, uint32_t max_crc_blocks, const RowInfo *rows,
                     JobState *states, const CrcDeviceTables *tabs, const uint32_t *partials, const uint32_t *adler_parts, Result *results);
// table training: sums[0..288) += the 16-bit adjusted histogram of every image (hist_all: 288 counters per image)
void launch_train_accumulate(hipStream_t s, const uint32_t *hist_all, uint32_t n_images, uint64_t *sums);
// dst[0..16) |= src[0..16): the 16-byte piece two neighbouring band windows share (each holds zeros where the other's bits are)
void launch_or_piece(hipStream_t s, uint8_t *dst, const uint8_t *src);
// rezero: leave the counters that were read zeroed (the next 2-pass submission's histogram pass needs no clearing in front of it)
void launch_build_dynamic(hipStream_t s, const Job *jobs, uint32_t n_jobs, const uint32_t *hist, TokenTable *tables, uint32_t rezero);

} // namespace fpng_amd
