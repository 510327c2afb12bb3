// crc_geometry.h -- how a file's bytes are cut into CRC ranges and how the ranges' partials are folded: the ONE text of the rule,
// shared by scan_job and finalize_job (kernels.hip), crc_fold_partials (crc_device.h) and the host's counts of a file's ranges
// (api.cpp crc_ranges_of, pipeline.cpp crc_ranges_for_end).  Plain C++, host and device, no HIP in it, so that the rule can be
// checked without a GPU (tests/cpp/crc_geometry.cpp; tests/assemble_geometry.py restates the comment below in Python).
//
//   A file is 58 head bytes, the zlib stream (zlib_size bytes, its last 4 the Adler-32), 16 tail bytes.  The CRC covers the data
//   [58, data_end), data_end = 58 + zlib_size - 4.
//
//   end_aligned = round_up(data_end, 16)          pad = end_aligned - data_end   (0 .. 15 zero bytes counted behind the data)
//
//   range size 2^rl, chosen per file by the scan:
//       span = 58 + zlib_size
//       want = max(4, 2048 / n_jobs)              (integer division; n_jobs = the files of the submission)
//       rl   = the least of 12 .. 16 with  (span >> rl) + 1 <= want  and  (span >> rl) + 1 <= crc_blocks,  else 16
//       rl   = 16 for a row band               (crc_blocks: the job's bound, ceil(max encoded size / 64 KiB) + 1)
//
//   range j (j = 0, 1, ...) is [end_aligned - (j + 1) * 2^rl, end_aligned - j * 2^rl): the ranges hang off the END of the data.
//       n_ranges = ceil((end_aligned - 48) / 2^rl)        (48 = the last multiple of 16 at or in front of the data's first byte)
//       the farthest range holds  sliver = (end_aligned - 48) mod 2^rl  bytes from 48 on (0: it is a full range), the first
//       10 of them head bytes that count as zero
//
//   fold (one workgroup of 256 threads): every thread takes 2^g consecutive partials,
//       g = the least with 256 * 2^g >= n_ranges
//   multiplies partial i of its group by fold[rl - 12][i] (i < 2^g <= 256) and its group by fold[rl + g - 12][thread], where
//   fold[e - 12][t] = x^(8 * 2^e * t), e = 12 .. 24 (CrcDeviceTables::fold[13][256]).  Both indices hold while a file has at
//   most 2^16 ranges (g <= 8), which every file below 4 GiB has at rl = 16; the smaller sizes are chosen only for files of at
//   most crc_blocks ranges.  The pad is undone with inv_row_pad[pad].
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FPNG_GEOM_FN __host__ __device__ inline
#else
#define FPNG_GEOM_FN inline
#endif

namespace fpng_amd {

constexpr uint32_t kCrcRangeLog2Min = 12, kCrcRangeLog2Max = 16;
constexpr uint32_t kCrcFoldThreads = 256;                 // = kCrcBlock (crc_device.h)
constexpr uint32_t kCrcFoldRows = 13, kCrcFoldCols = 256; // CrcDeviceTables::fold
constexpr uint32_t kCrcFirstPiece = 48;                   // the 16-byte piece the data's first byte (offset 58) lies in

// span = 58 + zlib_size
FPNG_GEOM_FN uint32_t crc_range_log2_for(uint64_t span, uint32_t n_jobs, uint32_t crc_blocks, bool whole_png)
{
    uint32_t want = 2048u / n_jobs; // blocks this job should get (512 / 256 / 128 measured: no better for single frames)
    want = want < 4u ? 4u : want;
    uint32_t rl = kCrcRangeLog2Min;
    while (rl < kCrcRangeLog2Max && (((span >> rl) + 1 > want) || ((span >> rl) + 1 > crc_blocks))) rl++;
    if (!whole_png) rl = kCrcRangeLog2Max; // row bands: every rank must cut the file into the same ranges (their CRC partials are XOR-ed)
    return rl;
}

FPNG_GEOM_FN int64_t crc_data_end(uint64_t zlib_size) { return (int64_t)(58 + zlib_size - 4); }
FPNG_GEOM_FN int64_t crc_end_aligned(int64_t data_end) { return (data_end + 15) & ~15ll; }
FPNG_GEOM_FN uint32_t crc_pad(int64_t data_end) { return (uint32_t)(crc_end_aligned(data_end) - data_end); }
FPNG_GEOM_FN uint32_t crc_n_ranges(int64_t end_aligned, uint32_t rl) { return (uint32_t)((end_aligned - kCrcFirstPiece + (1ll << rl) - 1) >> rl); }
FPNG_GEOM_FN uint32_t crc_sliver(int64_t end_aligned, uint32_t rl) { return (uint32_t)((end_aligned - kCrcFirstPiece) & ((1ll << rl) - 1)); }

// each thread of the fold takes 2^g consecutive partials
FPNG_GEOM_FN uint32_t crc_fold_depth(uint32_t n_ranges)
{
    uint32_t g = 0;
    while (((uint64_t)kCrcFoldThreads << g) < n_ranges) g++;
    return g;
}
// rows of CrcDeviceTables::fold: the powers inside a thread's group (columns 0 .. 2^g - 1), and the groups' (column = thread)
FPNG_GEOM_FN uint32_t crc_fold_step_row(uint32_t rl) { return rl - kCrcRangeLog2Min; }
FPNG_GEOM_FN uint32_t crc_fold_group_row(uint32_t rl, uint32_t g) { return rl + g - kCrcRangeLog2Min; }

} // namespace fpng_amd
