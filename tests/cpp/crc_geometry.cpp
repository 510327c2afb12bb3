// crc_geometry.cpp -- prints the rule of fpng_amd/csrc/crc_geometry.h for the files tests/test_crc_geometry_cpu.py sends on standard
// input, one "<span> <n_jobs> <crc_blocks>" per line (span = 58 + zlib_size: the file's size less its 16 tail bytes).  Per file one line:
//   "<span> <n_jobs> <crc_blocks> <rl> <n_ranges> <g> <pad> <sliver> <fold step row> <fold group row>"
// It also reads the entries of a table shaped like CrcDeviceTables::fold that a fold of this file reads last -- the step row's
// column 2^g - 1 and the group row's column 255 -- so that an index outside the table stops the program under the sanitizers.
// Host-only: built with the system's C++ compiler and its sanitizers, no HIP.
#include "crc_geometry.h"

#include <cstdio>
#include <cstring>

int main()
{
    using namespace fpng_amd;
    typedef uint32_t FoldRow[kCrcFoldCols];
    FoldRow *fold = new FoldRow[kCrcFoldRows];
    memset(fold, 0, sizeof(FoldRow) * kCrcFoldRows);
    unsigned long long span;
    unsigned n_jobs, crc_blocks;
    unsigned long lines = 0;
    uint32_t sum = 0;
    while (scanf("%llu %u %u", &span, &n_jobs, &crc_blocks) == 3) {
        if (span < 64 || !n_jobs || !crc_blocks) {
            fprintf(stderr, "file %llu %u %u is no file\n", span, n_jobs, crc_blocks);
            return 2;
        }
        const uint32_t rl = crc_range_log2_for(span, n_jobs, crc_blocks, true);
        const int64_t data_end = crc_data_end(span - 58), end_aligned = crc_end_aligned(data_end);
        const uint32_t n_ranges = crc_n_ranges(end_aligned, rl), g = crc_fold_depth(n_ranges);
        const uint32_t step_row = crc_fold_step_row(rl), group_row = crc_fold_group_row(rl, g);
        sum += fold[step_row][(1u << g) - 1u] + fold[group_row][kCrcFoldThreads - 1u];
        printf("%llu %u %u %u %u %u %u %u %u %u\n", span, n_jobs, crc_blocks, rl, n_ranges, g, crc_pad(data_end), crc_sliver(end_aligned, rl), step_row, group_row);
        lines++;
    }
    delete[] fold;
    if (!feof(stdin) || sum) {
        fprintf(stderr, "bad input behind %lu files\n", lines);
        return 2;
    }
    // a row band's files are cut into ranges of 64 KiB whatever their size
    if (crc_range_log2_for(4096, 1, 70000, false) != kCrcRangeLog2Max) return 3;
    return 0;
}
