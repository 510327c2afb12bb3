// resize_bounds.cpp -- prints what the resize kernels' LDS layout rests on (fpng_amd/csrc/resize.h) for the pairs
// tests/test_resize_bounds_cpu.py sends on standard input, one "<filter> <in> <out>" per line.  Per pair one line:
//   "<filter> <in> <out> <resize_max_taps> <resize_tile_rows> <resize_tile_lds(taps, taps, rows)> <count> <span>"
// count: the most taps any output sample has (resize_taps_of); span: the most source samples any run of min(kResizeTileH, out)
// consecutive output samples reaches (end - begin of resize_source_span) -- what a tile's T buffer must hold.
// Host-only: built with the system's C++ compiler and its sanitizers, no HIP.
#include "resize.h"

#include <cstdio>

int main()
{
    using namespace fpng_amd;
    unsigned filter, in, out;
    unsigned long lines = 0;
    while (scanf("%u %u %u", &filter, &in, &out) == 3) {
        if (filter >= kResizeFilters || !resize_scale_ok(in, out, filter)) {
            fprintf(stderr, "pair %u %u %u is outside the limits\n", filter, in, out);
            return 2;
        }
        const uint32_t taps = resize_max_taps(in, out, filter), rows = resize_tile_rows(in, out, filter);
        uint32_t most_count = 0, most_span = 0;
        for (uint32_t o = 0; o < out; o++) {
            uint32_t first = 0;
            const uint32_t count = resize_taps_of(filter, in, out, o, &first);
            if (count > most_count) most_count = count;
        }
        const uint32_t n = out < kResizeTileH ? out : kResizeTileH;
        for (uint32_t o0 = 0; o0 + n <= out; o0++) {
            uint32_t begin = 0, end = 0;
            resize_source_span(filter, in, out, o0, n, &begin, &end);
            if (end - begin > most_span) most_span = end - begin;
        }
        printf("%u %u %u %u %u %u %u %u\n", filter, in, out, taps, rows, resize_tile_lds(taps, taps, rows), most_count, most_span);
        lines++;
    }
    if (!feof(stdin)) {
        fprintf(stderr, "bad input behind %lu pairs\n", lines);
        return 2;
    }
    return 0;
}
