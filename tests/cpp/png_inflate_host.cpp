// png_inflate_host.cpp -- the general decode tier's per-wave logic (fpng_amd/csrc/png_inflate_core.h) on the CPU, lane by lane:
//     png_inflate_host <desired_chans> <file.png>...      one line per file:  <status> <w> <h> <channels_in_file> <hash> <guard>
// hash: the sum over the w * h * desired_chans pixel bytes of (byte + 1) * ((index + 1) * 0x9E3779B97F4A7C15), mod 2^64, 0 where the header is refused; guard: 1 when the bytes around the
// pixels and the scanlines are untouched.  The buffers have exactly the sizes the GPU path gives them (plus the guard bands, which
// the sanitizer build leaves out so that the first byte outside is the sanitizer's), so tests/test_png_inflate_cpu.py runs this
// program plainly and under -fsanitize=address,undefined.
#include "png_inflate_core.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace fpng_amd::pngi;

#ifndef PNGI_GUARD
#define PNGI_GUARD 64
#endif

int main(int argc, char **argv)
{
    if (argc < 3) {
        fprintf(stderr, "usage: %s <desired_chans> <file.png>...\n", argv[0]);
        return 2;
    }
    const uint32_t desired = (uint32_t)atoi(argv[1]);
    if (desired != 3 && desired != 4) return 2;
    InflateShared *ish = new InflateShared;
    UnfilterShared *ush = new UnfilterShared;
    for (int a = 2; a < argc; a++) {
        FILE *fp = fopen(argv[a], "rb");
        if (!fp) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        fseek(fp, 0, SEEK_END);
        const long size = ftell(fp);
        fseek(fp, 0, SEEK_SET);
        uint8_t *data = new uint8_t[size > 0 ? size : 1]; // (exactly the file: a read behind it is the sanitizer's)
        if (size > 0 && fread(data, 1, (size_t)size, fp) != (size_t)size) return 2;
        fclose(fp);
        File f = {};
        uint32_t chans = 0;
        uint32_t status = check_ihdr(data, (uint32_t)size, f.w, f.h, f.color, f.bpp, chans);
        unsigned long long hash = 0;
        int guard = 1;
        if (!status) {
            f.data = data, f.size = (uint32_t)size, f.dst_c = desired;
            f.scan_bytes = (uint64_t)f.h * (1 + (uint64_t)f.w * f.bpp);
            const size_t out_bytes = (size_t)f.w * f.h * desired;
            uint8_t *scan = new uint8_t[f.scan_bytes + 2 * PNGI_GUARD], *out = new uint8_t[out_bytes + 2 * PNGI_GUARD];
            memset(scan, 0xA5, f.scan_bytes + 2 * PNGI_GUARD), memset(out, 0xA5, out_bytes + 2 * PNGI_GUARD);
            f.scan = scan + PNGI_GUARD, f.out = out + PNGI_GUARD;
            State st = {};
            memset(ish, 0x5A, sizeof *ish), memset(ush, 0x5A, sizeof *ush); // (nothing is read that was not written: stale values would show)
            status = pngi_inflate(*ish, f, st);
            if (!status) status = pngi_unfilter(*ush, f, st);
            if (!status && f.color == 3 && st.trns_len) chans = 4;
            for (uint32_t i = 0; i < PNGI_GUARD; i++)
                guard &= scan[i] == 0xA5 && scan[PNGI_GUARD + f.scan_bytes + i] == 0xA5 && out[i] == 0xA5 && out[PNGI_GUARD + out_bytes + i] == 0xA5;
            for (size_t i = 0; i < out_bytes; i++) hash += (f.out[i] + 1ull) * ((i + 1) * 0x9E3779B97F4A7C15ull);
            if (status) hash = 0;
            delete[] scan;
            delete[] out;
        }
        printf("%u %u %u %u %016llx %d\n", status, f.w, f.h, chans, hash, guard);
        delete[] data;
    }
    delete ish;
    delete ush;
    return 0;
}
