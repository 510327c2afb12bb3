// png_unfilter_box_host.cpp -- the views call's per-wave logic (fpng_amd/csrc/png_inflate_core.h: pngi_inflate with only the rows a
// box needs kept, then pngi_unfilter_box) on the CPU, lane by lane:
//     png_unfilter_box_host <planes> <x> <y> <w> <h> <file.png>...      one line per file:  <status> <hash> <guard>
// status: the tier's, or 68 where the box is empty or leaves the image (nothing is run then); hash: the sum over the planes * w * h
// plane bytes of (byte + 1) * ((index + 1) * 0x9E3779B97F4A7C15), mod 2^64, 0 where the status is not 0; guard: 1 when the bytes
// around the planes and the scanlines are untouched.  The scanlines are (y + h) * (1 + bytes per row) bytes and the planes
// planes * w * h, exactly what the GPU path gives them (plus the guard bands, which the sanitizer build leaves out so that the first
// byte outside is the sanitizer's), so tests/test_png_views_box_cpu.py runs this program plainly and under
// -fsanitize=address,undefined.
#include "png_inflate_core.h"

#include <cstdio>
#include <cstdlib>

using namespace fpng_amd::pngi;

#ifndef PNGI_GUARD
#define PNGI_GUARD 64
#endif

int main(int argc, char **argv)
{
    if (argc < 7) {
        fprintf(stderr, "usage: %s <planes> <x> <y> <w> <h> <file.png>...\n", argv[0]);
        return 2;
    }
    Box box = {};
    box.n_planes = (uint32_t)atoi(argv[1]);
    box.x = (uint32_t)strtoul(argv[2], nullptr, 10), box.y = (uint32_t)strtoul(argv[3], nullptr, 10);
    box.w = (uint32_t)strtoul(argv[4], nullptr, 10), box.h = (uint32_t)strtoul(argv[5], nullptr, 10);
    if (box.n_planes != 3 && box.n_planes != 4) return 2;
    InflateShared *ish = new InflateShared;
    UnfilterShared *ush = new UnfilterShared;
    for (int a = 6; a < argc; a++) {
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
        if (!status && (!box.w || !box.h || (uint64_t)box.x + box.w > f.w || (uint64_t)box.y + box.h > f.h)) status = 68;
        unsigned long long hash = 0;
        int guard = 1;
        if (!status) {
            const uint64_t stride = 1 + (uint64_t)f.w * f.bpp;
            f.data = data, f.size = (uint32_t)size;
            f.scan_bytes = (uint64_t)(box.y + box.h) * stride, f.need_bytes = (uint64_t)f.h * stride; // (kept: the box's rows and those above)
            const size_t plane_bytes = (size_t)box.w * box.h * box.n_planes;
            uint8_t *scan = new uint8_t[f.scan_bytes + 2 * PNGI_GUARD], *planes = new uint8_t[plane_bytes + 2 * PNGI_GUARD];
            memset(scan, 0xA5, f.scan_bytes + 2 * PNGI_GUARD), memset(planes, 0xA5, plane_bytes + 2 * PNGI_GUARD);
            f.scan = scan + PNGI_GUARD, box.planes = planes + PNGI_GUARD;
            State st = {};
            memset(ish, 0x5A, sizeof *ish), memset(ush, 0x5A, sizeof *ush); // (nothing is read that was not written: stale values would show)
            status = pngi_inflate(*ish, f, st);
            if (!status) status = pngi_unfilter_box(*ush, f, st, box);
            for (uint32_t i = 0; i < PNGI_GUARD; i++)
                guard &= scan[i] == 0xA5 && scan[PNGI_GUARD + f.scan_bytes + i] == 0xA5 && planes[i] == 0xA5 && planes[PNGI_GUARD + plane_bytes + i] == 0xA5;
            for (size_t i = 0; i < plane_bytes; i++) hash += (box.planes[i] + 1ull) * ((i + 1) * 0x9E3779B97F4A7C15ull);
            if (status) hash = 0;
            delete[] scan;
            delete[] planes;
        }
        printf("%u %016llx %d\n", status, hash, guard);
        delete[] data;
    }
    delete ish;
    delete ush;
    return 0;
}
