// view_enhance_apply.cpp -- runs the host twin of the views calls' enhance stage (fpng_amd/csrc/view_enhance.h: enhance_apply_checked,
// the whole of fpng_amd_view_enhance_apply but for the error text) on the cases tests/test_views_enhance_cpu.py sends on standard
// input, one
//   "<w> <h> <kind> <op> <reserved> <factor>"                 (the factor as a C99 hexadecimal float: exact)
// per line.  The three source planes are, by kind: 0 in[c][y * w + x] = (7 x + 13 y + x y + 50 c) & 255; 1 solid 17 + c; 2 two values,
// (x + y) & 1 ? 255 : 0 + c; 3 a narrow range, 100 + ((x + 3 y + c) % 7) -- in a heap block of exactly 3 * w * h bytes, as the output
// is: a read or a write past either of them (the 3 x 3 filter at the frame) is the address sanitizer's to find.  Per case one line:
// "ok <the 3 * w * h bytes of E as hex>", or "refused <why>".  Host-only: built with the system's C++ compiler and its sanitizers,
// no HIP, nothing loaded into an interpreter.
#include "view_enhance.h"

#include <cstdio>
#include <cstdlib>

int main()
{
    using namespace fpng_amd;
    unsigned w, h, kind, op, reserved;
    float factor;
    unsigned long lines = 0;
    while (scanf("%u %u %u %u %u %a", &w, &h, &kind, &op, &reserved, &factor) == 6) {
        if (!w || !h || w > 4096 || h > 4096 || kind > 3) {
            fprintf(stderr, "case %lu is outside the program's limits\n", lines);
            return 2;
        }
        fpng_amd_view_enhance rec = {};
        rec.op = op, rec.factor = factor, rec.reserved[1] = reserved;
        const size_t n = (size_t)w * h;
        uint8_t *const in = (uint8_t *)malloc(3 * n), *const out = (uint8_t *)malloc(3 * n);
        if (!in || !out) return 3;
        for (unsigned c = 0; c < 3; c++)
            for (unsigned y = 0; y < h; y++)
                for (unsigned x = 0; x < w; x++)
                    in[c * n + (size_t)y * w + x] = kind == 0   ? (uint8_t)(7u * x + 13u * y + x * y + 50u * c)
                                                    : kind == 1 ? (uint8_t)(17u + c)
                                                    : kind == 2 ? (uint8_t)((x + y) & 1u ? 255u : c)
                                                                : (uint8_t)(100u + (x + 3u * y + c) % 7u);
        const char *why = nullptr;
        if (enhance_apply_checked(&rec, w, h, in, out, &why) != FPNG_AMD_OK)
            printf("refused %s\n", why);
        else {
            printf("ok ");
            for (size_t k = 0; k < 3 * n; k++) printf("%02x", out[k]);
            printf("\n");
        }
        free(in), free(out);
        lines++;
    }
    if (!feof(stdin)) {
        fprintf(stderr, "bad input behind %lu cases\n", lines);
        return 2;
    }
    return 0;
}
