// crc_device.h -- the device side of the CRC-32 arithmetic, shared by the encoder's CRC pass (kernels.hip: crc_kernel,
// finalize_kernel) and the decoder's check of a file's IDAT CRC (decode.hip: dec_crc_kernel, dec_verify_kernel).  All values are
// raw CRCs (init 0, no final xor) in the reflected representation of zlib: bit 31 is x^0.
#pragma once
#include "kernels.h"

#include <hip/hip_runtime.h>

namespace fpng_amd {

constexpr int kCrcBlock = 256; // threads of a workgroup that computes a range's partial or folds a file's partials
static_assert(kCrcBlock == (int)kCrcFoldThreads, "crc_fold_depth counts with the fold's workgroup");

typedef uint32_t crc_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) crc_u32x4 *crc_gptr_cu128;
typedef const __attribute__((address_space(1))) uint8_t *crc_gptr_cu8;

__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ uint32_t dev_mulmod(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
#pragma unroll 8
    for (int i = 31; i >= 0; i--) {
        r ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
    }
    return r;
}

// four independent products, interleaved (the single product is a chain of 32 dependent steps)
__device__ __forceinline__ void dev_mulmod4(const uint32_t (&a)[4], const uint32_t (&b_in)[4], uint32_t (&r)[4])
{
    uint32_t b[4] = {b_in[0], b_in[1], b_in[2], b_in[3]};
    r[0] = r[1] = r[2] = r[3] = 0;
#pragma unroll 4
    for (int i = 31; i >= 0; i--) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            r[k] ^= b[k] & (0u - ((a[k] >> i) & 1u));
            b[k] = (b[k] >> 1) ^ (0xEDB88320u & (0u - (b[k] & 1u)));
        }
    }
}
__device__ __forceinline__ uint32_t dev_crc_byte(uint32_t c, uint32_t byte)
{
    c ^= byte;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    return c;
}

// The raw CRC partial of one range of `range_bytes` bytes that ends at byte offset range_end of `base` (16-byte aligned, like base
// itself), by a workgroup of kCrcBlock threads: per step the lanes cover one row of kCrcRowBytes, each lane keeps the CRC of its own
// 16-byte stripe with slice-by-16 tables that already contain the jump to its next piece (tab: CrcDeviceTables::striped in LDS).
// Bytes outside [data_begin, data_end) count as zero and are not read unless they share an aligned 16 bytes with bytes inside.
// The partial sits one row behind range_end; thread 0 gets it.
__device__ __forceinline__ uint32_t crc_range_partial(crc_gptr_cu8 base, int64_t data_begin, int64_t data_end, int64_t range_end, uint32_t range_bytes,
                                                      const uint32_t (*tab)[256], const CrcDeviceTables *tabs, uint32_t *red)
{
    const uint32_t tid = threadIdx.x;
    uint32_t c = 0;
    for (uint32_t row = 0; row < range_bytes / kCrcRowBytes; row++) {
        const int64_t o = range_end - range_bytes + (int64_t)row * kCrcRowBytes + tid * 16;
        uint32_t w[4] = {0, 0, 0, 0};
        if (o + 16 > data_begin && o < data_end) {
            const crc_u32x4 d = *(crc_gptr_cu128)(base + o);
            w[0] = d.x, w[1] = d.y, w[2] = d.z, w[3] = d.w;
            if (o < data_begin || o + 16 > data_end) { // zero the bytes outside [data_begin, data_end)
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    uint32_t m = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        const int64_t pos = o + 4 * k + b;
                        if (pos >= data_begin && pos < data_end) m |= 0xFFu << (8 * b);
                    }
                    w[k] &= m;
                }
            }
        }
        w[0] ^= c;
        uint32_t n = 0;
#pragma unroll
        for (int k = 0; k < 4; k++)
            n ^= tab[4 * k + 0][w[k] & 0xFF] ^ tab[4 * k + 1][(w[k] >> 8) & 0xFF] ^ tab[4 * k + 2][(w[k] >> 16) & 0xFF] ^
                 tab[4 * k + 3][w[k] >> 24];
        c = n;
    }
    // lane stripes now sit at range_end + 16*tid: move them all to range_end + one block row, fold
    c = wave_xor(dev_mulmod(c, tabs->lane_fix[tid]));
    if ((tid & 63) == 0) red[tid >> 6] = c;
    __syncthreads();
    return red[0] ^ red[1] ^ red[2] ^ red[3];
}

// The fold of a file's partials by a workgroup of kCrcBlock threads.  Partial j (pj[j]) sits (j ranges of 2^rl bytes + one row)
// before the common end point, which lies `pad` (< 16) zero bytes behind the data's end:  T = XOR_j p_j * X^j  with X = x^(8 * 2^rl);
// all needed constants are tabulated.  Returns (to thread 0) the raw CRC of the data; *len_pow (thread 0) = x^(8 * len), the factor
// that advances a CRC state in front of the data over len bytes.  red: kCrcBlock / 64 + 1 words of LDS.
__device__ __forceinline__ uint32_t crc_fold_partials(const CrcDeviceTables *tabs, const uint32_t *pj, uint32_t n_ranges, uint32_t rl, uint64_t len, uint32_t pad,
                                                      uint32_t *red, uint32_t *len_pow_out)
{
    const uint32_t t = threadIdx.x;
    const uint32_t g = crc_fold_depth(n_ranges); // each thread folds G = 2^g consecutive partials (crc_geometry.h)
    const uint32_t G = 1u << g;
    // (the constants of the later steps are asked for now: their loads travel together with those of the partials instead of
    // one round trip each behind the fold)
    const uint32_t group_pow = tabs->fold[crc_fold_group_row(rl, g)][t];
    const uint32_t len_pow = (t < 6) ? tabs->pow_byte[t][(len >> (8 * t)) & 0xFF] : 0x80000000u; // 0x80000000 = 1
    const uint32_t unpad = tabs->inv_row_pad[pad];
    uint32_t v = 0;
    {
        // partial i of the group times x^(8*range*i): independent multiplications, four at a time (a Horner chain would
        // be G dependent ones: G = 32 for a 16384^2 image)
        const uint32_t *xp = tabs->fold[crc_fold_step_row(rl)];
        for (uint32_t i = 0; i < G; i += 4) {
            uint32_t a[4], b[4], r[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t j = t * G + i + k;
                a[k] = (i + k < G && j < n_ranges) ? pj[j] : 0u;
                b[k] = xp[(i + k) & 255u];
            }
            dev_mulmod4(a, b, r);
            v ^= r[0] ^ r[1] ^ r[2] ^ r[3];
        }
    }
    // the thread's group starts t * G ranges before the common end point: one multiplication by a tabulated power, then
    // the groups simply XOR together (no multiplications inside the reduction)
    if (v && t) v = dev_mulmod(v, group_pow);
    v = wave_xor(v);
    // x^(8*len): six tabulated factors (one per byte of the length), multiplied as a tree by lanes 0..7 of wave 0
    uint32_t f = len_pow;
    if (t < 64) {
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) {
            const uint32_t other = (uint32_t)__shfl_down((int)f, o, 8);
            f = dev_mulmod(f, other);
        }
    }
    if ((t & 63) == 0) red[t >> 6] = v;
    if (t == 0) red[kCrcBlock / 64] = f;
    __syncthreads();
    const uint32_t folded = red[0] ^ red[1] ^ red[2] ^ red[3];
    if (t == 0) *len_pow_out = red[kCrcBlock / 64];
    return t == 0 ? dev_mulmod(folded, unpad) : 0u;
}

} // namespace fpng_amd
