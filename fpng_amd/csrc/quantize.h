// quantize.h -- float source element -> PNG byte: the ONE text of the rule of fpng_amd_encode_submit_planar_float
// (include/fpng_amd.h), shared by every kernel that reads a float source (kernels.hip) and by the host function
// fpng_amd_quantize_float (api.cpp) that the CPU tests judge against the rule.
//
//   y    = fmaf((float)x, scale, bias)                     one fp32 fused multiply-add; f16 / bf16 widen exactly
//   byte = y is NaN ? 0 : (uint8) min(max(rint(y), 0), 255)       rint: round to nearest, ties to even
//
// The clamp comes first here: fmaxf / fminf return the operand that is a number, so a NaN leaves fmaxf(y, 0) as 0, and rounding
// a value already inside [0, 255] gives what clamping the rounded value gives (0 and 255 are integers, rint is monotonic).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FPNG_QUANT_FN __host__ __device__ inline
#else
#define FPNG_QUANT_FN inline
#endif

namespace fpng_amd {

// element types of a float source: the values of FPNG_AMD_F32 / _F16 / _BF16
constexpr uint32_t kF32 = 0, kF16 = 1, kBF16 = 2;

FPNG_QUANT_FN float bits_to_float(uint32_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    std::memcpy(&f, &u, 4);
    return f;
#endif
}

// binary16 bits -> the same value as fp32 (exact: every f16, denormals included, is an fp32 normal or zero)
FPNG_QUANT_FN float widen_f16(uint32_t h)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, (uint16_t)h);
#else
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    if (e == 31u) return bits_to_float(sign | 0x7F800000u | (m << 13)); // inf / NaN
    if (e) return bits_to_float(sign | ((e + 112u) << 23) | (m << 13));
    const float v = (float)m * 5.9604644775390625e-8f; // m * 2^-24: zero and the denormals
    return sign ? -v : v;
#endif
}
FPNG_QUANT_FN float widen_bf16(uint32_t h) { return bits_to_float(h << 16); }

// the element whose bits (16-bit types: in the low half) are `bits`
template <uint32_t DT> FPNG_QUANT_FN float widen(uint32_t bits)
{
    return DT == kF32 ? bits_to_float(bits) : DT == kF16 ? widen_f16(bits & 0xFFFFu) : widen_bf16(bits & 0xFFFFu);
}

// the second line of the rule on its own: what yuv.h rounds a colour matrix's sums with
FPNG_QUANT_FN uint32_t round_to_byte(float y)
{
    y = fminf(fmaxf(y, 0.0f), 255.0f); // (NaN -> 0)
    return (uint32_t)(int32_t)rintf(y);
}

FPNG_QUANT_FN uint32_t quantize(float x, float scale, float bias) { return round_to_byte(fmaf(x, scale, bias)); }

} // namespace fpng_amd
