// float_store.h -- how the decoder's destinations (bytes, or the elements of fpng_amd_decode_batch_planar_float, _crop, _resize and
// the views calls) round and store one element: the ONE text, shared by the kernels of decode.hip, resize.hip, resize_color.hip
// and view_post.hip.  Device code only.  kDtype: -1 bytes, else FPNG_AMD_F32 = 0, F16 = 1, BF16 = 2.
#pragma once
#include "decode.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fpng_amd {

// elements at any multiple of their size
typedef float __attribute__((aligned(4))) f32_a;
typedef uint16_t __attribute__((aligned(2))) u16_a;
// float -> the bits of a 2-byte element, round to nearest even (kDtype: FPNG_AMD_F16 = 1, FPNG_AMD_BF16 = 2)
template <int kDtype> __device__ __forceinline__ uint16_t half_bits(float f)
{
    asm("" : "+v"(f)); // (the fp32 result as it is: no fused multiply-add that rounds straight to the narrow type)
    if constexpr (kDtype == 1) return __builtin_bit_cast(uint16_t, (_Float16)f);
    else return __builtin_bit_cast(uint16_t, (__bf16)f);
}

// scale and bias of the FILE's channel c: a select, not an index into the argument, which would put it into private memory
__device__ __forceinline__ void float_scale_bias(const DecFloat &flt, uint32_t c, float &sc, float &bi)
{
    sc = c == 0 ? flt.scale[0] : c == 1 ? flt.scale[1] : c == 2 ? flt.scale[2] : flt.scale[3];
    bi = c == 0 ? flt.bias[0] : c == 1 ? flt.bias[1] : c == 2 ? flt.bias[2] : flt.bias[3];
}

// byte v of a channel with scale sc and bias bi -> the bits of the destination's element
template <int kDtype> __device__ __forceinline__ uint32_t byte_elem_bits(uint32_t v, float sc, float bi)
{
    if constexpr (kDtype < 0) return v;
    else {
        const float f = __builtin_fmaf((float)v, sc, bi);
        if constexpr (kDtype == 0) return __builtin_bit_cast(uint32_t, f);
        else return half_bits<kDtype>(f);
    }
}

// the float u (0 .. 255: a colour matrix's result, or the alpha byte) -> the bits of the destination's element; bytes round here
template <int kDtype> __device__ __forceinline__ uint32_t float_elem_bits(float u, float sc, float bi)
{
    if constexpr (kDtype < 0) return (uint32_t)__builtin_rintf(u); // (0 .. 255: ties to even)
    else {
        const float f = __builtin_fmaf(u, sc, bi);
        if constexpr (kDtype == 0) return __builtin_bit_cast(uint32_t, f);
        else return half_bits<kDtype>(f);
    }
}

// the bits b of an element to p
template <int kDtype> __device__ __forceinline__ void elem_store(uint8_t *p, uint32_t b)
{
    if constexpr (kDtype < 0) *p = (uint8_t)b;
    else if constexpr (kDtype == 0) *(f32_a *)p = __builtin_bit_cast(float, b);
    else *(u16_a *)p = (uint16_t)b;
}

} // namespace fpng_amd
