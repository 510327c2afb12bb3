// float_store.h -- how the decoder's float destinations (fpng_amd_decode_batch_planar_float, _crop, _resize) round and store one
// element: the ONE text, shared by the kernels of decode.hip and resize.hip.  Device code only.
#pragma once
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

} // namespace fpng_amd
