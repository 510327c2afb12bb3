// pack.h -- where the files of a packed submission (fpng_amd_encode_submit_packed, include/fpng_amd.h) go in the caller's arena:
// the ONE text of the placement rule, shared by pack_place_kernel (kernels.hip), which applies it to the sizes scan_kernel decided,
// and by the host function fpng_amd_pack_place (api.cpp) that the CPU tests judge against a model.
//
//   cursor = 0
//   for every file i, in descriptor order:
//       status_i != 0 (refused before placement: STORED_TOO_LARGE)  ->  offset 0, size 0, the cursor stays
//       offset_i = round_up(cursor, align) + lead
//       extent_i = round_up(png_size_i + kPackTail, 16)
//       cursor   = offset_i + extent_i                               whether or not the file fits
//       offset_i + extent_i <= arena_cap  ->  the file is written at arena + offset_i
//       else                              ->  status ARENA_FULL, offset 0, size 0, not a byte of it is written
//   total = offset + png_size of the last file that was written (0: none)
//
// round_up(cursor, align) is a multiple of `align`, so with  stride_i = round_up(lead + extent_i, align)  (0 for a file refused
// before placement) it is the exclusive prefix SUM of the strides: the rule is a plain scan, which is how the kernel computes it
// (wave scan + LDS across the waves).  The cursor never goes back, so every file behind the first one that does not fit is refused too.
//
// kPackTail (E): the bytes behind png_size that the chain may touch.  From the code: assemble_kernel and the stored forms store whole
// 16-byte pieces of the FILE (offsets that are multiples of 16 from its first byte), the last one ending at
// round_up(58 + zlib_size - 4, 16) <= png_size - 5 (png_size = 58 + zlib_size + 16); the head (scan / pack_heads_kernel) ends at
// round_up(58 + prefix bytes, 16), in front of the Adler-32; finalize_kernel stores single bytes up to png_size exactly; loads (the
// head pieces, a stored image's bytes for the CRC) stay inside the same pieces.  So E = 0, and the extent only rounds png_size up to
// the 16-byte piece that file starts must keep.  (fpng_amd_encode_image_sharded asks for + 64 for another reason: its band windows
// are copied in whole 16-byte pieces that may begin and end outside the band.)
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FPNG_PACK_FN __host__ __device__ inline
#else
#define FPNG_PACK_FN inline
#endif

namespace fpng_amd {

constexpr uint32_t kPackTail = 0;
constexpr uint32_t kPackMinAlign = 16, kPackMaxAlign = 65536, kPackMaxLead = 65536;
// JobState::status / fpng_amd_packed_result.status: the file found no room in the arena (FPNG_AMD_STATUS_ARENA_FULL)
constexpr uint32_t kStatusArenaFull = 2;

FPNG_PACK_FN uint64_t pack_extent(uint64_t png_size) { return (png_size + kPackTail + 15u) & ~15ull; }

// what file i adds to the aligned cursor: 0 when it was refused before placement
FPNG_PACK_FN uint64_t pack_stride(uint64_t png_size, uint32_t status_in, uint32_t align, uint32_t lead)
{
    return status_in ? 0u : (lead + pack_extent(png_size) + (align - 1u)) & ~(uint64_t)(align - 1u);
}

// file i, given the sum of the strides in front of it: does it fit, and where.  Returns the file's status.
FPNG_PACK_FN uint32_t pack_place_one(uint64_t strides_before, uint64_t png_size, uint32_t status_in, uint32_t lead, uint64_t arena_cap, uint64_t *offset)
{
    const uint64_t off = strides_before + lead;
    const bool fits = !status_in && off + pack_extent(png_size) <= arena_cap;
    *offset = fits ? off : 0u;
    return status_in ? status_in : (fits ? 0u : kStatusArenaFull);
}

// 0 = the default of 16; a power of two in [16, 65536], else 0 (invalid)
FPNG_PACK_FN uint32_t pack_align_of(uint32_t align)
{
    if (!align) return kPackMinAlign;
    return (align >= kPackMinAlign && align <= kPackMaxAlign && !(align & (align - 1u))) ? align : 0u;
}
FPNG_PACK_FN bool pack_lead_ok(uint32_t lead) { return !(lead & 15u) && lead <= kPackMaxLead; }

} // namespace fpng_amd
