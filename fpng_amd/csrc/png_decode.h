// png_decode.h -- the general decode tier between its host side (png_decode_api.cpp) and its kernels (png_inflate.hip)
#pragma once
#include "png_inflate_core.h"

#include <hip/hip_runtime_api.h>

namespace fpng_amd {

// files, states: device arrays of n records.  png_inflate_kernel fills states[i] (status, PLTE / tRNS places) and files[i].scan;
// png_unfilter_kernel, behind it on the stream, writes files[i].out for the files whose status is still 0 and sets the status of
// those whose scanlines are at fault.  n < 2^31 (one workgroup per file).  ev (or NULL): three events, recorded in front of, between
// and behind the two launches.
void launch_png_decode(hipStream_t s, const pngi::File *files, pngi::State *states, uint32_t n, hipEvent_t *ev = nullptr);

// The views call's two launches (png_views_api.cpp), between which the host reads the states: png_inflate_kernel alone, then
// png_unfilter_box_kernel, which stores box i of file i -- inside the image, files[i].scan holding rows 0 .. y + h - 1 -- as planes
// for the files whose status is 0 and sets the status of those whose visited scanlines are at fault.  boxes: a device array of n
// records; those of files whose status is not 0 are not read.
void launch_png_inflate(hipStream_t s, const pngi::File *files, pngi::State *states, uint32_t n);
void launch_png_unfilter_box(hipStream_t s, const pngi::File *files, pngi::State *states, const pngi::Box *boxes, uint32_t n);

} // namespace fpng_amd
