// png_inflate.hip -- the general decode tier's kernels: ordinary PNG files, one 64-thread workgroup (one wavefront) per file.
// The per-wave logic is png_inflate_core.h (which the CPU tests run as it is); here are only the LDS, the records and the launches.
//   png_inflate_kernel   chunks -> zlib stream -> the file's filtered scanlines in the decode scratch, the last 32 KiB of output in
//                        an LDS ring that serves the matches' sources (no read-back of global memory the wave has just stored)
//   png_unfilter_kernel  filters 0-4 over skewed bands of 64 rows, grey / palette / tRNS expansion, the pixels
//   png_unfilter_box_kernel  the same walk over the rows and pixels that a box of the image needs; the box as tight uint8 planes in
//                        the scratch, where the views stage's resize kernels read them (png_views_api.cpp).  Each lane stores the
//                        pixel it has reconstructed, a byte per plane
// No workgroup waits for another one in any of them; the kernel boundary orders the scanlines between them.
#include "png_decode.h"

#include <hip/hip_runtime.h>

namespace fpng_amd {
namespace {

using namespace pngi;

__global__ __launch_bounds__(kWave) void png_inflate_kernel(const File *files, State *states)
{
    __shared__ InflateShared sh;
    const File f = files[blockIdx.x];
    State st;
    pngi_inflate(sh, f, st);
    if (!threadIdx.x) states[blockIdx.x] = st;
}

__global__ __launch_bounds__(kWave) void png_unfilter_kernel(const File *files, State *states)
{
    __shared__ UnfilterShared sh;
    const File f = files[blockIdx.x];
    const State st = states[blockIdx.x];
    if (st.status) return; // (the same answer in every lane)
    const Box none = {}; // (the walk itself, not pngi_unfilter: one more level of inlining costs this kernel a register)
    const uint32_t status = pngi_unfilter_walk<false>(sh, f, st, none);
    if (status && !threadIdx.x) states[blockIdx.x].status = status;
}

__global__ __launch_bounds__(kWave) void png_unfilter_box_kernel(const File *files, State *states, const Box *boxes)
{
    __shared__ UnfilterShared sh;
    const File f = files[blockIdx.x];
    const State st = states[blockIdx.x];
    if (st.status) return; // (the same answer in every lane)
    const uint32_t status = pngi_unfilter_walk<true>(sh, f, st, boxes[blockIdx.x]); // (the record where it lies: pngi_unfilter_walk)
    if (status && !threadIdx.x) states[blockIdx.x].status = status;
}

} // namespace

void launch_png_inflate(hipStream_t s, const pngi::File *files, pngi::State *states, uint32_t n)
{
    if (n) hipLaunchKernelGGL(png_inflate_kernel, dim3(n), dim3(pngi::kWave), 0, s, files, states);
}

void launch_png_unfilter_box(hipStream_t s, const pngi::File *files, pngi::State *states, const pngi::Box *boxes, uint32_t n)
{
    if (n) hipLaunchKernelGGL(png_unfilter_box_kernel, dim3(n), dim3(pngi::kWave), 0, s, files, states, boxes);
}

void launch_png_decode(hipStream_t s, const pngi::File *files, pngi::State *states, uint32_t n, hipEvent_t *ev)
{
    if (!n) return;
    if (ev) (void)hipEventRecord(ev[0], s);
    hipLaunchKernelGGL(png_inflate_kernel, dim3(n), dim3(pngi::kWave), 0, s, files, states);
    if (ev) (void)hipEventRecord(ev[1], s);
    hipLaunchKernelGGL(png_unfilter_kernel, dim3(n), dim3(pngi::kWave), 0, s, files, states);
    if (ev) (void)hipEventRecord(ev[2], s);
}

} // namespace fpng_amd
