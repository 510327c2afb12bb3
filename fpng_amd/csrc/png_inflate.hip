// png_inflate.hip -- the general decode tier's two kernels: ordinary PNG files, one 64-thread workgroup (one wavefront) per file.
// The per-wave logic is png_inflate_core.h (which the CPU tests run as it is); here are only the LDS, the records and the launches.
//   png_inflate_kernel   chunks -> zlib stream -> the file's filtered scanlines in the decode scratch, the last 32 KiB of output in
//                        an LDS ring that serves the matches' sources (no read-back of global memory the wave has just stored)
//   png_unfilter_kernel  filters 0-4 over skewed bands of 64 rows, grey / palette / tRNS expansion, the pixels
// No workgroup waits for another one in either kernel; the kernel boundary orders the scanlines between them.
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
    const uint32_t status = pngi_unfilter(sh, f, st);
    if (status && !threadIdx.x) states[blockIdx.x].status = status;
}

} // namespace

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
