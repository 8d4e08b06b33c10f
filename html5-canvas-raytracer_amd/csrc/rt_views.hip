// rt_views.hip — the generator of a view's primary rays (include/rt_hip.h: rt_view_rays_device, rt_scene_trace_view_device): rows
// [first_row, first_row + rows) of a w x h view as ray records {org[3], dir[3]} in row order, the list rt_trace_rays takes.  One ray per
// work-item, grid (ceil(w / 256), rows) like rt_texels_blit's: the row is the workgroup's y, the column its x * 256 + the lane - no
// division by w, no loop.  The arithmetic is rt_views.h's, the host probe's own source, and this unit is built without FMA contraction:
// + - * / and sqrt only, correctly rounded on both sides, so a record carries the host's bits.
// Memory: a lane stores its 48 bytes as three 16-byte stores, the way lit_load_ray reads them back, so a wave fills 3072 contiguous
// bytes - whole lines.  Plain stores: the band is read at once by the trace kernel and should still be in L2 or the Infinity Cache.
// The panorama's row entry {sin, cos of the latitude} is the same for the whole workgroup - a scalar load -, its column entry one
// 16-byte vector load per lane.  No LDS, no scratch (tests/test_views_resources.py).  No test switches: one object for both libraries.
#include <hip/hip_runtime.h>

#include "rt_views.h"

namespace {
typedef double d2 __attribute__((vector_size(16)));
}

__global__ void __launch_bounds__(RT_VIEWS_WG) rt_view_rays_kernel(const rt_view_params P, const uint32_t first_row, double *__restrict__ rays) {
  const uint32_t x = blockIdx.x * RT_VIEWS_WG + threadIdx.x;
  if (x >= P.w) return;
  const uint32_t row = blockIdx.y, y = first_row + row;                  // (wave-uniform)
  double sl = 0.0, cl = 0.0, sa = 0.0, ca = 0.0;
  if (P.model == RT_VIEWS_EQUIRECT) {
    const d2 lo = ((const d2 *)P.lon)[x];
    sl = lo[0]; cl = lo[1];
    sa = P.lat[2u * (size_t)y]; ca = P.lat[2u * (size_t)y + 1u];
  }
  double r[6];
  rt_view_ray_of(P, x, y, sl, cl, sa, ca, r);
  d2 *q = (d2 *)(rays + 6u * ((size_t)row * P.w + x));
  const d2 a = {r[0], r[1]}, b = {r[2], r[3]}, c = {r[4], r[5]};
  q[0] = a; q[1] = b; q[2] = c;
}

extern "C" int rt_launch_view_rays(const rt_view_params *P, uint32_t first_row, uint32_t rows, double *d_rays, void *hip_stream) {
  const uint32_t wgs_x = (P->w + RT_VIEWS_WG - 1u) / RT_VIEWS_WG;
  for (uint32_t done = 0; done < rows; done += RT_VIEWS_MAX_ROWS) {
    const uint32_t m = rows - done < RT_VIEWS_MAX_ROWS ? rows - done : RT_VIEWS_MAX_ROWS;
    hipLaunchKernelGGL(rt_view_rays_kernel, dim3(wgs_x, m), dim3(RT_VIEWS_WG), 0, (hipStream_t)hip_stream, *P, first_row + done,
                       d_rays + 6u * ((size_t)done * P->w));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return (int)hipSuccess;
}

extern "C" void rt_view_rays_host(const rt_view_params *P, uint32_t first_row, uint32_t rows, double *out) {
  for (uint32_t row = 0; row < rows; row++)
    for (uint32_t x = 0; x < P->w; x++) rt_view_ray(*P, x, first_row + row, out + 6u * ((size_t)row * P->w + x));
}
