// rt_view_samples.hip — the three kernels of a sampled view (include/rt_hip.h: rt_view_sample_rays_device,
// rt_scene_trace_view_samples_device): n rays per pixel - sub-pixel offsets, a thin lens - averaged on the GPU.  No trace kernel knows of
// it: per band and per sample the generator below writes a ray list, the rt_trace_rays launch traces it into a slab of the workspace,
// and the two small kernels below add the slabs up in binary64 and store the mean.
//   rt_view_sample_rays_kernel   rt_view_rays_kernel's shape: one ray per work-item, grid (ceil(w / 256), rows), the row is the
//                                workgroup's y - no division by w, no loop -, three 16-byte stores per lane, a wave fills 3072 contiguous
//                                bytes.  The sample and the lens come by value in the kernel arguments; the panorama's row entry is a
//                                scalar pair, its column entry one 16-byte vector load, both from the SAMPLE's tables.
//   rt_view_accumulate_kernel    acc[j] = acc[j] + rgb[j] over the 3 * pixels doubles of a band: one 16-byte pair per lane, flat grid, no
//                                loop; 3 * pixels is odd for an odd band, so the lane behind the last pair takes the single double.
//   rt_view_resolve_kernel       one pixel per lane: mean = (acc + last) / n - one correctly rounded division -, stored as rgb and / or
//                                through to_byte as rgba.  The last sample's accumulation is this kernel's addition.
// The arithmetic of the generator is rt_view_samples.h's, the host probe's own source; the unit is built without FMA contraction.  The
// slabs are 8-byte aligned (a band of an odd number of pixels puts the second slab 8 bytes off a 16-byte boundary): the pair accesses
// are 16-byte accesses at 8-byte aligned addresses, which global memory allows.  Plain stores: every slab is read back at once by the
// next launch.  No LDS, no scratch (tests/test_view_samples_resources.py).  No test switches: one object for both libraries.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rt_view_samples.h"

namespace {
#define RT_STRICT 1
#define RT_INF __builtin_inf()
#include "rt_kernel_math.h"      // to_byte: the store rule of main.js:195-198, as the ray-list kernel and rt_nodes.hip's fold use it

typedef double d2 __attribute__((vector_size(16)));
typedef double d2u __attribute__((vector_size(16), aligned(8)));     // a 16-byte access at an 8-byte aligned address
}  // namespace

__global__ void __launch_bounds__(RT_VIEWS_WG) rt_view_sample_rays_kernel(const rt_view_params P, const rt_view_sample_params S, const uint32_t first_row,
                                                                          double *__restrict__ rays) {
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
  rt_view_sample_ray_of(P, S, x, y, sl, cl, sa, ca, r);
  d2 *q = (d2 *)(rays + 6u * ((size_t)row * P.w + x));
  const d2 a = {r[0], r[1]}, b = {r[2], r[3]}, c = {r[4], r[5]};
  q[0] = a; q[1] = b; q[2] = c;
}

// doubles = 3 * pixels of the band; lane i takes doubles 2 i and 2 i + 1, the lane behind the last pair the odd one out
__global__ void __launch_bounds__(RT_VIEWS_WG) rt_view_accumulate_kernel(double *__restrict__ acc, const double *__restrict__ rgb, const uint64_t doubles) {
  const uint64_t i = (uint64_t)blockIdx.x * RT_VIEWS_WG + threadIdx.x, pairs = doubles >> 1;
  if (i < pairs) {
    d2u *a = (d2u *)acc + i;
    const d2u s = *a, t = ((const d2u *)rgb)[i];
    const d2u sum = {s[0] + t[0], s[1] + t[1]};
    *a = sum;
  } else if (i == pairs && (doubles & 1u)) {
    acc[doubles - 1u] = acc[doubles - 1u] + rgb[doubles - 1u];
  }
}

// last == NULL: n == 1, the accumulator holds the only sample
__global__ void __launch_bounds__(RT_VIEWS_WG) rt_view_resolve_kernel(const double *__restrict__ acc, const double *__restrict__ last, const double n,
                                                                      const uint32_t pixels, double *__restrict__ out_rgb, uint32_t *__restrict__ out_rgba) {
  const uint32_t i = blockIdx.x * RT_VIEWS_WG + threadIdx.x;
  if (i >= pixels) return;
  const double *a = acc + 3u * (size_t)i;
  double m[3] = {a[0], a[1], a[2]};
  if (last) { const double *l = last + 3u * (size_t)i; m[0] = m[0] + l[0]; m[1] = m[1] + l[1]; m[2] = m[2] + l[2]; }
  m[0] = m[0] / n; m[1] = m[1] / n; m[2] = m[2] / n;
  if (out_rgb) { double *o = out_rgb + 3u * (size_t)i; o[0] = m[0]; o[1] = m[1]; o[2] = m[2]; }
  if (out_rgba) out_rgba[i] = to_byte(m[0]) | (to_byte(m[1]) << 8) | (to_byte(m[2]) << 16) | 0xff000000u;
}

extern "C" int rt_launch_view_sample_rays(const rt_view_params *P, const rt_view_sample_params *S, uint32_t first_row, uint32_t rows, double *d_rays,
                                          void *hip_stream) {
  const uint32_t wgs_x = (P->w + RT_VIEWS_WG - 1u) / RT_VIEWS_WG;
  for (uint32_t done = 0; done < rows; done += RT_VIEWS_MAX_ROWS) {
    const uint32_t m = rows - done < RT_VIEWS_MAX_ROWS ? rows - done : RT_VIEWS_MAX_ROWS;
    hipLaunchKernelGGL(rt_view_sample_rays_kernel, dim3(wgs_x, m), dim3(RT_VIEWS_WG), 0, (hipStream_t)hip_stream, *P, *S, first_row + done,
                       d_rays + 6u * ((size_t)done * P->w));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return (int)hipSuccess;
}

extern "C" void rt_view_sample_rays_host(const rt_view_params *P, const rt_view_sample_params *S, uint32_t first_row, uint32_t rows, double *out) {
  for (uint32_t row = 0; row < rows; row++)
    for (uint32_t x = 0; x < P->w; x++) rt_view_sample_ray(*P, *S, x, first_row + row, out + 6u * ((size_t)row * P->w + x));
}

extern "C" int rt_launch_view_accumulate(double *d_acc, const double *d_rgb, uint32_t pixels, void *hip_stream) {
  const uint64_t doubles = 3u * (uint64_t)pixels, lanes = (doubles >> 1) + (doubles & 1u);            // (pixels < 2^31: fewer than 2^24 workgroups)
  hipLaunchKernelGGL(rt_view_accumulate_kernel, dim3((uint32_t)((lanes + RT_VIEWS_WG - 1u) / RT_VIEWS_WG)), dim3(RT_VIEWS_WG), 0, (hipStream_t)hip_stream,
                     d_acc, d_rgb, doubles);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_view_resolve(const double *d_acc, const double *d_last, uint32_t n, uint32_t pixels, double *d_rgb, uint8_t *d_rgba,
                                      void *hip_stream) {
  hipLaunchKernelGGL(rt_view_resolve_kernel, dim3((pixels + RT_VIEWS_WG - 1u) / RT_VIEWS_WG), dim3(RT_VIEWS_WG), 0, (hipStream_t)hip_stream, d_acc, d_last,
                     (double)n, pixels, d_rgb, (uint32_t *)d_rgba);
  return (int)hipGetLastError();
}
