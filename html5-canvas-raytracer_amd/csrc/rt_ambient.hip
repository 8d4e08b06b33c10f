// rt_ambient.hip — ambient occlusion (include/rt_hip.h: rt_ambient, rt_scene_ambient_device): n_samples shadow scans per receiver over
// the hemisphere of its facing normal, counted and summed on the GPU.  The receivers are hit records (what a ray list's `hits` output
// holds); the arithmetic that turns a record and a table entry into a segment is rt_ambient.h's, the host probe's own source, and
// the scan is rt_occlusion.hip's (rt_literal.h: lit_scan_step).  The unit is built without FMA contraction.  Two kernels:
//   rt_ambient_segments_kernel   the segments of ONE sample as a ray list (three 16-byte stores per lane) and their skips: what a
//                                caller feeds rt_scene_occlusion_device, rt_scene_order_rays_device or rt_scene_trace_rays_device
//                                themselves, and what the tests hold the fused kernel to.
//   rt_ambient_kernel            the fused form.  rt_occlusion.hip's mapping: one work-item per receiver, 256 receivers per workgroup;
//                                the record is read once and the frame kept in registers; the sample loop and the sphere loop are
//                                both wave-uniform; each sphere is two scalar loads from the uploaded blob (origin + r2, and albedo[4]
//                                at byte 96); a lane whose scan has met its opaque sphere goes idle and the wave leaves the sphere loop
//                                on an empty ballot.  No segment exists in memory: 8 to 20 bytes are stored per receiver.  With
//                                stride == 0 every receiver reads the same table entry: three scalar loads instead of three vector loads
//                                (a wave-uniform branch on a kernel argument).
// No LDS, no scratch (tests/test_ambient_resources.py).  No test switches: one object for both libraries.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rt_ambient.h"
#include "rt_fdlibm.h"

namespace {
#define RT_STRICT 1
#define RT_INF __builtin_inf()
#include "rt_kernel_math.h"      // to_byte: the store rule of main.js:195-198, as rt_view_resolve_kernel uses it

typedef double d2 __attribute__((vector_size(16)));

// the receiver of a record in device memory: object and inside as one 8-byte load, point and normal as six
__device__ __forceinline__ amb_receiver load_receiver(const rt_hit *hits, uint32_t i) {
  const rt_hit *H = hits + i;
  return amb_receiver_of(H->object, H->inside, H->point[0], H->point[1], H->point[2], H->normal[0], H->normal[1], H->normal[2]);
}
}  // namespace

__global__ void __launch_bounds__(RT_AMBIENT_WG) rt_ambient_segments_kernel(const rt_ambient_launch L) {
  const uint32_t i = blockIdx.x * RT_AMBIENT_WG + threadIdx.x;
  if (i >= L.n) return;
  const amb_receiver R = load_receiver(L.hits, i);
  const double *d = L.dirs + 3u * (size_t)amb_entry(L.base, i, L.stride, L.sample, L.n_dirs);
  double r[6];
  amb_segment(R, d[0], d[1], d[2], r);
  d2 *q = (d2 *)(L.rays + 6u * (size_t)i);
  const d2 a = {r[0], r[1]}, b = {r[2], r[3]}, c = {r[4], r[5]};
  q[0] = a; q[1] = b; q[2] = c;
  if (L.skip) L.skip[i] = R.skip;
}

__global__ void __launch_bounds__(RT_AMBIENT_WG) rt_ambient_kernel(const rt_ambient_launch L) {
  uint32_t i;
  if (!lit_ordered(L.order, blockIdx.x * RT_AMBIENT_WG + threadIdx.x, L.n, &i)) return;   // (past the list, or an order's entry that names no receiver)
  const amb_receiver R = load_receiver(L.hits, i);
  const uint32_t skip = (uint32_t)R.skip;                            // (-1 matches no j)
  const double eps = L.epsilon, len = L.radius;
  const char __attribute__((address_space(4))) *tab = (const char __attribute__((address_space(4))) *)L.objects;
  const double __attribute__((address_space(4))) *sdirs = (const double __attribute__((address_space(4))) *)L.dirs;
  const amb_walk W = amb_walk_of(L.base, i, L.stride, L.n_dirs);     // (one 64-bit reduction per receiver, none per sample)
  uint32_t count = 0;
  double acc = 0.0;
  for (uint32_t s = 0; s < L.n_samples; s++) {
    double d0, d1, d2v;
    if (L.stride == 0u) {                                            // one entry for the whole launch: scalar loads
      const double __attribute__((address_space(4))) *d = sdirs + 3u * (size_t)s;       // (e = s: s < n_samples <= n_dirs)
      d0 = d[0]; d1 = d[1]; d2v = d[2];
    } else {
      const double *d = L.dirs + 3u * (size_t)amb_walk_entry(W, s, L.n_dirs);
      d0 = d[0]; d1 = d[1]; d2v = d[2];
    }
    double dir[3];
    amb_dir(R, d0, d1, d2v, dir);
    // (rt_scene_occlusion_device's rule: a segment with a non-finite word is not traced - intensity NaN, blocker -1)
    const bool traced = R.scanned && lit_finite6(dir[0], dir[1], dir[2], 0.0, 0.0, 0.0);
    double li = 1.0;
    int32_t blocker = -1;
    bool live = traced;
    for (uint32_t j = 0; j < L.n_objects; j++) {
      if (__builtin_amdgcn_ballot_w64(live) == 0) break;             // no lane of the wave has a sphere left to meet
      const double __attribute__((address_space(4))) *g = (const double __attribute__((address_space(4))) *)(tab + (size_t)j * sizeof(rt_sphere));
      const double gx = g[0], gy = g[1], gz = g[2], r2 = g[3];
      const double a4 = g[12];                                       // albedo[4]: byte 96 of the record
      if (!live || j == skip) continue;
      lit_scan_step((int32_t)j, gx, gy, gz, r2, a4, R.p[0], R.p[1], R.p[2], dir[0], dir[1], dir[2], eps, len, &li, &blocker, &live);
    }
    if (!traced) li = __builtin_nan("");
    count += blocker < 0 ? 1u : 0u;
    acc = s == 0u ? li : acc + li;
  }
  const double open = (double)count / (double)L.n_samples;
  if (L.open) L.open[i] = open;
  if (L.intensity) L.intensity[i] = R.scanned ? acc / (double)L.n_samples : __builtin_nan("");
  if (L.rgba) { const uint32_t b = to_byte(open); L.rgba[i] = b | (b << 8) | (b << 16) | 0xff000000u; }
}

extern "C" int rt_launch_ambient_segments(const rt_ambient_launch *L, void *hip_stream) {
  hipLaunchKernelGGL(rt_ambient_segments_kernel, dim3((L->n + RT_AMBIENT_WG - 1u) / RT_AMBIENT_WG), dim3(RT_AMBIENT_WG), 0, (hipStream_t)hip_stream, *L);   // (n < 2^31)
  return (int)hipGetLastError();
}

extern "C" int rt_launch_ambient(const rt_ambient_launch *L, void *hip_stream) {
  hipLaunchKernelGGL(rt_ambient_kernel, dim3((L->n + RT_AMBIENT_WG - 1u) / RT_AMBIENT_WG), dim3(RT_AMBIENT_WG), 0, (hipStream_t)hip_stream, *L);
  return (int)hipGetLastError();
}

extern "C" void rt_ambient_segments_host(const rt_ambient_launch *L) {
  for (uint32_t i = 0; i < L->n; i++) {
    const rt_hit &H = L->hits[i];
    const amb_receiver R = amb_receiver_of(H.object, H.inside, H.point[0], H.point[1], H.point[2], H.normal[0], H.normal[1], H.normal[2]);
    const double *d = L->dirs + 3u * (size_t)amb_entry(L->base, i, L->stride, L->sample, L->n_dirs);
    amb_segment(R, d[0], d[1], d[2], L->rays + 6u * (size_t)i);
    if (L->skip) L->skip[i] = R.skip;
  }
}

extern "C" void rt_ambient_cosine_dirs_host(uint32_t n, double *out) {
  const double golden = M_PI * (3.0 - sqrt(5.0));
  for (uint32_t k = 0; k < n; k++) {
    const double u = ((double)k + 0.5) / (double)n, phi = (double)k * golden, r = sqrt(u);
    out[3u * (size_t)k] = r * fd_cos(phi); out[3u * (size_t)k + 1u] = r * fd_sin(phi); out[3u * (size_t)k + 2u] = sqrt(1.0 - u);
  }
}
