// rt_occlusion.hip — how much of a light reaches a point: the reference's shadow scan (main.js:293-304) for a list of segments
// (include/rt_hip.h: rt_scene_occlusion_device).  Not a closest-hit query, so not rt_hits.hip's ray_hit: the scan stops at the
// first opaque sphere in BLOB order, leaves one sphere out (the receiver, j != hit_i), compares against the light's distance
// instead of infinity and divides the shared intensity by albedo[4] for every transparent sphere it crosses (quirk q2).
//
// Semantics, per ray i {org, dir} with length[i], intensity[i], skip[i]:
//   li = intensity[i]; blocker = -1
//   for j in blob order, j != skip[i]:
//     t = intersectSphere(obj j, org, dir, null)            main.js:420-439, the epsilon rule included
//     if t < length[i]:                                     (false for a NaN t or a NaN length)
//       if albedo[4] != 0: li = li / albedo[4]  else: li = 0; blocker = j; break
// This file is compiled WITHOUT FMA contraction (csrc/Makefile), sqrt and the division are correctly rounded: the intensity carries
// the bits of the C restatement (oracle/rt_oracle.c) - no tolerance.
//
// MI355X mapping: one work-item per ray, 256 rays per workgroup.  The loop counter is wave-uniform, so each sphere is two scalar
// loads from the uploaded blob (origin + r2: the first 32 bytes of the record, and albedo[4] at byte 96).  A lane that has met its
// opaque sphere goes idle - its part of the loop body is masked off - and the loop's branch is a ballot over the wave: as soon as
// no lane is live the wave leaves, which a closest-hit scan can never do.  Results are vector stores at the ray's own index; an
// output the caller did not ask for, and an input it did not give, is a kernarg NULL, i.e. a wave-uniform branch.  No LDS.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rt_occlusion.h"

namespace {

#include "rt_literal.h"       // the scan step, the ray record, the order indirection

#define RT_OCCLUSION_WG 256u

// With L.order (an order as rt_scene_trace_rays_ordered_device takes it) work-item `item` takes ray i = order[item] - every input of
// ray i in, its outputs at index i out - and skips an entry that names no ray.  A ray with a non-finite component is not traced.
__global__ void __launch_bounds__(RT_OCCLUSION_WG) rt_occlusion_kernel(const rt_occlusion_launch L) {
  uint32_t i;
  if (!lit_ordered(L.order, blockIdx.x * RT_OCCLUSION_WG + threadIdx.x, L.n_rays, &i)) return;   // (past the list, or an order's entry that names no ray)
  const lit_ray R = lit_load_ray(L.rays, i);
  const double len = L.length ? L.length[i] : __builtin_inf();
  const uint32_t skip = L.skip ? (uint32_t)L.skip[i] : ~0u;         // (a value outside [0, n_objects) matches no j)
  double li = L.intensity_in ? L.intensity_in[i] : L.light_intensity;
  int32_t blocker = -1;
  bool live = R.finite;
  const double eps = L.epsilon;
  const char __attribute__((address_space(4))) *tab = (const char __attribute__((address_space(4))) *)L.objects;
  for (uint32_t j = 0; j < L.n_objects; j++) {
    if (__builtin_amdgcn_ballot_w64(live) == 0) break;              // no lane of the wave has a sphere left to meet
    const double __attribute__((address_space(4))) *g = (const double __attribute__((address_space(4))) *)(tab + (size_t)j * sizeof(rt_sphere));
    const double gx = g[0], gy = g[1], gz = g[2], r2 = g[3];
    const double a4 = g[12];                                        // albedo[4]: byte 96 of the record
    if (!live || j == skip) continue;
    lit_scan_step((int32_t)j, gx, gy, gz, r2, a4, R.ox, R.oy, R.oz, R.rx, R.ry, R.rz, eps, len, &li, &blocker, &live);
  }
  if (!R.finite) li = __builtin_nan("");
  if (L.intensity) L.intensity[i] = li;
  if (L.blocker) L.blocker[i] = blocker;
}

}  // namespace

extern "C" int rt_launch_occlusion(const rt_occlusion_launch *L, hipStream_t stream) {
  hipLaunchKernelGGL(rt_occlusion_kernel, dim3((L->n_rays + RT_OCCLUSION_WG - 1) / RT_OCCLUSION_WG), dim3(RT_OCCLUSION_WG), 0, stream, *L);   // (n_rays < 2^31)
  return (int)hipGetLastError();
}
