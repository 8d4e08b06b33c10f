// rt_gather.hip — gathered light (include/rt_hip.h: rt_gather, rt_scene_gather_device): the colour that arrives at a receiver from the
// rest of the scene, n_samples rays over the hemisphere of its facing normal, each traced as intersectWorld traces any ray, averaged on
// the GPU.  Nothing here is new arithmetic: the receiver, its frame, the table walk and the segment are rt_ambient.h's (the host probe's
// own source), the trace of a segment is rt_soft_walk.h's tree walk with the lights where they stand (rt_soft_trace at levels 0, bit for
// bit), and the fold is the sampled view's (acc = c_0; acc + c_s; acc / n).  Built as rt_soft.hip is: without FMA contraction, with the
// strict side of rt_kernel_math.h; no test switches: one object for both libraries.  One kernel:
//   rt_gather_kernel   rt_ambient_kernel's mapping: one work-item per receiver, 256 per workgroup, ceil(n / 256) workgroups (n < 2^31).
//                      The sample loop is wave-uniform, and inside it the walk's node loop runs while any lane of the wave has a node
//                      of THIS sample's tree to evaluate.  With stride == 0 sample s of neighbouring receivers is the same local
//                      direction from nearly the same place - the coherent axis, and the reason samples are not mapped to lanes; its
//                      table entry is three scalar loads.  No segment and no per-sample colour exists in memory: three doubles of
//                      accumulator per lane, 8 to 28 bytes stored per receiver.
// Registers.  Across the walk a lane keeps its index, the accumulator (three doubles) and the table walk, and nothing of the receiver:
// the record (80 bytes, the lane's own, in cache after the first sample) is read again and the frame rebuilt for every sample - ten
// loads, one division and a dozen multiplications against a tree walk.  That is what keeps the kernel at 128 VGPRs, four waves per
// SIMD as rt_soft_trace has them: with the record read once and the receiver kept across the walk it needs 140 and runs three, and
// was measured 4 to 12 % slower where the gathered rays diverge or go deep and 4 to 11 % faster only where they are cheapest (stride 0,
// depth 1): docs/EVIDENCE.md, "Gathered light".  The reads go through a volatile pointer: the record does not change, but without it
// the compiler hoists the loads out of the loop and the receiver is back in registers.  The stack is the walk's: the same bytes of
// scratch per lane as rt_soft_trace (tests/test_gather_resources.py reads both).
// One lane per receiver under-fills the GPU below a few thousand receivers (256 CUs x 4 SIMDs x 64 lanes = 65 536 lanes make ONE wave
// per SIMD): a short probe list is latency-bound here; the lanes-per-sample mapping for such lists is rt_probe_kernel (rt_probe.hip).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rt_gather.h"

namespace {
#define RT_STRICT 1
#define RT_INF __builtin_inf()
#include "rt_kernel_math.h"      // the strict side: what rt_soft_walk.h needs, and to_byte (the store rule of main.js:195-198)
#include "rt_soft_walk.h"        // soft_walk
}  // namespace

__global__ void __launch_bounds__(RT_GATHER_WG) rt_gather_kernel(const rt_gather_launch L) {
  uint32_t i;
  if (!lit_ordered(L.S.order, blockIdx.x * RT_GATHER_WG + threadIdx.x, L.S.n, &i)) return;   // (past the list, or an order's entry that names no receiver)
  const volatile rt_hit *H = L.hits + i;                             // (read again per sample: see "Registers" above)
  const double __attribute__((address_space(4))) *sdirs = (const double __attribute__((address_space(4))) *)L.dirs;
  const amb_walk W = amb_walk_of(L.base, i, L.stride, L.n_dirs);     // (one 64-bit reduction per receiver, none per sample)
  const amb_walk none = {0u, 0u};                                    // (the walk's table: read by its relit branch only)
  uint32_t pix = L.pix_base + i;                                     // pix_base + s * pix_stride + i
  double acc[3] = {0.0, 0.0, 0.0};
  for (uint32_t s = 0; s < L.n_samples; s++) {
    double d0, d1, d2;
    if (L.stride == 0u) {                                            // one entry for the whole launch: scalar loads
      const double __attribute__((address_space(4))) *d = sdirs + 3u * (size_t)s;       // (e = s: s < n_samples <= n_dirs)
      d0 = d[0]; d1 = d[1]; d2 = d[2];
    } else {
      const double *d = L.dirs + 3u * (size_t)amb_walk_entry(W, s, L.n_dirs);
      d0 = d[0]; d1 = d[1]; d2 = d[2];
    }
    // the segment of (i, s): rt_ambient.h's, six NaNs for a receiver that is not scanned
    const amb_receiver R = amb_receiver_of(H->object, H->inside, H->point[0], H->point[1], H->point[2], H->normal[0], H->normal[1], H->normal[2]);
    double seg[6];
    amb_segment(R, d0, d1, d2, seg);
    lit_ray ray;
    ray.ox = seg[0]; ray.oy = seg[1]; ray.oz = seg[2]; ray.rx = seg[3]; ray.ry = seg[4]; ray.rz = seg[5];
    ray.finite = lit_finite6(seg[0], seg[1], seg[2], seg[3], seg[4], seg[5]);   // (rt_soft_trace's rule: a ray that is not finite gives NaN x 3)
    double c[3];
    soft_walk<false>(L.S, ray, pix, none, c);
#pragma unroll
    for (int k = 0; k < 3; k++) acc[k] = s == 0u ? c[k] : acc[k] + c[k];
    pix += L.pix_stride;
  }
  const double ns = (double)L.n_samples;
  const double r = acc[0] / ns, g = acc[1] / ns, b = acc[2] / ns;
  if (L.S.rgb) { double *o = L.S.rgb + 3u * (size_t)i; o[0] = r; o[1] = g; o[2] = b; }
  if (L.S.rgba) L.S.rgba[i] = to_byte(r) | (to_byte(g) << 8) | (to_byte(b) << 16) | 0xff000000u;
}

extern "C" int rt_launch_gather(const rt_gather_launch *L, void *hip_stream) {
  hipLaunchKernelGGL(rt_gather_kernel, dim3((L->S.n + RT_GATHER_WG - 1u) / RT_GATHER_WG), dim3(RT_GATHER_WG), 0, (hipStream_t)hip_stream, *L);   // (n < 2^31)
  return (int)hipGetLastError();
}

extern "C" int rt_gather_scratch(size_t *bytes_per_lane) {
  hipFuncAttributes fa;
  const hipError_t e = hipFuncGetAttributes(&fa, (const void *)rt_gather_kernel);
  if (e == hipSuccess) *bytes_per_lane = (size_t)fa.localSizeBytes;
  return (int)e;
}
