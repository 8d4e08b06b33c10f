// rt_soft.hip — the soft trace in one launch (include/rt_hip.h: rt_scene_trace_rays_soft_device): rt_trace_rays_soft's picture without
// its wavefront loop.  Ray i is intersectWorld(segs, objects, org, dir) (main.js:216-336) walked depth-first over an explicit per-lane
// stack, and every step carries the bits of a kernel the tree already has:
//   a node      rt_nodes.hip's shade kernel: the closest hit in blob order, the sampler, the material's weights, the two directions
//   its lights  at tree level lv < levels rt_relight.hip's sample loop (displaced lights, clamped and weighted per sample, the fold
//               acc = x_0; acc + x_s; acc / n); at lv >= levels the shade kernel's own single pass, no division
//   its colour  rt_nodes.hip's fold: rgb*diffuse + rgb*specular + re + rf, re and rf 0.0 where a child was not visited and added all
//               the same, then jsmax(rgb*a0, jsmin(1, .)); a miss returns its sample
// The node evaluation restates rt_nodes_shade and rt_relight_kernel (about 150 lines): a header shared with rt_nodes.hip would have to
// leave that unit's device code byte-identical, and the two light loops are one loop here.  The walk itself - everything between a
// ray and its colour - is rt_soft_walk.h's soft_walk, which rt_gather.hip calls per sample too; this unit loads the ray, names its
// table walk and stores the colour.  Built as rt_relight.hip is: without FMA contraction, with the strict side of rt_kernel_math.h;
// no test switches: one object for both libraries.  One kernel:
//   rt_soft_trace   one work-item per ray, 256 per workgroup, ceil(n / 256) workgroups (n < 2^31: no grid-stride turn).  The lanes of a
//                   wave sit at different positions of their trees; the outer loop runs while any lane has a node to evaluate.  Inside
//                   it the sphere, light and sample loops are wave-uniform with lanes masked, a sphere is scalar loads from the blob,
//                   a light scalar loads from the kernel arguments, and a ballot ends a shadow scan.  The sample loop's trip count is
//                   the wave's maximum: a lane whose node is not relit takes part in sample 0 only, with the lights where they stand.
//                   With stride == 0 a sample's table entry is three scalar loads.
// The stack.  A frame is pushed when a node has a child to visit and holds what the fold needs after the children return:
// shade[3] (the running sum), amb[3] = rgb*a0, a3, a4, the hit point and the refract direction - 14 doubles; at most segs - 1 <= 15
// frames are live.  The state of a frame is two bits kept in registers (one word per lane for each: "the refract child is still to
// come", "the reflect child is out"), not in the frame.  The array is indexed by the lane's level: it lives in scratch, 1 680 B per
// lane against the 3 472 B of rt_trace_rays<true> (tests/test_soft_resources.py); a frame is written once and read once or twice per
// inner node, against hundreds of operations per node evaluation.  LDS was not used: 1 680 B x 256 lanes is 420 KiB per workgroup.
// The stars sampler's path is 1 at the root, 2 path for the reflect child and 2 path + 1 for the refract child; pix is the ROOT ray's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rt_soft.h"

namespace {
#define RT_STRICT 1
#define RT_INF __builtin_inf()
#include "rt_kernel_math.h"      // v3, dot, unit, reflect, min1, rt_sqrt / rt_rcp / rt_pow, star_uniform, to_int32_bit0, to_byte: the strict side
#include "rt_soft_walk.h"        // soft_walk: the tree walk described above, shared with rt_gather.hip
}  // namespace

__global__ void __launch_bounds__(RT_SOFT_WG) rt_soft_trace(const rt_soft_launch L) {
  uint32_t i;
  if (!lit_ordered(L.order, blockIdx.x * RT_SOFT_WG + threadIdx.x, L.n, &i)) return;   // (past the list, or an order's entry that names no ray)
  const lit_ray R = lit_load_ray(L.rays, i);
  const uint32_t pix = L.pix_base + i;                                   // the ROOT ray's index in the caller's list, at every level
  const amb_walk W = amb_walk_of(L.base, pix, L.stride, L.n_offs);       // (one 64-bit reduction per ray, none per node or sample)
  double val[3];
  soft_walk<true>(L, R, pix, W, val);
  if (L.rgb) { double *o = L.rgb + 3u * (size_t)i; o[0] = val[0]; o[1] = val[1]; o[2] = val[2]; }
  if (L.rgba) L.rgba[i] = to_byte(val[0]) | (to_byte(val[1]) << 8) | (to_byte(val[2]) << 16) | 0xff000000u;
}

extern "C" int rt_launch_soft(const rt_soft_launch *L, void *hip_stream) {
  hipLaunchKernelGGL(rt_soft_trace, dim3((L->n + RT_SOFT_WG - 1u) / RT_SOFT_WG), dim3(RT_SOFT_WG), 0, (hipStream_t)hip_stream, *L);   // (n < 2^31)
  return (int)hipGetLastError();
}

extern "C" int rt_soft_scratch(size_t *bytes_per_lane) {
  hipFuncAttributes fa;
  const hipError_t e = hipFuncGetAttributes(&fa, (const void *)rt_soft_trace);
  if (e == hipSuccess) *bytes_per_lane = (size_t)fa.localSizeBytes;
  return (int)e;
}
