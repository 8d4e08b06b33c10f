// rt_adaptive.hip — adaptive supersampling (include/rt_hip.h: rt_render_adaptive_device): the two launches that follow the ordinary
// colour launch of a supersample-1 frame on the caller's stream.
//   rt_adaptive_mark    the criterion (rt_adaptive.h: rt_adaptive_refines) on the finished frame B: the pixels that differ from a
//                       4-neighbour by the threshold or more go onto a list in the caller's workspace, and into the mask if one is asked for
//   rt_adaptive_refine  the listed pixels again, as the pixels of the k-supersampled strict frame: k x k samples of the k w x k h sample
//                       grid, each with the reference's own operation sequence, box-filtered, stored over B's
// The kernel boundary between the two separates the criterion, which reads B alone, from the stores that replace pixels of B.
// This unit includes rt_kernel.hip's four fragments with RT_STRICT 1 and is compiled without FMA contraction (csrc/Makefile), so a
// sample here is rt_retrace's sample: trace_pixel in ITEM mode - every sphere in the scene's own order, materials read from HBM, no
// wave-wide step inside the trace - on a launch record bound as rt_retrace's, whose frame size is the SAMPLE grid's: the stars
// sampler's pix is sy * (k w) + sx, the supersampled frame's.  The bytes are those of rt_render_tiles_device(..., RT_FLAG_STRICT_FP) on
// the same scene with header supersample k.
//
// MI355X mapping.  Mark: one work-item per pixel; a wave covers 64 consecutive pixels of one row and loads its row and the rows above
// and below as dwords (whole 256-byte pieces), the left and right neighbours come from the adjacent lanes (the wave's two end lanes
// load theirs); one ballot and at most one vector atomic add per wave on the counter word reserve the wave's places in the list.  The
// order of the list is whatever the atomics made it: no output depends on it (every entry is a different pixel).
// Refine: the count is only known on the device, so the grid is fixed and walks the list with a grid-stride loop; workgroups with
// nothing to do leave at once.  The k x k samples of one listed pixel sit in ADJACENT lanes - the same primary hit, nearly the same ray
// tree: they share control flow - 16 pixels per wave for k = 2, 4 for k = 4, 7 for k = 3 (lane 63 idle).  The sample bytes are summed
// across those lanes (k = 2, 4: xor shuffles inside the aligned group; k = 3: the group's first lane reads its eight neighbours), with the
// wave converged; the group's first lane stores the pixel.  No global atomics, no LDS allocation.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rt_device.h"
#include "rt_block.h"
#include "rt_adaptive.h"

#define RT_STRICT 1
#define RT_INF __builtin_inf()

namespace {

#include "rt_kernel_math.h"      // v3, unit, to_byte, the stars hash
#include "rt_kernel_entry.h"     // rt_cold_args (the launch record is every tracing kernel's FIRST argument)
#include "rt_kernel_tables.h"    // rt_load_*, rt_mtl_*, frame
#include "rt_kernel_trace.h"     // trace_pixel

// ---------------------------------------------------------------------------------------------------------------- mark
// grid: x - pieces of 64 pixels across a row; y - groups of four rows (one per wave of the workgroup)
__global__ void __launch_bounds__(256) rt_adaptive_mark(const rt_adaptive_mark_launch M) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t x = blockIdx.x * 64u + lane, y = blockIdx.y * 4u + (threadIdx.x >> 6);
  if (y >= M.h) return;                                              // wave-uniform
  const bool in = x < M.w;
  const uint32_t *__restrict__ row = M.frame + (size_t)y * M.w;
  const uint32_t c = in ? row[x] : 0u;
  // a neighbour outside the frame: the pixel itself (rt_adaptive.h)
  const uint32_t up = (in && y > 0u) ? (row - M.w)[x] : c;
  const uint32_t down = (in && y + 1u < M.h) ? (row + M.w)[x] : c;
  uint32_t left = __shfl_up(c, 1), right = __shfl_down(c, 1);
  if (lane == 0u) left = (in && x > 0u) ? row[x - 1u] : c;
  if (!in || x + 1u >= M.w) right = c;
  else if (lane == 63u) right = row[x + 1u];
  const bool refine = in && rt_adaptive_refines(c, left, right, up, down, M.threshold);
  if (M.mask != nullptr && in) M.mask[(size_t)y * M.w + x] = refine ? 1u : 0u;
  const unsigned long long votes = __ballot(refine);
  if (votes == 0ull) return;                                         // wave-uniform
  uint32_t base = 0u;
  if (lane == 0u) base = atomicAdd(M.work, (uint32_t)__popcll(votes));
  base = __shfl(base, 0);
  if (refine) M.work[RT_ADAPTIVE_HEADER_BYTES / 4u + base + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull))] = x | (y << 16);
}

// ---------------------------------------------------------------------------------------------------------------- refine
template <bool REFRACT, uint32_t K>
__global__ void __launch_bounds__(RT_WG_THREADS) rt_adaptive_refine(const rt_launch L, const rt_adaptive_refine_launch A) {
  constexpr uint32_t KK = K * K, PPW = 64u / KK;                     // samples per pixel; pixels per wave: 16, 7, 4
  const uint32_t count = A.work[0];
  const uint32_t n_waves = gridDim.x * (RT_WG_THREADS / 64u), wave = blockIdx.x * (RT_WG_THREADS / 64u) + (threadIdx.x >> 6);
  if ((uint64_t)blockIdx.x * (RT_WG_THREADS / 64u) * PPW >= count) return;     // workgroup-uniform: nothing to do
  const uint32_t lane = threadIdx.x & 63u, slot = lane / KK, sub = lane - slot * KK;
  const uint32_t *__restrict__ list = A.work + RT_ADAPTIVE_HEADER_BYTES / 4u;
  const rt_mtl *mtl = (const rt_mtl *)L.lds_image;                   // (HBM: nothing is staged here)
  const rt_texture_desc *tex = (const rt_texture_desc *)((const char *)L.lds_image + (size_t)L.n_objects * sizeof(rt_mtl));
  // (64-bit: wave x PPW stays below 2^32, a stride added to an index near a count of 2^30 need not)
  for (uint64_t first = (uint64_t)wave * PPW; first < count; first += (uint64_t)n_waves * PPW) {     // wave-uniform
    const uint64_t i = first + slot;
    const bool active = slot < PPW && i < count;
    uint32_t px = 0u, py = 0u, rg = 0u, b = 0u;                      // the sample's bytes: R | G << 16, B (a sum of 16 is below 2^12)
    if (active) {
      const uint32_t e = list[i];
      px = e & 0xffffu; py = e >> 16;
      const uint32_t sx = K * px + sub % K, sy = K * py + sub / K;
      // A1 primary ray (main.js:186-193), literally
      const double d0 = ((double)sx - L.proj_w) + 0.5, d1 = (L.proj_h - (double)sy) - 0.5, d2 = L.proj_d;
      const v3 o = mk(L.cam_origin[0], L.cam_origin[1], L.cam_origin[2]);
      const v3 target = mk(o.x + L.cam_axis_x[0] * d0 + L.cam_axis_y[0] * d0 + L.cam_axis_z[0] * d0,
                           o.y + L.cam_axis_x[1] * d1 + L.cam_axis_y[1] * d1 + L.cam_axis_z[1] * d1,
                           o.z + L.cam_axis_x[2] * d2 + L.cam_axis_y[2] * d2 + L.cam_axis_z[2] * d2);
      double rl;
      const v3 ray = unit(mk(target.x - o.x, target.y - o.y, target.z - o.z), &rl);
      double rgb[3];
      uint32_t cnt[3] = {0u, 0u, 0u};
      trace_pixel<REFRACT, false, false, false, true>(L, mtl, tex, nullptr, nullptr, rt_geom{0.0, 0.0, 0.0, 0.0}, 0u, 0.0, 0.0, 0.0, 0.0, o, ray, rgb, cnt, false, 0u, sx, sy, 0u);
      rg = to_byte(rgb[0]) | (to_byte(rgb[1]) << 16); b = to_byte(rgb[2]);
    }
    // the wave is converged here: every lane takes part in the cross-lane steps, an idle one with zeros
    if constexpr (K == 3u) {
      uint32_t srg = rg, sb = b;
#pragma unroll
      for (uint32_t j = 1u; j < KK; j++) { srg += __shfl(rg, (int)((lane + j) & 63u)); sb += __shfl(b, (int)((lane + j) & 63u)); }     // (right for sub == 0, the lane that stores)
      rg = srg; b = sb;
    } else {
#pragma unroll
      for (uint32_t m = 1u; m < KK; m <<= 1) { rg += __shfl_xor(rg, (int)m); b += __shfl_xor(b, (int)m); }
    }
    if (active && sub == 0u)
      A.out[(size_t)py * A.w + px] = rt_adaptive_box(rg & 0xffffu, K) | (rt_adaptive_box(rg >> 16, K) << 8) | (rt_adaptive_box(b, K) << 16) | 0xff000000u;
  }
}

const void *refine_kernel(int refract, uint32_t k) {
  switch ((refract ? 8u : 0u) | k) {
    case 2u: return (const void *)&rt_adaptive_refine<false, 2u>;
    case 3u: return (const void *)&rt_adaptive_refine<false, 3u>;
    case 4u: return (const void *)&rt_adaptive_refine<false, 4u>;
    case 10u: return (const void *)&rt_adaptive_refine<true, 2u>;
    case 11u: return (const void *)&rt_adaptive_refine<true, 3u>;
    case 12u: return (const void *)&rt_adaptive_refine<true, 4u>;
  }
  return nullptr;
}

}  // namespace

extern "C" int rt_launch_adaptive_mark(const rt_adaptive_mark_launch *M, hipStream_t stream) {
  hipLaunchKernelGGL(rt_adaptive_mark, dim3((M->w + 63u) / 64u, (M->h + 3u) / 4u), dim3(256), 0, stream, *M);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_adaptive_refine(const rt_launch *L, const rt_adaptive_refine_launch *A, int refract, uint32_t k, unsigned n_wg, hipStream_t stream) {
  const void *f = refine_kernel(refract, k);
  if (!f) return (int)hipErrorInvalidDeviceFunction;
  void *args[] = {(void *)L, (void *)A};
  (void)hipLaunchKernel(f, dim3(n_wg ? n_wg : 1u), dim3(RT_WG_THREADS), args, 0, stream);
  return (int)hipGetLastError();
}

extern "C" int rt_scratch_adaptive_refine(int refract, uint32_t k, size_t *bytes_per_lane) {
  const void *f = refine_kernel(refract, k);
  if (!f) return (int)hipErrorInvalidDeviceFunction;
  hipFuncAttributes fa;
  const hipError_t e = hipFuncGetAttributes(&fa, f);
  if (e == hipSuccess) *bytes_per_lane = (size_t)fa.localSizeBytes;
  return (int)e;
}
