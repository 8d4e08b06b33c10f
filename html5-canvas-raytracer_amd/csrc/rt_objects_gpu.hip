// rt_objects_gpu.hip — the sphere tables of a resident scene rebuilt ON THE GPU after rt_scene_set_objects and rt_scene_set_lights
// (rt_scene.hip): the copy of the host-written part of an object move, the bounce table, the shadow grids' masks and the
// light-anchored records of a light move.  rt_tables.cpp builds the same tables on
// the host (rt_scene_upload, and the tests' oracle); both use the per-element arithmetic of rt_objects.h.  Compiled without FMA
// contraction, like rt_tables.cpp: both builds state the same words.
//
//   rt_objects_copy   the staged part of a move (pinned host memory) into the scene's arena, one 16-byte piece per work-item;
//   rt_bounce_build   one work-item per (sphere i, cell c, 64-bit word w): the bits of the 64 loop spheres of word w that a ray
//                     leaving i in the directions of cell c can meet.  The workgroup's first wave states the 64 (i, j) pairs in LDS
//                     first (rt_bounce_pair_of); the cell cones come from the arena (host-computed at upload: no transcendental here).
//                     Every word is written - zero in the rows of spheres that neither reflect nor refract - with no atomics, and
//                     the stores of a wave are coalesced along c;
//   rt_sgrid_build    one work-item per (listed light k, cell c, word w), the same shape: the first wave states its 64 spheres' cell
//                     spans in light k's frame (the header, written by the host: its centroid is a sequential sum), then every
//                     work-item ORs the spheres whose span covers its cell.  The lights come by value in the kernarg segment
//                     (rt_light_list): all of them after an object move, the moved ones after a light move;
//   rt_light_anchor   a light move: one work-item per (ordering, listed light, sphere) writes the sphere's record anchored at the
//                     light's new position (rt_objects.h: rt_anchored, what fill_object_block states on the host) from the block's own
//                     sphere records; the work-items behind them copy the moved lights' grid headers (host-computed, pinned memory),
//                     one double each.  Plain stores, one per output record or word.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_objects.h"
#include "rt_objects_gpu.h"

namespace {

constexpr uint32_t WG = 128;

__global__ void __launch_bounds__(256) rt_objects_copy(uint4 *dst, const uint4 *src, uint32_t n16) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n16) dst[i] = src[i];
}

// grid (ceil(RT_BCELLS / WG), words, n_objects)
__global__ void __launch_bounds__(WG) rt_bounce_build(const rt_sphere *objs, uint32_t n_loop, const double *cones, uint64_t *tab) {
  __shared__ rt_bounce_pair pairs[64];
  const uint32_t i = blockIdx.z, w = blockIdx.y, words = gridDim.y, t = threadIdx.x;
  const uint32_t c = blockIdx.x * WG + t;
  const rt_sphere &oi = objs[i];
  const bool used = rt_bounce_row_used(oi);          // (uniform)
  const uint32_t j0 = w * 64u, nj = n_loop - j0 < 64u ? n_loop - j0 : 64u;
  if (used) {
    if (t < nj) pairs[t] = rt_bounce_pair_of(oi, sqrt(oi.r2), objs[j0 + t]);
    __syncthreads();
  }
  if (c >= RT_BCELLS) return;
  uint64_t bits = 0;
  if (used)
    for (uint32_t k = 0; k < nj; k++)
      if (rt_bounce_cell_hit(pairs[k], cones, c)) bits |= 1ull << k;
  tab[((size_t)i * RT_BCELLS + c) * words + w] = bits;
}

// grid (ceil(cells / WG), words, L.n); `grid` = the shadow-grid buffer of n_lights lights (rt_tables.cpp: build_shadow_grid's layout),
// headers written
__global__ void __launch_bounds__(WG) rt_sgrid_build(const rt_sphere *objs, uint32_t n_loop, uint32_t n_lights, const rt_light_list L, uint64_t *grid) {
  __shared__ uint32_t span[64];
  __shared__ uint32_t in_front[2];
  const uint32_t k = L.k[blockIdx.z], w = blockIdx.y, words = gridDim.y, t = threadIdx.x;
  const double Lp[3] = {L.xyz[blockIdx.z][0], L.xyz[blockIdx.z][1], L.xyz[blockIdx.z][2]};
  constexpr uint32_t G = RT_SGRID, cells = RT_SGRID * RT_SGRID + 1u;
  const uint32_t c = blockIdx.x * WG + t;
  const double *hk = (const double *)grid + 16u * k;
  const uint32_t j0 = w * 64u, nj = n_loop - j0 < 64u ? n_loop - j0 : 64u;
  if (t < 64u) {
    bool front = false;
    if (t < nj) {
      rt_geom q;
      front = !rt_shadow_rect(hk, Lp, objs[j0 + t].origin, objs[j0 + t].r2, &q);
      span[t] = front ? rt_sgrid_span(q, hk) : 0u;
    }
    const uint64_t m = __ballot(front);
    if (t == 0) { in_front[0] = (uint32_t)m; in_front[1] = (uint32_t)(m >> 32); }
  }
  __syncthreads();
  if (c >= cells) return;
  const uint64_t front = (uint64_t)in_front[0] | (uint64_t)in_front[1] << 32;
  uint64_t bits;
  if (c == G * G) {
    bits = nj == 64u ? ~0ull : (1ull << nj) - 1ull;                          // the "every sphere" cell
  } else {
    bits = 0;
    const uint32_t ix = c % G, iy = c / G;
    for (uint32_t j = 0; j < nj; j++)
      if (((front >> j) & 1ull) && rt_sgrid_in_span(span[j], ix, iy)) bits |= 1ull << j;
  }
  uint64_t *masks = grid + (size_t)n_lights * 16u;
  masks[((size_t)k * cells + c) * words + w] = bits;
}

// grid (ceil((n_ord * L.n * n_objects + 16 * L.n) / 256)); objs_b, grid: NULL without ordering B / shadow grids
__global__ void __launch_bounds__(256) rt_light_anchor(const rt_sphere *objs_a, const rt_sphere *objs_b, uint32_t n_ord, uint32_t n_objects, uint32_t n_lights,
                                                       const rt_light_list L, rt_geom *geom, double *grid, const double *headers) {
  const uint32_t id = blockIdx.x * 256u + threadIdx.x;
  const uint32_t n_rec = n_ord * L.n * n_objects;
  if (id < n_rec) {
    const uint32_t i = id % n_objects, j = (id / n_objects) % L.n, ord = id / (n_objects * L.n);
    const rt_sphere &o = (ord ? objs_b : objs_a)[i];
    const double a[3] = {L.xyz[j][0], L.xyz[j][1], L.xyz[j][2]};
    geom[((size_t)ord * (1u + n_lights) + 1u + L.k[j]) * n_objects + i] = rt_anchored(o.origin, o.r2, a);
  } else if (grid && id - n_rec < 16u * L.n) {
    const uint32_t h = id - n_rec;
    grid[16u * L.k[h / 16u] + h % 16u] = headers[h];
  }
}

}  // namespace

extern "C" int rt_launch_objects_copy(void *dst, const void *pinned_src, size_t bytes, hipStream_t stream) {
  const uint32_t n16 = (uint32_t)((bytes + 15u) / 16u);
  if (n16) hipLaunchKernelGGL(rt_objects_copy, dim3((n16 + 255u) / 256u), dim3(256), 0, stream, (uint4 *)dst, (const uint4 *)pinned_src, n16);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_bounce_build(const rt_sphere *loop_objs, uint32_t n_objects, uint32_t n_loop, const double *cones, uint64_t *table, hipStream_t stream) {
  const uint32_t words = (n_loop + 63u) / 64u;
  hipLaunchKernelGGL(rt_bounce_build, dim3((RT_BCELLS + WG - 1u) / WG, words, n_objects), dim3(WG), 0, stream, loop_objs, n_loop, cones, table);
  return (int)hipGetLastError();
}

// (a list whose indices do not lie in [0, n_lights) would store outside the block: refused, hipErrorInvalidValue)
static bool light_list_ok(const rt_light_list *L, uint32_t n_lights) {
  if (!L || L->n > RT_MAX_LIGHTS || n_lights > RT_MAX_LIGHTS) return false;
  for (uint32_t j = 0; j < L->n; j++) if (L->k[j] >= n_lights) return false;
  return true;
}

extern "C" int rt_launch_sgrid_build(const rt_sphere *loop_objs, uint32_t n_loop, uint32_t n_lights, const rt_light_list *lights, uint64_t *grid, hipStream_t stream) {
  if (!light_list_ok(lights, n_lights)) return (int)hipErrorInvalidValue;
  const uint32_t words = (n_loop + 63u) / 64u, cells = RT_SGRID * RT_SGRID + 1u;
  if (lights->n) hipLaunchKernelGGL(rt_sgrid_build, dim3((cells + WG - 1u) / WG, words, lights->n), dim3(WG), 0, stream, loop_objs, n_loop, n_lights, *lights, grid);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_light_anchor(const rt_sphere *objs_a, const rt_sphere *objs_b, uint32_t n_ord, uint32_t n_objects, uint32_t n_lights, const rt_light_list *lights,
                                      rt_geom *geom, double *grid, const double *pinned_headers, hipStream_t stream) {
  if (!light_list_ok(lights, n_lights) || n_ord < 1u || n_ord > 2u || (n_ord == 2u && !objs_b)) return (int)hipErrorInvalidValue;
  const uint32_t n = n_ord * lights->n * n_objects + (grid ? 16u * lights->n : 0u);
  if (n) hipLaunchKernelGGL(rt_light_anchor, dim3((n + 255u) / 256u), dim3(256), 0, stream, objs_a, objs_b, n_ord, n_objects, n_lights, *lights, geom, grid, pinned_headers);
  return (int)hipGetLastError();
}
