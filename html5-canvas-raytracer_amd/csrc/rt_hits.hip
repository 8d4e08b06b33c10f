// rt_hits.hip — what is under a sample: the primary hit of every sample of a frame (object id, depth, normal), of single
// sample points (pick: the whole hit record) and of caller-supplied rays (rt_scene_trace_rays_device: the same record per ray).  The reference computes all of it per ray and throws it away after shading
// (main.js:216-231, :440-449: hit_i, hit.t, hit.p, hit.n, the inside flag behind hit.l, hit.u / hit.v).
//
// Semantics (include/rt_hip.h: rt_render_hits_device, rt_scene_pick), per sample of the k w x k h sample grid:
//   * the primary ray of main.js:184-193 with the reference's operation order, dist indexed by component (quirk q1);
//   * the closest hit over the spheres in BLOB order - the host's sorted `objects`, main.js:159-163 - with strict <, first wins
//     (main.js:223-231), each test the reference's own intersectSphere (main.js:420-451: the generic discriminant r2 - d2);
//   * hit.p = p + d t, hit.n = (hit.p - origin) * (1 / |hit.p - origin|) (quirk q7); u, v with two divisions each (q6) and
//     fdlibm's atan2 / asin (rt_fdlibm.h).
// This file is compiled WITHOUT FMA contraction (csrc/Makefile), so t, p and n carry the bits of the C restatement
// (oracle/rt_oracle.c) - no tolerance.  The sphere test, the closest-hit step and the hit record are rt_literal.h's, which the other list
// kernels share; with the colour kernels it shares fdlibm's functions and rt_trace_rays' list head, nothing else: no launch table, no cull,
// no camera-anchored tables (primary rays only; the loop is short and every sphere is a scalar load).
//
// MI355X mapping: one work-item per sample, 256 samples of one sample row per workgroup (grid y walks the rows of the band); the
// sphere table is read from the uploaded blob with scalar loads (s_load_dwordx8 per sphere: origin + r2, wave-uniform); the three
// outputs are stored as 256 consecutive int32 / double / 3 x float32 per workgroup; an output the caller did not ask for is a
// kernarg NULL, i.e. a wave-uniform branch.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rt_hits.h"

namespace {

#include "rt_literal.h"       // the sphere test, the closest-hit step, the hit record, the ray record; rt_fdlibm.h

#define RT_HITS_WG 256u

struct hit_core {
  int32_t id;                // sphere index (blob order) | inside << 16, or -1
  double t, p[3], n[3];
};

// the first hit of the ray (o, r), r as given: main.js:220-231, 420-451, 440-449 (rt_literal.h), every sphere a scalar load
__device__ __forceinline__ hit_core ray_hit(const rt_hits_launch &L, const double ox, const double oy, const double oz, const double rx, const double ry,
                                            const double rz) {
  const double eps = L.epsilon;
  double ht = __builtin_inf();
  int32_t hi = -1, hin = 0;
  const char __attribute__((address_space(4))) *tab = (const char __attribute__((address_space(4))) *)L.objects;
  for (uint32_t i = 0; i < L.n_objects; i++) {
    // origin[3], r2: the first 32 bytes of the 192-byte rt_sphere record, one scalar load
    const double __attribute__((address_space(4))) *g = (const double __attribute__((address_space(4))) *)(tab + (size_t)i * sizeof(rt_sphere));
    lit_closest_step((int32_t)i, g[0], g[1], g[2], g[3], ox, oy, oz, rx, ry, rz, eps, &ht, &hi, &hin);
  }
  hit_core H;
  H.t = ht;
  if (hi < 0) {
    H.id = -1;
    H.p[0] = H.p[1] = H.p[2] = 0.0; H.n[0] = H.n[1] = H.n[2] = 0.0;
    return H;
  }
  H.id = hi | (hin << 16);
  const rt_sphere *s = L.objects + hi;                   // (per lane: the sphere this lane hit)
  lit_hit_point(ox, oy, oz, rx, ry, rz, ht, s->origin[0], s->origin[1], s->origin[2], H.p, H.n);
  return H;
}

// the primary hit of sample (sx, sy): the ray of main.js:184-193, then ray_hit
__device__ __forceinline__ hit_core primary_hit(const rt_hits_launch &L, uint32_t sx, uint32_t sy) {
  const double d0 = ((double)sx - L.proj_w) + 0.5, d1 = (L.proj_h - (double)sy) - 0.5, d2 = L.proj_d;
  const double ox = L.cam[0], oy = L.cam[1], oz = L.cam[2];
  const double tx = ox + L.cam[3] * d0 + L.cam[6] * d0 + L.cam[9] * d0;
  const double ty = oy + L.cam[4] * d1 + L.cam[7] * d1 + L.cam[10] * d1;
  const double tz = oz + L.cam[5] * d2 + L.cam[8] * d2 + L.cam[11] * d2;
  double rx = tx - ox, ry = ty - oy, rz = tz - oz;
  (void)lit_unit(&rx, &ry, &rz);
  return ray_hit(L, ox, oy, oz, rx, ry, rz);
}

// the record rt_scene_pick and rt_scene_trace_rays_device return (include/rt_hip.h: rt_hit): u, v of main.js:446-447
__device__ __forceinline__ rt_hit hit_record(const hit_core &H) {
  rt_hit r;
  r.object = H.id < 0 ? -1 : (H.id & 0xffff);
  r.inside = H.id < 0 ? 0 : (H.id >> 16);
  r.t = H.t;
  for (int c = 0; c < 3; c++) { r.point[c] = H.p[c]; r.normal[c] = H.n[c]; }
  r.u = 0.0; r.v = 0.0;
  if (H.id >= 0) lit_hit_uv(H.n, &r.u, &r.v);
  return r;
}

// rt_render_hits_device: the samples of `tiles` (in output rows; tile slot i holds its k tile_rows sample rows one after another),
// band sample row by band sample row
__global__ void __launch_bounds__(RT_HITS_WG) rt_hits_kernel(const rt_hits_launch L) {
  const uint32_t sx = blockIdx.x * RT_HITS_WG + threadIdx.x;
  if (sx >= L.sw) return;
  const uint32_t rows_per_tile = L.k * L.tile_rows;
  for (uint32_t brow = blockIdx.y; brow < L.band_rows; brow += gridDim.y) {
    const uint32_t tile_i = brow / rows_per_tile, trow = brow - tile_i * rows_per_tile;
    const uint32_t sy = (L.tile_first + tile_i * L.tile_stride) * rows_per_tile + trow;
    if (sy >= L.sh) continue;                            // (a last tile that runs past the frame: those rows are not stored)
    const hit_core H = primary_hit(L, sx, sy);
    const size_t i = (size_t)brow * L.sw + sx;
    if (L.id) L.id[i] = H.id;
    if (L.depth) L.depth[i] = H.t;
    if (L.normal) {
      float *o = L.normal + 3u * i;
      o[0] = (float)H.n[0]; o[1] = (float)H.n[1]; o[2] = (float)H.n[2];
    }
  }
}

// rt_scene_pick: one work-item per sample point {x, y}
__global__ void __launch_bounds__(RT_HITS_WG) rt_pick_kernel(const rt_hits_launch L) {
  const uint32_t j = blockIdx.x * RT_HITS_WG + threadIdx.x;
  if (j >= L.n_points) return;
  const uint32_t sx = L.points[2u * j], sy = L.points[2u * j + 1u];
  L.hits[j] = hit_record(primary_hit(L, sx, sy));
}

// rt_scene_trace_rays_device, `hits`: one work-item per caller-supplied ray {org[3], dir[3]} (three 16-byte loads from the 16-byte
// aligned list), the direction as given.  A ray with a non-finite component is not traced: the miss record.  With L.ray_order
// (rt_scene_trace_rays_ordered_device) work-item `item` takes ray j = ray_order[item] - record j in, record j out - and skips an entry
// that names no ray.
__global__ void __launch_bounds__(RT_HITS_WG) rt_ray_hit_kernel(const rt_hits_launch L) {
  uint32_t j;
  if (!lit_ordered(L.ray_order, blockIdx.x * RT_HITS_WG + threadIdx.x, L.n_rays, &j)) return;   // (past the list, or an order's entry that names no ray)
  const lit_ray R = lit_load_ray(L.rays, j);
  hit_core H;
  H.id = -1; H.t = __builtin_inf(); H.p[0] = H.p[1] = H.p[2] = 0.0; H.n[0] = H.n[1] = H.n[2] = 0.0;
  if (R.finite) H = ray_hit(L, R.ox, R.oy, R.oz, R.rx, R.ry, R.rz);
  L.hits[j] = hit_record(H);
}

}  // namespace

extern "C" int rt_launch_ray_hits(const rt_hits_launch *L, hipStream_t stream) {
  hipLaunchKernelGGL(rt_ray_hit_kernel, dim3((L->n_rays + RT_HITS_WG - 1) / RT_HITS_WG), dim3(RT_HITS_WG), 0, stream, *L);   // (n_rays < 2^31)
  return (int)hipGetLastError();
}

extern "C" int rt_launch_hits(const rt_hits_launch *L, hipStream_t stream) {
  const uint32_t gy = L->band_rows < 65535u ? L->band_rows : 65535u;
  hipLaunchKernelGGL(rt_hits_kernel, dim3((L->sw + RT_HITS_WG - 1) / RT_HITS_WG, gy), dim3(RT_HITS_WG), 0, stream, *L);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_pick(const rt_hits_launch *L, hipStream_t stream) {
  hipLaunchKernelGGL(rt_pick_kernel, dim3((L->n_points + RT_HITS_WG - 1) / RT_HITS_WG), dim3(RT_HITS_WG), 0, stream, *L);
  return (int)hipGetLastError();
}
