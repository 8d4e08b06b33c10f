// rt_nodes.hip — wavefront tracing of ray lists (include/rt_hip.h: rt_scene_shade_rays_device, rt_scene_spawn_rays_device,
// rt_scene_fold_nodes_device): one level of the reference's intersectWorld (main.js:216-336) per launch instead of its recursion.
//   shade   ray i -> node i: the closest hit, the sampled colour, the diffuse and specular terms of the light loop, the material's
//           three weights and the two directions the reference would recurse into - everything of intersectWorld but its two
//           recursive calls (main.js:268-278) and the sum that needs their results (main.js:322-336)
//   spawn   the children of a level's nodes, compacted into the next level's ray list (by parent, reflect before refract)
//   fold    main.js:322-336 for a level's nodes, their children's colours gathered through the links spawn wrote
// This file is compiled WITHOUT FMA contraction (csrc/Makefile), sqrt and the division are correctly rounded, atan2 / asin are
// fdlibm's (rt_fdlibm.h) and pow is OCML's, as in the strict build of rt_kernel.hip: a node carries the bits of the C restatement
// (oracle/rt_oracle.c), and shade / spawn / fold level by level give rt_trace_rays' rgb bit for bit.  The arithmetic helpers are the
// strict side of rt_kernel_math.h, included here as rt_kernel.hip includes it; the closest-hit step, the hit record, the shadow-scan
// step, the workgroup scan and jsmin / jsmax are rt_literal.h's, which rt_hits.hip, rt_occlusion.hip and rt_rays_order.hip share.
//
// MI355X mapping.  Shade: one work-item per ray, 256 per workgroup.  The hit loop, the light loop and the shadow scans run at the top
// level of the kernel over wave-uniform indices - a lane that has no part in a step is masked, it does not branch around the loop -
// so each sphere is a scalar load from the uploaded blob (origin + r2, and albedo[4] in the scans) and each light a scalar load from
// the kernarg segment; a ballot ends a shadow scan when no lane is live.  The hit sphere's material, the texture descriptor and the
// texel are per-lane loads.  There is no recursion, no stack and no dynamically indexed private array: no scratch memory (the
// recursive rt_trace_rays<true> reserves 3 472 B per lane; tests/test_nodes_resources.py holds this file's kernels to 0).  The node is
// 200 bytes, 8-byte aligned: twelve 16-byte stores and one of 8.
// Spawn: three launches - children per workgroup of 256 parents, an exclusive scan of those totals by one workgroup, and a scatter in
// which every workgroup ranks its own parents again - plain vector stores, no atomics: the order is stable and the same on every run.
// Fold: one work-item per node, two gathers of 24 bytes through the links.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rt_nodes.h"

namespace {

#define RT_STRICT 1
#define RT_INF __builtin_inf()
#include "rt_literal.h"          // lit_closest_step, lit_hit_point / lit_hit_uv, lit_scan_step, lit_load_ray, workgroup_exclusive, jsmin / jsmax
#include "rt_kernel_math.h"      // v3, unit, reflect, min1, rt_sqrt / rt_rcp / rt_pow, rt_atan2_asin (fdlibm), star_uniform, to_int32_bit0, to_byte

typedef double __attribute__((ext_vector_type(2))) d2;
typedef double __attribute__((ext_vector_type(2), aligned(8))) d2u;     // a 16-byte access at an 8-byte aligned address (global memory allows it)

static_assert(sizeof(rt_node) == 200 && offsetof(rt_node, sample) == 80 && offsetof(rt_node, reflect_dir) == 144 && offsetof(rt_node, children) == 192,
              "rt_node: the stores below go by these offsets");

typedef const double __attribute__((address_space(4))) *kdouble;

// ---------------------------------------------------------------------------------------------------------------- shade
__global__ void __launch_bounds__(RT_NODES_WG) rt_nodes_shade(const rt_shade_launch L) {
  uint32_t i;
  if (!lit_ordered(L.order, blockIdx.x * RT_NODES_WG + threadIdx.x, L.n_rays, &i)) return;   // (past the list, or an order's entry that names no ray)
  const lit_ray R = lit_load_ray(L.rays, i);
  const v3 p = mk(R.ox, R.oy, R.oz), d = mk(R.rx, R.ry, R.rz);
  const double eps = L.epsilon;
  const uint32_t N = L.n_objects;
  const char __attribute__((address_space(4))) *tab = (const char __attribute__((address_space(4))) *)L.objects;
  d2u *out = (d2u *)(L.nodes + i);

  // ---- the closest hit: main.js:220-231, 420-451, every sphere in blob order, strict <, first wins
  double ht = __builtin_inf();
  int32_t hi = -1, hin = 0;
  for (uint32_t j = 0; j < N; j++) {
    const kdouble g = (kdouble)(tab + (size_t)j * sizeof(rt_sphere));
    const double gx = g[0], gy = g[1], gz = g[2], r2 = g[3];
    if (!R.finite) continue;
    lit_closest_step((int32_t)j, gx, gy, gz, r2, p.x, p.y, p.z, d.x, d.y, d.z, eps, &ht, &hi, &hin);
  }
  const bool hit = hi >= 0;
  const rt_sphere *s = L.objects + (hit ? hi : 0);                      // (per lane: the sphere this lane hit; a miss reads sphere 0 and uses nothing of it)

  // ---- hit.p, hit.n, u, v (main.js:440-447), stored at once
  v3 h = mk(0.0, 0.0, 0.0), n = mk(0.0, 0.0, 0.0);
  double hu = 0.0, hv = 0.0;
  if (hit) {
    double hp[3], hn[3];
    lit_hit_point(p.x, p.y, p.z, d.x, d.y, d.z, ht, s->origin[0], s->origin[1], s->origin[2], hp, hn);
    lit_hit_uv(hn, &hu, &hv);
    h = mk(hp[0], hp[1], hp[2]); n = mk(hn[0], hn[1], hn[2]);
  }
  {
    const unsigned long long head = (unsigned long long)(uint32_t)hi | ((unsigned long long)(uint32_t)hin << 32);
    d2u w;
    w.x = __builtin_bit_cast(double, head); w.y = ht; out[0] = w;
    w.x = h.x; w.y = h.y; out[1] = w;
    w.x = h.z; w.y = n.x; out[2] = w;
    w.x = n.y; w.y = n.z; out[3] = w;
    w.x = hu; w.y = hv; out[4] = w;
  }
  const v3 l = hin ? mk(-n.x, -n.y, -n.z) : n;                           // hit.l, quirk q5
  const double a0 = hit ? s->albedo[0] : 0.0, a1 = hit ? s->albedo[1] : 0.0, a2 = hit ? s->albedo[2] : 0.0;
  const double a3 = hit ? s->albedo[3] : 0.0, a4 = hit ? s->albedo[4] : 0.0;

  // ---- the sampler (main.js:320), as the strict build of trace_pixel has it
  double col[3];
  if (!hit) {
    const double nan = __builtin_nan("");
    col[0] = R.finite ? L.miss_color[0] : nan; col[1] = R.finite ? L.miss_color[1] : nan; col[2] = R.finite ? L.miss_color[2] : nan;
  } else {
    const int kind = s->sampler_kind;
    if (kind == RT_SAMPLER_TEXTURE) {
      const uint32_t ti = (uint32_t)s->texture < RT_MAX_TEXTURES ? (uint32_t)s->texture : 0u;   // memory safety only: the upload checked it
      const rt_texture_desc td = L.textures[ti];
      const double xd = ceil(hu * (double)td.width) - 1.0, yd = ceil(hv * (double)td.height) - 1.0;
      uint32_t xi = (xd > 0.0) ? (uint32_t)xd : 0u, yi = (yd > 0.0) ? (uint32_t)yd : 0u;
      xi = min(xi, td.width - 1u); yi = min(yi, td.height - 1u);      // memory safety only; u,v <= 1
      const uint32_t texel = *(const uint32_t *)(L.texel_base + td.texels_offset + ((size_t)yi * td.width + xi) * 4u);
      col[0] = (double)(texel & 255u) / 255.0; col[1] = (double)((texel >> 8) & 255u) / 255.0; col[2] = (double)((texel >> 16) & 255u) / 255.0;
      if (xd != xd || yd != yd) col[0] = col[1] = col[2] = __builtin_nan("");   // texels[NaN] is undefined in JS
    } else if (kind == RT_SAMPLER_CHECKER) {
      const double u = fd_atan2(-n.y, -n.x) / M_PI / 2.0 + 0.5;         // main.js:127 (its own axes)
      const double v = fd_asin(-n.z) / (M_PI / 2.0) / 2.0 + 0.5;        // main.js:128
      const int c = to_int32_bit0(u * s->checker_freq[0]) ^ to_int32_bit0(v * s->checker_freq[1]);
      const double *cc = &s->checker_color[0][0] + 3 * c;
      col[0] = cc[0]; col[1] = cc[1]; col[2] = cc[2];
    } else if (kind == RT_SAMPLER_STARS) {
      const uint32_t pix = L.pix ? L.pix[i] : L.pix_base + i, path = L.path ? L.path[i] : 1u;
      double c = star_uniform(pix, 0u, path, lowbias32(L.stars_seed));
      c = (c >= s->checker_freq[0]) ? 0.0 : c * s->checker_freq[1];     // main.js:137-138
      col[0] = col[1] = col[2] = c;
    } else { col[0] = s->color[0]; col[1] = s->color[1]; col[2] = s->color[2]; }
  }

  // ---- lights and shadow scans (main.js:280-318).  Every lane of the wave walks the loops; `shading` / `lit` / `live` mask its part
  const bool shading = hit && (a1 > 0.0 || a2 > 0.0);
  double diffuse = 0.0, specular = 0.0;
  double li = L.light_intensity;                                        // one intensity, carried from light to light (q2)
  const double spec_e = s->specular_exponent;
  for (uint32_t k = 0; k < L.n_lights; k++) {
    const double *lk = (const double *)((const char *)&L.lights[0][0] + (uint32_t)(k * 24u));   // (the kernarg segment: a scalar load)
    const double lkx = lk[0], lky = lk[1], lkz = lk[2];
    const v3 sraw = mk(lkx - h.x, lky - h.y, lkz - h.z);
    const double lmag = dot(sraw, sraw);
    double llen;
    const v3 sv = unit(sraw, &llen);
    const double sdot = dot(sv, l);
    const bool lit = shading && !(sdot <= 0.0);                          // surface faces away (main.js:292)
    // the shadow scan (rt_occlusion.hip's loop) from the hit point along sv, the hit sphere left out (a lane whose intensity is 0 already can gain nothing)
    bool live = lit && li != 0.0;
    int32_t blocker;                                                    // (the scan names it; a node does not keep it)
    for (uint32_t j = 0; j < N; j++) {
      if (__builtin_amdgcn_ballot_w64(live) == 0) break;                // no lane of the wave has a sphere left to meet
      const kdouble g = (kdouble)(tab + (size_t)j * sizeof(rt_sphere));
      const double gx = g[0], gy = g[1], gz = g[2], r2 = g[3];
      const double o4 = g[12];                                          // albedo[4]: byte 96 of the record
      if (!live || (int32_t)j == hi) continue;
      lit_scan_step((int32_t)j, gx, gy, gz, r2, o4, h.x, h.y, h.z, sv.x, sv.y, sv.z, eps, llen, &li, &blocker, &live);   // (a transparent occluder brightens: q2)
    }
    if (lit && li != 0.0) {
      diffuse += li * sdot / lmag;                                      // main.js:306
      if (a2 > 0.0) {                                                   // main.js:307-314
        double ql;
        const v3 q = unit(reflect(mk(-sv.x, -sv.y, -sv.z), l), &ql);
        const double spd = d.x * -q.x + d.y * -q.y + d.z * -q.z;
        if (spd > 0.0) specular += rt_pow(spd, spec_e);
      }
    }
  }
  if (shading) { diffuse = min1(diffuse) * a1; specular = min1(specular) * a2; }
  {
    d2u w;
    w.x = col[0]; w.y = col[1]; out[5] = w;
    w.x = col[2]; w.y = diffuse; out[6] = w;
    w.x = specular; w.y = a0; out[7] = w;
    w.x = a3; w.y = a4; out[8] = w;
  }

  // ---- the two directions (main.js:233-266), whatever the depth left
  v3 r = mk(0.0, 0.0, 0.0); double rlen = 0.0;
  if (a3 > 0.0) r = unit(reflect(d, n), &rlen);
  v3 f = mk(0.0, 0.0, 0.0); double flen = 0.0;
  if (a4 > 0.0) {
    const double dn = dot(d, n);
    double cosi = -((dn < -1.0) ? -1.0 : min1(dn));                    // -Math.max(-1, Math.min(1, dot))
    v3 nn = n; double eta;
    if (cosi < 0.0) { cosi = -cosi; nn = mk(-n.x, -n.y, -n.z); eta = s->refract_index; }
    else eta = rt_rcp(s->refract_index);
    const double kk = 1.0 - eta * eta * (1.0 - cosi * cosi);
    if (kk > 0.0) {
      const double q = eta * cosi - rt_sqrt(kk);
      f = mk(d.x * eta + nn.x * q, d.y * eta + nn.y * q, d.z * eta + nn.z * q);
    } else f = reflect(d, nn);                                         // total internal reflection
    f = unit(f, &flen);
  }
  const bool go_r = rlen != 0.0, go_f = flen != 0.0;
  if (!go_r) r = mk(0.0, 0.0, 0.0);
  if (!go_f) f = mk(0.0, 0.0, 0.0);
  {
    d2u w;
    w.x = r.x; w.y = r.y; out[9] = w;
    w.x = r.z; w.y = f.x; out[10] = w;
    w.x = f.y; w.y = f.z; out[11] = w;
    *(unsigned long long *)(out + 12) = (unsigned long long)((go_r ? 1u : 0u) | (go_f ? 2u : 0u));   // children, reserved = 0
  }
}

// ---------------------------------------------------------------------------------------------------------------- spawn
__device__ __forceinline__ uint32_t children_of(const rt_node *nodes, uint32_t i, uint32_t n) { return i < n ? (nodes[i].children & 3u) : 0u; }

// workgroup b: the children of parents [256 b, 256 b + 256) -> totals[b]
__global__ void __launch_bounds__(RT_NODES_WG) rt_nodes_spawn_count(const rt_spawn_launch L) {
  __shared__ uint32_t s_tmp[RT_NODES_WG];
  const uint32_t ch = children_of(L.nodes, blockIdx.x * RT_NODES_WG + threadIdx.x, L.n);
  uint32_t total;
  (void)workgroup_exclusive<RT_NODES_WG>((ch & 1u) + (ch >> 1), s_tmp, &total);
  if (threadIdx.x == 0u) L.totals[blockIdx.x] = total;
}

// one workgroup: totals[0..tiles) -> exclusive prefixes; *count = the sum (rt_rays_order.hip: rt_order_scan)
__global__ void __launch_bounds__(RT_NODES_WG) rt_nodes_spawn_scan(const rt_spawn_launch L, uint32_t tiles) {
  __shared__ uint32_t s_tmp[RT_NODES_WG];
  uint32_t carry = 0u;
  for (uint32_t base = 0; base < tiles; base += RT_NODES_WG) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < tiles ? L.totals[i] : 0u;
    uint32_t total;
    const uint32_t ex = workgroup_exclusive<RT_NODES_WG>(v, s_tmp, &total);
    if (i < tiles) L.totals[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0u) *L.count = carry;
}

// workgroup b ranks its parents again and writes their children and links
__global__ void __launch_bounds__(RT_NODES_WG) rt_nodes_spawn_scatter(const rt_spawn_launch L) {
  __shared__ uint32_t s_tmp[RT_NODES_WG];
  const uint32_t i = blockIdx.x * RT_NODES_WG + threadIdx.x;
  const uint32_t ch = children_of(L.nodes, i, L.n);
  uint32_t total;
  const uint32_t at = L.totals[blockIdx.x] + workgroup_exclusive<RT_NODES_WG>((ch & 1u) + (ch >> 1), s_tmp, &total);
  if (i >= L.n) return;
  const uint32_t c_r = at, c_f = at + (ch & 1u);                     // (< 2n: the prefixes are of these very counts)
  L.links[2u * (size_t)i] = (ch & 1u) ? (int32_t)c_r : -1;
  L.links[2u * (size_t)i + 1u] = (ch & 2u) ? (int32_t)c_f : -1;
  if (ch == 0u) return;
  const uint32_t pix = L.pix ? L.pix[i] : L.pix_base + i, path = L.path ? L.path[i] : 1u;
  const double *q = (const double *)(L.nodes + i);
  const double px = q[2], py = q[3], pz = q[4];                       // hit.point; q[18..20] reflect_dir, q[21..23] refract_dir
  if (ch & 1u) {
    d2 *o = (d2 *)(L.child_rays + 6u * (size_t)c_r);
    d2 w;
    w.x = px; w.y = py; o[0] = w;
    w.x = pz; w.y = q[18]; o[1] = w;
    w.x = q[19]; w.y = q[20]; o[2] = w;
    if (L.child_pix) L.child_pix[c_r] = pix;
    if (L.child_path) L.child_path[c_r] = 2u * path;
  }
  if (ch & 2u) {
    d2 *o = (d2 *)(L.child_rays + 6u * (size_t)c_f);
    d2 w;
    w.x = px; w.y = py; o[0] = w;
    w.x = pz; w.y = q[21]; o[1] = w;
    w.x = q[22]; w.y = q[23]; o[2] = w;
    if (L.child_pix) L.child_pix[c_f] = pix;
    if (L.child_path) L.child_path[c_f] = 2u * path + 1u;
  }
}

// ---------------------------------------------------------------------------------------------------------------- fold
__global__ void __launch_bounds__(RT_NODES_WG) rt_nodes_fold(const rt_fold_launch L) {
  const uint32_t i = blockIdx.x * RT_NODES_WG + threadIdx.x;
  if (i >= L.n) return;
  const rt_node *nd = L.nodes + i;
  const double *q = (const double *)nd;
  double rgb[3] = {q[10], q[11], q[12]};                              // a miss: the sample itself (main.js:231)
  if (nd->hit.object >= 0) {
    const double diffuse = q[13], specular = q[14], a0 = q[15], a3 = q[16], a4 = q[17];
    double re[3] = {0.0, 0.0, 0.0}, rf[3] = {0.0, 0.0, 0.0};
    if (L.links) {
      const int32_t lr = L.links[2u * (size_t)i], lf = L.links[2u * (size_t)i + 1u];
      if (lr >= 0) { const double *c = L.child_rgb + 3u * (size_t)lr; re[0] = c[0] * a3; re[1] = c[1] * a3; re[2] = c[2] * a3; }
      if (lf >= 0) { const double *c = L.child_rgb + 3u * (size_t)lf; rf[0] = c[0] * a4; rf[1] = c[1] * a4; rf[2] = c[2] * a4; }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double shade = rgb[c] * diffuse + rgb[c] * specular + re[c] + rf[c];
      rgb[c] = jsmax(rgb[c] * a0, jsmin(1.0, shade));
    }
  }
  if (L.rgb) { double *o = L.rgb + 3u * (size_t)i; o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2]; }
  if (L.rgba) L.rgba[i] = to_byte(rgb[0]) | (to_byte(rgb[1]) << 8) | (to_byte(rgb[2]) << 16) | 0xff000000u;
}

}  // namespace

extern "C" int rt_launch_shade_nodes(const rt_shade_launch *L, hipStream_t stream) {
  hipLaunchKernelGGL(rt_nodes_shade, dim3((L->n_rays + RT_NODES_WG - 1u) / RT_NODES_WG), dim3(RT_NODES_WG), 0, stream, *L);   // (n_rays < 2^31)
  return (int)hipGetLastError();
}

extern "C" int rt_launch_spawn_nodes(const rt_spawn_launch *L, hipStream_t stream) {
  const uint32_t tiles = rt_spawn_tiles(L->n);
  hipLaunchKernelGGL(rt_nodes_spawn_count, dim3(tiles), dim3(RT_NODES_WG), 0, stream, *L);
  hipLaunchKernelGGL(rt_nodes_spawn_scan, dim3(1u), dim3(RT_NODES_WG), 0, stream, *L, tiles);
  hipLaunchKernelGGL(rt_nodes_spawn_scatter, dim3(tiles), dim3(RT_NODES_WG), 0, stream, *L);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_fold_nodes(const rt_fold_launch *L, hipStream_t stream) {
  hipLaunchKernelGGL(rt_nodes_fold, dim3((L->n + RT_NODES_WG - 1u) / RT_NODES_WG), dim3(RT_NODES_WG), 0, stream, *L);
  return (int)hipGetLastError();
}
