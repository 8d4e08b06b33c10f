// rt_relight.hip — relit nodes (include/rt_hip.h: rt_scene_relight_nodes_device): the two numbers of a wavefront node the lights decide,
// diffuse and specular, computed again over n_samples displaced copies of the lights and their mean written back into the node.  Per
// sample it is the light loop of rt_nodes.hip's shade kernel (main.js:280-318) operation for operation, with the light's position
// replaced by rt_lighting.h's lgt_light_pos; the table entry of a sample is rt_ambient.h's walk, as rt_lighting.hip takes it; the terms
// are clamped and weighted per sample (main.js:316-317) and folded as a sampled view folds: the mean of the nodes rt_nodes_shade writes
// for the same ray in n_samples scenes whose lights were moved on the host.  The unit is built without FMA contraction, with the strict
// side of rt_kernel_math.h (pow is OCML's), as rt_nodes.hip is.  One kernel:
//   rt_relight_kernel    rt_nodes_shade's mapping: one work-item per node, 256 per workgroup; the node's hit record and the ray's
//                        direction are read once, the hit sphere's albedo[1], albedo[2] and specular exponent are one per-lane load;
//                        the sample loop, the light loop and the sphere loop are wave-uniform; a light is three scalar loads from the
//                        kernel arguments, a sphere two from the uploaded blob (origin + r2, and albedo[4] at byte 96); a ballot ends a
//                        scan when no lane is live.  With stride == 0 every node reads the same table entry: three scalar loads; with
//                        light_radius == 0 the table is not read.  16 bytes are stored per node, at byte 104.
// It follows the shade kernel's loop, not rt_lighting.hip's: no scan is started for a light once the carried intensity is 0.
// No LDS, no scratch (tests/test_relight_resources.py).  No test switches: one object for both libraries.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rt_relight.h"

namespace {
#define RT_STRICT 1
#define RT_INF __builtin_inf()
#include "rt_kernel_math.h"      // v3, dot, unit, reflect, min1, rt_pow: the strict side, as rt_nodes.hip includes it

typedef double __attribute__((ext_vector_type(2), aligned(8))) d2u;     // a 16-byte access at an 8-byte aligned address (global memory allows it)
typedef const double __attribute__((address_space(4))) *kdouble;        // scalar loads: the address is wave-uniform

static_assert(sizeof(rt_node) == 200 && offsetof(rt_node, diffuse) == 104 && offsetof(rt_node, specular) == 112, "rt_node: the store below goes by these offsets");
static_assert(offsetof(rt_sphere, albedo) == 64 && offsetof(rt_sphere, specular_exponent) == 56, "rt_sphere: albedo[4] is byte 96");
}  // namespace

__global__ void __launch_bounds__(RT_RELIGHT_WG) rt_relight_kernel(const rt_relight_launch L) {
  uint32_t i;
  if (!lit_ordered(L.order, blockIdx.x * RT_RELIGHT_WG + threadIdx.x, L.n, &i)) return;   // (past the list, or an order's entry that names no node)
  const lit_ray R = lit_load_ray(L.rays, i);
  const v3 d = mk(R.rx, R.ry, R.rz);
  const rt_hit *H = &L.nodes[i].hit;
  const int32_t hi = H->object, hin = H->inside;
  const v3 h = mk(H->point[0], H->point[1], H->point[2]), n = mk(H->normal[0], H->normal[1], H->normal[2]);
  const bool hit = hi >= 0;
  const uint32_t N = L.n_objects;
  const rt_sphere *sp = L.objects + ((uint32_t)hi < N ? (uint32_t)hi : 0u);   // (per lane; a miss reads sphere 0 and uses nothing of it; memory safety for a foreign node)
  const double a1 = hit ? sp->albedo[1] : 0.0, a2 = hit ? sp->albedo[2] : 0.0;
  const double spec_e = sp->specular_exponent;
  const v3 l = hin ? mk(-n.x, -n.y, -n.z) : n;                           // hit.l, quirk q5
  const bool shading = hit && (a1 > 0.0 || a2 > 0.0);
  const double eps = L.epsilon, radius = L.light_radius;
  const char __attribute__((address_space(4))) *tab = (const char __attribute__((address_space(4))) *)L.objects;
  const kdouble soffs = (kdouble)L.offs;
  const amb_walk W = amb_walk_of(L.base, L.pix ? L.pix[i] : i, L.stride, L.n_offs);   // (one 64-bit reduction per node, none per sample)
  double acc_d = 0.0, acc_s = 0.0;
  for (uint32_t s = 0; s < L.n_samples; s++) {
    double o[3] = {0.0, 0.0, 0.0};
    if (radius != 0.0) {
      if (L.stride == 0u) {                                              // one entry for the whole launch: scalar loads
        const kdouble q = soffs + 3u * (size_t)s;                        // (e = s: s < n_samples <= n_offs)
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
      } else {
        const double *q = L.offs + 3u * (size_t)amb_walk_entry(W, s, L.n_offs);
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
      }
    }
    // ---- rt_nodes_shade's lights and shadow scans (main.js:280-318), the light displaced
    double diffuse = 0.0, specular = 0.0;
    double li = L.light_intensity;                                       // one intensity, carried from light to light (q2)
    for (uint32_t k = 0; k < L.n_lights; k++) {
      const double light[3] = {L.lights[k][0], L.lights[k][1], L.lights[k][2]};   // (the kernel arguments: scalar loads)
      double pos[3];
      lgt_light_pos(light, radius, o, pos);
      const v3 sraw = mk(pos[0] - h.x, pos[1] - h.y, pos[2] - h.z);
      const double lmag = dot(sraw, sraw);
      double llen;
      const v3 sv = unit(sraw, &llen);
      const double sdot = dot(sv, l);
      const bool lit = shading && !(sdot <= 0.0);                        // surface faces away (main.js:292)
      bool live = lit && li != 0.0;                                      // (a lane whose intensity is 0 already can gain nothing: shade's rule)
      int32_t blocker;
      for (uint32_t j = 0; j < N; j++) {
        if (__builtin_amdgcn_ballot_w64(live) == 0) break;               // no lane of the wave has a sphere left to meet
        const kdouble g = (kdouble)(tab + (size_t)j * sizeof(rt_sphere));
        const double gx = g[0], gy = g[1], gz = g[2], r2 = g[3];
        const double o4 = g[12];                                         // albedo[4]: byte 96 of the record
        if (!live || (int32_t)j == hi) continue;
        lit_scan_step((int32_t)j, gx, gy, gz, r2, o4, h.x, h.y, h.z, sv.x, sv.y, sv.z, eps, llen, &li, &blocker, &live);
      }
      if (lit && li != 0.0) {
        diffuse += li * sdot / lmag;                                     // main.js:306
        if (a2 > 0.0) {                                                  // main.js:307-314
          double ql;
          const v3 q = unit(reflect(mk(-sv.x, -sv.y, -sv.z), l), &ql);
          const double spd = d.x * -q.x + d.y * -q.y + d.z * -q.z;
          if (spd > 0.0) specular += rt_pow(spd, spec_e);
        }
      }
    }
    const double diffuse_s = min1(diffuse) * a1, specular_s = min1(specular) * a2;   // main.js:316-317, per sample
    acc_d = s == 0u ? diffuse_s : acc_d + diffuse_s;
    acc_s = s == 0u ? specular_s : acc_s + specular_s;
  }
  d2u w;
  w.x = shading ? acc_d / (double)L.n_samples : 0.0;                     // (a miss, or neither albedo[1] nor [2] > 0: what shade wrote)
  w.y = shading ? acc_s / (double)L.n_samples : 0.0;
  *(d2u *)((char *)(L.nodes + i) + offsetof(rt_node, diffuse)) = w;
}

extern "C" int rt_launch_relight(const rt_relight_launch *L, void *hip_stream) {
  hipLaunchKernelGGL(rt_relight_kernel, dim3((L->n + RT_RELIGHT_WG - 1u) / RT_RELIGHT_WG), dim3(RT_RELIGHT_WG), 0, (hipStream_t)hip_stream, *L);   // (n < 2^31)
  return (int)hipGetLastError();
}
