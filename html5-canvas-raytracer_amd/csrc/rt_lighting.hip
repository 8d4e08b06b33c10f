// rt_lighting.hip — sampled lights (include/rt_hip.h: rt_lighting, rt_scene_lighting_device): the reference's light loop (main.js:283-306)
// per receiver, n_samples times with every light displaced by a table entry times light_radius, folded on the GPU.  The receivers are
// hit records; the arithmetic that turns a record, a light and a table entry into a segment is rt_lighting.h's, the host probe's own
// source, and the scan is rt_occlusion.hip's (rt_literal.h: lit_scan_step), started with the intensity the light before left (quirk q2).
// The unit is built without FMA contraction.  One kernel:
//   rt_lighting_kernel   rt_ambient_kernel's mapping: one work-item per receiver, 256 receivers per workgroup; the record is read once;
//                        the sample loop, the light loop and the sphere loop are all wave-uniform; a light is three scalar loads from the
//                        kernel arguments, a sphere two from the uploaded blob (origin + r2, and albedo[4] at byte 96); a lane that does
//                        not face the light, or whose scan has met its opaque sphere, is not live, and the wave leaves the sphere loop on
//                        an empty ballot.  No segment exists in memory: 8 to 28 bytes are stored per receiver.  With stride == 0 every
//                        receiver reads the same table entry: three scalar loads instead of three vector loads; with light_radius == 0
//                        the table is not read (both wave-uniform branches on kernel arguments).
// No scan is skipped for an intensity that is already 0: a glass sphere divides it by albedo[4], and rt_scene_validate admits a negative
// albedo[4] (the quotient is -0, other bytes) and a NaN (the quotient is NaN, and the light after contributes).
// No LDS, no scratch (tests/test_lighting_resources.py).  No test switches: one object for both libraries.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rt_lighting.h"
#include "rt_fdlibm.h"

namespace {
#define RT_STRICT 1
#define RT_INF __builtin_inf()
#include "rt_kernel_math.h"      // to_byte: the store rule of main.js:195-198, as rt_ambient_kernel uses it

typedef const double __attribute__((address_space(4))) *sdouble_ptr;     // scalar loads: the address is wave-uniform
}  // namespace

__global__ void __launch_bounds__(RT_LIGHTING_WG) rt_lighting_kernel(const rt_lighting_launch L) {
  uint32_t i;
  if (!lit_ordered(L.order, blockIdx.x * RT_LIGHTING_WG + threadIdx.x, L.n, &i)) return;   // (past the list, or an order's entry that names no receiver)
  const rt_hit *H = L.hits + i;
  const lgt_receiver R = lgt_receiver_of(H->object, H->inside, H->point[0], H->point[1], H->point[2], H->normal[0], H->normal[1], H->normal[2]);
  const uint32_t skip = (uint32_t)R.skip;                            // (-1 matches no j)
  const double eps = L.epsilon, radius = L.light_radius;
  const char __attribute__((address_space(4))) *tab = (const char __attribute__((address_space(4))) *)L.objects;
  const sdouble_ptr soffs = (sdouble_ptr)L.offs;
  const amb_walk W = amb_walk_of(L.base, i, L.stride, L.n_offs);     // (one 64-bit reduction per receiver, none per sample)
  uint32_t contributed = 0;
  double acc_d = 0.0, acc_i = 0.0;
  for (uint32_t s = 0; s < L.n_samples; s++) {
    double o[3] = {0.0, 0.0, 0.0};
    if (radius != 0.0) {
      if (L.stride == 0u) {                                          // one entry for the whole launch: scalar loads
        const sdouble_ptr d = soffs + 3u * (size_t)s;                // (e = s: s < n_samples <= n_offs)
        o[0] = d[0]; o[1] = d[1]; o[2] = d[2];
      } else {
        const double *d = L.offs + 3u * (size_t)amb_walk_entry(W, s, L.n_offs);
        o[0] = d[0]; o[1] = d[1]; o[2] = d[2];
      }
    }
    double li = L.light_intensity, diffuse = 0.0;
    for (uint32_t k = 0; k < L.n_lights; k++) {
      const double light[3] = {L.lights[k][0], L.lights[k][1], L.lights[k][2]};
      double pos[3];
      lgt_light_pos(light, radius, o, pos);
      const lgt_segment S = lgt_segment_of(R.p, R.l, pos);
      const bool faces = R.scanned && lgt_faces(S);
      const bool traced = lgt_traced(S);
      int32_t blocker = -1;
      bool live = faces && traced;
      for (uint32_t j = 0; j < L.n_objects; j++) {
        if (__builtin_amdgcn_ballot_w64(live) == 0) break;           // no lane of the wave has a sphere left to meet
        const sdouble_ptr g = (sdouble_ptr)(tab + (size_t)j * sizeof(rt_sphere));
        const double gx = g[0], gy = g[1], gz = g[2], r2 = g[3];
        const double a4 = g[12];                                     // albedo[4]: byte 96 of the record
        if (!live || j == skip) continue;
        lit_scan_step((int32_t)j, gx, gy, gz, r2, a4, R.p[0], R.p[1], R.p[2], S.sv[0], S.sv[1], S.sv[2], eps, S.len, &li, &blocker, &live);
      }
      if (!faces) continue;
      if (!traced) li = __builtin_nan("");
      lgt_contribute(S, li, &diffuse, &contributed);
    }
    acc_d = s == 0u ? diffuse : acc_d + diffuse;
    acc_i = s == 0u ? li : acc_i + li;
  }
  const double nan = __builtin_nan("");
  const double diffuse = R.scanned ? acc_d / (double)L.n_samples : nan;
  if (L.diffuse) L.diffuse[i] = diffuse;
  if (L.intensity) L.intensity[i] = R.scanned ? acc_i / (double)L.n_samples : nan;
  if (L.lit) L.lit[i] = L.n_lights ? (double)contributed / (double)(L.n_samples * L.n_lights) : 0.0;
  if (L.rgba) { const uint32_t b = to_byte(jsmin(1.0, diffuse)); L.rgba[i] = b | (b << 8) | (b << 16) | 0xff000000u; }
}

extern "C" int rt_launch_lighting(const rt_lighting_launch *L, void *hip_stream) {
  hipLaunchKernelGGL(rt_lighting_kernel, dim3((L->n + RT_LIGHTING_WG - 1u) / RT_LIGHTING_WG), dim3(RT_LIGHTING_WG), 0, (hipStream_t)hip_stream, *L);   // (n < 2^31)
  return (int)hipGetLastError();
}

extern "C" void rt_lighting_segments_host(const rt_lighting_launch *L, uint32_t sample, uint32_t light, double *rays, double *length, double *mag,
                                          double *dot, int32_t *skip) {
  const double nan = __builtin_nan("");
  for (uint32_t i = 0; i < L->n; i++) {
    const rt_hit &H = L->hits[i];
    const lgt_receiver R = lgt_receiver_of(H.object, H.inside, H.point[0], H.point[1], H.point[2], H.normal[0], H.normal[1], H.normal[2]);
    double *q = rays + 6u * (size_t)i;
    if (skip) skip[i] = R.skip;
    if (!R.scanned) {
      for (int c = 0; c < 6; c++) q[c] = nan;
      if (length) length[i] = nan;
      if (mag) mag[i] = nan;
      if (dot) dot[i] = nan;
      continue;
    }
    const double *o = L->light_radius == 0.0 ? nullptr : L->offs + 3u * (size_t)amb_entry(L->base, i, L->stride, sample, L->n_offs);
    double pos[3];
    lgt_light_pos(L->lights[light], L->light_radius, o, pos);
    const lgt_segment S = lgt_segment_of(R.p, R.l, pos);
    q[0] = R.p[0]; q[1] = R.p[1]; q[2] = R.p[2]; q[3] = S.sv[0]; q[4] = S.sv[1]; q[5] = S.sv[2];
    if (length) length[i] = S.len;
    if (mag) mag[i] = S.mag;
    if (dot) dot[i] = S.sd;
  }
}

extern "C" void rt_lighting_sphere_offsets_host(uint32_t n, double *out) {
  const double golden = M_PI * (3.0 - sqrt(5.0));
  for (uint32_t k = 0; k < n; k++) {
    const double z = 1.0 - (2.0 * (double)k + 1.0) / (double)n, phi = (double)k * golden, r = sqrt(1.0 - z * z);
    out[3u * (size_t)k] = r * fd_cos(phi); out[3u * (size_t)k + 1u] = r * fd_sin(phi); out[3u * (size_t)k + 2u] = z;
  }
}
