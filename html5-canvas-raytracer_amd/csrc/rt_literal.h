// rt_literal.h - the literal primitives of the ray-list kernels: the reference's intersectSphere with its epsilon rule, one step of the
// closest-hit loop and of the shadow scan, the hit record, the ray record of a list and its finite test, the order indirection, Math.min /
// Math.max and the workgroup scan.  Literal: operation for operation with main.js, for units compiled WITHOUT FMA contraction
// (csrc/Makefile: -ffp-contract=off; sqrt and `/` correctly rounded), so that what is built from these carries the bits of the C
// restatement (oracle/rt_oracle.c) - no tolerance.  Used by rt_hits.hip, rt_occlusion.hip, rt_nodes.hip, rt_rays_order.hip, the list head
// of rt_trace_rays (rt_kernel.hip) and, for the finite test, the host side of rt_frame.hip; tests/host/literal_check.cpp compiles it
// with a plain host compiler and holds it to the restatement on a CPU.
// The functions work on values: a kernel keeps its own loads (a sphere's origin, r2 and albedo[4] are scalar loads from the blob) and
// its own masking and ballots, and hands over what it loaded.  A .hip unit includes this inside its anonymous namespace, as it does
// rt_fdlibm.h.
#ifndef RT_LITERAL_H
#define RT_LITERAL_H

#include <math.h>
#include <stdint.h>

#include "rt_fdlibm.h"

#if defined(__HIPCC__)
#define RT_LIT __host__ __device__ __forceinline__
#else
#define RT_LIT static inline
#endif
// tests/host/literal_check.cpp counts the exits taken, by the numbers below; the kernels compile this away
#ifndef RT_LIT_EXIT
#define RT_LIT_EXIT(k)
#endif

// Math.min / Math.max (oracle/rt_oracle.c: jsmin, jsmax): NaN if either argument is
RT_LIT double jsmin(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : (a < b ? a : b); }
RT_LIT double jsmax(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : (a > b ? a : b); }

// normal3D (main.js:62-66): v * (1 / |v|) in place, the zero vector left as it is -> |v|
RT_LIT double lit_unit(double *x, double *y, double *z) {
  const double l = sqrt(*x * *x + *y * *y + *z * *z);
  if (l != 0.0) { const double k = 1.0 / l; *x *= k; *y *= k; *z *= k; }
  return l;
}

// intersectSphere (main.js:420-439) of the sphere at g with squared radius r2 and the ray (o, r), r as given: where the sphere is met at
// or beyond epsilon, met(t, inside) with inside = (t0 < eps) || (t1 < eps) (main.js:445); where it is not, nothing.  (A callback, not a
// returned flag or a returned +Infinity: inlined, a sphere that is not met leaves the caller's loop body as a `continue` does - with a
// flag the kernels re-join and test it, with +Infinity they run the caller's comparison for every sphere; both were measurably slower.)
template <class MET>
RT_LIT void lit_sphere(double gx, double gy, double gz, double r2, double ox, double oy, double oz, double rx, double ry, double rz, double eps,
                       MET met) {
  const double lx = gx - ox, ly = gy - oy, lz = gz - oz;
  const double tca = rx * lx + ry * ly + rz * lz;
  const double dd = (lx * lx + ly * ly + lz * lz) - tca * tca;
  if (dd > r2) { RT_LIT_EXIT(0); return; }                            // 0: the line passes the sphere
  const double thc = sqrt(r2 - dd);
  const double t0 = tca - thc, t1 = tca + thc;
  double t;
  if (t0 < t1) {                                                      // 1: both behind  2: t1, the ray starts inside  3: t0
    if (t0 < eps) { if (t1 < eps) { RT_LIT_EXIT(1); return; } RT_LIT_EXIT(2); t = t1; } else { RT_LIT_EXIT(3); t = t0; }
  } else {                                                            // t0 == t1 (a tangent ray: thc == 0) or unordered (a NaN thc)
    // 4: both behind  5: t0 - needs thc < 0, which sqrt never gives: written as the reference has it  6: t1 (a NaN thc: t is NaN)
    if (t1 < eps) { if (t0 < eps) { RT_LIT_EXIT(4); return; } RT_LIT_EXIT(5); t = t0; } else { RT_LIT_EXIT(6); t = t1; }
  }
  met(t, (t0 < eps) || (t1 < eps));
}

// one sphere of the closest-hit loop (main.js:220-231): sphere j in blob order, strict <, so the first of equals wins
RT_LIT void lit_closest_step(int32_t j, double gx, double gy, double gz, double r2, double ox, double oy, double oz, double rx, double ry, double rz,
                             double eps, double *ht, int32_t *hi, int32_t *hin) {
  lit_sphere(gx, gy, gz, r2, ox, oy, oz, rx, ry, rz, eps, [=](double t, bool inside) {
    if (t < *ht) { *ht = t; *hi = j; *hin = inside; }
  });
}

// one sphere of the shadow scan (main.js:293-304) - sphere j, not the one the caller leaves out - with albedo[4] = a4, towards a light
// `len` away (t < len is false for a NaN t or a NaN len): glass divides the intensity (quirk q2); an opaque sphere ends the scan: *li = 0,
// *blocker = j, *live = false.  (The opaque arm does all three, so that it stays a branch of its own: a4 is wave-uniform in the kernels,
// and a wave in front of an opaque sphere skips the division.)
RT_LIT void lit_scan_step(int32_t j, double gx, double gy, double gz, double r2, double a4, double ox, double oy, double oz, double rx, double ry,
                          double rz, double eps, double len, double *li, int32_t *blocker, bool *live) {
  lit_sphere(gx, gy, gz, r2, ox, oy, oz, rx, ry, rz, eps, [=](double t, bool) {
    if (t < len) {
      if (a4 != 0.0) { RT_LIT_EXIT(8); *li = *li / a4; }               // 8: glass
      else { RT_LIT_EXIT(9); *li = 0.0; *blocker = j; *live = false; } // 9: opaque
    } else { RT_LIT_EXIT(7); }                                         // 7: met, but not before the light
  });
}

// the hit record (main.js:440-445): p = o + r t, n = (p - g) * (1 / |p - g|) with normal3D's guard (quirk q7)
RT_LIT void lit_hit_point(double ox, double oy, double oz, double rx, double ry, double rz, double t, double gx, double gy, double gz, double p[3],
                          double n[3]) {
  p[0] = ox + rx * t; p[1] = oy + ry * t; p[2] = oz + rz * t;
  n[0] = p[0] - gx; n[1] = p[1] - gy; n[2] = p[2] - gz;
  (void)lit_unit(&n[0], &n[1], &n[2]);
}
// hit.u, hit.v (main.js:446-447): two successive divisions each (quirk q6), fdlibm's atan2 / asin
RT_LIT void lit_hit_uv(const double n[3], double *u, double *v) {
  *u = fd_atan2(-n[2], -n[0]) / M_PI / 2 + 0.5;
  *v = fd_asin(-n[1]) / (M_PI / 2) / 2 + 0.5;
}

// x - x is 0 for every finite x and NaN otherwise: whether all six words of a ray record {org[3], dir[3]} are finite
RT_LIT bool lit_finite6(double a, double b, double c, double d, double e, double f) {
  return (a - a) + (b - b) + (c - c) + (d - d) + (e - e) + (f - f) == 0.0;
}

// record j of a 16-byte aligned ray list: three 16-byte loads.  A ray that is not finite is not traced.
struct lit_ray { double ox, oy, oz, rx, ry, rz; bool finite; };
RT_LIT lit_ray lit_load_ray(const double *rays, uint32_t j) {
  typedef double d2 __attribute__((vector_size(16)));
  const d2 *q = (const d2 *)(rays + 6u * (size_t)j);
  const d2 a = q[0], b = q[1], c = q[2];
  lit_ray R;
  R.ox = a[0]; R.oy = a[1]; R.oz = b[0]; R.rx = b[1]; R.ry = c[0]; R.rz = c[1];
  R.finite = lit_finite6(a[0], a[1], b[0], b[1], c[0], c[1]);
  return R;
}

// the head of a list kernel: work-item `item` of n takes ray *j = order[item] (order NULL: the list's own order) - record j in, results
// at j out -> false for a work-item past the list and for an entry that names no ray, which is skipped
RT_LIT bool lit_ordered(const uint32_t *order, uint32_t item, uint32_t n, uint32_t *j) {
  if (item >= n) return false;
  *j = order ? order[item] : item;
  return *j < n;
}

#if defined(__HIPCC__)
// the exclusive prefix of v over the workgroup's WG work-items (tmp: WG words of LDS); *total = the sum
template <uint32_t WG>
__device__ __forceinline__ uint32_t workgroup_exclusive(uint32_t v, volatile uint32_t *tmp, uint32_t *total) {
  const uint32_t t = threadIdx.x;
  __syncthreads();                                              // (tmp may still be read from the previous use)
  tmp[t] = v;
  __syncthreads();
  for (uint32_t off = 1u; off < WG; off <<= 1) {
    const uint32_t below = t >= off ? tmp[t - off] : 0u;
    __syncthreads();
    tmp[t] += below;
    __syncthreads();
  }
  *total = tmp[WG - 1u];
  return tmp[t] - v;
}
#endif

#endif
