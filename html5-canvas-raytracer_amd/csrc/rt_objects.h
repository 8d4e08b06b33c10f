// rt_objects.h — the per-element arithmetic of the sphere tables (shadow grids, bounce table), written once for the host
// (rt_tables.cpp: build_shadow_grid, build_bounce_table - what rt_scene_upload uploads, and the tests' oracle) and for the device
// (rt_objects_gpu.hip: the same tables rebuilt after rt_scene_set_objects).  Plain binary64, IEEE sqrt and division, no contraction
// (both translation units are compiled without it), like rt_block.h: the two builds give the same words.
#ifndef RT_OBJECTS_H
#define RT_OBJECTS_H

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "rt_block.h"
#include "rt_device.h"

// finite (not NaN, not infinite)
RT_HD inline bool rt_finite(double x) { return fabs(x) <= DBL_MAX; }

// A sphere anchored at a point `a` (a light: the object block's [anchored at light k] records): {o - a, |o - a|^2 - r2}, the constant
// term of the ray-sphere quadratic for rays that start at `a`.  fill_object_block (rt_scene.hip) and the light move's kernel
// (rt_objects_gpu.hip: rt_light_anchor) both state it from here.
RT_HD inline rt_geom rt_anchored(const double origin[3], double r2, const double a[3]) {
  const double lx = origin[0] - a[0], ly = origin[1] - a[1], lz = origin[2] - a[2];
  return rt_geom{lx, ly, lz, (lx * lx + ly * ly + lz * lz) - r2};
}

// The root interval of the quadratic of one axis of a cull rectangle (rt_tables.cpp: cull_rect states the geometry); the whole axis
// where the image is unbounded along it or the case is doubtful.
RT_HD inline void rt_axis_bounds(double c_axis, double c_z, double s_axis, double s_z, double r2, double *lo, double *hi) {
  *lo = -INFINITY; *hi = INFINITY;
  const double A = s_axis * s_axis * (c_z * c_z - r2);
  const double B = -2.0 * c_axis * c_z * s_axis * s_z;
  const double Cq = s_z * s_z * (c_axis * c_axis - r2);
  const double disc = B * B - 4.0 * A * Cq;
  if (!(A > 1e-12 * s_axis * s_axis * (c_z * c_z + r2)) || !(disc >= 0.0)) return;   // image unbounded along this axis (or degenerate)
  const double sq = sqrt(disc);
  const double x1 = (-B - sq) / (2.0 * A), x2 = (-B + sq) / (2.0 * A);
  if (!(x1 <= x2) || !rt_finite(x1) || !rt_finite(x2)) return;
  *lo = x1 - 1e-7 * (1.0 + fabs(x1));                 // margins far above rounding, far below a pixel (1/D >= 1.5e-5)
  *hi = x2 + 1e-7 * (1.0 + fabs(x2));
}

// ---- shadow grids: a sphere's rectangle in the light's frame (x'/z', y'/z'); true: wholly behind the light (only the "every
// sphere" cell holds it).  `frame` = the light's header {x'[3], y'[3], z'[3], ...}.
RT_HD inline bool rt_shadow_rect(const double *frame, const double Lp[3], const double origin[3], double r2, rt_geom *q) {
  const double *x = frame, *y = frame + 3, *z = frame + 6;
  const double c[3] = {origin[0] - Lp[0], origin[1] - Lp[1], origin[2] - Lp[2]};
  const double cx = x[0] * c[0] + x[1] * c[1] + x[2] * c[2], cy = y[0] * c[0] + y[1] * c[1] + y[2] * c[2], cq = z[0] * c[0] + z[1] * c[1] + z[2] * c[2];
  const double r = sqrt(r2);
  *q = rt_geom{-INFINITY, INFINITY, -INFINITY, INFINITY};
  if (cq + r * (1.0 + 1e-9) + 1e-9 < 0.0) return true;   // wholly behind the light: cannot lie between it and a point in front
  const double kk = (cx * cx + cy * cy + cq * cq) - r2;
  if (kk > 1e-9 * r2 && r2 > 0.0) {
    rt_axis_bounds(cx, cq, 1.0, 1.0, r2, &q->ox, &q->oy);
    rt_axis_bounds(cy, cq, 1.0, 1.0, r2, &q->oz, &q->r2);
  }
  return false;
}

// the kernel's own mapping of a frame coordinate to a grid cell
RT_HD inline uint32_t rt_sgrid_cell(double v, double g0, double inv) {
  const double f = fmin(fmax((v - g0) * inv, 0.0), (double)(RT_SGRID - 1u));
  return (uint32_t)f;
}

// the cells [ix0, ix1] x [iy0, iy1] a rectangle covers, packed ix0 | ix1 << 8 | iy0 << 16 | iy1 << 24 (RT_SGRID <= 256)
RT_HD inline uint32_t rt_sgrid_span(const rt_geom &q, const double *frame) {
  const double gx0 = frame[9], gy0 = frame[10], inv_cw = frame[11], inv_ch = frame[12];
  return rt_sgrid_cell(q.ox, gx0, inv_cw) | rt_sgrid_cell(q.oy, gx0, inv_cw) << 8 | rt_sgrid_cell(q.oz, gy0, inv_ch) << 16 | rt_sgrid_cell(q.r2, gy0, inv_ch) << 24;
}
RT_HD inline bool rt_sgrid_in_span(uint32_t span, uint32_t ix, uint32_t iy) {
  return ix >= (span & 255u) && ix <= ((span >> 8) & 255u) && iy >= ((span >> 16) & 255u) && iy <= (span >> 24);
}

// ---- bounce table: rays leave a sphere only if it reflects or refracts (albedo[3] > 0 or albedo[4] > 0, main.js:233,246)
RT_HD inline bool rt_bounce_row_used(const rt_sphere &o) { return (o.albedo[3] > 0.0) || (o.albedo[4] > 0.0); }

// what a ray leaving sphere i needs to know of loop sphere j (rt_tables.cpp: build_bounce_table states the geometry)
struct rt_bounce_pair { double D0, D1, D2, Ld, sa, ca; uint32_t everywhere; };
RT_HD inline rt_bounce_pair rt_bounce_pair_of(const rt_sphere &oi, double ri, const rt_sphere &oj) {
  rt_bounce_pair p;
  p.D0 = oj.origin[0] - oi.origin[0]; p.D1 = oj.origin[1] - oi.origin[1]; p.D2 = oj.origin[2] - oi.origin[2];
  p.Ld = sqrt(p.D0 * p.D0 + p.D1 * p.D1 + p.D2 * p.D2);
  const double R = (ri + sqrt(oj.r2)) * (1.0 + 1e-9);
  p.everywhere = (!(R < p.Ld * (1.0 - 1e-9)) || !rt_finite(R) || !rt_finite(p.Ld)) ? 1u : 0u;   // overlapping / containing / degenerate: all cells
  p.sa = 0.0; p.ca = 0.0;
  if (!p.everywhere) { p.sa = R / p.Ld; p.ca = sqrt(fmax(0.0, 1.0 - p.sa * p.sa)); }
  return p;
}

// Cell cones: per cell of the cube map its centre direction and the cos / sin of its half-angle, structure of arrays
// [cx | cy | cz | cos | sin] x RT_BCELLS (host-computed once: rt_tables.cpp bounce_cell_cones).
RT_HD inline bool rt_bounce_cell_hit(const rt_bounce_pair &p, const double *cones, uint32_t c) {
  if (p.everywhere) return true;
  const double cx = cones[c], cy = cones[RT_BCELLS + c], cz = cones[2u * RT_BCELLS + c], cc = cones[3u * RT_BCELLS + c], cs = cones[4u * RT_BCELLS + c];
  const double dotp = cx * p.D0 + cy * p.D1 + cz * p.D2;                       // |D| cos(angle)
  // angle(centre, D) <= alpha + half  <=>  cos(angle) >= cos(alpha + half); alpha, half in (0, pi/2), so the sum is < pi
  const double cos_sum = p.ca * cc - p.sa * cs, sin_sum = p.sa * cc + p.ca * cs;
  return (sin_sum <= 0.0) || (dotp >= p.Ld * (cos_sum - 1e-12));
}

#endif
