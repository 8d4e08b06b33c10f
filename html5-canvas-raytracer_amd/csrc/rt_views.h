// rt_views.h - the camera models of a view (include/rt_hip.h: rt_view): the primary ray of pixel (x, y) of a w x h view, one source for
// the host probe (rt_view_rays) and the generator kernel (rt_views.hip: rt_view_rays_kernel).  Like rt_literal.h it is literal: for
// units compiled WITHOUT FMA contraction (-ffp-contract=off), where + - * / and sqrt are correctly rounded on both sides, so the
// device's rays carry the host's bits - no tolerance.  No transcendental function runs here: the panorama's sines and cosines are
// separable (w longitudes, h latitudes) and come in as tables; the perspective models' tan() is taken once per view on the host
// (rt_view_proj_d).  Nothing of HIP is included: tests/host/views_check.cpp compiles this with a plain host compiler.
// The operation order of every expression below is part of the contract (include/rt_hip.h states it; tests/views_util.py restates it).
#ifndef RT_VIEWS_H
#define RT_VIEWS_H

#include <math.h>
#include <stdint.h>

#include "rt_literal.h"       // RT_LIT, lit_unit (the reference's normal3D)

#define RT_VIEWS_WG 256u          // work-items per workgroup of the generator: one ray each
#define RT_VIEWS_MAX_ROWS 65535u  // rows of one launch (the grid's y)

// the models (include/rt_hip.h: RT_VIEW_*)
#define RT_VIEWS_REFERENCE 0u
#define RT_VIEWS_PINHOLE 1u
#define RT_VIEWS_ORTHO 2u
#define RT_VIEWS_EQUIRECT 3u

// a view at one frame size, as the generator takes it (by value: the kernel reads it from its kernarg segment)
struct rt_view_params {
  uint32_t model, w, h, reserved;
  double proj_w, proj_h, proj_d;   // w / 2.0, h / 2.0, and (the perspective models) proj_w / tan(fov / 2), main.js:102-105
  double scale;                    // ORTHO: world units per pixel
  double o[3], ax[3], ay[3], az[3];
  const double *lon, *lat;         // EQUIRECT: {sin, cos} per column / per row, 16-byte aligned (host memory for the probe, device memory for the kernel)
};

// main.js:102-105 as rt_api.hip: launch_geometry has it for a frame (host only: tan is the host's)
static inline double rt_view_proj_d(double fov_deg, double proj_w) {
  const double projA = fov_deg * M_PI / 180.0;
  return proj_w / tan(projA / 2.0);
}

// the angles of the panorama's tables (tools/panorama.py's expressions, in its order): column x's longitude, row y's latitude
static inline double rt_view_lon(uint32_t x, uint32_t w) { return 2.0 * M_PI * ((double)x + 0.5) / (double)w - M_PI; }
static inline double rt_view_lat(uint32_t y, uint32_t h) { return M_PI / 2.0 - M_PI * ((double)y + 0.5) / (double)h; }

// The ray of pixel (x, y): out = {org[3], dir[3]}.  {sl, cl} and {sa, ca} are the column's and the row's table entries (EQUIRECT; any
// value otherwise): the caller keeps its own loads, as with rt_literal.h - the kernel's are a scalar pair and one 16-byte vector load.
RT_LIT void rt_view_ray_of(const rt_view_params &P, uint32_t x, uint32_t y, double sl, double cl, double sa, double ca, double out[6]) {
  const double X = ((double)x - P.proj_w) + 0.5, Y = (P.proj_h - (double)y) - 0.5;       // main.js:186
  double org[3] = {P.o[0], P.o[1], P.o[2]}, dir[3];
  if (P.model == RT_VIEWS_REFERENCE) {
    // main.js:186-193: dist is indexed by COMPONENT (quirk q1), the additions in the reference's order, between3D
    const double d[3] = {X, Y, P.proj_d};
    for (int c = 0; c < 3; c++) {
      const double target = ((P.o[c] + P.ax[c] * d[c]) + P.ay[c] * d[c]) + P.az[c] * d[c];
      dir[c] = target - P.o[c];
    }
  } else if (P.model == RT_VIEWS_PINHOLE) {
    for (int c = 0; c < 3; c++) dir[c] = (P.ax[c] * X + P.ay[c] * Y) + P.az[c] * P.proj_d;
  } else if (P.model == RT_VIEWS_ORTHO) {
    const double sx = X * P.scale, sy = Y * P.scale;
    for (int c = 0; c < 3; c++) { org[c] = (P.o[c] + P.ax[c] * sx) + P.ay[c] * sy; dir[c] = P.az[c]; }
  } else {
    const double l0 = ca * sl, l1 = sa, l2 = ca * cl;
    for (int c = 0; c < 3; c++) dir[c] = (P.ax[c] * l0 + P.ay[c] * l1) + P.az[c] * l2;
  }
  (void)lit_unit(&dir[0], &dir[1], &dir[2]);
  out[0] = org[0]; out[1] = org[1]; out[2] = org[2]; out[3] = dir[0]; out[4] = dir[1]; out[5] = dir[2];
}

// ... with the table entries read from P.lon / P.lat where the model has them
RT_LIT void rt_view_ray(const rt_view_params &P, uint32_t x, uint32_t y, double out[6]) {
  const bool tables = P.model == RT_VIEWS_EQUIRECT;
  const double sl = tables ? P.lon[2u * (size_t)x] : 0.0, cl = tables ? P.lon[2u * (size_t)x + 1u] : 0.0;
  const double sa = tables ? P.lat[2u * (size_t)y] : 0.0, ca = tables ? P.lat[2u * (size_t)y + 1u] : 0.0;
  rt_view_ray_of(P, x, y, sl, cl, sa, ca, out);
}

// rt_views.hip: rows [first_row, first_row + rows) of the view into d_rays (16-byte aligned, rows * w records), asynchronous on
// `hip_stream` (a hipStream_t), in launches of at most RT_VIEWS_MAX_ROWS rows -> a hipError_t as int; and the same rows on the host
// (the restatement the device is held to: compiled without FMA contraction, like the kernel)
extern "C" int rt_launch_view_rays(const rt_view_params *P, uint32_t first_row, uint32_t rows, double *d_rays, void *hip_stream);
extern "C" void rt_view_rays_host(const rt_view_params *P, uint32_t first_row, uint32_t rows, double *out);

#endif
