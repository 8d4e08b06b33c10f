// rt_view_samples.h - one SAMPLE of a view (include/rt_hip.h: rt_view_sample, rt_view_lens): the ray of pixel (x, y) moved by a sub-pixel
// offset (dx, dy) and, for a PINHOLE with a thin lens, leaving the lens point (lu, lv) towards the pixel's point on the plane of focus.
// One source for the host probe (rt_view_sample_rays) and the generator kernel (rt_view_samples.hip: rt_view_sample_rays_kernel).
// Literal like rt_views.h: for units compiled WITHOUT FMA contraction, + - * / and sqrt only, so the device's rays carry the host's
// bits.  Nothing of HIP is included: tests/host/view_samples_check.cpp compiles this with a plain host compiler.
// The operation order of every expression below is part of the contract (include/rt_hip.h states it; tests/view_samples_util.py
// restates it).  rt_view_ray_of is not used: with dx == dy == 0 and no lens the expressions below are its own, bit for bit - X and Y are
// never -0, so adding 0.0 changes nothing.
#ifndef RT_VIEW_SAMPLES_H
#define RT_VIEW_SAMPLES_H

#include "rt_views.h"         // rt_view_params, the models, RT_VIEWS_WG / RT_VIEWS_MAX_ROWS, rt_view_lon / rt_view_lat
#include "rt_literal.h"       // RT_LIT, lit_unit (the reference's normal3D)

#define RT_VIEW_SAMPLES_MAX 1024u   // samples of one sampled trace

// a sample and the lens, as the generator takes them (by value: 48 bytes of the kernel's arguments); radius == 0: no lens
struct rt_view_sample_params {
  double dx, dy;                   // the sub-pixel offset in pixels, dy downwards like y (EQUIRECT: lives in the tables, not read)
  double lu, lv;                   // the lens point on the unit disk (read with radius > 0 only)
  double radius, focus;            // PINHOLE: the lens' radius along ax / ay, the distance of the plane of focus along az
};

// the angles of the panorama's tables for a sample: rt_view_lon / rt_view_lat with the offset added to (double)x + 0.5
static inline double rt_view_sample_lon(uint32_t x, uint32_t w, double dx) { return 2.0 * M_PI * (((double)x + 0.5) + dx) / (double)w - M_PI; }
static inline double rt_view_sample_lat(uint32_t y, uint32_t h, double dy) { return M_PI / 2.0 - M_PI * (((double)y + 0.5) + dy) / (double)h; }

// The sample's ray of pixel (x, y): out = {org[3], dir[3]}.  {sl, cl} and {sa, ca} are the column's and the row's entries of the SAMPLE's
// tables (EQUIRECT; any value otherwise): the caller keeps its own loads, as with rt_view_ray_of.
RT_LIT void rt_view_sample_ray_of(const rt_view_params &P, const rt_view_sample_params &S, uint32_t x, uint32_t y, double sl, double cl, double sa,
                                  double ca, double out[6]) {
  const double X = (((double)x - P.proj_w) + 0.5) + S.dx, Y = ((P.proj_h - (double)y) - 0.5) - S.dy;
  double org[3] = {P.o[0], P.o[1], P.o[2]}, dir[3];
  if (P.model == RT_VIEWS_REFERENCE) {
    const double d[3] = {X, Y, P.proj_d};
    for (int c = 0; c < 3; c++) {
      const double target = ((P.o[c] + P.ax[c] * d[c]) + P.ay[c] * d[c]) + P.az[c] * d[c];
      dir[c] = target - P.o[c];
    }
  } else if (P.model == RT_VIEWS_PINHOLE) {
    for (int c = 0; c < 3; c++) dir[c] = (P.ax[c] * X + P.ay[c] * Y) + P.az[c] * P.proj_d;
    if (S.radius > 0.0) {
      // every sample of a pixel passes through o + raw * f, on the plane `focus` away along az (orthonormal axes)
      const double f = S.focus / P.proj_d, lx = S.lu * S.radius, ly = S.lv * S.radius;
      for (int c = 0; c < 3; c++) {
        const double off = P.ax[c] * lx + P.ay[c] * ly;
        org[c] = P.o[c] + off;
        dir[c] = dir[c] * f - off;
      }
    }
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

// ... with the table entries read from P.lon / P.lat (the SAMPLE's tables) where the model has them
RT_LIT void rt_view_sample_ray(const rt_view_params &P, const rt_view_sample_params &S, uint32_t x, uint32_t y, double out[6]) {
  const bool tables = P.model == RT_VIEWS_EQUIRECT;
  const double sl = tables ? P.lon[2u * (size_t)x] : 0.0, cl = tables ? P.lon[2u * (size_t)x + 1u] : 0.0;
  const double sa = tables ? P.lat[2u * (size_t)y] : 0.0, ca = tables ? P.lat[2u * (size_t)y + 1u] : 0.0;
  rt_view_sample_ray_of(P, S, x, y, sl, cl, sa, ca, out);
}

// rt_view_samples.hip.  Every launch is asynchronous on `hip_stream` (a hipStream_t) and returns a hipError_t as int.
// rows [first_row, first_row + rows) of the sample's rays into d_rays (16-byte aligned, rows * w records), in launches of at most
// RT_VIEWS_MAX_ROWS rows; P->lon / P->lat are the sample's own tables.  And the same rows on the host: the restatement.
extern "C" int rt_launch_view_sample_rays(const rt_view_params *P, const rt_view_sample_params *S, uint32_t first_row, uint32_t rows, double *d_rays,
                                          void *hip_stream);
extern "C" void rt_view_sample_rays_host(const rt_view_params *P, const rt_view_sample_params *S, uint32_t first_row, uint32_t rows, double *out);
// acc[j] = acc[j] + rgb[j] for the 3 * pixels doubles of a band (both 8-byte aligned; pixels >= 1)
extern "C" int rt_launch_view_accumulate(double *d_acc, const double *d_rgb, uint32_t pixels, void *hip_stream);
// per pixel and channel mean = (acc + last) / n (d_last NULL: acc / n), into d_rgb (3 doubles per pixel, or NULL) and d_rgba (the store
// rule of main.js:195-198 with alpha 255, or NULL)
extern "C" int rt_launch_view_resolve(const double *d_acc, const double *d_last, uint32_t n, uint32_t pixels, double *d_rgb, uint8_t *d_rgba,
                                      void *hip_stream);

#endif
