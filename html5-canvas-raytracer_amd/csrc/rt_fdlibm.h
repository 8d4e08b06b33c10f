// rt_fdlibm.h - fdlibm's atan2 / asin (Sun's published algorithms, as the JavaScript engines' Math.atan2 / Math.asin), restated
// operation for operation for device code compiled WITHOUT FMA contraction (-ffp-contract=off; `/` and sqrt correctly rounded).
// Shared by the strict trace kernels (rt_kernel.hip, RT_STRICT) and the primary-hit kernels (rt_hits.hip).  Same code as
// oracle/fdlibm_trig.h, which the CPU tests compare with Node's Math.atan2 / Math.asin bit for bit on 0.9 M vectors.
#ifndef RT_FDLIBM_H
#define RT_FDLIBM_H

#include <math.h>
#include <stdint.h>

// (device code of the kernels, and - through rt_block.h - the launch table's host and device builds: the same operations, the same bits)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FD_FN __host__ __device__ __forceinline__
#else
#define FD_FN static inline
#endif

FD_FN uint32_t fd_hi(double x) { return (uint32_t)(__builtin_bit_cast(unsigned long long, x) >> 32); }
FD_FN uint32_t fd_lo(double x) { return (uint32_t)__builtin_bit_cast(unsigned long long, x); }
FD_FN double fd_atan(double x) {
  const double hi0 = 4.63647609000806093515e-01, hi1 = 7.85398163397448278999e-01, hi2 = 9.82793723247329054082e-01, hi3 = 1.57079632679489655800e+00;
  const double lo0 = 2.26987774529616870924e-17, lo1 = 3.06161699786838301793e-17, lo2 = 1.39033110312309984516e-17, lo3 = 6.12323399573676603587e-17;
  const double a0 = 3.33333333333329318027e-01, a1 = -1.99999999998764832476e-01, a2 = 1.42857142725034663711e-01, a3 = -1.11111104054623557880e-01,
               a4 = 9.09088713343650656196e-02, a5 = -7.69187620504482999495e-02, a6 = 6.66107313738753120669e-02, a7 = -5.83357013379057348645e-02,
               a8 = 4.97687799461593236017e-02, a9 = -3.65315727442169155270e-02, a10 = 1.62858201153657823623e-02;
  const int32_t hx = (int32_t)fd_hi(x);
  const uint32_t ix = (uint32_t)hx & 0x7fffffffu;
  int id;
  if (ix >= 0x44100000u) {                                            // |x| >= 2^66
    if (ix > 0x7ff00000u || (ix == 0x7ff00000u && fd_lo(x) != 0u)) return x + x;
    return hx > 0 ? hi3 + lo3 : -hi3 - lo3;
  }
  if (ix < 0x3fdc0000u) { if (ix < 0x3e200000u) return x; id = -1; }   // |x| < 0.4375 (< 2^-29: x)
  else {
    x = __builtin_fabs(x);
    if (ix < 0x3ff30000u) { if (ix < 0x3fe60000u) { id = 0; x = (2.0 * x - 1.0) / (2.0 + x); } else { id = 1; x = (x - 1.0) / (x + 1.0); } }
    else { if (ix < 0x40038000u) { id = 2; x = (x - 1.5) / (1.0 + 1.5 * x); } else { id = 3; x = -1.0 / x; } }
  }
  const double z = x * x, w = z * z;
  const double s1 = z * (a0 + w * (a2 + w * (a4 + w * (a6 + w * (a8 + w * a10)))));
  const double s2 = w * (a1 + w * (a3 + w * (a5 + w * (a7 + w * a9))));
  if (id < 0) return x - x * (s1 + s2);
  const double ahi = id == 0 ? hi0 : (id == 1 ? hi1 : (id == 2 ? hi2 : hi3)), alo = id == 0 ? lo0 : (id == 1 ? lo1 : (id == 2 ? lo2 : lo3));
  const double r = ahi - ((x * (s1 + s2) - alo) - x);
  return hx < 0 ? -r : r;
}
FD_FN double fd_atan2(double y, double x) {
  const double tiny = 1.0e-300, pi_o_4 = 7.8539816339744827900E-01, pi_o_2 = 1.5707963267948965580E+00, pi = 3.1415926535897931160E+00, pi_lo = 1.2246467991473531772E-16;
  const int32_t hx = (int32_t)fd_hi(x), hy = (int32_t)fd_hi(y);
  const uint32_t lx = fd_lo(x), ly = fd_lo(y), ix = (uint32_t)hx & 0x7fffffffu, iy = (uint32_t)hy & 0x7fffffffu;
  if ((ix | ((lx | (0u - lx)) >> 31)) > 0x7ff00000u || (iy | ((ly | (0u - ly)) >> 31)) > 0x7ff00000u) return x + y;     // NaN
  if ((((uint32_t)hx - 0x3ff00000u) | lx) == 0u) return fd_atan(y);                                                    // x == 1
  int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);                                                                          // 2 * sign(x) + sign(y)
  if ((iy | ly) == 0u) { if (m < 2) return y; return m == 2 ? pi + tiny : -pi - tiny; }                                   // y == 0
  if ((ix | lx) == 0u) return (hy < 0) ? -pi_o_2 - tiny : pi_o_2 + tiny;                                                 // x == 0
  if (ix == 0x7ff00000u) {
    if (iy == 0x7ff00000u) return m == 0 ? pi_o_4 + tiny : (m == 1 ? -pi_o_4 - tiny : (m == 2 ? 3.0 * pi_o_4 + tiny : -3.0 * pi_o_4 - tiny));
    return m == 0 ? 0.0 : (m == 1 ? -0.0 : (m == 2 ? pi + tiny : -pi - tiny));
  }
  if (iy == 0x7ff00000u) return (hy < 0) ? -pi_o_2 - tiny : pi_o_2 + tiny;
  const int32_t k = (int32_t)(iy - ix) >> 20;
  double z;
  if (k > 60) { z = pi_o_2 + 0.5 * pi_lo; m &= 1; }                                                                      // |y / x| > 2^60
  else if (hx < 0 && k < -60) z = 0.0;                                                                                  // 0 > |y| / x > -2^-60
  else z = fd_atan(__builtin_fabs(y / x));
  return m == 0 ? z : (m == 1 ? -z : (m == 2 ? pi - (z - pi_lo) : (z - pi_lo) - pi));
}
FD_FN double fd_asin(double x) {
  const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, pio4_hi = 7.85398163397448278999e-01;
  const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01, pS3 = -4.00555345006794114027e-02,
               pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05;
  const double qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01, qS4 = 7.70381505559019352791e-02;
  const int32_t hx = (int32_t)fd_hi(x);
  const uint32_t ix = (uint32_t)hx & 0x7fffffffu;
  if (ix >= 0x3ff00000u) {                                            // |x| >= 1
    if (((ix - 0x3ff00000u) | fd_lo(x)) == 0u) return x * pio2_hi + x * pio2_lo;
    return (x - x) / (x - x);                                         // NaN
  }
  if (ix < 0x3fe00000u) {                                             // |x| < 0.5
    if (ix < 0x3e400000u) return x;
    const double t = x * x;
    const double p = t * (pS0 + t * (pS1 + t * (pS2 + t * (pS3 + t * (pS4 + t * pS5)))));
    const double q = 1.0 + t * (qS1 + t * (qS2 + t * (qS3 + t * qS4)));
    return x + x * (p / q);
  }
  const double w0 = 1.0 - __builtin_fabs(x);
  double t = w0 * 0.5;
  const double p = t * (pS0 + t * (pS1 + t * (pS2 + t * (pS3 + t * (pS4 + t * pS5)))));
  const double q = 1.0 + t * (qS1 + t * (qS2 + t * (qS3 + t * qS4)));
  const double s = sqrt(t);
  if (ix >= 0x3FEF3333u) { const double w = p / q; t = pio2_hi - (2.0 * (s + s * w) - pio2_lo); }                       // |x| > 0.975
  else {
    const double w = __builtin_bit_cast(double, __builtin_bit_cast(unsigned long long, s) & 0xffffffff00000000ull);
    const double c = (t - w * w) / (s + w), r = p / q;
    const double p2 = 2.0 * s * r - (pio2_lo - 2.0 * c), q2 = pio4_hi - 2.0 * w;
    t = pio4_hi - (p2 - q2);
  }
  return hx > 0 ? t : -t;
}

// fdlibm's sin / cos for HOST-built tables (rt_ambient_cosine_dirs): k_sin.c and k_cos.c (FreeBSD msun's form of the latter) behind
// the two- and three-term Cody-Waite reduction of e_rem_pio2.c's medium range, |x| < 2^19 * (pi / 2); beyond it, and for a non-finite x,
// NaN - no caller here comes near.  No kernel calls these: the device runs no transcendental function.
FD_FN double fd_k_sin(double x, double y) {
  const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
               S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  if ((fd_hi(x) & 0x7fffffffu) < 0x3e400000u) return x;                 // |x| < 2^-27
  const double z = x * x, v = z * x, r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
  return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
FD_FN double fd_k_cos(double x, double y) {
  const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
               C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  if ((fd_hi(x) & 0x7fffffffu) < 0x3e400000u) return 1.0;
  const double z = x * x, w = z * z, r = z * (C1 + z * (C2 + z * C3)) + (w * w) * (C4 + z * (C5 + z * C6));
  const double hz = 0.5 * z, t = 1.0 - hz;
  return t + (((1.0 - t) - hz) + (z * r - x * y));
}
// x = n * (pi / 2) + (y0 + y1), |y0 + y1| <= pi / 4 -> n & 3; -1 outside the medium range
FD_FN int fd_rem_pio2(double x, double *y0, double *y1) {
  const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00, pio2_1t = 6.07710050650619224932e-11,
               pio2_2 = 6.07710050630396597660e-11, pio2_2t = 2.02226624879595063154e-21, pio2_3 = 2.02226624871116645580e-21,
               pio2_3t = 8.47842766036889956997e-32;
  const uint32_t ix = fd_hi(x) & 0x7fffffffu;
  if (ix <= 0x3fe921fbu) { *y0 = x; *y1 = 0.0; return 0; }              // |x| <= pi / 4
  if (ix >= 0x413921fbu) return -1;                                     // |x| >= 2^19 * (pi / 2), Inf, NaN
  const double t0 = x < 0.0 ? -x : x;
  const int n = (int)(t0 * invpio2 + 0.5);
  const double fn = (double)n;
  double r = t0 - fn * pio2_1, w = fn * pio2_1t, a = r - w;
  const int j = (int)(ix >> 20);
  if (j - (int)((fd_hi(a) >> 20) & 0x7ffu) > 16) {                      // the second term: good to 118 bits
    double t = r;
    w = fn * pio2_2; r = t - w; w = fn * pio2_2t - ((t - r) - w); a = r - w;
    if (j - (int)((fd_hi(a) >> 20) & 0x7ffu) > 49) {                    // the third: 151 bits, covers every case
      t = r;
      w = fn * pio2_3; r = t - w; w = fn * pio2_3t - ((t - r) - w); a = r - w;
    }
  }
  const double b = (r - a) - w;
  if (x < 0.0) { *y0 = -a; *y1 = -b; return (-n) & 3; }
  *y0 = a; *y1 = b;
  return n & 3;
}
FD_FN double fd_sin(double x) {
  double a, b;
  const int n = fd_rem_pio2(x, &a, &b);
  if (n < 0) return x - x == 0.0 ? __builtin_nan("") : x - x;
  return n == 0 ? fd_k_sin(a, b) : n == 1 ? fd_k_cos(a, b) : n == 2 ? -fd_k_sin(a, b) : -fd_k_cos(a, b);
}
FD_FN double fd_cos(double x) {
  double a, b;
  const int n = fd_rem_pio2(x, &a, &b);
  if (n < 0) return x - x == 0.0 ? __builtin_nan("") : x - x;
  return n == 0 ? fd_k_cos(a, b) : n == 1 ? -fd_k_sin(a, b) : n == 2 ? -fd_k_cos(a, b) : fd_k_sin(a, b);
}

#endif
