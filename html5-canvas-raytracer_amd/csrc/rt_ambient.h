// rt_ambient.h - ambient occlusion (include/rt_hip.h: rt_ambient): the segment that sample s of receiver i scans, built from the
// receiver's hit record.  One source for the host probe (rt_ambient_segments), the generator kernel and the fused kernel
// (rt_ambient.hip).  Literal like rt_view_samples.h: for units compiled WITHOUT FMA contraction, + - * / and sqrt only (and the sign
// copy of the frame), so the device's segments carry the host's bits.  Nothing of HIP is included: tests/host/ambient_check.cpp
// compiles this with a plain host compiler.  The operation order of every expression below is part of the contract
// (include/rt_hip.h states it; tests/ambient_util.py restates it).
#ifndef RT_AMBIENT_H
#define RT_AMBIENT_H

#include "rt_literal.h"       // RT_LIT, lit_unit (the reference's normal3D), lit_finite6
#include "../../include/rt_hip.h"

#define RT_AMBIENT_WG 256u              // receivers per workgroup
#define RT_AMBIENT_MAX_SAMPLES 1024u
#define RT_AMBIENT_MAX_DIRS 65536u

// what a receiver's hit record gives every one of its samples: the origin, the facing normal with its frame, the sphere left out
struct amb_receiver {
  double p[3], l[3], t[3], bt[3];
  int32_t skip;                 // H.object, or -1: not scanned
  bool scanned;
};

// the frame around the unit vector l (Duff et al. 2017, "Building an Orthonormal Basis, Revisited"): no branch, no square root
RT_LIT void amb_frame(const double l[3], double t[3], double bt[3]) {
  const double sg = __builtin_copysign(1.0, l[2]);
  const double a = -1.0 / (sg + l[2]);
  const double b = (l[0] * l[1]) * a;
  t[0] = 1.0 + (sg * (l[0] * l[0])) * a; t[1] = sg * b; t[2] = -sg * l[0];
  bt[0] = b; bt[1] = sg + (l[1] * l[1]) * a; bt[2] = -l[1];
}

// A miss (object < 0) and a record with a non-finite word in point or normal are not scanned.  l = hit.l of main.js:445.
RT_LIT amb_receiver amb_receiver_of(int32_t object, int32_t inside, double p0, double p1, double p2, double n0, double n1, double n2) {
  amb_receiver R;
  R.scanned = object >= 0 && lit_finite6(p0, p1, p2, n0, n1, n2);
  R.skip = R.scanned ? object : -1;
  R.p[0] = p0; R.p[1] = p1; R.p[2] = p2;
  R.l[0] = inside ? -n0 : n0; R.l[1] = inside ? -n1 : n1; R.l[2] = inside ? -n2 : n2;
  amb_frame(R.l, R.t, R.bt);
  return R;
}

// the table entry of sample s of receiver i: 64-bit unsigned arithmetic, wrapping at 2^64 before the reduction
RT_LIT uint32_t amb_entry(uint64_t base, uint64_t i, uint32_t stride, uint32_t s, uint32_t n_dirs) {
  return (uint32_t)(((base + i) * (uint64_t)stride + (uint64_t)s) % (uint64_t)n_dirs);
}

// ... for every sample of one receiver with ONE 64-bit reduction: P = (base + i) * stride and r0 = P % n_dirs once, then, unless
// P + s wraps (the exact expression again), r0 + s with one conditional subtraction - s < n_samples <= n_dirs, so r0 + s < 2 n_dirs
struct amb_walk { uint64_t P; uint32_t r0; };
RT_LIT amb_walk amb_walk_of(uint64_t base, uint64_t i, uint32_t stride, uint32_t n_dirs) {
  amb_walk W;
  W.P = (base + i) * (uint64_t)stride;
  W.r0 = (uint32_t)(W.P % (uint64_t)n_dirs);
  return W;
}
RT_LIT uint32_t amb_walk_entry(const amb_walk &W, uint32_t s, uint32_t n_dirs) {
  if (W.P + (uint64_t)s < W.P) return (uint32_t)((W.P + (uint64_t)s) % (uint64_t)n_dirs);
  const uint32_t e = W.r0 + s;
  return e >= n_dirs ? e - n_dirs : e;
}

// the world direction of the local direction d (z along l), through the reference's normal3D
RT_LIT void amb_dir(const amb_receiver &R, double d0, double d1, double d2, double dir[3]) {
  for (int c = 0; c < 3; c++) dir[c] = (R.t[c] * d0 + R.bt[c] * d1) + R.l[c] * d2;
  (void)lit_unit(&dir[0], &dir[1], &dir[2]);
}

// the segment {org[3], dir[3]} of a receiver for the local direction d; six NaNs for a receiver that is not scanned
RT_LIT void amb_segment(const amb_receiver &R, double d0, double d1, double d2, double out[6]) {
  if (!R.scanned) { for (int c = 0; c < 6; c++) out[c] = __builtin_nan(""); return; }
  double dir[3];
  amb_dir(R, d0, d1, d2, dir);
  out[0] = R.p[0]; out[1] = R.p[1]; out[2] = R.p[2]; out[3] = dir[0]; out[4] = dir[1]; out[5] = dir[2];
}

// rt_ambient.hip.  Passed by value in the kernel arguments: everything here is wave-uniform.
struct rt_ambient_launch {
  const rt_sphere *objects;        // the scene's current sphere table, in blob order (the fused kernel only)
  const rt_hit *hits;              // n receivers (8-byte aligned)
  const uint32_t *order;           // n entries, work-item j takes receiver order[j]; or NULL
  const double *dirs;              // n_dirs local directions, 3 doubles each
  double *open, *intensity;        // the fused kernel's outputs, any of them NULL
  uint32_t *rgba;
  double *rays;                    // the generator's outputs: the segments of `sample` (16-byte aligned) and their skips (or NULL)
  int32_t *skip;
  uint64_t base;
  double radius, epsilon;
  uint32_t n_objects, n;
  uint32_t n_samples, n_dirs, stride, sample;
};

// Every launch is asynchronous on `hip_stream` (a hipStream_t) and returns a hipError_t as int.
extern "C" int rt_launch_ambient_segments(const rt_ambient_launch *L, void *hip_stream);
extern "C" int rt_launch_ambient(const rt_ambient_launch *L, void *hip_stream);
// the generator on the host: the restatement (L->hits, L->dirs, L->rays, L->skip in HOST memory; no order)
extern "C" void rt_ambient_segments_host(const rt_ambient_launch *L);
// the cosine-weighted spiral of include/rt_hip.h (rt_ambient_cosine_dirs), with rt_fdlibm.h's sine and cosine
extern "C" void rt_ambient_cosine_dirs_host(uint32_t n, double *out);

#endif
