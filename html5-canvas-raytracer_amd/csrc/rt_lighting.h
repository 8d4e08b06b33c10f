// rt_lighting.h - sampled lights (include/rt_hip.h: rt_lighting): the segment that sample s of receiver i scans towards light k, built
// from the receiver's hit record, and the step of the reference's light loop (main.js:283-306) that follows its scan.  One source for
// the host probe (rt_lighting_segments) and the fused kernel (rt_lighting.hip).  Literal like rt_ambient.h: for units compiled
// WITHOUT FMA contraction, + - * / and sqrt only, so the device's segments carry the host's bits.  Nothing of HIP is included:
// tests/host/lighting_check.cpp compiles this with a plain host compiler.  The operation order of every expression below is part of
// the contract (include/rt_hip.h states it; tests/lighting_util.py restates it).
#ifndef RT_LIGHTING_H
#define RT_LIGHTING_H

#include "rt_ambient.h"       // amb_entry, amb_walk: the table entry of a sample; rt_literal.h; include/rt_hip.h

#define RT_LIGHTING_WG 256u              // receivers per workgroup
#define RT_LIGHTING_MAX_SAMPLES 1024u
#define RT_LIGHTING_MAX_OFFS 65536u

// what a receiver's hit record gives every one of its segments: amb_receiver without its frame, which no light reads
struct lgt_receiver {
  double p[3], l[3];
  int32_t skip;                 // H.object, or -1: not scanned
  bool scanned;
};

// A miss (object < 0) and a record with a non-finite word in point or normal are not scanned.  l = hit.l of main.js:445.
RT_LIT lgt_receiver lgt_receiver_of(int32_t object, int32_t inside, double p0, double p1, double p2, double n0, double n1, double n2) {
  lgt_receiver R;
  R.scanned = object >= 0 && lit_finite6(p0, p1, p2, n0, n1, n2);
  R.skip = R.scanned ? object : -1;
  R.p[0] = p0; R.p[1] = p1; R.p[2] = p2;
  R.l[0] = inside ? -n0 : n0; R.l[1] = inside ? -n1 : n1; R.l[2] = inside ? -n2 : n2;
  return R;
}

// where light `light` stands in a sample whose table entry is o: the light itself at radius 0 (the table is not read: o may be NULL)
RT_LIT void lgt_light_pos(const double light[3], double light_radius, const double *o, double pos[3]) {
  if (light_radius == 0.0) { pos[0] = light[0]; pos[1] = light[1]; pos[2] = light[2]; return; }
  for (int c = 0; c < 3; c++) pos[c] = light[c] + light_radius * o[c];
}

// main.js:287-291: shadow_vec, light_mag, light_len, shadow_dot of the point p facing l and a light at pos
struct lgt_segment { double sv[3], mag, len, sd; };
RT_LIT lgt_segment lgt_segment_of(const double p[3], const double l[3], const double pos[3]) {
  lgt_segment S;
  S.sv[0] = pos[0] - p[0]; S.sv[1] = pos[1] - p[1]; S.sv[2] = pos[2] - p[2];
  S.mag = (S.sv[0] * S.sv[0] + S.sv[1] * S.sv[1]) + S.sv[2] * S.sv[2];
  S.len = sqrt(S.mag);
  if (S.len != 0.0) { const double k = 1.0 / S.len; S.sv[0] = S.sv[0] * k; S.sv[1] = S.sv[1] * k; S.sv[2] = S.sv[2] * k; }
  S.sd = (S.sv[0] * l[0] + S.sv[1] * l[1]) + S.sv[2] * l[2];
  return S;
}

// main.js:292: the surface faces the light - `if (shadow_dot <= 0) continue`, so a NaN shadow_dot goes on
RT_LIT bool lgt_faces(const lgt_segment &S) { return !(S.sd <= 0.0); }

// rt_scene_occlusion_device's rule for the segment {p, sv}: a non-finite word and it is not scanned (p is finite: the receiver is scanned)
RT_LIT bool lgt_traced(const lgt_segment &S) { return lit_finite6(S.sv[0], S.sv[1], S.sv[2], 0.0, 0.0, 0.0); }

// main.js:305-306 behind the scan that left li: what the light adds to the sample's diffuse sum, and whether it counts as lit
RT_LIT void lgt_contribute(const lgt_segment &S, double li, double *diffuse, uint32_t *contributed) {
  if (li == 0.0) return;
  *diffuse = *diffuse + (li * S.sd) / S.mag;
  *contributed += 1u;
}

// rt_lighting.hip.  Passed by value in the kernel arguments: everything here is wave-uniform.
struct rt_lighting_launch {
  const rt_sphere *objects;        // the scene's current sphere table, in blob order
  const rt_hit *hits;              // n receivers (8-byte aligned)
  const uint32_t *order;           // n entries, work-item j takes receiver order[j]; or NULL
  const double *offs;              // n_offs offsets, 3 doubles each (not read at light_radius 0)
  double *diffuse, *intensity, *lit;   // the outputs, any of them NULL
  uint32_t *rgba;
  uint64_t base;
  double light_radius, epsilon, light_intensity;
  uint32_t n_objects, n;
  uint32_t n_samples, n_offs, stride, n_lights;
  double lights[RT_MAX_LIGHTS][3]; // the scene's current lights, by value as every launch carries them
};

// Asynchronous on `hip_stream` (a hipStream_t); returns a hipError_t as int.
extern "C" int rt_launch_lighting(const rt_lighting_launch *L, void *hip_stream);
// the probe: the segments of (sample, light) on the host (L->hits, L->offs in HOST memory; no order; any output but rays may be NULL)
extern "C" void rt_lighting_segments_host(const rt_lighting_launch *L, uint32_t sample, uint32_t light, double *rays, double *length, double *mag,
                                          double *dot, int32_t *skip);
// the spiral of include/rt_hip.h (rt_lighting_sphere_offsets), with rt_fdlibm.h's sine and cosine
extern "C" void rt_lighting_sphere_offsets_host(uint32_t n, double *out);

#endif
