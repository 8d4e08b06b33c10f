// Launch record of the relight kernel (rt_relight.hip), shared with its host side (rt_relight_api.hip).  Not part of the ABI.
#ifndef RT_RELIGHT_H
#define RT_RELIGHT_H

#include "rt_lighting.h"      // lgt_light_pos; rt_ambient.h's table walk; rt_literal.h; include/rt_hip.h

#define RT_RELIGHT_WG 256u               // nodes per workgroup

// Passed by value in the kernel arguments: everything here is wave-uniform.
struct rt_relight_launch {
  const rt_sphere *objects;        // the scene's current sphere table, in blob order
  const double *rays;              // n records {org[3], dir[3]} (16-byte aligned): the list the nodes were shaded from
  const uint32_t *order;           // n entries, work-item j takes node order[j]; or NULL
  const uint32_t *pix;             // per node, or NULL = i
  const double *offs;              // n_offs offsets, 3 doubles each (not read at light_radius 0)
  rt_node *nodes;                  // n records (8-byte aligned): bytes 104..119 are written
  uint64_t base;
  double light_radius, epsilon, light_intensity;
  uint32_t n_objects, n;
  uint32_t n_samples, n_offs, stride, n_lights;
  double lights[RT_MAX_LIGHTS][3]; // the scene's current lights, by value as every launch carries them
};

// Asynchronous on `hip_stream` (a hipStream_t); returns a hipError_t as int.
extern "C" int rt_launch_relight(const rt_relight_launch *L, void *hip_stream);

#endif
