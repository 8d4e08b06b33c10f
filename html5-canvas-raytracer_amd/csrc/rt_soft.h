// Launch record of the soft trace kernel (rt_soft.hip), shared with its host side (rt_soft_api.hip).  Not part of the ABI.
#ifndef RT_SOFT_H
#define RT_SOFT_H

#include "rt_lighting.h"      // lgt_light_pos; rt_ambient.h's table walk; rt_literal.h; include/rt_hip.h

#define RT_SOFT_WG 256u                  // rays per workgroup
#define RT_SOFT_FRAMES (RT_MAX_SEGS - 1u)   // live stack frames of a lane at most: a node of the last level has no children
#define RT_SOFT_FRAME_DOUBLES 14u        // shade[3], amb[3], a3, a4, the hit point [3], the refract direction [3]

// Passed by value in the kernel arguments: everything here is wave-uniform.
struct rt_soft_launch {
  const rt_sphere *objects;        // the scene's current sphere table, in blob order
  const rt_texture_desc *textures; // RT_MAX_TEXTURES descriptors; texels_offset is relative to texel_base
  const uint8_t *texel_base;
  const double *rays;              // n records {org[3], dir[3]} (16-byte aligned)
  const uint32_t *order;           // n entries, work-item j takes ray order[j]; or NULL
  const double *offs;              // n_offs offsets, 3 doubles each (not read at light_radius 0)
  double *rgb;                     // 3 per ray, or NULL
  uint32_t *rgba;                  // one word per ray, or NULL
  uint64_t base;
  double light_radius, epsilon, light_intensity;
  double miss_color[3];
  uint32_t n_objects, n;
  uint32_t n_samples, n_offs, stride, n_lights;
  uint32_t levels;                 // tree levels lv < levels take their light terms from the sampled loop
  uint32_t segs;                   // the CALL's depth (0: no level is shaded)
  uint32_t pix_base;               // ray i of the call is ray pix_base + i of the caller's list
  uint32_t stars_seed;
  double lights[RT_MAX_LIGHTS][3]; // the scene's current lights, by value as every launch carries them
};

// Asynchronous on `hip_stream` (a hipStream_t); returns a hipError_t as int.
extern "C" int rt_launch_soft(const rt_soft_launch *L, void *hip_stream);
// the kernel's private segment, bytes per lane, from the code object (for the scratch guard); returns a hipError_t as int
extern "C" int rt_soft_scratch(size_t *bytes_per_lane);

#endif
