// Launch record of the gather kernel (rt_gather.hip), shared with its host side (rt_gather_api.hip).  Not part of the ABI.
#ifndef RT_GATHER_H
#define RT_GATHER_H

#include "rt_soft.h"          // rt_soft_launch: the record the tree walk reads (rt_soft_walk.h); rt_ambient.h's receiver and table walk

#define RT_GATHER_WG 256u                // receivers per workgroup

// Passed by value in the kernel arguments: everything here is wave-uniform.
struct rt_gather_launch {
  // What the walk reads of the scene and the call: objects, textures, texel_base, epsilon, light_intensity, miss_color, n_objects,
  // n_lights, lights, stars_seed and segs (the CALL's depth).  The gather's own: order, rgb, rgba and n (the receivers).  Not read:
  // rays, offs, base, light_radius, n_samples, n_offs, stride, levels, pix_base (the walk is instantiated without its relit branch).
  rt_soft_launch S;
  const rt_hit *hits;              // n receivers (8-byte aligned)
  const double *dirs;              // n_dirs local directions, 3 doubles each
  uint64_t base;
  uint32_t n_samples, n_dirs, stride;
  uint32_t pix_base, pix_stride;   // pix of sample s of receiver i = pix_base + s * pix_stride + i (at most 2^31 - 1: the entry points check it)
};

// Asynchronous on `hip_stream` (a hipStream_t); returns a hipError_t as int.
extern "C" int rt_launch_gather(const rt_gather_launch *L, void *hip_stream);
// the kernel's private segment, bytes per lane, from the code object (for the scratch guard); returns a hipError_t as int
extern "C" int rt_gather_scratch(size_t *bytes_per_lane);

#endif
