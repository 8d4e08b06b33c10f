// Launch record of the occlusion kernel (rt_occlusion.hip), shared with its host side (rt_launch.hip).  Not part of the ABI.
#ifndef RT_OCCLUSION_H
#define RT_OCCLUSION_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rt_hip.h"

// Passed by value in the kernarg segment: everything here is wave-uniform.
struct rt_occlusion_launch {
  const rt_sphere *objects;        // the scene's current sphere table, in blob order
  const double *rays;              // n_rays records {org[3], dir[3]} (16-byte aligned)
  const uint32_t *order;           // n_rays entries, work-item j takes ray order[j]; or NULL
  const double *length;            // per ray, or NULL = +Infinity
  const double *intensity_in;      // per ray, or NULL = light_intensity
  const int32_t *skip;             // per ray, or NULL = no sphere is left out
  double *intensity;               // outputs, either of them NULL
  int32_t *blocker;
  double epsilon;
  double light_intensity;          // the scene's current one
  uint32_t n_objects;
  uint32_t n_rays;
};

extern "C" int rt_launch_occlusion(const rt_occlusion_launch *L, hipStream_t stream);

#endif
