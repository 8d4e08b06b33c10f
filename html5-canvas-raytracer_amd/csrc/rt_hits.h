// Launch record of the primary-hit kernels (rt_hits.hip), shared with their host side (rt_launch.hip).  Not part of the ABI.
#ifndef RT_HITS_H
#define RT_HITS_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rt_hip.h"

// Passed by value in the kernarg segment: everything here is wave-uniform.
struct rt_hits_launch {
  const rt_sphere *objects;        // the uploaded blob's sphere table, in blob order
  int32_t *id;                     // rt_render_hits_device outputs, any of them NULL
  double *depth;
  float *normal;
  const uint32_t *points;          // rt_scene_pick: n_points {x, y} sample coordinates ...
  rt_hit *hits;                    // ... and their records
  double cam[12];                  // origin, axisX, axisY, axisZ (the scene's current camera)
  double proj_w, proj_h, proj_d;   // of the SAMPLE grid, in binary64 on the host (main.js:102-105)
  double epsilon;
  uint32_t n_objects;
  uint32_t sw, sh;                 // sample grid: k w x k h
  uint32_t k;                      // supersample factor (1 .. 4)
  uint32_t tile_rows, tile_first, tile_stride;   // rt_tiles, in OUTPUT rows
  uint32_t band_rows;              // sample rows of the call's band: n_tiles x k x tile_rows
  uint32_t n_points;
  // rt_scene_trace_rays_device: n_rays records {org[3], dir[3]} (16-byte aligned) ... and their records in `hits`
  const double *rays;
  uint32_t n_rays;
  const uint32_t *ray_order;       // rt_scene_trace_rays_ordered_device: n_rays entries, work-item j takes ray ray_order[j]; or NULL
};

extern "C" int rt_launch_hits(const rt_hits_launch *L, hipStream_t stream);
extern "C" int rt_launch_pick(const rt_hits_launch *L, hipStream_t stream);
extern "C" int rt_launch_ray_hits(const rt_hits_launch *L, hipStream_t stream);

#endif
