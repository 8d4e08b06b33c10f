// Launch records of the node kernels (rt_nodes.hip: shade, spawn, fold), shared with their host side (rt_nodes_api.hip).  Not part of the ABI.
#ifndef RT_NODES_H
#define RT_NODES_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rt_hip.h"

#define RT_NODES_WG 256u

// Passed by value in the kernarg segment: everything here is wave-uniform.
struct rt_shade_launch {
  const rt_sphere *objects;        // the scene's current sphere table, in blob order
  const rt_texture_desc *textures; // RT_MAX_TEXTURES descriptors; texels_offset is relative to texel_base
  const uint8_t *texel_base;
  const double *rays;              // n_rays records {org[3], dir[3]} (16-byte aligned)
  const uint32_t *order;           // n_rays entries, work-item j takes ray order[j]; or NULL
  const uint32_t *pix, *path;      // per ray, or NULL = pix_base + i / 1
  rt_node *nodes;                  // n_rays records (8-byte aligned)
  double lights[RT_MAX_LIGHTS][3];
  double miss_color[3];
  double epsilon;
  double light_intensity;          // the scene's current one
  uint32_t n_objects, n_lights;
  uint32_t n_rays;
  uint32_t pix_base;               // the host form's chunk: ray i of the call is ray pix_base + i of the caller's list
  uint32_t stars_seed;
};

struct rt_spawn_launch {
  const rt_node *nodes;            // n parents
  const uint32_t *pix, *path;      // the parents', or NULL = pix_base + i / 1
  double *child_rays;              // 2n records (16-byte aligned)
  uint32_t *child_pix, *child_path;// 2n entries each, or NULL
  int32_t *links;                  // 2n entries
  uint32_t *count;                 // one word
  uint32_t *totals;                // the workspace: one word per workgroup of RT_NODES_WG parents
  uint32_t n;
  uint32_t pix_base;
};

struct rt_fold_launch {
  const rt_node *nodes;            // n nodes
  const int32_t *links;            // 2n entries, or NULL = the deepest level
  const double *child_rgb;         // 3 per child
  double *rgb;                     // 3 per node, or NULL
  uint32_t *rgba;                  // one word per node, or NULL
  uint32_t n;
};

// workgroups of RT_NODES_WG parents a spawn of n nodes runs (n < 2^31)
static inline uint32_t rt_spawn_tiles(uint64_t n) { return (uint32_t)((n + RT_NODES_WG - 1u) / RT_NODES_WG); }

extern "C" int rt_launch_shade_nodes(const rt_shade_launch *L, hipStream_t stream);
extern "C" int rt_launch_spawn_nodes(const rt_spawn_launch *L, hipStream_t stream);
extern "C" int rt_launch_fold_nodes(const rt_fold_launch *L, hipStream_t stream);

#endif
