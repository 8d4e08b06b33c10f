// rt_objects_gpu.h — the device-side rebuild of a resident scene's sphere tables (rt_objects_gpu.hip), as rt_scene.hip drives it.
#ifndef RT_OBJECTS_GPU_H
#define RT_OBJECTS_GPU_H

#include <stdint.h>

#include "../../include/rt_hip.h"

#ifdef __HIPCC__
// `bytes` of pinned host memory into device memory (multiple of 16 bytes read; both 16-byte aligned)
extern "C" int rt_launch_objects_copy(void *dst, const void *pinned_src, size_t bytes, hipStream_t stream);
// the bounce table of `n_objects` spheres in loop order (rt_tables.cpp: build_bounce_table's layout); cones: bounce_cell_cones
extern "C" int rt_launch_bounce_build(const rt_sphere *loop_objs, uint32_t n_objects, uint32_t n_loop, const double *cones, uint64_t *table, hipStream_t stream);
// the masks of the shadow grids (build_shadow_grid's layout) whose headers `grid` already holds; lights: 3 doubles each
extern "C" int rt_launch_sgrid_build(const rt_sphere *loop_objs, uint32_t n_loop, uint32_t n_lights, const double *lights, uint64_t *grid, hipStream_t stream);
#endif

#endif
