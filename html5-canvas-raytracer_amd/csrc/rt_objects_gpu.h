// rt_objects_gpu.h — the device-side rebuild of a resident scene's sphere tables (rt_objects_gpu.hip) after an object move or a light
// move, as rt_scene.hip drives it.
#ifndef RT_OBJECTS_GPU_H
#define RT_OBJECTS_GPU_H

#include <stdint.h>

#include "../../include/rt_hip.h"
#include "rt_device.h"

// Some lights of a scene, by value in the kernarg segment (at most 16 x 24 bytes of positions): entry j is light k[j] at xyz[j]
struct rt_light_list { uint32_t n, k[RT_MAX_LIGHTS]; double xyz[RT_MAX_LIGHTS][3]; };

#ifdef __HIPCC__
// `bytes` of pinned host memory into device memory (multiple of 16 bytes read; both 16-byte aligned)
extern "C" int rt_launch_objects_copy(void *dst, const void *pinned_src, size_t bytes, hipStream_t stream);
// the bounce table of `n_objects` spheres in loop order (rt_tables.cpp: build_bounce_table's layout); cones: bounce_cell_cones
extern "C" int rt_launch_bounce_build(const rt_sphere *loop_objs, uint32_t n_objects, uint32_t n_loop, const double *cones, uint64_t *table, hipStream_t stream);
// the masks of the shadow grids (build_shadow_grid's layout, `n_lights` grids) of the lights in `lights`, whose headers `grid` already holds
extern "C" int rt_launch_sgrid_build(const rt_sphere *loop_objs, uint32_t n_loop, uint32_t n_lights, const rt_light_list *lights, uint64_t *grid, hipStream_t stream);
// A light move on an object block whose sphere records are current: the records anchored at the lights in `lights`, in each of the
// block's `n_ord` orderings (`geom`: per ordering [plain N | anchored at light k: NL x N]; objs[ord]: that ordering's sphere records),
// and - `grid` not NULL - those lights' shadow-grid headers, 16 doubles per entry of `lights`, from pinned host memory
extern "C" int rt_launch_light_anchor(const rt_sphere *objs_a, const rt_sphere *objs_b, uint32_t n_ord, uint32_t n_objects, uint32_t n_lights, const rt_light_list *lights,
                                      rt_geom *geom, double *grid, const double *pinned_headers, hipStream_t stream);
#endif

#endif
