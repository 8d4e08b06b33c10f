// rt_nodes_api.hip — the device entry points of the wavefront form (include/rt_hip.h: rt_scene_shade_rays_device,
// rt_scene_spawn_rays_device, rt_scene_fold_nodes_device; kernels: rt_nodes.hip).  No launch decision: shade reads the current
// generation's spheres in blob order, the lights, light intensity, epsilon, miss colour, textures and stars seed - camera, launch
// tables and flags play no part - so it comes behind the scene's preparation like every other launch; spawn and fold read nodes and
// nothing of the scene, and wait for no edit.  The host form (rt_trace_rays_wavefront) is rt_frame.hip's, beside rt_trace_rays.

#include "rt_api_internal.h"

namespace rt_api {
int ray_list_count_check(uint64_t n, const char *what);      // rt_launch.hip
int ray_list_align_check(const double *rays, const char *what);

int shade_check(uint64_t n, const double *rays, const uint32_t *order, const uint32_t *pix, const uint32_t *path, const rt_node *nodes, const char *what) {
  if (!rays || !nodes) return fail(RT_ERR_INVALID, "%s: NULL rays or nodes", what);
  if (int rc = ray_list_count_check(n, what)) return rc;
  if (int rc = ray_list_align_check(rays, what)) return rc;
  if ((uintptr_t)nodes & 7u) return fail(RT_ERR_INVALID, "%s: misaligned nodes (8 bytes)", what);
  if (((uintptr_t)order & 3u) || ((uintptr_t)pix & 3u) || ((uintptr_t)path & 3u)) return fail(RT_ERR_INVALID, "%s: misaligned order, pix or path (4 bytes)", what);
  return RT_OK;
}

int shade_launch(rt_scene_dev *s, uint32_t n, uint32_t base, const double *d_rays, const uint32_t *d_order, const uint32_t *d_pix, const uint32_t *d_path,
                 rt_node *d_nodes, hipStream_t stream, rt_stats *stats) {
  stats_clock clock;
  const rt_scene_header &hd = s->hd;
  rt_shade_launch L;
  memset(&L, 0, sizeof L);
  {
    std::lock_guard<std::mutex> lk(s->launch_mu);
    if (int rc = enter_launch(s, stream)) return rc;
    L.objects = (const rt_sphere *)(obj_block(s) + s->o_objs);   // this generation's spheres, in blob order
    L.light_intensity = hd.light_intensity;                      // (rt_scene_set_light_intensity: this launch's)
    L.stars_seed = hd.stars_seed;                                // (rt_scene_set_stars_seed: this launch's)
    memcpy(L.lights, s->lights, sizeof L.lights);
  }
  L.textures = s->d_texdesc;
  L.texel_base = (const uint8_t *)s->d_blob;
  memcpy(L.miss_color, hd.miss_color, sizeof L.miss_color);
  L.epsilon = hd.epsilon;
  L.n_objects = hd.n_objects; L.n_lights = hd.n_lights;
  L.rays = d_rays; L.order = d_order; L.pix = d_pix; L.path = d_path; L.nodes = d_nodes;
  L.n_rays = n; L.pix_base = base;
  if (int rc = clock.start(stats, stream)) return rc;
  const int err = rt_launch_shade_nodes(&L, stream);
  if (err != 0) return fail(RT_ERR_DEVICE, "node shade kernel launch: %s", hipGetErrorString((hipError_t)err));
  return clock.finish(stats, n);
}

int spawn_check(uint64_t n, const rt_node *nodes, const uint32_t *pix, const uint32_t *path, const double *child_rays, const uint32_t *child_pix,
                const uint32_t *child_path, const int32_t *links, const uint32_t *count, const void *work, size_t work_bytes, const char *what) {
  if (!nodes || !child_rays || !links || !count || !work) return fail(RT_ERR_INVALID, "%s: NULL nodes, child rays, links, count or workspace", what);
  if (int rc = ray_list_count_check(n, what)) return rc;
  if (int rc = ray_list_align_check(child_rays, what)) return rc;
  if ((uintptr_t)nodes & 7u) return fail(RT_ERR_INVALID, "%s: misaligned nodes (8 bytes)", what);
  if (((uintptr_t)pix & 3u) || ((uintptr_t)path & 3u) || ((uintptr_t)child_pix & 3u) || ((uintptr_t)child_path & 3u) || ((uintptr_t)links & 3u) ||
      ((uintptr_t)count & 3u) || ((uintptr_t)work & 3u))
    return fail(RT_ERR_INVALID, "%s: misaligned pix, path, links, count or workspace (4 bytes)", what);
  if (work_bytes < rt_nodes_spawn_work_bytes(n))
    return fail(RT_ERR_INVALID, "%s: work_bytes %llu below rt_nodes_spawn_work_bytes(%llu) = %llu", what, (unsigned long long)work_bytes,
                (unsigned long long)n, (unsigned long long)rt_nodes_spawn_work_bytes(n));
  return RT_OK;
}

int spawn_launch(uint32_t n, uint32_t base, const rt_node *d_nodes, const uint32_t *d_pix, const uint32_t *d_path, double *d_child_rays, uint32_t *d_child_pix,
                 uint32_t *d_child_path, int32_t *d_links, uint32_t *d_count, void *d_work, hipStream_t stream) {
  rt_spawn_launch L;
  memset(&L, 0, sizeof L);
  L.nodes = d_nodes; L.pix = d_pix; L.path = d_path;
  L.child_rays = d_child_rays; L.child_pix = d_child_pix; L.child_path = d_child_path;
  L.links = d_links; L.count = d_count; L.totals = (uint32_t *)d_work;
  L.n = n; L.pix_base = base;
  const int err = rt_launch_spawn_nodes(&L, stream);
  if (err != 0) return fail(RT_ERR_DEVICE, "node spawn launch: %s", hipGetErrorString((hipError_t)err));
  return RT_OK;
}

int fold_check(uint64_t n, const rt_node *nodes, const int32_t *links, const double *child_rgb, const double *rgb, const uint8_t *rgba, const char *what) {
  if (!nodes) return fail(RT_ERR_INVALID, "%s: NULL nodes", what);
  if (int rc = ray_list_count_check(n, what)) return rc;
  if (!rgb && !rgba) return fail(RT_ERR_INVALID, "%s: every output is NULL", what);
  if (links && !child_rgb) return fail(RT_ERR_INVALID, "%s: links without the children's rgb", what);
  if (((uintptr_t)nodes & 7u) || ((uintptr_t)child_rgb & 7u) || ((uintptr_t)rgb & 7u) || ((uintptr_t)links & 3u) || ((uintptr_t)rgba & 3u))
    return fail(RT_ERR_INVALID, "%s: misaligned pointer (nodes and rgb need 8 bytes, links and rgba 4)", what);
  return RT_OK;
}

int fold_launch(uint32_t n, const rt_node *d_nodes, const int32_t *d_links, const double *d_child_rgb, double *d_rgb, uint8_t *d_rgba, hipStream_t stream) {
  rt_fold_launch L;
  memset(&L, 0, sizeof L);
  L.nodes = d_nodes; L.links = d_links; L.child_rgb = d_child_rgb; L.rgb = d_rgb; L.rgba = (uint32_t *)d_rgba; L.n = n;
  const int err = rt_launch_fold_nodes(&L, stream);
  if (err != 0) return fail(RT_ERR_DEVICE, "node fold kernel launch: %s", hipGetErrorString((hipError_t)err));
  return RT_OK;
}
}  // namespace rt_api

// (the arguments first: they are judged without a scene, and before a device is touched)
extern "C" int rt_scene_shade_rays_device(rt_scene_dev *s, uint64_t n, const double *d_rays, const uint32_t *d_order, const uint32_t *d_pix,
                                          const uint32_t *d_path, rt_node *d_nodes, void *hip_stream, rt_stats *stats) {
  int rc = shade_check(n, d_rays, d_order, d_pix, d_path, d_nodes, "rt_scene_shade_rays_device");
  if (rc) return rc;
  if (!s) return fail(RT_ERR_STATE, "rt_scene_shade_rays_device: NULL scene handle");
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return shade_launch(s, (uint32_t)n, 0u, d_rays, d_order, d_pix, d_path, d_nodes, stream, stats);
}

extern "C" size_t rt_nodes_spawn_work_bytes(uint64_t n) { return (n == 0 || n >= (1ull << 31)) ? 0 : (size_t)rt_spawn_tiles(n) * sizeof(uint32_t); }

extern "C" int rt_scene_spawn_rays_device(rt_scene_dev *s, uint64_t n, const rt_node *d_nodes, const uint32_t *d_pix, const uint32_t *d_path,
                                          double *d_child_rays, uint32_t *d_child_pix, uint32_t *d_child_path, int32_t *d_links, uint32_t *d_count,
                                          void *d_work, size_t work_bytes, void *hip_stream) {
  int rc = spawn_check(n, d_nodes, d_pix, d_path, d_child_rays, d_child_pix, d_child_path, d_links, d_count, d_work, work_bytes, "rt_scene_spawn_rays_device");
  if (rc) return rc;
  if (!s) return fail(RT_ERR_STATE, "rt_scene_spawn_rays_device: NULL scene handle");
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return spawn_launch((uint32_t)n, 0u, d_nodes, d_pix, d_path, d_child_rays, d_child_pix, d_child_path, d_links, d_count, d_work, stream);
}

extern "C" int rt_scene_fold_nodes_device(rt_scene_dev *s, uint64_t n, const rt_node *d_nodes, const int32_t *d_links, const double *d_child_rgb,
                                          double *d_rgb, uint8_t *d_rgba, void *hip_stream) {
  int rc = fold_check(n, d_nodes, d_links, d_child_rgb, d_rgb, d_rgba, "rt_scene_fold_nodes_device");
  if (rc) return rc;
  if (!s) return fail(RT_ERR_STATE, "rt_scene_fold_nodes_device: NULL scene handle");
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return fold_launch((uint32_t)n, d_nodes, d_links, d_child_rgb, d_rgb, d_rgba, stream);
}
