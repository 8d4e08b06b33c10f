// rt_relight_api.hip — relit nodes (include/rt_hip.h: rt_scene_relight_nodes_device; kernel: rt_relight.hip): the argument check, the
// launch and the device entry point.  The parameters are a struct rt_lighting, judged by rt_lighting_api.hip's own checks.  The kernel
// reads the scene's current spheres, epsilon, lights and light intensity, taken under launch_mu as rt_lighting_api.hip's launch takes
// them, so it comes behind the scene's preparation like every other launch.  The host forms (rt_relight_rays, rt_trace_rays_soft) are
// rt_frame.hip's, beside rt_shade_rays and rt_trace_rays_wavefront, whose chunked list call and level loop they share.
#include "rt_api_internal.h"
#include "rt_relight.h"

namespace rt_api {
int ray_list_count_check(uint64_t n, const char *what);      // rt_launch.hip
int ray_list_align_check(const double *rays, const char *what);

int relight_check(const struct rt_lighting *a, const double *d_offs, uint64_t n, const double *rays, const uint32_t *order, const uint32_t *pix,
                  const rt_node *nodes, const char *what) {
  if (int rc = lighting_device_check(a, d_offs, what)) return rc;
  if (!rays || !nodes) return fail(RT_ERR_INVALID, "%s: NULL rays or nodes", what);
  if (int rc = ray_list_count_check(n, what)) return rc;
  if (int rc = ray_list_align_check(rays, what)) return rc;
  if ((uintptr_t)nodes & 7u) return fail(RT_ERR_INVALID, "%s: misaligned nodes (8 bytes)", what);
  if (((uintptr_t)order & 3u) || ((uintptr_t)pix & 3u)) return fail(RT_ERR_INVALID, "%s: misaligned order or pix (4 bytes)", what);
  return RT_OK;
}

int relight_launch(rt_scene_dev *s, const struct rt_lighting &a, const double *d_offs, uint32_t n, const double *d_rays, const uint32_t *d_order,
                   const uint32_t *d_pix, rt_node *d_nodes, hipStream_t stream, rt_stats *stats) {
  stats_clock clock;
  rt_relight_launch L;
  memset(&L, 0, sizeof L);
  {
    std::lock_guard<std::mutex> lk(s->launch_mu);
    if (int rc = enter_launch(s, stream)) return rc;
    L.objects = (const rt_sphere *)(obj_block(s) + s->o_objs);   // this generation's spheres, in blob order
    L.light_intensity = s->hd.light_intensity;                   // (rt_scene_set_light_intensity, rt_scene_set_lights: this launch's)
    memcpy(L.lights, s->lights, sizeof L.lights);
  }
  L.epsilon = s->hd.epsilon;
  L.n_objects = s->hd.n_objects; L.n_lights = s->hd.n_lights;
  L.rays = d_rays; L.order = d_order; L.pix = d_pix; L.offs = d_offs; L.nodes = d_nodes; L.n = n;
  L.base = a.base; L.light_radius = a.light_radius;
  L.n_samples = a.n_samples; L.n_offs = a.n_offs; L.stride = a.stride;
  if (int rc = clock.start(stats, stream)) return rc;
  const int err = rt_launch_relight(&L, (void *)stream);
  if (err != 0) return fail(RT_ERR_DEVICE, "relight kernel launch: %s", hipGetErrorString((hipError_t)err));
  return clock.finish(stats, n);
}
}  // namespace rt_api

// (the arguments first: they are judged without a scene, and before a device is touched)
extern "C" int rt_scene_relight_nodes_device(rt_scene_dev *s, const struct rt_lighting *a, const double *d_offs, uint64_t n, const double *d_rays,
                                             const uint32_t *d_order, const uint32_t *d_pix, rt_node *d_nodes, void *hip_stream, rt_stats *stats) {
  const char *what = "rt_scene_relight_nodes_device";
  int rc = relight_check(a, d_offs, n, d_rays, d_order, d_pix, d_nodes, what);
  if (rc) return rc;
  if (!s) return fail(RT_ERR_STATE, "%s: NULL scene handle", what);
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return relight_launch(s, *a, d_offs, (uint32_t)n, d_rays, d_order, d_pix, d_nodes, stream, stats);
}
