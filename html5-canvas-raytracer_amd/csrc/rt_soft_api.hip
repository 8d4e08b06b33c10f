// rt_soft_api.hip — the soft trace in one launch (include/rt_hip.h: rt_scene_trace_rays_soft_device, rt_scene_trace_view_soft_device,
// rt_trace_rays_soft_recursive, rt_trace_view_soft; kernel: rt_soft.hip): the argument check, the launch, the two device entry points
// and the two host forms.  The parameters are a struct rt_lighting, judged by rt_lighting_api.hip's own checks.  The kernel reads what
// rt_nodes.hip's shade kernel and rt_relight.hip read - the scene's current spheres, epsilon, lights, light intensity, miss colour,
// textures and stars seed, taken under launch_mu - so it comes behind the scene's preparation like every other launch.  It keeps a
// stack in scratch memory: its figure goes through scratch_guard before the launch.
// The host forms are rows and a step for the chunk drivers of rt_api_internal.h.
// A view is traced in bands of whole rows as rt_views_api.hip's trace_view_bands does it: a band's rays are generated into the
// workspace (rt_view_rays_device) and traced with pix_base = y * w, so pixel i = y * w + x is ray i whatever the band.
#include "rt_api_internal.h"
#include "rt_soft.h"

namespace rt_api {
int ray_list_count_check(uint64_t n, const char *what);      // rt_launch.hip
int ray_list_align_check(const double *rays, const char *what);
}  // namespace rt_api

namespace {
// the depth and outputs of a soft trace: rays_check's rules (rt_launch.hip) without hit records, which the recursive rt_scene_trace_rays_device holds
int soft_outputs_check(uint32_t segs, const rt_ray_outputs *out, const char *what) {
  if (!out) return fail(RT_ERR_INVALID, "%s: NULL outputs", what);
  if (segs > RT_MAX_SEGS) return fail(RT_ERR_INVALID, "%s: segs %u not in 0..%u (0 = the scene's depth)", what, segs, RT_MAX_SEGS);
  if (out->hits) return fail(RT_ERR_INVALID, "%s: no hit records (rt_scene_trace_rays_device holds them)", what);
  if (!out->rgb && !out->rgba) return fail(RT_ERR_INVALID, "%s: every output is NULL", what);
  if (((uintptr_t)out->rgb & 7u) || ((uintptr_t)out->rgba & 3u)) return fail(RT_ERR_INVALID, "%s: misaligned output (rgb needs 8 bytes, rgba 4)", what);
  return RT_OK;
}

// a list of n rays that are rays [pix_base, pix_base + n) of the caller's list
int soft_list_check(uint64_t n, const double *rays, const uint32_t *order, uint32_t pix_base, const char *what) {
  if (!rays) return fail(RT_ERR_INVALID, "%s: NULL rays", what);
  if (int rc = ray_list_count_check(n, what)) return rc;
  if ((uint64_t)pix_base + n > (1ull << 31)) return fail(RT_ERR_INVALID, "%s: pix_base %u + n %llu above 2^31", what, pix_base, (unsigned long long)n);
  if (int rc = ray_list_align_check(rays, what)) return rc;
  if ((uintptr_t)order & 3u) return fail(RT_ERR_INVALID, "%s: misaligned order (4 bytes)", what);
  return RT_OK;
}

// the kernel's scratch figure, asked once
int soft_scratch(size_t *out) {
  static std::mutex mu;
  static size_t cached;
  static bool have;
  std::lock_guard<std::mutex> lk(mu);
  if (!have) {
    size_t b = 0;
    const int e = rt_soft_scratch(&b);
    if (e != 0) return fail(RT_ERR_DEVICE, "hipFuncGetAttributes: %s", hipGetErrorString((hipError_t)e));
    cached = b; have = true;
  }
  *out = cached;
  return RT_OK;
}

// rays [0, n) of d_rays, rays [pix_base, pix_base + n) of the caller's list, with the description's base as given
int soft_launch(rt_scene_dev *s, const struct rt_lighting &a, const double *d_offs, uint32_t levels, uint32_t n, const double *d_rays, const uint32_t *d_order,
                uint32_t pix_base, uint32_t segs, const rt_ray_outputs &out, hipStream_t stream, rt_stats *stats) {
  stats_clock clock;
  const rt_scene_header &hd = s->hd;
  rt_soft_launch L;
  memset(&L, 0, sizeof L);
  {
    std::lock_guard<std::mutex> lk(s->launch_mu);
    if (int rc = enter_launch(s, stream)) return rc;
    L.objects = (const rt_sphere *)(obj_block(s) + s->o_objs);   // this generation's spheres, in blob order
    L.light_intensity = hd.light_intensity;                      // (rt_scene_set_light_intensity, rt_scene_set_lights: this launch's)
    L.stars_seed = hd.stars_seed;                                // (rt_scene_set_stars_seed: this launch's)
    memcpy(L.lights, s->lights, sizeof L.lights);
  }
  L.textures = s->d_texdesc;
  L.texel_base = (const uint8_t *)s->d_blob;
  memcpy(L.miss_color, hd.miss_color, sizeof L.miss_color);
  L.epsilon = hd.epsilon;
  L.n_objects = hd.n_objects; L.n_lights = hd.n_lights;
  L.rays = d_rays; L.order = d_order; L.offs = d_offs; L.rgb = out.rgb; L.rgba = (uint32_t *)out.rgba; L.n = n;
  L.base = a.base; L.light_radius = a.light_radius;
  L.n_samples = a.n_samples; L.n_offs = a.n_offs; L.stride = a.stride;
  L.levels = levels;
  L.segs = segs ? segs : hd.segs;                                // the CALL's depth
  if (L.segs > RT_MAX_SEGS) return fail(RT_ERR_INVALID, "the soft trace kernel: depth %u above %u", L.segs, RT_MAX_SEGS);   // (the stack's size)
  L.pix_base = pix_base;
  size_t per_lane = 0;
  if (int rc = soft_scratch(&per_lane)) return rc;
  const uint64_t n_wg = ((uint64_t)n + RT_SOFT_WG - 1u) / RT_SOFT_WG;
  if (int rc = scratch_guard(G.dev[s->device], stream, per_lane, n_wg * (RT_SOFT_WG / 64u), "the soft trace kernel (rt_soft_trace)")) return rc;
  if (int rc = clock.start(stats, stream)) return rc;
  const int err = rt_launch_soft(&L, (void *)stream);
  if (err != 0) return fail(RT_ERR_DEVICE, "soft trace kernel launch: %s", hipGetErrorString((hipError_t)err));
  return clock.finish(stats, n);
}

// The view's rows [row0, row_end) in bands of at most band_rows: generated into d_work and traced with pix_base = y * w into the outputs'
// records from row out_row0 on.  One stream: a band's generation comes behind the trace that read the workspace before it.
int soft_view_bands(rt_scene_dev *s, const rt_view *v, uint32_t w, uint32_t h, const struct rt_lighting &a, const double *d_offs, uint32_t levels, uint32_t row0,
                    uint32_t row_end, uint32_t band_rows, uint32_t segs, const rt_ray_outputs &out, uint32_t out_row0, double *d_work, hipStream_t stream) {
  return for_bands(row0, row_end, band_rows, [&](uint32_t y, uint32_t m) {
    if (int rc = rt_view_rays_device(s->device, v, w, h, y, m, d_work, (void *)stream)) return rc;
    const size_t at = (size_t)(y - out_row0) * w;         // of the band's first record in the outputs
    const rt_ray_outputs band = {out.rgb ? out.rgb + 3u * at : nullptr, out.rgba ? out.rgba + 4u * at : nullptr, nullptr};
    return soft_launch(s, a, d_offs, levels, m * w, d_work, nullptr, y * w, segs, band, stream, nullptr);
  });
}
}  // namespace

// (the arguments first: they are judged without a scene, and before a device is touched)
extern "C" int rt_scene_trace_rays_soft_device(rt_scene_dev *s, const struct rt_lighting *a, const double *d_offs, uint32_t levels, uint64_t n,
                                               const double *d_rays, const uint32_t *d_order, uint32_t pix_base, uint32_t segs, const rt_ray_outputs *d_out,
                                               void *hip_stream, rt_stats *stats) {
  const char *what = "rt_scene_trace_rays_soft_device";
  int rc = lighting_device_check(a, d_offs, what);
  if (rc) return rc;
  if ((rc = soft_list_check(n, d_rays, d_order, pix_base, what))) return rc;
  if ((rc = soft_outputs_check(segs, d_out, what))) return rc;
  if (!s) return fail(RT_ERR_STATE, "%s: NULL scene handle", what);
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return soft_launch(s, *a, d_offs, levels, (uint32_t)n, d_rays, d_order, pix_base, segs, *d_out, stream, stats);
}

extern "C" size_t rt_soft_view_work_bytes(uint32_t w, uint32_t h) {
  // the whole view in one band, as rt_view_work_bytes
  return view_size_ok(w, h) ? (size_t)w * h * 48u : 0;
}

extern "C" int rt_scene_trace_view_soft_device(rt_scene_dev *s, const rt_view *v, uint32_t w, uint32_t h, const struct rt_lighting *a, const double *d_offs,
                                               uint32_t levels, uint32_t segs, const rt_ray_outputs *d_out, void *d_work, size_t work_bytes, void *hip_stream,
                                               rt_stats *stats) {
  const char *what = "rt_scene_trace_view_soft_device";
  int rc = rt_view_validate(v, w, h);
  if (rc) return rc;
  if ((rc = lighting_device_check(a, d_offs, what))) return rc;
  if ((rc = soft_outputs_check(segs, d_out, what))) return rc;
  uint32_t band_rows = 0;
  if ((rc = view_work_check(d_work, work_bytes, w, h, 48u, "rays", what, &band_rows))) return rc;
  if (!s) return fail(RT_ERR_STATE, "%s: NULL scene handle", what);
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return timed(stream, stats, (uint64_t)w * h,
               [&] { return soft_view_bands(s, v, w, h, *a, d_offs, levels, 0u, h, band_rows, segs, *d_out, 0u, (double *)d_work, stream); });
}

// Host form: the list goes through rt_render's resident scene in chunks of RT_RAY_CHUNK rays (chunked_list_call); chunk c is traced
// with pix_base = c * RT_RAY_CHUNK, so ray i keeps pix = i and its table entries however the list is cut.  The table goes up once.
// `binned`: each chunk is ordered on the GPU first (rt_rays_order.hip), which changes which rays share a wave and no result.
extern "C" int rt_trace_rays_soft_recursive(const void *blob, size_t bytes, const struct rt_lighting *a, const double *offs, uint32_t levels, uint64_t n,
                                            const double *rays, uint32_t segs, int binned, const rt_ray_outputs *ho, rt_stats *stats) {
  const char *what = "rt_trace_rays_soft_recursive";
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = rt_lighting_validate(a, offs))) return rc;
  if ((rc = soft_list_check(n, rays, nullptr, 0u, what))) return rc;
  if ((rc = soft_outputs_check(segs, ho, what))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  device_mem d_offs;                 // the table (released behind the call, whose every chunk has been waited for)
  if ((rc = lighting_upload_offs(*a, offs, &d_offs, call.stream))) return rc;
  const chunk_row rows[3] = {row_in(rays, 48u), row_out(ho->rgb, 24u), row_out(ho->rgba, 4u)};
  return chunked_list_call(call, n, rows, 3, binned != 0, stats, [&](uint32_t m, uint64_t base, void *const *d, const uint32_t *d_order, rt_stats *st) {
    const rt_ray_outputs dout = {(double *)d[1], (uint8_t *)d[2], nullptr};
    return soft_launch(call.s, *a, (const double *)d_offs.h, levels, m, (const double *)d[0], d_order, (uint32_t)base, segs, dout, call.stream, st);
  });
}

// Host form on rt_render's resident scene, as rt_trace_view: chunks of whole rows of at most RT_RAY_CHUNK rays; a longer row is its own chunk
extern "C" int rt_trace_view_soft(const void *blob, size_t bytes, const rt_view *v, uint32_t w, uint32_t h, const struct rt_lighting *a, const double *offs,
                                  uint32_t levels, uint32_t segs, const rt_ray_outputs *ho, rt_stats *stats) {
  const char *what = "rt_trace_view_soft";
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = rt_view_validate(v, w, h))) return rc;
  if ((rc = rt_lighting_validate(a, offs))) return rc;
  if ((rc = soft_outputs_check(segs, ho, what))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  device_mem d_offs;                 // the table
  device_bufs<2> tables;             // the panorama's
  rt_view dv;
  if ((rc = lighting_upload_offs(*a, offs, &d_offs, call.stream))) return rc;
  if ((rc = view_upload_tables(*v, w, h, 1u, call.stream, &tables, &dv))) return rc;
  const chunk_row rows[3] = {row_scratch((size_t)w * 48u), row_out(ho->rgb, (size_t)w * 24u), row_out(ho->rgba, (size_t)w * 4u)};
  return chunked_view_call(call, w, h, rows, 3, stats, [&](uint32_t y, uint32_t m, void *const *d) {
    const rt_ray_outputs dout = {(double *)d[1], (uint8_t *)d[2], nullptr};
    return soft_view_bands(call.s, &dv, w, h, *a, (const double *)d_offs.h, levels, y, y + m, m, segs, dout, y, (double *)d[0], call.stream);
  });
}
