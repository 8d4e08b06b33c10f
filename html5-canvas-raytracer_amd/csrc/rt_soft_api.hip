// rt_soft_api.hip — the soft trace in one launch (include/rt_hip.h: rt_scene_trace_rays_soft_device, rt_scene_trace_view_soft_device,
// rt_trace_rays_soft_recursive, rt_trace_view_soft; kernel: rt_soft.hip): the argument check, the launch, the two device entry points
// and the two host forms.  The parameters are a struct rt_lighting, judged by rt_lighting_api.hip's own checks.  The kernel reads what
// rt_nodes.hip's shade kernel and rt_relight.hip read - the scene's current spheres, epsilon, lights, light intensity, miss colour,
// textures and stars seed, taken under launch_mu - so it comes behind the scene's preparation like every other launch.  It keeps a
// stack in scratch memory: its figure goes through scratch_guard before the launch.
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

bool soft_view_size_ok(uint32_t w, uint32_t h) { return w != 0 && h != 0 && (uint64_t)w * h < (1ull << 31); }

// The view's rows [row0, row_end) in bands of at most band_rows: generated into d_work and traced with pix_base = y * w into the outputs'
// records from row out_row0 on.  One stream: a band's generation comes behind the trace that read the workspace before it.
int soft_view_bands(rt_scene_dev *s, const rt_view *v, uint32_t w, uint32_t h, const struct rt_lighting &a, const double *d_offs, uint32_t levels, uint32_t row0,
                    uint32_t row_end, uint32_t band_rows, uint32_t segs, const rt_ray_outputs &out, uint32_t out_row0, double *d_work, hipStream_t stream) {
  for (uint32_t y = row0; y < row_end; y += band_rows) {
    const uint32_t m = row_end - y < band_rows ? row_end - y : band_rows;
    if (int rc = rt_view_rays_device(s->device, v, w, h, y, m, d_work, (void *)stream)) return rc;
    const size_t at = (size_t)(y - out_row0) * w;         // of the band's first record in the outputs
    const rt_ray_outputs band = {out.rgb ? out.rgb + 3u * at : nullptr, out.rgba ? out.rgba + 4u * at : nullptr, nullptr};
    if (int rc = soft_launch(s, a, d_offs, levels, m * w, d_work, nullptr, y * w, segs, band, stream, nullptr)) return rc;
  }
  return RT_OK;
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
  return soft_view_size_ok(w, h) ? (size_t)w * h * 48u : 0;
}

extern "C" int rt_scene_trace_view_soft_device(rt_scene_dev *s, const rt_view *v, uint32_t w, uint32_t h, const struct rt_lighting *a, const double *d_offs,
                                               uint32_t levels, uint32_t segs, const rt_ray_outputs *d_out, void *d_work, size_t work_bytes, void *hip_stream,
                                               rt_stats *stats) {
  const char *what = "rt_scene_trace_view_soft_device";
  int rc = rt_view_validate(v, w, h);
  if (rc) return rc;
  if ((rc = lighting_device_check(a, d_offs, what))) return rc;
  if ((rc = soft_outputs_check(segs, d_out, what))) return rc;
  if (!d_work || ((uintptr_t)d_work & 15u)) return fail(RT_ERR_INVALID, "%s: NULL or misaligned workspace (16 bytes)", what);
  const uint64_t row_bytes = (uint64_t)w * 48u;
  if (work_bytes < row_bytes) return fail(RT_ERR_INVALID, "%s: work_bytes %llu below one row of rays, %llu", what, (unsigned long long)work_bytes, (unsigned long long)row_bytes);
  if (!s) return fail(RT_ERR_STATE, "%s: NULL scene handle", what);
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  const uint64_t fit = work_bytes / row_bytes;
  const uint32_t band_rows = fit < h ? (uint32_t)fit : h;
  stats_clock clock;
  if ((rc = clock.start(stats, stream))) return rc;
  if ((rc = soft_view_bands(s, v, w, h, *a, d_offs, levels, 0u, h, band_rows, segs, *d_out, 0u, (double *)d_work, stream))) return rc;
  return clock.finish(stats, (uint64_t)w * h);
}

// Host form: the list goes through rt_render's resident scene in chunks of RT_RAY_CHUNK rays and one set of device buffers; chunk c is
// traced with pix_base = c * RT_RAY_CHUNK, so ray i keeps pix = i and its table entries however the list is cut.  The table goes up
// once.  `binned`: each chunk is ordered on the GPU first (rt_rays_order.hip), which changes which rays share a wave and no result.
extern "C" int rt_trace_rays_soft_recursive(const void *blob, size_t bytes, const struct rt_lighting *a, const double *offs, uint32_t levels, uint64_t n,
                                            const double *rays, uint32_t segs, int binned, const rt_ray_outputs *ho, rt_stats *stats) {
  const char *what = "rt_trace_rays_soft_recursive";
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = rt_lighting_validate(a, offs))) return rc;
  if ((rc = soft_list_check(n, rays, nullptr, 0u, what))) return rc;
  if ((rc = soft_outputs_check(segs, ho, what))) return rc;
  if (!G.inited) return fail(RT_ERR_STATE, "rt_init has not been called");
  std::lock_guard<std::mutex> lk(G.mu);
  stats_clock clock;
  rt_scene_dev *s = nullptr;
  if ((rc = resident_scene(0, blob, bytes, &s))) return rc;
  if ((rc = ensure_device(0))) return rc;
  hipStream_t stream = G.dev[0].stream;
  const size_t chunk = n < RT_RAY_CHUNK ? (size_t)n : (size_t)RT_RAY_CHUNK;
  device_mem d_rays, d_rgb, d_rgba, d_offs, d_order, d_work;      // of one chunk; the table (released on every way out)
  HIP_TRY(hipMalloc(&d_rays.h, chunk * 48u));
  if (ho->rgb) HIP_TRY(hipMalloc(&d_rgb.h, chunk * 24u));
  if (ho->rgba) HIP_TRY(hipMalloc(&d_rgba.h, chunk * 4u));
  if (binned) {
    HIP_TRY(hipMalloc(&d_order.h, chunk * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&d_work.h, rt_rays_order_work_bytes(chunk)));
  }
  if ((rc = lighting_upload_offs(*a, offs, &d_offs, stream))) return rc;
  const rt_ray_outputs dout = {(double *)d_rgb.h, (uint8_t *)d_rgba.h, nullptr};
  double kernel_ms = 0.0;
  for (uint64_t base = 0; base < n; base += chunk) {
    const size_t m = n - base < chunk ? (size_t)(n - base) : chunk;
    HIP_TRY(hipMemcpyAsync(d_rays.h, rays + 6u * base, m * 48u, hipMemcpyHostToDevice, stream));
    rt_stats st;
    if (binned) {
      stats_clock step;
      if ((rc = step.start(stats, stream))) return rc;
      if ((rc = order_rays_launch((uint32_t)m, (const double *)d_rays.h, (uint32_t *)d_order.h, d_work.h, stream))) return rc;
      if ((rc = step.finish(stats ? &st : nullptr, m))) return rc;
      if (stats) kernel_ms += st.kernel_ms;
    }
    if ((rc = soft_launch(s, *a, (const double *)d_offs.h, levels, (uint32_t)m, (const double *)d_rays.h, (const uint32_t *)d_order.h, (uint32_t)base, segs, dout,
                          stream, stats ? &st : nullptr)))
      return rc;
    if (stats) kernel_ms += st.kernel_ms;
    if (ho->rgb) HIP_TRY(hipMemcpyAsync(ho->rgb + 3u * base, d_rgb.h, m * 24u, hipMemcpyDeviceToHost, stream));
    if (ho->rgba) HIP_TRY(hipMemcpyAsync(ho->rgba + 4u * base, d_rgba.h, m * 4u, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->kernel_ms = kernel_ms;
    stats->pixels = n;
    stats->total_ms = clock.host_ms();
  }
  return RT_OK;
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
  if (!G.inited) return fail(RT_ERR_STATE, "rt_init has not been called");
  std::lock_guard<std::mutex> lk(G.mu);
  stats_clock clock;
  rt_scene_dev *s = nullptr;
  if ((rc = resident_scene(0, blob, bytes, &s))) return rc;
  if ((rc = ensure_device(0))) return rc;
  hipStream_t stream = G.dev[0].stream;
  uint64_t chunk_rows = RT_RAY_CHUNK / w;
  if (chunk_rows < 1u) chunk_rows = 1u;
  if (chunk_rows > h) chunk_rows = h;
  const size_t chunk = (size_t)chunk_rows * w;
  device_mem d_rays, d_rgb, d_rgba, d_offs, d_lon, d_lat;         // of one chunk; the table; the panorama's tables (released on every way out)
  HIP_TRY(hipMalloc(&d_rays.h, chunk * 48u));
  if (ho->rgb) HIP_TRY(hipMalloc(&d_rgb.h, chunk * 24u));
  if (ho->rgba) HIP_TRY(hipMalloc(&d_rgba.h, chunk * 4u));
  if ((rc = lighting_upload_offs(*a, offs, &d_offs, stream))) return rc;
  rt_view dv = *v;
  if (v->model == RT_VIEW_EQUIRECT) {
    HIP_TRY(hipMalloc(&d_lon.h, (size_t)w * 16u));
    HIP_TRY(hipMalloc(&d_lat.h, (size_t)h * 16u));
    HIP_TRY(hipMemcpyAsync(d_lon.h, v->lon, (size_t)w * 16u, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_lat.h, v->lat, (size_t)h * 16u, hipMemcpyHostToDevice, stream));
    dv.lon = (const double *)d_lon.h; dv.lat = (const double *)d_lat.h;
  }
  const rt_ray_outputs dout = {(double *)d_rgb.h, (uint8_t *)d_rgba.h, nullptr};
  double kernel_ms = 0.0;
  for (uint32_t y = 0; y < h; y += (uint32_t)chunk_rows) {
    const uint32_t m = h - y < chunk_rows ? h - y : (uint32_t)chunk_rows;
    const size_t at = (size_t)y * w, cnt = (size_t)m * w;
    stats_clock step;
    rt_stats st;
    if ((rc = step.start(stats, stream))) return rc;
    if ((rc = soft_view_bands(s, &dv, w, h, *a, (const double *)d_offs.h, levels, y, y + m, m, segs, dout, y, (double *)d_rays.h, stream))) return rc;
    if ((rc = step.finish(stats ? &st : nullptr, cnt))) return rc;
    if (stats) kernel_ms += st.kernel_ms;
    if (ho->rgb) HIP_TRY(hipMemcpyAsync(ho->rgb + 3u * at, d_rgb.h, cnt * 24u, hipMemcpyDeviceToHost, stream));
    if (ho->rgba) HIP_TRY(hipMemcpyAsync(ho->rgba + 4u * at, d_rgba.h, cnt * 4u, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->kernel_ms = kernel_ms;
    stats->pixels = (uint64_t)w * h;
    stats->total_ms = clock.host_ms();
  }
  return RT_OK;
}
