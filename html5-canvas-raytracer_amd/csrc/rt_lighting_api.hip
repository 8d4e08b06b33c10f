// rt_lighting_api.hip — sampled lights (include/rt_hip.h: rt_lighting): the host logic (validation, the offset table, the host probe),
// the launch of rt_lighting.hip's kernel, and the host forms: a list of receivers through device buffers in chunks, and a whole view
// whose rays, hit records and scans never leave the device.  The kernel reads the scene's current spheres, epsilon, lights and light
// intensity; the last two are the host copies every launch carries by value, taken under launch_mu with the sphere block
// (rt_scene_set_lights and rt_scene_set_light_intensity write them under it).  The chunk driver, the prologue and the band loop are
// the ones every host form shares (rt_api_internal.h); a band's first half - rays, hit records - is rt_views_api.hip's view_band_hits.
#include "rt_api_internal.h"
#include "rt_lighting.h"

static_assert(sizeof(struct rt_lighting) == 32 && sizeof(rt_hit) == 80, "a lighting description travels as 32 bytes, a receiver is 80");

namespace {
int lighting_check(const struct rt_lighting *a, const char *what) {
  if (!a) return fail(RT_ERR_INVALID, "%s: NULL lighting description", what);
  if (a->n_samples < 1u || a->n_samples > RT_LIGHTING_MAX_SAMPLES) return fail(RT_ERR_INVALID, "%s: n_samples %u not in 1..%u", what, a->n_samples, RT_LIGHTING_MAX_SAMPLES);
  if (a->n_offs < a->n_samples || a->n_offs > RT_LIGHTING_MAX_OFFS)
    return fail(RT_ERR_INVALID, "%s: n_offs %u not in n_samples..%u", what, a->n_offs, RT_LIGHTING_MAX_OFFS);
  if (a->reserved != 0u) return fail(RT_ERR_INVALID, "%s: reserved %u not 0", what, a->reserved);
  if (!std::isfinite(a->light_radius) || a->light_radius < 0.0) return fail(RT_ERR_INVALID, "%s: light_radius %g not finite and >= 0", what, a->light_radius);
  return RT_OK;
}

// ... and a table in HOST memory
int lighting_table_check(const struct rt_lighting *a, const double *offs, const char *what) {
  if (int rc = lighting_check(a, what)) return rc;
  if (!offs) return fail(RT_ERR_INVALID, "%s: NULL offset table", what);
  for (uint32_t e = 0; e < a->n_offs; e++)
    if (!std::isfinite(offs[3u * (size_t)e]) || !std::isfinite(offs[3u * (size_t)e + 1u]) || !std::isfinite(offs[3u * (size_t)e + 2u]))
      return fail(RT_ERR_INVALID, "%s: offset %u has a non-finite component", what, e);
  return RT_OK;
}

int lighting_outputs_check(const rt_lighting_outputs *out, const char *what) {
  if (!out) return fail(RT_ERR_INVALID, "%s: NULL outputs", what);
  if (!out->diffuse && !out->intensity && !out->lit && !out->rgba) return fail(RT_ERR_INVALID, "%s: every output is NULL", what);
  if (((uintptr_t)out->diffuse & 7u) || ((uintptr_t)out->intensity & 7u) || ((uintptr_t)out->lit & 7u) || ((uintptr_t)out->rgba & 3u))
    return fail(RT_ERR_INVALID, "%s: misaligned output (diffuse, intensity and lit need 8 bytes, rgba 4)", what);
  return RT_OK;
}

// a device table: NULL only where it is not read
int lighting_offs_check(const struct rt_lighting &a, const double *d_offs, const char *what) {
  if ((!d_offs && a.light_radius != 0.0) || ((uintptr_t)d_offs & 7u)) return fail(RT_ERR_INVALID, "%s: NULL or misaligned offset table (8 bytes)", what);
  return RT_OK;
}

rt_lighting_launch launch_of(const struct rt_lighting &a, const double *offs, uint32_t n, const rt_hit *hits) {
  rt_lighting_launch L;
  memset(&L, 0, sizeof L);
  L.hits = hits; L.offs = offs; L.n = n;
  L.base = a.base; L.light_radius = a.light_radius;
  L.n_samples = a.n_samples; L.n_offs = a.n_offs; L.stride = a.stride;
  return L;
}

// the fused kernel for receivers [0, n) of d_hits with the description's base as given
int lighting_launch(rt_scene_dev *s, const struct rt_lighting &a, const double *d_offs, uint32_t n, const rt_hit *d_hits, const uint32_t *d_order,
                    const rt_lighting_outputs &out, hipStream_t stream, rt_stats *stats) {
  stats_clock clock;
  rt_lighting_launch L = launch_of(a, d_offs, n, d_hits);
  {
    std::lock_guard<std::mutex> lk(s->launch_mu);
    if (int rc = enter_launch(s, stream)) return rc;
    L.objects = (const rt_sphere *)(obj_block(s) + s->o_objs);   // this generation's spheres, in blob order
    L.light_intensity = s->hd.light_intensity;                   // (rt_scene_set_light_intensity, rt_scene_set_lights: this launch's)
    memcpy(L.lights, s->lights, sizeof L.lights);
  }
  L.epsilon = s->hd.epsilon;
  L.n_objects = s->hd.n_objects; L.n_lights = s->hd.n_lights;
  L.order = d_order;
  L.diffuse = out.diffuse; L.intensity = out.intensity; L.lit = out.lit; L.rgba = out.rgba;
  if (int rc = clock.start(stats, stream)) return rc;
  const int err = rt_launch_lighting(&L, (void *)stream);
  if (err != 0) return fail(RT_ERR_DEVICE, "lighting kernel launch: %s", hipGetErrorString((hipError_t)err));
  return clock.finish(stats, n);
}

constexpr uint32_t RT_LIGHTING_VIEW_BAND_BYTES = 128u;    // per pixel of a band: the ray 48, its hit record 80

// The view's rows [row0, row_end) in bands of at most band_rows: per band the rays (rt_views.hip), their hit records (rt_hits.hip) and the
// fused kernel with base = a.base + y * w, so that pixel i = y * w + x is receiver i whatever the band.  The outputs' first record is
// pixel out_row0 * w.  One stream: every launch comes behind the one that wrote what it reads.  (The view was checked by the caller.)
int lighting_view_bands(rt_scene_dev *s, const rt_view *v, uint32_t w, uint32_t h, const struct rt_lighting &a, const double *d_offs, uint32_t row0,
                        uint32_t row_end, uint32_t band_rows, const rt_lighting_outputs &out, uint32_t out_row0, void *d_work, hipStream_t stream) {
  double *rays = (double *)d_work;
  rt_hit *hits = (rt_hit *)(rays + 6u * ((size_t)band_rows * w));
  return for_bands(row0, row_end, band_rows, [&](uint32_t y, uint32_t m) {
    if (int rc = view_band_hits(s, v, w, h, y, m, rays, hits, stream)) return rc;
    struct rt_lighting ab = a;
    ab.base = a.base + (uint64_t)y * w;
    const size_t at = (size_t)(y - out_row0) * w;
    const rt_lighting_outputs band = {out.diffuse ? out.diffuse + at : nullptr, out.intensity ? out.intensity + at : nullptr, out.lit ? out.lit + at : nullptr,
                                      out.rgba ? out.rgba + at : nullptr};
    return lighting_launch(s, ab, d_offs, m * w, hits, nullptr, band, stream, nullptr);
  });
}

// the outputs of a host form as the rows of a chunked call: `each` records per unit (a list: 1, a view: w), and a chunk's on the device
void output_rows(const rt_lighting_outputs &ho, size_t each, chunk_row *rows) {
  rows[0] = row_out(ho.diffuse, each * 8u); rows[1] = row_out(ho.intensity, each * 8u); rows[2] = row_out(ho.lit, each * 8u); rows[3] = row_out(ho.rgba, each * 4u);
}
rt_lighting_outputs device_outputs(void *const *d) { return rt_lighting_outputs{(double *)d[0], (double *)d[1], (double *)d[2], (uint32_t *)d[3]}; }

// the table of a host form in device memory: not allocated where it is not read
int upload_offs(const struct rt_lighting &a, const double *offs, device_mem *d_offs, hipStream_t stream) {
  if (a.light_radius == 0.0) return RT_OK;
  HIP_TRY(hipMalloc(&d_offs->h, (size_t)a.n_offs * 24u));
  HIP_TRY(hipMemcpyAsync(d_offs->h, offs, (size_t)a.n_offs * 24u, hipMemcpyHostToDevice, stream));
  return RT_OK;
}
}  // namespace

// what the relit nodes (rt_relight_api.hip, rt_frame.hip) share with this unit: the checks of a description with a device table, and the upload
namespace rt_api {
int lighting_device_check(const struct rt_lighting *a, const double *d_offs, const char *what) {
  if (int rc = lighting_check(a, what)) return rc;
  return lighting_offs_check(*a, d_offs, what);
}
int lighting_upload_offs(const struct rt_lighting &a, const double *offs, device_mem *d_offs, hipStream_t stream) { return upload_offs(a, offs, d_offs, stream); }
}  // namespace rt_api

extern "C" int rt_lighting_validate(const struct rt_lighting *a, const double *offs) { return lighting_table_check(a, offs, "rt_lighting_validate"); }

extern "C" int rt_lighting_sphere_offsets(uint32_t n, double *out_3n) {
  if (n < 1u || n > RT_LIGHTING_MAX_OFFS || !out_3n) return fail(RT_ERR_INVALID, "rt_lighting_sphere_offsets: n %u not in 1..%u, or a NULL output", n, RT_LIGHTING_MAX_OFFS);
  rt_lighting_sphere_offsets_host(n, out_3n);
  return RT_OK;
}

extern "C" int rt_lighting_segments(const struct rt_lighting *a, const double *offs, uint32_t n_lights, const double *lights_xyz, uint64_t n, const rt_hit *hits,
                                    uint32_t sample, uint32_t light, double *out_rays, double *out_length, double *out_mag, double *out_dot, int32_t *out_skip) {
  const char *what = "rt_lighting_segments";
  int rc = lighting_table_check(a, offs, what);
  if (rc) return rc;
  if (n_lights < 1u || n_lights > RT_MAX_LIGHTS || !lights_xyz) return fail(RT_ERR_INVALID, "%s: n_lights %u not in 1..%u, or NULL lights", what, n_lights, RT_MAX_LIGHTS);
  if ((rc = receiver_count_check(n, what))) return rc;
  if (sample >= a->n_samples) return fail(RT_ERR_INVALID, "%s: sample %u not below n_samples %u", what, sample, a->n_samples);
  if (light >= n_lights) return fail(RT_ERR_INVALID, "%s: light %u not below n_lights %u", what, light, n_lights);
  if (!hits || !out_rays) return fail(RT_ERR_INVALID, "%s: NULL hit records or ray output", what);
  rt_lighting_launch L = launch_of(*a, offs, (uint32_t)n, hits);
  L.n_lights = n_lights;
  memcpy(L.lights, lights_xyz, (size_t)n_lights * 24u);
  rt_lighting_segments_host(&L, sample, light, out_rays, out_length, out_mag, out_dot, out_skip);
  return RT_OK;
}

// (the arguments first: they are judged without a scene, and before a device is touched)
extern "C" int rt_scene_lighting_device(rt_scene_dev *s, const struct rt_lighting *a, const double *d_offs, uint64_t n, const rt_hit *d_hits,
                                        const uint32_t *d_order, const rt_lighting_outputs *d_out, void *hip_stream, rt_stats *stats) {
  const char *what = "rt_scene_lighting_device";
  int rc = lighting_check(a, what);
  if (rc) return rc;
  if ((rc = receiver_count_check(n, what))) return rc;
  if ((rc = lighting_offs_check(*a, d_offs, what))) return rc;
  if (!d_hits || ((uintptr_t)d_hits & 7u)) return fail(RT_ERR_INVALID, "%s: NULL or misaligned hit records (8 bytes)", what);
  if ((rc = lighting_outputs_check(d_out, what))) return rc;
  if ((uintptr_t)d_order & 3u) return fail(RT_ERR_INVALID, "%s: misaligned order (4 bytes)", what);
  if (!s) return fail(RT_ERR_STATE, "%s: NULL scene handle", what);
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return lighting_launch(s, *a, d_offs, (uint32_t)n, d_hits, d_order, *d_out, stream, stats);
}

extern "C" int rt_lighting(const void *blob, size_t bytes, const struct rt_lighting *a, const double *offs, uint64_t n, const rt_hit *hits,
                           const rt_lighting_outputs *ho, rt_stats *stats) {
  const char *what = "rt_lighting";
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = lighting_table_check(a, offs, what))) return rc;
  if (n == 0) return fail(RT_ERR_INVALID, "%s: n is 0", what);
  if (!hits) return fail(RT_ERR_INVALID, "%s: NULL hit records", what);
  if ((rc = lighting_outputs_check(ho, what))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  device_mem d_offs;                 // the table (released behind the call, whose every chunk has been waited for)
  if ((rc = upload_offs(*a, offs, &d_offs, call.stream))) return rc;
  chunk_row rows[5] = {row_in(hits, sizeof(rt_hit))};
  output_rows(*ho, 1u, rows + 1);
  return chunked_list_call(call, n, rows, 5, false, stats, [&](uint32_t m, uint64_t at, void *const *d, const uint32_t *, rt_stats *st) {
    struct rt_lighting ac = *a;
    ac.base = a->base + at;          // receiver `at + i` of the list is receiver i of this chunk
    return lighting_launch(call.s, ac, (const double *)d_offs.h, m, (const rt_hit *)d[0], nullptr, device_outputs(d + 1), call.stream, st);
  });
}

extern "C" size_t rt_lighting_view_work_bytes(uint32_t w, uint32_t h) {
  // the whole view in one band, as rt_ambient_view_work_bytes
  return view_size_ok(w, h) ? (size_t)w * h * RT_LIGHTING_VIEW_BAND_BYTES : 0;
}

extern "C" int rt_scene_lighting_view_device(rt_scene_dev *s, const rt_view *v, uint32_t w, uint32_t h, const struct rt_lighting *a, const double *d_offs,
                                             const rt_lighting_outputs *d_out, void *d_work, size_t work_bytes, void *hip_stream, rt_stats *stats) {
  const char *what = "rt_scene_lighting_view_device";
  if (!s) return fail(RT_ERR_STATE, "%s: NULL scene handle", what);
  int rc = rt_view_validate(v, w, h);
  if (rc) return rc;
  if ((rc = lighting_check(a, what))) return rc;
  if ((rc = lighting_offs_check(*a, d_offs, what))) return rc;
  if ((rc = lighting_outputs_check(d_out, what))) return rc;
  uint32_t band_rows = 0;
  if ((rc = view_work_check(d_work, work_bytes, w, h, RT_LIGHTING_VIEW_BAND_BYTES, "a band", what, &band_rows))) return rc;
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return timed(stream, stats, (uint64_t)w * h, [&] { return lighting_view_bands(s, v, w, h, *a, d_offs, 0u, h, band_rows, *d_out, 0u, d_work, stream); });
}

extern "C" int rt_lighting_view(const void *blob, size_t bytes, const rt_view *v, uint32_t w, uint32_t h, const struct rt_lighting *a, const double *offs,
                                const rt_lighting_outputs *ho, rt_stats *stats) {
  const char *what = "rt_lighting_view";
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = rt_view_validate(v, w, h))) return rc;
  if ((rc = lighting_table_check(a, offs, what))) return rc;
  if ((rc = lighting_outputs_check(ho, what))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  device_mem d_offs;                 // the table
  device_bufs<2> tables;             // the panorama's
  rt_view dv;
  if ((rc = upload_offs(*a, offs, &d_offs, call.stream))) return rc;
  if ((rc = view_upload_tables(*v, w, h, 1u, call.stream, &tables, &dv))) return rc;
  chunk_row rows[5] = {row_scratch((size_t)w * RT_LIGHTING_VIEW_BAND_BYTES)};
  output_rows(*ho, w, rows + 1);
  return chunked_view_call(call, w, h, rows, 5, stats, [&](uint32_t y, uint32_t m, void *const *d) {
    return lighting_view_bands(call.s, &dv, w, h, *a, (const double *)d_offs.h, y, y + m, m, device_outputs(d + 1), y, d[0], call.stream);
  });
}
