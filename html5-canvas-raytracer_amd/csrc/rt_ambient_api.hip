// rt_ambient_api.hip — ambient occlusion (include/rt_hip.h: rt_ambient): the host logic (validation, the cosine table, the host probe),
// the launches of rt_ambient.hip's two kernels, and the host forms: a list of receivers through device buffers in chunks, and a whole
// view whose rays, hit records and scans never leave the device (the chunk driver, the prologue and the band loop are the ones every
// host form shares: rt_api_internal.h).  The fused kernel reads the scene's current spheres and epsilon and nothing else of it, so its
// launch is rt_scene_occlusion_device's: behind the scene's preparation (enter_launch), on any stream.
#include "rt_api_internal.h"
#include "rt_ambient.h"

static_assert(sizeof(struct rt_ambient) == 32 && sizeof(rt_hit) == 80, "an ambient description travels as 32 bytes, a receiver is 80");

namespace {
int ambient_check(const struct rt_ambient *a, const char *what) {
  if (!a) return fail(RT_ERR_INVALID, "%s: NULL ambient description", what);
  if (a->n_samples < 1u || a->n_samples > RT_AMBIENT_MAX_SAMPLES) return fail(RT_ERR_INVALID, "%s: n_samples %u not in 1..%u", what, a->n_samples, RT_AMBIENT_MAX_SAMPLES);
  if (a->n_dirs < a->n_samples || a->n_dirs > RT_AMBIENT_MAX_DIRS)
    return fail(RT_ERR_INVALID, "%s: n_dirs %u not in n_samples..%u", what, a->n_dirs, RT_AMBIENT_MAX_DIRS);
  if (a->reserved != 0u) return fail(RT_ERR_INVALID, "%s: reserved %u not 0", what, a->reserved);
  if (!(a->radius > 0.0)) return fail(RT_ERR_INVALID, "%s: radius %g not above 0", what, a->radius);
  return RT_OK;
}

// ... and a table in HOST memory
int ambient_table_check(const struct rt_ambient *a, const double *dirs, const char *what) {
  if (int rc = ambient_check(a, what)) return rc;
  if (!dirs) return fail(RT_ERR_INVALID, "%s: NULL direction table", what);
  for (uint32_t e = 0; e < a->n_dirs; e++)
    if (!std::isfinite(dirs[3u * (size_t)e]) || !std::isfinite(dirs[3u * (size_t)e + 1u]) || !std::isfinite(dirs[3u * (size_t)e + 2u]))
      return fail(RT_ERR_INVALID, "%s: direction %u has a non-finite component", what, e);
  return RT_OK;
}

int ambient_outputs_check(const rt_ambient_outputs *out, const char *what) {
  if (!out) return fail(RT_ERR_INVALID, "%s: NULL outputs", what);
  if (!out->open && !out->intensity && !out->rgba) return fail(RT_ERR_INVALID, "%s: every output is NULL", what);
  if (((uintptr_t)out->open & 7u) || ((uintptr_t)out->intensity & 7u) || ((uintptr_t)out->rgba & 3u))
    return fail(RT_ERR_INVALID, "%s: misaligned output (open and intensity need 8 bytes, rgba 4)", what);
  return RT_OK;
}

int ambient_inputs_check(const double *dirs, const rt_hit *hits, const char *what) {
  if (!dirs || !hits) return fail(RT_ERR_INVALID, "%s: NULL direction table or hit records", what);
  if (((uintptr_t)dirs & 7u) || ((uintptr_t)hits & 7u)) return fail(RT_ERR_INVALID, "%s: misaligned direction table or hit records (8 bytes)", what);
  return RT_OK;
}

rt_ambient_launch launch_of(const struct rt_ambient &a, const double *dirs, uint32_t n, const rt_hit *hits) {
  rt_ambient_launch L;
  memset(&L, 0, sizeof L);
  L.hits = hits; L.dirs = dirs; L.n = n;
  L.base = a.base; L.radius = a.radius;
  L.n_samples = a.n_samples; L.n_dirs = a.n_dirs; L.stride = a.stride;
  return L;
}

// the fused kernel for receivers [0, n) of d_hits with the description's base as given
int ambient_launch(rt_scene_dev *s, const struct rt_ambient &a, const double *d_dirs, uint32_t n, const rt_hit *d_hits, const uint32_t *d_order,
                   const rt_ambient_outputs &out, hipStream_t stream, rt_stats *stats) {
  stats_clock clock;
  rt_ambient_launch L = launch_of(a, d_dirs, n, d_hits);
  {
    std::lock_guard<std::mutex> lk(s->launch_mu);
    if (int rc = enter_launch(s, stream)) return rc;
    L.objects = (const rt_sphere *)(obj_block(s) + s->o_objs);   // this generation's spheres, in blob order
  }
  L.epsilon = s->hd.epsilon;
  L.n_objects = s->hd.n_objects;
  L.order = d_order;
  L.open = out.open; L.intensity = out.intensity; L.rgba = out.rgba;
  if (int rc = clock.start(stats, stream)) return rc;
  const int err = rt_launch_ambient(&L, (void *)stream);
  if (err != 0) return fail(RT_ERR_DEVICE, "ambient kernel launch: %s", hipGetErrorString((hipError_t)err));
  return clock.finish(stats, n);
}

constexpr uint32_t RT_AMBIENT_VIEW_BAND_BYTES = 128u;     // per pixel of a band: the ray 48, its hit record 80

// The view's rows [row0, row_end) in bands of at most band_rows: per band the rays (rt_views.hip), their hit records (rt_hits.hip) and the
// fused kernel with base = a.base + y * w, so that pixel i = y * w + x is receiver i whatever the band.  The outputs' first record is
// pixel out_row0 * w.  One stream: every launch comes behind the one that wrote what it reads.  (The view was checked by the caller.)
int ambient_view_bands(rt_scene_dev *s, const rt_view *v, uint32_t w, uint32_t h, const struct rt_ambient &a, const double *d_dirs, uint32_t row0,
                       uint32_t row_end, uint32_t band_rows, const rt_ambient_outputs &out, uint32_t out_row0, void *d_work, hipStream_t stream) {
  double *rays = (double *)d_work;
  rt_hit *hits = (rt_hit *)(rays + 6u * ((size_t)band_rows * w));
  return for_bands(row0, row_end, band_rows, [&](uint32_t y, uint32_t m) {
    if (int rc = view_band_hits(s, v, w, h, y, m, rays, hits, stream)) return rc;
    struct rt_ambient ab = a;
    ab.base = a.base + (uint64_t)y * w;
    const size_t at = (size_t)(y - out_row0) * w;
    const rt_ambient_outputs band = {out.open ? out.open + at : nullptr, out.intensity ? out.intensity + at : nullptr, out.rgba ? out.rgba + at : nullptr};
    return ambient_launch(s, ab, d_dirs, m * w, hits, nullptr, band, stream, nullptr);
  });
}

// the table of a host form in device memory
int upload_dirs(const struct rt_ambient &a, const double *dirs, device_mem *d_dirs, hipStream_t stream) {
  HIP_TRY(hipMalloc(&d_dirs->h, (size_t)a.n_dirs * 24u));
  HIP_TRY(hipMemcpyAsync(d_dirs->h, dirs, (size_t)a.n_dirs * 24u, hipMemcpyHostToDevice, stream));
  return RT_OK;
}

// the outputs of a host form as the rows of a chunked call: `each` records per unit (a list: 1, a view: w), and a chunk's on the device
void output_rows(const rt_ambient_outputs &ho, size_t each, chunk_row *rows) {
  rows[0] = row_out(ho.open, each * 8u); rows[1] = row_out(ho.intensity, each * 8u); rows[2] = row_out(ho.rgba, each * 4u);
}
rt_ambient_outputs device_outputs(void *const *d) { return rt_ambient_outputs{(double *)d[0], (double *)d[1], (uint32_t *)d[2]}; }
}  // namespace

int rt_api::receiver_count_check(uint64_t n, const char *what) {
  return (n == 0 || n >= (1ull << 31)) ? fail(RT_ERR_INVALID, "%s: n %llu not in 1..2^31 - 1", what, (unsigned long long)n) : RT_OK;
}

extern "C" int rt_ambient_validate(const struct rt_ambient *a, const double *dirs) { return ambient_table_check(a, dirs, "rt_ambient_validate"); }

extern "C" int rt_ambient_cosine_dirs(uint32_t n, double *out_3n) {
  if (n < 1u || n > RT_AMBIENT_MAX_DIRS || !out_3n) return fail(RT_ERR_INVALID, "rt_ambient_cosine_dirs: n %u not in 1..%u, or a NULL output", n, RT_AMBIENT_MAX_DIRS);
  rt_ambient_cosine_dirs_host(n, out_3n);
  return RT_OK;
}

extern "C" int rt_ambient_segments(const struct rt_ambient *a, const double *dirs, uint64_t n, const rt_hit *hits, uint32_t sample, double *out_rays,
                                   int32_t *out_skip) {
  const char *what = "rt_ambient_segments";
  int rc = ambient_table_check(a, dirs, what);
  if (rc) return rc;
  if ((rc = receiver_count_check(n, what))) return rc;
  if (sample >= a->n_samples) return fail(RT_ERR_INVALID, "%s: sample %u not below n_samples %u", what, sample, a->n_samples);
  if (!hits || !out_rays) return fail(RT_ERR_INVALID, "%s: NULL hit records or ray output", what);
  rt_ambient_launch L = launch_of(*a, dirs, (uint32_t)n, hits);
  L.sample = sample; L.rays = out_rays; L.skip = out_skip;
  rt_ambient_segments_host(&L);
  return RT_OK;
}

extern "C" int rt_ambient_segments_device(int device, const struct rt_ambient *a, const double *d_dirs, uint64_t n, const rt_hit *d_hits, uint32_t sample,
                                          double *d_rays, int32_t *d_skip, void *hip_stream) {
  const char *what = "rt_ambient_segments_device";
  int rc = ambient_check(a, what);
  if (rc) return rc;
  if ((rc = receiver_count_check(n, what))) return rc;
  if (sample >= a->n_samples) return fail(RT_ERR_INVALID, "%s: sample %u not below n_samples %u", what, sample, a->n_samples);
  if ((rc = ambient_inputs_check(d_dirs, d_hits, what))) return rc;
  if (!d_rays || ((uintptr_t)d_rays & 15u)) return fail(RT_ERR_INVALID, "%s: NULL or misaligned ray list (16 bytes)", what);
  if ((uintptr_t)d_skip & 3u) return fail(RT_ERR_INVALID, "%s: misaligned skip (4 bytes)", what);
  hipStream_t stream = nullptr;
  if ((rc = device_stream(device, hip_stream, &stream))) return rc;
  rt_ambient_launch L = launch_of(*a, d_dirs, (uint32_t)n, d_hits);
  L.sample = sample; L.rays = d_rays; L.skip = d_skip;
  const int err = rt_launch_ambient_segments(&L, (void *)stream);
  if (err != 0) return fail(RT_ERR_DEVICE, "ambient segment generator launch: %s", hipGetErrorString((hipError_t)err));
  return RT_OK;
}

// (the arguments first: they are judged without a scene, and before a device is touched)
extern "C" int rt_scene_ambient_device(rt_scene_dev *s, const struct rt_ambient *a, const double *d_dirs, uint64_t n, const rt_hit *d_hits,
                                       const uint32_t *d_order, const rt_ambient_outputs *d_out, void *hip_stream, rt_stats *stats) {
  const char *what = "rt_scene_ambient_device";
  int rc = ambient_check(a, what);
  if (rc) return rc;
  if ((rc = receiver_count_check(n, what))) return rc;
  if ((rc = ambient_inputs_check(d_dirs, d_hits, what))) return rc;
  if ((rc = ambient_outputs_check(d_out, what))) return rc;
  if ((uintptr_t)d_order & 3u) return fail(RT_ERR_INVALID, "%s: misaligned order (4 bytes)", what);
  if (!s) return fail(RT_ERR_STATE, "%s: NULL scene handle", what);
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return ambient_launch(s, *a, d_dirs, (uint32_t)n, d_hits, d_order, *d_out, stream, stats);
}

extern "C" int rt_ambient(const void *blob, size_t bytes, const struct rt_ambient *a, const double *dirs, uint64_t n, const rt_hit *hits,
                          const rt_ambient_outputs *ho, rt_stats *stats) {
  const char *what = "rt_ambient";
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = ambient_table_check(a, dirs, what))) return rc;
  if (n == 0) return fail(RT_ERR_INVALID, "%s: n is 0", what);
  if (!hits) return fail(RT_ERR_INVALID, "%s: NULL hit records", what);
  if ((rc = ambient_outputs_check(ho, what))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  device_mem d_dirs;                 // the table (released behind the call, whose every chunk has been waited for)
  if ((rc = upload_dirs(*a, dirs, &d_dirs, call.stream))) return rc;
  chunk_row rows[4] = {row_in(hits, sizeof(rt_hit))};
  output_rows(*ho, 1u, rows + 1);
  return chunked_list_call(call, n, rows, 4, false, stats, [&](uint32_t m, uint64_t at, void *const *d, const uint32_t *, rt_stats *st) {
    struct rt_ambient ac = *a;
    ac.base = a->base + at;          // receiver `at + i` of the list is receiver i of this chunk
    return ambient_launch(call.s, ac, (const double *)d_dirs.h, m, (const rt_hit *)d[0], nullptr, device_outputs(d + 1), call.stream, st);
  });
}

extern "C" size_t rt_ambient_view_work_bytes(uint32_t w, uint32_t h) {
  // the whole view in one band, as rt_view_work_bytes and for its reason: small launches are dear
  return view_size_ok(w, h) ? (size_t)w * h * RT_AMBIENT_VIEW_BAND_BYTES : 0;
}

extern "C" int rt_scene_ambient_view_device(rt_scene_dev *s, const rt_view *v, uint32_t w, uint32_t h, const struct rt_ambient *a, const double *d_dirs,
                                            const rt_ambient_outputs *d_out, void *d_work, size_t work_bytes, void *hip_stream, rt_stats *stats) {
  const char *what = "rt_scene_ambient_view_device";
  if (!s) return fail(RT_ERR_STATE, "%s: NULL scene handle", what);
  int rc = rt_view_validate(v, w, h);
  if (rc) return rc;
  if ((rc = ambient_check(a, what))) return rc;
  if (!d_dirs || ((uintptr_t)d_dirs & 7u)) return fail(RT_ERR_INVALID, "%s: NULL or misaligned direction table (8 bytes)", what);
  if ((rc = ambient_outputs_check(d_out, what))) return rc;
  uint32_t band_rows = 0;
  if ((rc = view_work_check(d_work, work_bytes, w, h, RT_AMBIENT_VIEW_BAND_BYTES, "a band", what, &band_rows))) return rc;
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return timed(stream, stats, (uint64_t)w * h, [&] { return ambient_view_bands(s, v, w, h, *a, d_dirs, 0u, h, band_rows, *d_out, 0u, d_work, stream); });
}

extern "C" int rt_ambient_view(const void *blob, size_t bytes, const rt_view *v, uint32_t w, uint32_t h, const struct rt_ambient *a, const double *dirs,
                               const rt_ambient_outputs *ho, rt_stats *stats) {
  const char *what = "rt_ambient_view";
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = rt_view_validate(v, w, h))) return rc;
  if ((rc = ambient_table_check(a, dirs, what))) return rc;
  if ((rc = ambient_outputs_check(ho, what))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  device_mem d_dirs;                 // the table
  device_bufs<2> tables;             // the panorama's
  rt_view dv;
  if ((rc = upload_dirs(*a, dirs, &d_dirs, call.stream))) return rc;
  if ((rc = view_upload_tables(*v, w, h, 1u, call.stream, &tables, &dv))) return rc;
  chunk_row rows[4] = {row_scratch((size_t)w * RT_AMBIENT_VIEW_BAND_BYTES)};
  output_rows(*ho, w, rows + 1);
  return chunked_view_call(call, w, h, rows, 4, stats, [&](uint32_t y, uint32_t m, void *const *d) {
    return ambient_view_bands(call.s, &dv, w, h, *a, (const double *)d_dirs.h, y, y + m, m, device_outputs(d + 1), y, d[0], call.stream);
  });
}
