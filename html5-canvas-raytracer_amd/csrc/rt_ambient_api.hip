// rt_ambient_api.hip — ambient occlusion (include/rt_hip.h: rt_ambient): the host logic (validation, the cosine table, the host probe),
// the launches of rt_ambient.hip's two kernels, and the host forms: a list of receivers through device buffers in chunks, and a whole
// view whose rays, hit records and scans never leave the device.  The fused kernel reads the scene's current spheres and epsilon and
// nothing else of it, so its launch is rt_scene_occlusion_device's: behind the scene's preparation (enter_launch), on any stream.
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

int ambient_count_check(uint64_t n, const char *what) {
  return (n == 0 || n >= (1ull << 31)) ? fail(RT_ERR_INVALID, "%s: n %llu not in 1..2^31 - 1", what, (unsigned long long)n) : RT_OK;
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

bool ambient_view_size_ok(uint32_t w, uint32_t h) { return w != 0 && h != 0 && (uint64_t)w * h < (1ull << 31); }

// The view's rows [row0, row_end) in bands of at most band_rows: per band the rays (rt_views.hip), their hit records (rt_hits.hip) and the
// fused kernel with base = a.base + y * w, so that pixel i = y * w + x is receiver i whatever the band.  The outputs' first record is
// pixel out_row0 * w.  One stream: every launch comes behind the one that wrote what it reads.  (The view was checked by the caller.)
int ambient_view_bands(rt_scene_dev *s, const rt_view *v, uint32_t w, uint32_t h, const struct rt_ambient &a, const double *d_dirs, uint32_t row0,
                       uint32_t row_end, uint32_t band_rows, const rt_ambient_outputs &out, uint32_t out_row0, void *d_work, hipStream_t stream) {
  double *rays = (double *)d_work;
  rt_hit *hits = (rt_hit *)(rays + 6u * ((size_t)band_rows * w));
  for (uint32_t y = row0; y < row_end; y += band_rows) {
    const uint32_t m = row_end - y < band_rows ? row_end - y : band_rows;
    if (int rc = rt_view_rays_device(s->device, v, w, h, y, m, rays, (void *)stream)) return rc;
    const rt_ray_outputs into = {nullptr, nullptr, hits};
    if (int rc = trace_rays_launch(s, m * w, y * w, rays, nullptr, 1u, into, stream, nullptr)) return rc;
    struct rt_ambient ab = a;
    ab.base = a.base + (uint64_t)y * w;
    const size_t at = (size_t)(y - out_row0) * w;
    const rt_ambient_outputs band = {out.open ? out.open + at : nullptr, out.intensity ? out.intensity + at : nullptr, out.rgba ? out.rgba + at : nullptr};
    if (int rc = ambient_launch(s, ab, d_dirs, m * w, hits, nullptr, band, stream, nullptr)) return rc;
  }
  return RT_OK;
}

// the outputs of one chunk in device memory, and their way back
struct chunk_outputs {
  device_mem open, intensity, rgba;
  int alloc(const rt_ambient_outputs &ho, size_t chunk) {
    if (ho.open) HIP_TRY(hipMalloc(&open.h, chunk * 8u));
    if (ho.intensity) HIP_TRY(hipMalloc(&intensity.h, chunk * 8u));
    if (ho.rgba) HIP_TRY(hipMalloc(&rgba.h, chunk * 4u));
    return RT_OK;
  }
  rt_ambient_outputs dev() const { return rt_ambient_outputs{(double *)open.h, (double *)intensity.h, (uint32_t *)rgba.h}; }
  int copy_back(const rt_ambient_outputs &ho, size_t at, size_t n, hipStream_t stream) {
    if (ho.open) HIP_TRY(hipMemcpyAsync(ho.open + at, open.h, n * 8u, hipMemcpyDeviceToHost, stream));
    if (ho.intensity) HIP_TRY(hipMemcpyAsync(ho.intensity + at, intensity.h, n * 8u, hipMemcpyDeviceToHost, stream));
    if (ho.rgba) HIP_TRY(hipMemcpyAsync(ho.rgba + at, rgba.h, n * 4u, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return RT_OK;
  }
};
}  // namespace

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
  if ((rc = ambient_count_check(n, what))) return rc;
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
  if ((rc = ambient_count_check(n, what))) return rc;
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
  if ((rc = ambient_count_check(n, what))) return rc;
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
  if (!G.inited) return fail(RT_ERR_STATE, "rt_init has not been called");
  std::lock_guard<std::mutex> lk(G.mu);
  stats_clock clock;
  rt_scene_dev *s = nullptr;
  if ((rc = resident_scene(0, blob, bytes, &s))) return rc;
  if ((rc = ensure_device(0))) return rc;
  hipStream_t stream = G.dev[0].stream;
  const size_t chunk = n < RT_AMBIENT_CHUNK ? (size_t)n : (size_t)RT_AMBIENT_CHUNK;
  device_mem d_hits, d_dirs;         // of one chunk; the table (released on every way out)
  chunk_outputs d_out;
  HIP_TRY(hipMalloc(&d_hits.h, chunk * sizeof(rt_hit)));
  HIP_TRY(hipMalloc(&d_dirs.h, (size_t)a->n_dirs * 24u));
  if ((rc = d_out.alloc(*ho, chunk))) return rc;
  HIP_TRY(hipMemcpyAsync(d_dirs.h, dirs, (size_t)a->n_dirs * 24u, hipMemcpyHostToDevice, stream));
  double kernel_ms = 0.0;
  for (uint64_t at = 0; at < n; at += RT_AMBIENT_CHUNK) {
    const size_t m = n - at < RT_AMBIENT_CHUNK ? (size_t)(n - at) : (size_t)RT_AMBIENT_CHUNK;
    HIP_TRY(hipMemcpyAsync(d_hits.h, hits + at, m * sizeof(rt_hit), hipMemcpyHostToDevice, stream));
    struct rt_ambient ac = *a;
    ac.base = a->base + at;          // receiver `at + i` of the list is receiver i of this chunk
    rt_stats st;
    if ((rc = ambient_launch(s, ac, (const double *)d_dirs.h, (uint32_t)m, (const rt_hit *)d_hits.h, nullptr, d_out.dev(), stream, stats ? &st : nullptr))) return rc;
    if (stats) kernel_ms += st.kernel_ms;
    if ((rc = d_out.copy_back(*ho, (size_t)at, m, stream))) return rc;
  }
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->kernel_ms = kernel_ms;
    stats->pixels = n;
    stats->total_ms = clock.host_ms();
  }
  return RT_OK;
}

extern "C" size_t rt_ambient_view_work_bytes(uint32_t w, uint32_t h) {
  // the whole view in one band, as rt_view_work_bytes and for its reason: small launches are dear
  return ambient_view_size_ok(w, h) ? (size_t)w * h * RT_AMBIENT_VIEW_BAND_BYTES : 0;
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
  if (!d_work || ((uintptr_t)d_work & 15u)) return fail(RT_ERR_INVALID, "%s: NULL or misaligned workspace (16 bytes)", what);
  const uint64_t row_bytes = (uint64_t)w * RT_AMBIENT_VIEW_BAND_BYTES;
  if (work_bytes < row_bytes) return fail(RT_ERR_INVALID, "%s: work_bytes %llu below one row of a band, %llu", what, (unsigned long long)work_bytes, (unsigned long long)row_bytes);
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  const uint64_t fit = work_bytes / row_bytes;
  const uint32_t band_rows = fit < h ? (uint32_t)fit : h;
  stats_clock clock;
  if ((rc = clock.start(stats, stream))) return rc;
  if ((rc = ambient_view_bands(s, v, w, h, *a, d_dirs, 0u, h, band_rows, *d_out, 0u, d_work, stream))) return rc;
  return clock.finish(stats, (uint64_t)w * h);
}

extern "C" int rt_ambient_view(const void *blob, size_t bytes, const rt_view *v, uint32_t w, uint32_t h, const struct rt_ambient *a, const double *dirs,
                               const rt_ambient_outputs *ho, rt_stats *stats) {
  const char *what = "rt_ambient_view";
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = rt_view_validate(v, w, h))) return rc;
  if ((rc = ambient_table_check(a, dirs, what))) return rc;
  if ((rc = ambient_outputs_check(ho, what))) return rc;
  if (!G.inited) return fail(RT_ERR_STATE, "rt_init has not been called");
  std::lock_guard<std::mutex> lk(G.mu);
  stats_clock clock;
  rt_scene_dev *s = nullptr;
  if ((rc = resident_scene(0, blob, bytes, &s))) return rc;
  if ((rc = ensure_device(0))) return rc;
  hipStream_t stream = G.dev[0].stream;
  // chunks of whole rows of at most RT_AMBIENT_CHUNK pixels; a longer row is its own chunk
  uint64_t chunk_rows = RT_AMBIENT_CHUNK / w;
  if (chunk_rows < 1u) chunk_rows = 1u;
  if (chunk_rows > h) chunk_rows = h;
  const size_t chunk = (size_t)chunk_rows * w;
  device_mem d_work, d_dirs, d_lon, d_lat;      // of one chunk; the table; the panorama's tables (released on every way out)
  chunk_outputs d_out;
  HIP_TRY(hipMalloc(&d_work.h, chunk * RT_AMBIENT_VIEW_BAND_BYTES));
  HIP_TRY(hipMalloc(&d_dirs.h, (size_t)a->n_dirs * 24u));
  if ((rc = d_out.alloc(*ho, chunk))) return rc;
  HIP_TRY(hipMemcpyAsync(d_dirs.h, dirs, (size_t)a->n_dirs * 24u, hipMemcpyHostToDevice, stream));
  rt_view dv = *v;
  if (v->model == RT_VIEW_EQUIRECT) {
    HIP_TRY(hipMalloc(&d_lon.h, (size_t)w * 16u));
    HIP_TRY(hipMalloc(&d_lat.h, (size_t)h * 16u));
    HIP_TRY(hipMemcpyAsync(d_lon.h, v->lon, (size_t)w * 16u, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_lat.h, v->lat, (size_t)h * 16u, hipMemcpyHostToDevice, stream));
    dv.lon = (const double *)d_lon.h; dv.lat = (const double *)d_lat.h;
  }
  double kernel_ms = 0.0;
  for (uint32_t y = 0; y < h; y += (uint32_t)chunk_rows) {
    const uint32_t m = h - y < chunk_rows ? h - y : (uint32_t)chunk_rows;
    stats_clock step;
    rt_stats st;
    if ((rc = step.start(stats, stream))) return rc;
    if ((rc = ambient_view_bands(s, &dv, w, h, *a, (const double *)d_dirs.h, y, y + m, m, d_out.dev(), y, d_work.h, stream))) return rc;
    if ((rc = step.finish(stats ? &st : nullptr, (uint64_t)m * w))) return rc;
    if (stats) kernel_ms += st.kernel_ms;
    if ((rc = d_out.copy_back(*ho, (size_t)y * w, (size_t)m * w, stream))) return rc;
  }
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->kernel_ms = kernel_ms;
    stats->pixels = (uint64_t)w * h;
    stats->total_ms = clock.host_ms();
  }
  return RT_OK;
}
