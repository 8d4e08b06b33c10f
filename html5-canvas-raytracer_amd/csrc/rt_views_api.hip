// rt_views_api.hip — views (include/rt_hip.h: rt_view): the host logic (validation, the panorama's tables, the host probe), the
// generator's launch (rt_views.hip) and the two traces of a whole view.  A view is traced in bands of whole rows: each band is
// generated into the caller's workspace and handed to the launch of a caller's ray list (rt_launch.hip: trace_rays_launch) with its
// base, so ray i = y * w + x keeps pix = i and no trace kernel knows that the list was made here.  The generator reads nothing of a
// scene: rt_view_rays_device waits for no edit and takes no part in rt_scene_sync.h; the trace launch behind it waits as it always does.
// Sampled views (rt_view_sample, rt_view_lens; rt_view_samples.h / .hip) run the same band loop with n generate-and-trace steps per
// band, an accumulator and a resolve: the second half of this file.  The host forms are rows and a step for chunked_view_call
// (rt_api_internal.h): a chunk is whole rows of at most RT_RAY_CHUNK pixels, and the band workspace is the chunk's scratch.
#include "rt_api_internal.h"
#include "rt_views.h"
#include "rt_view_samples.h"

static_assert(sizeof(rt_view_sample) == 32 && sizeof(rt_view_lens) == 16 && sizeof(rt_view_sample_params) == 48, "a sample travels as 32 bytes, with its lens as 48");
static_assert(RT_VIEWS_REFERENCE == RT_VIEW_REFERENCE && RT_VIEWS_PINHOLE == RT_VIEW_PINHOLE && RT_VIEWS_ORTHO == RT_VIEW_ORTHO &&
              RT_VIEWS_EQUIRECT == RT_VIEW_EQUIRECT, "rt_views.h restates the models of include/rt_hip.h");

// what every unit that traces a view shares (rt_api_internal.h)
namespace rt_api {
bool view_size_ok(uint32_t w, uint32_t h) { return w != 0 && h != 0 && (uint64_t)w * h < (1ull << 31); }

int view_work_check(const void *d_work, size_t work_bytes, uint32_t w, uint32_t h, uint32_t pixel_bytes, const char *noun, const char *what, uint32_t *band_rows) {
  if (!d_work || ((uintptr_t)d_work & 15u)) return fail(RT_ERR_INVALID, "%s: NULL or misaligned workspace (16 bytes)", what);
  const uint64_t row_bytes = (uint64_t)w * pixel_bytes;
  if (work_bytes < row_bytes) return fail(RT_ERR_INVALID, "%s: work_bytes %llu below one row of %s, %llu", what, (unsigned long long)work_bytes, noun, (unsigned long long)row_bytes);
  const uint64_t fit = work_bytes / row_bytes;
  *band_rows = fit < h ? (uint32_t)fit : h;
  return RT_OK;
}

int view_upload_tables(const rt_view &v, uint32_t w, uint32_t h, uint32_t n_tables, hipStream_t stream, device_bufs<2> *mem, rt_view *dv) {
  *dv = v;
  if (v.model != RT_VIEW_EQUIRECT) return RT_OK;
  const size_t lon_bytes = (size_t)w * 16u * n_tables, lat_bytes = (size_t)h * 16u * n_tables;
  HIP_TRY(hipMalloc(&mem->p[0], lon_bytes));
  HIP_TRY(hipMalloc(&mem->p[1], lat_bytes));
  HIP_TRY(hipMemcpyAsync(mem->p[0], v.lon, lon_bytes, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(mem->p[1], v.lat, lat_bytes, hipMemcpyHostToDevice, stream));
  dv->lon = (const double *)mem->p[0]; dv->lat = (const double *)mem->p[1];
  return RT_OK;
}

int view_band_hits(rt_scene_dev *s, const rt_view *v, uint32_t w, uint32_t h, uint32_t y, uint32_t m, double *d_rays, rt_hit *d_hits, hipStream_t stream) {
  if (int rc = rt_view_rays_device(s->device, v, w, h, y, m, d_rays, (void *)stream)) return rc;
  const rt_ray_outputs into = {nullptr, nullptr, d_hits};
  return trace_rays_launch(s, m * w, y * w, d_rays, nullptr, 1u, into, stream, nullptr);
}
}  // namespace rt_api

namespace {
bool finite3(const double *a) { return std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]); }

int view_check(const rt_view *v, uint32_t w, uint32_t h, const char *what) {
  if (!v) return fail(RT_ERR_INVALID, "%s: NULL view", what);
  if (v->model > RT_VIEW_EQUIRECT || v->reserved != 0) return fail(RT_ERR_INVALID, "%s: unknown model %u or reserved %u not 0", what, v->model, v->reserved);
  if (!view_size_ok(w, h)) return fail(RT_ERR_INVALID, "%s: view size %ux%u: w and h must be at least 1 and w * h below 2^31", what, w, h);
  if (!finite3(v->origin) || !finite3(v->axis_x) || !finite3(v->axis_y) || !finite3(v->axis_z))
    return fail(RT_ERR_INVALID, "%s: a non-finite origin or axis component", what);
  if ((v->model == RT_VIEW_REFERENCE || v->model == RT_VIEW_PINHOLE) && !(v->fov_deg > 0.0 && v->fov_deg < 180.0))
    return fail(RT_ERR_INVALID, "%s: fov_deg %g not in (0, 180)", what, v->fov_deg);
  if (v->model == RT_VIEW_ORTHO && !(std::isfinite(v->scale) && v->scale > 0.0)) return fail(RT_ERR_INVALID, "%s: scale %g not finite and above 0", what, v->scale);
  if (v->model == RT_VIEW_EQUIRECT && (!v->lon || !v->lat || (((uintptr_t)v->lon | (uintptr_t)v->lat) & 15u)))
    return fail(RT_ERR_INVALID, "%s: NULL or misaligned panorama tables (16 bytes)", what);
  return RT_OK;
}

int view_rows_check(uint32_t h, uint32_t first_row, uint32_t rows, const char *what) {
  if ((uint64_t)first_row + rows > h) return fail(RT_ERR_INVALID, "%s: rows %u..%llu leave the view's %u", what, first_row, (unsigned long long)first_row + rows, h);
  return RT_OK;
}

// what rays_check asks of a list's depth and outputs (rt_launch.hip), for a list the library makes itself
int view_outputs_check(uint32_t segs, const rt_ray_outputs *out, const char *what) {
  if (!out) return fail(RT_ERR_INVALID, "%s: NULL outputs", what);
  if (segs > RT_MAX_SEGS) return fail(RT_ERR_INVALID, "%s: segs %u not in 0..%u (0 = the scene's depth)", what, segs, RT_MAX_SEGS);
  if (!out->rgb && !out->rgba && !out->hits) return fail(RT_ERR_INVALID, "%s: every output is NULL", what);
  if (((uintptr_t)out->rgb & 7u) || ((uintptr_t)out->rgba & 3u) || ((uintptr_t)out->hits & 7u))
    return fail(RT_ERR_INVALID, "%s: misaligned output (rgb and hits need 8 bytes, rgba 4)", what);
  return RT_OK;
}

// a checked view at one frame size, as the generator takes it
rt_view_params view_params(const rt_view &v, uint32_t w, uint32_t h) {
  rt_view_params P;
  memset(&P, 0, sizeof P);
  P.model = v.model; P.w = w; P.h = h;
  P.proj_w = (double)w / 2.0; P.proj_h = (double)h / 2.0;
  if (v.model == RT_VIEW_REFERENCE || v.model == RT_VIEW_PINHOLE) P.proj_d = rt_view_proj_d(v.fov_deg, P.proj_w);
  P.scale = v.scale;
  memcpy(P.o, v.origin, sizeof P.o); memcpy(P.ax, v.axis_x, sizeof P.ax); memcpy(P.ay, v.axis_y, sizeof P.ay); memcpy(P.az, v.axis_z, sizeof P.az);
  if (v.model == RT_VIEW_EQUIRECT) { P.lon = v.lon; P.lat = v.lat; }
  return P;
}

int view_rays_launch(const rt_view_params &P, uint32_t first_row, uint32_t rows, double *d_rays, hipStream_t stream) {
  const int err = rt_launch_view_rays(&P, first_row, rows, d_rays, (void *)stream);
  if (err != 0) return fail(RT_ERR_DEVICE, "view generator launch: %s", hipGetErrorString((hipError_t)err));
  return RT_OK;
}

// The view's rows in bands of at most band_rows: generated into d_work, traced with base = first_row * w into the outputs' records
// from there on.  One stream: a band's generation comes behind the trace that read the workspace before it.
int trace_view_bands(rt_scene_dev *s, const rt_view_params &P, uint32_t row0, uint32_t row_end, uint32_t band_rows, uint32_t segs, const rt_ray_outputs &out,
                     uint32_t out_row0, double *d_work, hipStream_t stream) {
  return for_bands(row0, row_end, band_rows, [&](uint32_t y, uint32_t m) {
    if (int rc = view_rays_launch(P, y, m, d_work, stream)) return rc;
    const size_t at = (size_t)(y - out_row0) * P.w;       // of the band's first record in the outputs
    const rt_ray_outputs band = {out.rgb ? out.rgb + 3u * at : nullptr, out.rgba ? out.rgba + 4u * at : nullptr, out.hits ? out.hits + at : nullptr};
    return trace_rays_launch(s, m * P.w, y * P.w, d_work, nullptr, segs, band, stream, nullptr);
  });
}

// ---- sampled views: sub-pixel offsets and a thin lens (rt_view_samples.h), averaged on the GPU
constexpr uint32_t RT_VIEW_SAMPLE_BAND_BYTES = 96u;      // per pixel of a band: rays 48, one sample's rgb 24, the accumulator 24

int view_samples_check(const rt_view *v, uint32_t w, uint32_t h, const rt_view_lens *lens, uint32_t n, const rt_view_sample *samples, const char *what) {
  if (int rc = view_check(v, w, h, what)) return rc;
  if (n < 1u || n > RT_VIEW_SAMPLES_MAX) return fail(RT_ERR_INVALID, "%s: %u samples not in 1..%u", what, n, RT_VIEW_SAMPLES_MAX);
  if ((uint64_t)n * w * h > (1ull << 32)) return fail(RT_ERR_INVALID, "%s: %u samples of a %ux%u view: n * w * h above 2^32", what, n, w, h);
  if (!samples) return fail(RT_ERR_INVALID, "%s: NULL samples", what);
  for (uint32_t s = 0; s < n; s++)
    if (!std::isfinite(samples[s].dx) || !std::isfinite(samples[s].dy) || !std::isfinite(samples[s].lu) || !std::isfinite(samples[s].lv))
      return fail(RT_ERR_INVALID, "%s: sample %u has a non-finite component", what, s);
  if (lens) {
    if (!(std::isfinite(lens->radius) && lens->radius >= 0.0)) return fail(RT_ERR_INVALID, "%s: lens radius %g negative or not finite", what, lens->radius);
    if (lens->radius > 0.0 && v->model != RT_VIEW_PINHOLE) return fail(RT_ERR_INVALID, "%s: a lens is for RT_VIEW_PINHOLE only (model %u)", what, v->model);
    if (lens->radius > 0.0 && !(std::isfinite(lens->focus) && lens->focus > 0.0)) return fail(RT_ERR_INVALID, "%s: lens focus %g not finite and above 0", what, lens->focus);
  }
  return RT_OK;
}

rt_view_sample_params sample_params(const rt_view_sample &s, const rt_view_lens *lens) {
  const bool on = lens && lens->radius > 0.0;
  return rt_view_sample_params{s.dx, s.dy, s.lu, s.lv, on ? lens->radius : 0.0, on ? lens->focus : 0.0};
}

// the view with the panorama's tables of sample `table` (one table per sample back to back: 2 w and 2 h doubles each)
rt_view_params view_params_of_table(rt_view_params P, uint32_t table) {
  if (P.model == RT_VIEWS_EQUIRECT) { P.lon += 2u * (size_t)P.w * table; P.lat += 2u * (size_t)P.h * table; }
  return P;
}

#define VIEW_LAUNCH(call, name) do { const int err_ = (call); if (err_ != 0) return fail(RT_ERR_DEVICE, name " launch: %s", hipGetErrorString((hipError_t)err_)); } while (0)

// The view's rows in bands of at most band_rows, n samples per pixel.  d_work holds, for band_rows * w pixels, the rays (48 bytes each),
// one sample's rgb (24) and the accumulator (24).  Per band and per sample in order: generate, trace with base = s * w * h + y * w
// (sample 0 straight into the accumulator, the others into the rgb slab), accumulate; the last sample's addition is the resolve's.
// One stream: every launch comes behind the one that wrote what it reads.
int trace_view_sample_bands(rt_scene_dev *s, const rt_view_params &P, const rt_view_lens *lens, uint32_t n, const rt_view_sample *samples, uint32_t row0,
                            uint32_t row_end, uint32_t band_rows, uint32_t segs, const rt_ray_outputs &out, uint32_t out_row0, void *d_work,
                            hipStream_t stream) {
  const size_t band = (size_t)band_rows * P.w;
  double *rays = (double *)d_work, *slab = rays + 6u * band, *acc = slab + 3u * band;
  return for_bands(row0, row_end, band_rows, [&](uint32_t y, uint32_t m) {
    const uint32_t pixels = m * P.w;
    for (uint32_t k = 0; k < n; k++) {
      const rt_view_params Pk = view_params_of_table(P, k);
      const rt_view_sample_params S = sample_params(samples[k], lens);
      VIEW_LAUNCH(rt_launch_view_sample_rays(&Pk, &S, y, m, rays, (void *)stream), "view sample generator");
      const rt_ray_outputs into = {k == 0 ? acc : slab, nullptr, nullptr};
      const uint32_t base = (uint32_t)((uint64_t)k * P.w * P.h + (uint64_t)y * P.w);           // (n * w * h <= 2^32: base + pixels - 1 < 2^32)
      if (int rc = trace_rays_launch(s, pixels, base, rays, nullptr, segs, into, stream, nullptr)) return rc;
      if (k != 0 && k + 1u != n) VIEW_LAUNCH(rt_launch_view_accumulate(acc, slab, pixels, (void *)stream), "view accumulate");
    }
    const size_t at = (size_t)(y - out_row0) * P.w;       // of the band's first pixel in the outputs
    VIEW_LAUNCH(rt_launch_view_resolve(acc, n > 1u ? slab : nullptr, n, pixels, out.rgb ? out.rgb + 3u * at : nullptr, out.rgba ? out.rgba + 4u * at : nullptr,
                                       (void *)stream), "view resolve");
    return (int)RT_OK;
  });
}

int view_sample_outputs_check(uint32_t segs, const rt_ray_outputs *out, const char *what) {
  if (int rc = view_outputs_check(segs, out, what)) return rc;
  if (out->hits) return fail(RT_ERR_INVALID, "%s: hits must be NULL (a mean of hit records means nothing)", what);
  return RT_OK;
}
}  // namespace

extern "C" int rt_view_validate(const rt_view *v, uint32_t w, uint32_t h) { return view_check(v, w, h, "rt_view_validate"); }

extern "C" int rt_view_equirect_tables(uint32_t w, uint32_t h, double *lon, double *lat) {
  if (!lon || !lat || w == 0 || h == 0) return fail(RT_ERR_INVALID, "rt_view_equirect_tables: a NULL table, w == 0 or h == 0");
  for (uint32_t x = 0; x < w; x++) { const double a = rt_view_lon(x, w); lon[2u * (size_t)x] = sin(a); lon[2u * (size_t)x + 1u] = cos(a); }
  for (uint32_t y = 0; y < h; y++) { const double a = rt_view_lat(y, h); lat[2u * (size_t)y] = sin(a); lat[2u * (size_t)y + 1u] = cos(a); }
  return RT_OK;
}

extern "C" int rt_view_rays(const rt_view *v, uint32_t w, uint32_t h, uint32_t first_row, uint32_t rows, double *out) {
  int rc = view_check(v, w, h, "rt_view_rays");
  if (rc) return rc;
  if (!out) return fail(RT_ERR_INVALID, "rt_view_rays: NULL output");
  if ((rc = view_rows_check(h, first_row, rows, "rt_view_rays"))) return rc;
  const rt_view_params P = view_params(*v, w, h);
  rt_view_rays_host(&P, first_row, rows, out);
  return RT_OK;
}

extern "C" int rt_view_rays_device(int device, const rt_view *v, uint32_t w, uint32_t h, uint32_t first_row, uint32_t rows, double *d_rays,
                                   void *hip_stream) {
  int rc = view_check(v, w, h, "rt_view_rays_device");
  if (rc) return rc;
  if (!d_rays || ((uintptr_t)d_rays & 15u)) return fail(RT_ERR_INVALID, "rt_view_rays_device: NULL or misaligned ray list (16 bytes)");
  if ((rc = view_rows_check(h, first_row, rows, "rt_view_rays_device"))) return rc;
  if (rows == 0) return RT_OK;
  hipStream_t stream = nullptr;
  if ((rc = device_stream(device, hip_stream, &stream))) return rc;
  return view_rays_launch(view_params(*v, w, h), first_row, rows, d_rays, stream);
}

extern "C" size_t rt_view_work_bytes(uint32_t w, uint32_t h) {
  // the whole view in one band: at 3840 x 2160 bands of 2^16, 2^18 and 2^20 rays cost default14 10.7, 3.8 and 1.7 ms against 0.91 ms
  // for the whole view (docs/EVIDENCE.md, "Views")
  return view_size_ok(w, h) ? (size_t)w * h * 48u : 0;
}

extern "C" int rt_scene_trace_view_device(rt_scene_dev *s, const rt_view *v, uint32_t w, uint32_t h, uint32_t segs, const rt_ray_outputs *d_out,
                                          void *d_work, size_t work_bytes, void *hip_stream, rt_stats *stats) {
  const char *what = "rt_scene_trace_view_device";
  if (!s) return fail(RT_ERR_STATE, "%s: NULL scene handle", what);
  int rc = view_check(v, w, h, what);
  if (rc) return rc;
  if ((rc = view_outputs_check(segs, d_out, what))) return rc;
  uint32_t band_rows = 0;
  if ((rc = view_work_check(d_work, work_bytes, w, h, 48u, "rays", what, &band_rows))) return rc;
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return timed(stream, stats, (uint64_t)w * h, [&] { return trace_view_bands(s, view_params(*v, w, h), 0u, h, band_rows, segs, *d_out, 0u, (double *)d_work, stream); });
}

extern "C" int rt_trace_view(const void *blob, size_t bytes, const rt_view *v, uint32_t w, uint32_t h, uint32_t segs, const rt_ray_outputs *ho,
                             rt_stats *stats) {
  const char *what = "rt_trace_view";
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = view_check(v, w, h, what))) return rc;
  if ((rc = view_outputs_check(segs, ho, what))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  device_bufs<2> tables;
  rt_view dv;
  if ((rc = view_upload_tables(*v, w, h, 1u, call.stream, &tables, &dv))) return rc;
  const rt_view_params P = view_params(dv, w, h);
  const chunk_row rows[4] = {row_scratch((size_t)w * 48u), row_out(ho->rgb, (size_t)w * 24u), row_out(ho->rgba, (size_t)w * 4u), row_out(ho->hits, (size_t)w * sizeof(rt_hit))};
  return chunked_view_call(call, w, h, rows, 4, stats, [&](uint32_t y, uint32_t m, void *const *d) {
    const rt_ray_outputs dout = {(double *)d[1], (uint8_t *)d[2], (rt_hit *)d[3]};
    return trace_view_bands(call.s, P, y, y + m, m, segs, dout, y, (double *)d[0], call.stream);
  });
}

// ---------------------------------------------------------------------------------------------------------------- sampled views
extern "C" int rt_view_samples_validate(const rt_view *v, uint32_t w, uint32_t h, const rt_view_lens *lens, uint32_t n, const rt_view_sample *samples) {
  return view_samples_check(v, w, h, lens, n, samples, "rt_view_samples_validate");
}

extern "C" int rt_view_samples_grid(uint32_t k, rt_view_sample *out) {
  if (k < 1u || k > 32u || !out) return fail(RT_ERR_INVALID, "rt_view_samples_grid: k %u not in 1..32, or a NULL output", k);
  for (uint32_t j = 0; j < k; j++)
    for (uint32_t i = 0; i < k; i++) {
      rt_view_sample &s = out[(size_t)j * k + i];
      s.dx = ((double)i + 0.5) / (double)k - 0.5;
      s.dy = ((double)j + 0.5) / (double)k - 0.5;
      // Shirley's concentric map of (a, b) = (2 dx, 2 dy) in [-1, 1]^2 onto the unit disk
      const double a = 2.0 * s.dx, b = 2.0 * s.dy;
      double r, phi;
      if (a == 0.0 && b == 0.0) { r = 0.0; phi = 0.0; }
      else if (fabs(a) > fabs(b)) { r = a; phi = (M_PI / 4.0) * (b / a); }
      else { r = b; phi = M_PI / 2.0 - (M_PI / 4.0) * (a / b); }
      s.lu = r * cos(phi); s.lv = r * sin(phi);
    }
  return RT_OK;
}

extern "C" int rt_view_equirect_sample_tables(uint32_t w, uint32_t h, uint32_t n, const rt_view_sample *samples, double *lon, double *lat) {
  if (!lon || !lat || !samples || w == 0 || h == 0 || n == 0) return fail(RT_ERR_INVALID, "rt_view_equirect_sample_tables: a NULL pointer, w == 0, h == 0 or n == 0");
  for (uint32_t s = 0; s < n; s++) {
    double *lo = lon + 2u * (size_t)w * s, *la = lat + 2u * (size_t)h * s;
    for (uint32_t x = 0; x < w; x++) { const double a = rt_view_sample_lon(x, w, samples[s].dx); lo[2u * (size_t)x] = sin(a); lo[2u * (size_t)x + 1u] = cos(a); }
    for (uint32_t y = 0; y < h; y++) { const double a = rt_view_sample_lat(y, h, samples[s].dy); la[2u * (size_t)y] = sin(a); la[2u * (size_t)y + 1u] = cos(a); }
  }
  return RT_OK;
}

extern "C" int rt_view_sample_rays(const rt_view *v, uint32_t w, uint32_t h, const rt_view_lens *lens, const rt_view_sample *sample, uint32_t table,
                                   uint32_t first_row, uint32_t rows, double *out) {
  const char *what = "rt_view_sample_rays";
  int rc = view_samples_check(v, w, h, lens, 1u, sample, what);
  if (rc) return rc;
  if (!out) return fail(RT_ERR_INVALID, "%s: NULL output", what);
  if ((rc = view_rows_check(h, first_row, rows, what))) return rc;
  const rt_view_params P = view_params_of_table(view_params(*v, w, h), table);
  const rt_view_sample_params S = sample_params(*sample, lens);
  rt_view_sample_rays_host(&P, &S, first_row, rows, out);
  return RT_OK;
}

extern "C" int rt_view_sample_rays_device(int device, const rt_view *v, uint32_t w, uint32_t h, const rt_view_lens *lens, const rt_view_sample *sample,
                                          uint32_t table, uint32_t first_row, uint32_t rows, double *d_rays, void *hip_stream) {
  const char *what = "rt_view_sample_rays_device";
  int rc = view_samples_check(v, w, h, lens, 1u, sample, what);
  if (rc) return rc;
  if (!d_rays || ((uintptr_t)d_rays & 15u)) return fail(RT_ERR_INVALID, "%s: NULL or misaligned ray list (16 bytes)", what);
  if ((rc = view_rows_check(h, first_row, rows, what))) return rc;
  if (rows == 0) return RT_OK;
  hipStream_t stream = nullptr;
  if ((rc = device_stream(device, hip_stream, &stream))) return rc;
  const rt_view_params P = view_params_of_table(view_params(*v, w, h), table);
  const rt_view_sample_params S = sample_params(*sample, lens);
  VIEW_LAUNCH(rt_launch_view_sample_rays(&P, &S, first_row, rows, d_rays, (void *)stream), "view sample generator");
  return RT_OK;
}

extern "C" size_t rt_view_samples_work_bytes(uint32_t w, uint32_t h) {
  // the whole view in one band, as rt_view_work_bytes and for its reason: a band costs n trace launches, and small launches are dear
  return view_size_ok(w, h) ? (size_t)w * h * RT_VIEW_SAMPLE_BAND_BYTES : 0;
}

extern "C" int rt_scene_trace_view_samples_device(rt_scene_dev *s, const rt_view *v, uint32_t w, uint32_t h, const rt_view_lens *lens, uint32_t n,
                                                  const rt_view_sample *samples, uint32_t segs, const rt_ray_outputs *d_out, void *d_work, size_t work_bytes,
                                                  void *hip_stream, rt_stats *stats) {
  const char *what = "rt_scene_trace_view_samples_device";
  if (!s) return fail(RT_ERR_STATE, "%s: NULL scene handle", what);
  int rc = view_samples_check(v, w, h, lens, n, samples, what);
  if (rc) return rc;
  if ((rc = view_sample_outputs_check(segs, d_out, what))) return rc;
  uint32_t band_rows = 0;
  if ((rc = view_work_check(d_work, work_bytes, w, h, RT_VIEW_SAMPLE_BAND_BYTES, "a band", what, &band_rows))) return rc;
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return timed(stream, stats, (uint64_t)w * h,
               [&] { return trace_view_sample_bands(s, view_params(*v, w, h), lens, n, samples, 0u, h, band_rows, segs, *d_out, 0u, d_work, stream); });
}

extern "C" int rt_trace_view_samples(const void *blob, size_t bytes, const rt_view *v, uint32_t w, uint32_t h, const rt_view_lens *lens, uint32_t n,
                                     const rt_view_sample *samples, uint32_t segs, const rt_ray_outputs *ho, rt_stats *stats) {
  const char *what = "rt_trace_view_samples";
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = view_samples_check(v, w, h, lens, n, samples, what))) return rc;
  if ((rc = view_sample_outputs_check(segs, ho, what))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  device_bufs<2> tables;                               // the panorama's tables of all samples
  rt_view dv;
  if ((rc = view_upload_tables(*v, w, h, n, call.stream, &tables, &dv))) return rc;
  const rt_view_params P = view_params(dv, w, h);
  const chunk_row rows[3] = {row_scratch((size_t)w * RT_VIEW_SAMPLE_BAND_BYTES), row_out(ho->rgb, (size_t)w * 24u), row_out(ho->rgba, (size_t)w * 4u)};
  return chunked_view_call(call, w, h, rows, 3, stats, [&](uint32_t y, uint32_t m, void *const *d) {
    const rt_ray_outputs dout = {(double *)d[1], (uint8_t *)d[2], nullptr};
    return trace_view_sample_bands(call.s, P, lens, n, samples, y, y + m, m, segs, dout, y, d[0], call.stream);
  });
}
