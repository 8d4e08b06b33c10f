// rt_gather_api.hip — gathered light (include/rt_hip.h: rt_gather; kernel: rt_gather.hip): the argument checks, the launch, the two
// device entry points and the two host forms.  The kernel reads what the soft trace reads - the scene's current spheres, epsilon,
// lights, light intensity, miss colour, textures and stars seed, taken under launch_mu - so it comes behind the scene's preparation
// like every other launch, and it keeps the walk's stack in scratch memory: its figure goes through scratch_guard before the launch.
// The host forms are rows and a step for the chunk drivers of rt_api_internal.h; a view is gathered in bands of whole rows as
// rt_ambient_api.hip's ambient_view_bands does it: a band's rays, their hit records, the fused kernel with base and pix_base advanced
// by y * w, so pixel i = y * w + x is receiver i whatever the band.
#include "rt_api_internal.h"
#include "rt_gather.h"

static_assert(sizeof(struct rt_gather) == 32 && offsetof(struct rt_gather, base) == 16 && offsetof(struct rt_gather, pix_base) == 24 &&
                  sizeof(rt_gather_outputs) == 16 && sizeof(rt_hit) == 80,
              "a gather description travels as 32 bytes without padding, a receiver is 80");

// ---- what the probe call (rt_probe_api.hip) shares: declared in rt_api_internal.h
namespace rt_api {
// the shared fields as rt_ambient_validate judges them, and the depth
int gather_check(const struct rt_gather *a, const char *what) {
  if (!a) return fail(RT_ERR_INVALID, "%s: NULL gather description", what);
  if (a->n_samples < 1u || a->n_samples > RT_AMBIENT_MAX_SAMPLES) return fail(RT_ERR_INVALID, "%s: n_samples %u not in 1..%u", what, a->n_samples, RT_AMBIENT_MAX_SAMPLES);
  if (a->n_dirs < a->n_samples || a->n_dirs > RT_AMBIENT_MAX_DIRS)
    return fail(RT_ERR_INVALID, "%s: n_dirs %u not in n_samples..%u", what, a->n_dirs, RT_AMBIENT_MAX_DIRS);
  if (a->segs > RT_MAX_SEGS) return fail(RT_ERR_INVALID, "%s: segs %u not in 0..%u (0 = the scene's depth)", what, a->segs, RT_MAX_SEGS);
  return RT_OK;
}

// ... and a table in HOST memory
int gather_table_check(const struct rt_gather *a, const double *dirs, const char *what) {
  if (int rc = gather_check(a, what)) return rc;
  if (!dirs) return fail(RT_ERR_INVALID, "%s: NULL direction table", what);
  for (uint32_t e = 0; e < a->n_dirs; e++)
    if (!std::isfinite(dirs[3u * (size_t)e]) || !std::isfinite(dirs[3u * (size_t)e + 1u]) || !std::isfinite(dirs[3u * (size_t)e + 2u]))
      return fail(RT_ERR_INVALID, "%s: direction %u has a non-finite component", what, e);
  return RT_OK;
}

// n receivers that are receivers [pix_base, pix_base + n) of every sample's list: the soft call's bound on pix, for the last sample
int gather_count_check(const struct rt_gather &a, uint64_t n, const char *what) {
  if (n == 0 || n >= (1ull << 31)) return fail(RT_ERR_INVALID, "%s: n %llu not in 1..2^31 - 1", what, (unsigned long long)n);
  if ((uint64_t)a.pix_base + (uint64_t)(a.n_samples - 1u) * a.pix_stride + n > (1ull << 31))
    return fail(RT_ERR_INVALID, "%s: pix_base %u + (n_samples %u - 1) * pix_stride %u + n %llu above 2^31", what, a.pix_base, a.n_samples, a.pix_stride,
                (unsigned long long)n);
  return RT_OK;
}

}  // namespace rt_api

namespace {
int gather_outputs_check(const rt_gather_outputs *out, const char *what) {
  if (!out) return fail(RT_ERR_INVALID, "%s: NULL outputs", what);
  if (!out->rgb && !out->rgba) return fail(RT_ERR_INVALID, "%s: every output is NULL", what);
  if (((uintptr_t)out->rgb & 7u) || ((uintptr_t)out->rgba & 3u)) return fail(RT_ERR_INVALID, "%s: misaligned output (rgb needs 8 bytes, rgba 4)", what);
  return RT_OK;
}

// the kernel's scratch figure, asked once
int gather_scratch(size_t *out) {
  static std::mutex mu;
  static size_t cached;
  static bool have;
  std::lock_guard<std::mutex> lk(mu);
  if (!have) {
    size_t b = 0;
    const int e = rt_gather_scratch(&b);
    if (e != 0) return fail(RT_ERR_DEVICE, "hipFuncGetAttributes: %s", hipGetErrorString((hipError_t)e));
    cached = b; have = true;
  }
  *out = cached;
  return RT_OK;
}

}  // namespace

// the launch record for receivers [0, n) of d_hits with the description's base and pix_base as given: the scene's state of THIS launch,
// taken under launch_mu behind the scene's preparation (shared with rt_probe_api.hip, whose kernel reads the same record)
int rt_api::gather_record(rt_scene_dev *s, const struct rt_gather &a, const double *d_dirs, uint32_t n, const rt_hit *d_hits, const uint32_t *d_order,
                          double *rgb, uint32_t *rgba, hipStream_t stream, rt_gather_launch *out) {
  const rt_scene_header &hd = s->hd;
  rt_gather_launch &L = *out;
  memset(&L, 0, sizeof L);
  {
    std::lock_guard<std::mutex> lk(s->launch_mu);
    if (int rc = enter_launch(s, stream)) return rc;
    L.S.objects = (const rt_sphere *)(obj_block(s) + s->o_objs);   // this generation's spheres, in blob order
    L.S.light_intensity = hd.light_intensity;                      // (rt_scene_set_light_intensity, rt_scene_set_lights: this launch's)
    L.S.stars_seed = hd.stars_seed;                                // (rt_scene_set_stars_seed: this launch's)
    memcpy(L.S.lights, s->lights, sizeof L.S.lights);
  }
  L.S.textures = s->d_texdesc;
  L.S.texel_base = (const uint8_t *)s->d_blob;
  memcpy(L.S.miss_color, hd.miss_color, sizeof L.S.miss_color);
  L.S.epsilon = hd.epsilon;
  L.S.n_objects = hd.n_objects; L.S.n_lights = hd.n_lights;
  L.S.n_samples = 1u;                                              // (the walk's own sample loop: not entered without its relit branch)
  L.S.order = d_order; L.S.rgb = rgb; L.S.rgba = rgba; L.S.n = n;
  L.S.segs = a.segs ? a.segs : hd.segs;                            // the CALL's depth
  if (L.S.segs > RT_MAX_SEGS) return fail(RT_ERR_INVALID, "the gather kernel: depth %u above %u", L.S.segs, RT_MAX_SEGS);   // (the stack's size)
  L.hits = d_hits; L.dirs = d_dirs;
  L.base = a.base; L.n_samples = a.n_samples; L.n_dirs = a.n_dirs; L.stride = a.stride;
  L.pix_base = a.pix_base; L.pix_stride = a.pix_stride;
  return RT_OK;
}

namespace {
// the fused kernel for receivers [0, n) of d_hits with the description's base and pix_base as given
int gather_launch(rt_scene_dev *s, const struct rt_gather &a, const double *d_dirs, uint32_t n, const rt_hit *d_hits, const uint32_t *d_order,
                  const rt_gather_outputs &out, hipStream_t stream, rt_stats *stats) {
  stats_clock clock;
  rt_gather_launch L;
  if (int rc = gather_record(s, a, d_dirs, n, d_hits, d_order, out.rgb, out.rgba, stream, &L)) return rc;
  size_t per_lane = 0;
  if (int rc = gather_scratch(&per_lane)) return rc;
  const uint64_t n_wg = ((uint64_t)n + RT_GATHER_WG - 1u) / RT_GATHER_WG;
  if (int rc = scratch_guard(G.dev[s->device], stream, per_lane, n_wg * (RT_GATHER_WG / 64u), "the gather kernel (rt_gather_kernel)")) return rc;
  if (int rc = clock.start(stats, stream)) return rc;
  const int err = rt_launch_gather(&L, (void *)stream);
  if (err != 0) return fail(RT_ERR_DEVICE, "gather kernel launch: %s", hipGetErrorString((hipError_t)err));
  return clock.finish(stats, n);
}

constexpr uint32_t RT_GATHER_VIEW_BAND_BYTES = 128u;      // per pixel of a band: the ray 48, its hit record 80

// The view's rows [row0, row_end) in bands of at most band_rows, as ambient_view_bands: per band the rays, their hit records and the
// fused kernel for the piece that starts at pixel y * w.  The outputs' first record is pixel out_row0 * w.  One stream.
int gather_view_bands(rt_scene_dev *s, const rt_view *v, uint32_t w, uint32_t h, const struct rt_gather &a, const double *d_dirs, uint32_t row0,
                      uint32_t row_end, uint32_t band_rows, const rt_gather_outputs &out, uint32_t out_row0, void *d_work, hipStream_t stream) {
  double *rays = (double *)d_work;
  rt_hit *hits = (rt_hit *)(rays + 6u * ((size_t)band_rows * w));
  return for_bands(row0, row_end, band_rows, [&](uint32_t y, uint32_t m) {
    if (int rc = view_band_hits(s, v, w, h, y, m, rays, hits, stream)) return rc;
    const size_t at = (size_t)(y - out_row0) * w;
    const rt_gather_outputs band = {out.rgb ? out.rgb + 3u * at : nullptr, out.rgba ? out.rgba + at : nullptr};
    return gather_launch(s, gather_piece_of(a, (uint64_t)y * w), d_dirs, m * w, hits, nullptr, band, stream, nullptr);
  });
}

// the table of a host form in device memory
int upload_dirs(const struct rt_gather &a, const double *dirs, device_mem *d_dirs, hipStream_t stream) {
  HIP_TRY(hipMalloc(&d_dirs->h, (size_t)a.n_dirs * 24u));
  HIP_TRY(hipMemcpyAsync(d_dirs->h, dirs, (size_t)a.n_dirs * 24u, hipMemcpyHostToDevice, stream));
  return RT_OK;
}
}  // namespace

extern "C" int rt_gather_validate(const struct rt_gather *a, const double *dirs) { return gather_table_check(a, dirs, "rt_gather_validate"); }

// (the arguments first: they are judged without a scene, and before a device is touched)
extern "C" int rt_scene_gather_device(rt_scene_dev *s, const struct rt_gather *a, const double *d_dirs, uint64_t n, const rt_hit *d_hits,
                                      const uint32_t *d_order, const rt_gather_outputs *d_out, void *hip_stream, rt_stats *stats) {
  const char *what = "rt_scene_gather_device";
  int rc = gather_check(a, what);
  if (rc) return rc;
  if ((rc = gather_count_check(*a, n, what))) return rc;
  if (!d_dirs || !d_hits) return fail(RT_ERR_INVALID, "%s: NULL direction table or hit records", what);
  if (((uintptr_t)d_dirs & 7u) || ((uintptr_t)d_hits & 7u)) return fail(RT_ERR_INVALID, "%s: misaligned direction table or hit records (8 bytes)", what);
  if ((rc = gather_outputs_check(d_out, what))) return rc;
  if ((uintptr_t)d_order & 3u) return fail(RT_ERR_INVALID, "%s: misaligned order (4 bytes)", what);
  if (!s) return fail(RT_ERR_STATE, "%s: NULL scene handle", what);
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return gather_launch(s, *a, d_dirs, (uint32_t)n, d_hits, d_order, *d_out, stream, stats);
}

extern "C" int rt_gather(const void *blob, size_t bytes, const struct rt_gather *a, const double *dirs, uint64_t n, const rt_hit *hits,
                         const rt_gather_outputs *ho, rt_stats *stats) {
  const char *what = "rt_gather";
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = gather_table_check(a, dirs, what))) return rc;
  if ((rc = gather_count_check(*a, n, what))) return rc;
  if (!hits) return fail(RT_ERR_INVALID, "%s: NULL hit records", what);
  if ((rc = gather_outputs_check(ho, what))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  device_mem d_dirs;                 // the table (released behind the call, whose every chunk has been waited for)
  if ((rc = upload_dirs(*a, dirs, &d_dirs, call.stream))) return rc;
  const chunk_row rows[3] = {row_in(hits, sizeof(rt_hit)), row_out(ho->rgb, 24u), row_out(ho->rgba, 4u)};
  return chunked_list_call(call, n, rows, 3, false, stats, [&](uint32_t m, uint64_t at, void *const *d, const uint32_t *, rt_stats *st) {
    const rt_gather_outputs dout = {(double *)d[1], (uint32_t *)d[2]};
    return gather_launch(call.s, gather_piece_of(*a, at), (const double *)d_dirs.h, m, (const rt_hit *)d[0], nullptr, dout, call.stream, st);
  });
}

extern "C" size_t rt_gather_view_work_bytes(uint32_t w, uint32_t h) {
  // the whole view in one band, as rt_view_work_bytes and for its reason: small launches are dear
  return view_size_ok(w, h) ? (size_t)w * h * RT_GATHER_VIEW_BAND_BYTES : 0;
}

extern "C" int rt_scene_gather_view_device(rt_scene_dev *s, const rt_view *v, uint32_t w, uint32_t h, const struct rt_gather *a, const double *d_dirs,
                                           const rt_gather_outputs *d_out, void *d_work, size_t work_bytes, void *hip_stream, rt_stats *stats) {
  const char *what = "rt_scene_gather_view_device";
  if (!s) return fail(RT_ERR_STATE, "%s: NULL scene handle", what);
  int rc = rt_view_validate(v, w, h);
  if (rc) return rc;
  if ((rc = gather_check(a, what))) return rc;
  if ((rc = gather_count_check(*a, (uint64_t)w * h, what))) return rc;
  if (!d_dirs || ((uintptr_t)d_dirs & 7u)) return fail(RT_ERR_INVALID, "%s: NULL or misaligned direction table (8 bytes)", what);
  if ((rc = gather_outputs_check(d_out, what))) return rc;
  uint32_t band_rows = 0;
  if ((rc = view_work_check(d_work, work_bytes, w, h, RT_GATHER_VIEW_BAND_BYTES, "a band", what, &band_rows))) return rc;
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return timed(stream, stats, (uint64_t)w * h, [&] { return gather_view_bands(s, v, w, h, *a, d_dirs, 0u, h, band_rows, *d_out, 0u, d_work, stream); });
}

extern "C" int rt_gather_view(const void *blob, size_t bytes, const rt_view *v, uint32_t w, uint32_t h, const struct rt_gather *a, const double *dirs,
                              const rt_gather_outputs *ho, rt_stats *stats) {
  const char *what = "rt_gather_view";
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = rt_view_validate(v, w, h))) return rc;
  if ((rc = gather_table_check(a, dirs, what))) return rc;
  if ((rc = gather_count_check(*a, (uint64_t)w * h, what))) return rc;
  if ((rc = gather_outputs_check(ho, what))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  device_mem d_dirs;                 // the table
  device_bufs<2> tables;             // the panorama's
  rt_view dv;
  if ((rc = upload_dirs(*a, dirs, &d_dirs, call.stream))) return rc;
  if ((rc = view_upload_tables(*v, w, h, 1u, call.stream, &tables, &dv))) return rc;
  const chunk_row rows[3] = {row_scratch((size_t)w * RT_GATHER_VIEW_BAND_BYTES), row_out(ho->rgb, (size_t)w * 24u), row_out(ho->rgba, (size_t)w * 4u)};
  return chunked_view_call(call, w, h, rows, 3, stats, [&](uint32_t y, uint32_t m, void *const *d) {
    const rt_gather_outputs dout = {(double *)d[1], (uint32_t *)d[2]};
    return gather_view_bands(call.s, &dv, w, h, *a, (const double *)d_dirs.h, y, y + m, m, dout, y, d[0], call.stream);
  });
}
