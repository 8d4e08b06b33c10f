// rt_probe_api.hip — probes (include/rt_hip.h: rt_probe_outputs; kernel: rt_probe.hip): the argument checks, the launch, the device
// entry point, the host form and the spherical-harmonics weights.  The description is rt_gather's and is judged by rt_gather_api.hip's
// own checks; the launch record is that unit's too (gather_record: the scene's state under launch_mu, behind its preparation), with the
// weights, the coefficients and the block size beside it.  The kernel keeps the walk's stack in scratch memory: its figure goes through
// scratch_guard for n workgroups of B / 64 waves.
#include "rt_api_internal.h"
#include "rt_probe.h"

static_assert(sizeof(rt_probe_outputs) == 24 && offsetof(rt_probe_outputs, coef) == 16, "three pointers");

namespace {
// the weights' count, and that weights and coefficients come together or not at all
int probe_weights_check(const void *weights, uint32_t n_weights, const char *what) {
  if (n_weights > RT_PROBE_MAX_WEIGHTS) return fail(RT_ERR_INVALID, "%s: n_weights %u above %u", what, n_weights, RT_PROBE_MAX_WEIGHTS);
  if ((n_weights != 0u) != (weights != nullptr))
    return fail(RT_ERR_INVALID, "%s: n_weights %u %s a weight table", what, n_weights, weights ? "with" : "without");
  if ((uintptr_t)weights & 7u) return fail(RT_ERR_INVALID, "%s: misaligned weights (8 bytes)", what);
  return RT_OK;
}

// ... and a table in HOST memory
int probe_tables_check(const struct rt_gather *a, const double *dirs, const double *weights, uint32_t n_weights, const char *what) {
  if (int rc = gather_table_check(a, dirs, what)) return rc;
  if (int rc = probe_weights_check(weights, n_weights, what)) return rc;
  for (size_t q = 0; q < (size_t)a->n_dirs * n_weights; q++)
    if (!std::isfinite(weights[q])) return fail(RT_ERR_INVALID, "%s: weight %zu of entry %zu is not finite", what, q % n_weights, q / n_weights);
  return RT_OK;
}

int probe_outputs_check(const rt_probe_outputs *out, const void *weights, const char *what) {
  if (!out) return fail(RT_ERR_INVALID, "%s: NULL outputs", what);
  if (!out->rgb && !out->rgba && !out->coef) return fail(RT_ERR_INVALID, "%s: every output is NULL", what);
  if ((out->coef != nullptr) != (weights != nullptr)) return fail(RT_ERR_INVALID, "%s: weights and coef come together or not at all", what);
  if (((uintptr_t)out->rgb & 7u) || ((uintptr_t)out->rgba & 3u) || ((uintptr_t)out->coef & 7u))
    return fail(RT_ERR_INVALID, "%s: misaligned output (rgb and coef need 8 bytes, rgba 4)", what);
  return RT_OK;
}

// the kernel's scratch figure, asked once
int probe_scratch(size_t *out) {
  static std::mutex mu;
  static size_t cached;
  static bool have;
  std::lock_guard<std::mutex> lk(mu);
  if (!have) {
    size_t b = 0;
    const int e = rt_probe_scratch(&b);
    if (e != 0) return fail(RT_ERR_DEVICE, "hipFuncGetAttributes: %s", hipGetErrorString((hipError_t)e));
    cached = b; have = true;
  }
  *out = cached;
  return RT_OK;
}

// the probe kernel for receivers [0, n) of d_hits with the description's base and pix_base as given
int probe_launch(rt_scene_dev *s, const struct rt_gather &a, const double *d_dirs, const double *d_weights, uint32_t n_weights, uint32_t n,
                 const rt_hit *d_hits, const uint32_t *d_order, const rt_probe_outputs &out, hipStream_t stream, rt_stats *stats) {
  stats_clock clock;
  rt_probe_launch L;
  memset(&L, 0, sizeof L);
  if (int rc = gather_record(s, a, d_dirs, n, d_hits, d_order, out.rgb, out.rgba, stream, &L.G)) return rc;
  L.weights = d_weights; L.coef = out.coef; L.n_weights = n_weights;
  L.block = rt_probe_block(a.n_samples);
  size_t per_lane = 0;
  if (int rc = probe_scratch(&per_lane)) return rc;
  if (int rc = scratch_guard(G.dev[s->device], stream, per_lane, (uint64_t)n * (L.block / 64u), "the probe kernel (rt_probe_kernel)")) return rc;
  if (int rc = clock.start(stats, stream)) return rc;
  const int err = rt_launch_probe(&L, (void *)stream);
  if (err != 0) return fail(RT_ERR_DEVICE, "probe kernel launch: %s", hipGetErrorString((hipError_t)err));
  return clock.finish(stats, n);
}

// a table of a host form in device memory
int upload_table(const double *host, size_t bytes, device_mem *d, hipStream_t stream) {
  HIP_TRY(hipMalloc(&d->h, bytes));
  HIP_TRY(hipMemcpyAsync(d->h, host, bytes, hipMemcpyHostToDevice, stream));
  return RT_OK;
}
}  // namespace

extern "C" int rt_probes_validate(const struct rt_gather *a, const double *dirs, const double *weights, uint32_t n_weights) {
  return probe_tables_check(a, dirs, weights, n_weights, "rt_probes_validate");
}

// include/rt_hip.h states each value's operations and their order; no product is fused with the subtraction behind it
extern "C" int rt_probe_sh9_weights(uint32_t n, const double *dirs, double *out) {
#pragma clang fp contract(off)
  if (!dirs || !out) return fail(RT_ERR_INVALID, "rt_probe_sh9_weights: NULL pointer");
  if (n == 0 || n > RT_AMBIENT_MAX_DIRS) return fail(RT_ERR_INVALID, "rt_probe_sh9_weights: n %u not in 1..%u", n, RT_AMBIENT_MAX_DIRS);
  for (uint32_t i = 0; i < n; i++) {
    const double x = dirs[3u * (size_t)i], y = dirs[3u * (size_t)i + 1u], z = dirs[3u * (size_t)i + 2u];
    double *o = out + 9u * (size_t)i;
    o[0] = 0.28209479177387814;
    o[1] = 0.4886025119029199 * y; o[2] = 0.4886025119029199 * z; o[3] = 0.4886025119029199 * x;
    o[4] = 1.0925484305920792 * (x * y); o[5] = 1.0925484305920792 * (y * z); o[6] = 1.0925484305920792 * (x * z);
    o[7] = 0.31539156525252005 * ((3.0 * (z * z)) - 1.0);
    o[8] = 0.5462742152960396 * ((x * x) - (y * y));
  }
  return RT_OK;
}

// (the arguments first: they are judged without a scene, and before a device is touched)
extern "C" int rt_scene_gather_probes_device(rt_scene_dev *s, const struct rt_gather *a, const double *d_dirs, const double *d_weights, uint32_t n_weights,
                                             uint64_t n, const rt_hit *d_hits, const uint32_t *d_order, const rt_probe_outputs *d_out, void *hip_stream,
                                             rt_stats *stats) {
  const char *what = "rt_scene_gather_probes_device";
  int rc = gather_check(a, what);
  if (rc) return rc;
  if ((rc = gather_count_check(*a, n, what))) return rc;
  if (!d_dirs || !d_hits) return fail(RT_ERR_INVALID, "%s: NULL direction table or hit records", what);
  if (((uintptr_t)d_dirs & 7u) || ((uintptr_t)d_hits & 7u)) return fail(RT_ERR_INVALID, "%s: misaligned direction table or hit records (8 bytes)", what);
  if ((rc = probe_weights_check(d_weights, n_weights, what))) return rc;
  if ((rc = probe_outputs_check(d_out, d_weights, what))) return rc;
  if ((uintptr_t)d_order & 3u) return fail(RT_ERR_INVALID, "%s: misaligned order (4 bytes)", what);
  if (!s) return fail(RT_ERR_STATE, "%s: NULL scene handle", what);
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return probe_launch(s, *a, d_dirs, d_weights, n_weights, (uint32_t)n, d_hits, d_order, *d_out, stream, stats);
}

extern "C" int rt_gather_probes(const void *blob, size_t bytes, const struct rt_gather *a, const double *dirs, const double *weights, uint32_t n_weights,
                                uint64_t n, const rt_hit *hits, const rt_probe_outputs *ho, rt_stats *stats) {
  const char *what = "rt_gather_probes";
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = probe_tables_check(a, dirs, weights, n_weights, what))) return rc;
  if ((rc = gather_count_check(*a, n, what))) return rc;
  if (!hits) return fail(RT_ERR_INVALID, "%s: NULL hit records", what);
  if ((rc = probe_outputs_check(ho, weights, what))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  device_mem d_dirs, d_weights;      // the tables (released behind the call, whose every chunk has been waited for)
  if ((rc = upload_table(dirs, (size_t)a->n_dirs * 24u, &d_dirs, call.stream))) return rc;
  if (n_weights && (rc = upload_table(weights, (size_t)a->n_dirs * n_weights * 8u, &d_weights, call.stream))) return rc;
  const chunk_row rows[4] = {row_in(hits, sizeof(rt_hit)), row_out(ho->rgb, 24u), row_out(ho->rgba, 4u), row_out(ho->coef, 24u * (size_t)n_weights)};
  return chunked_list_call(call, n, rows, 4, false, stats, [&](uint32_t m, uint64_t at, void *const *d, const uint32_t *, rt_stats *st) {
    const rt_probe_outputs dout = {(double *)d[1], (uint32_t *)d[2], (double *)d[3]};
    return probe_launch(call.s, gather_piece_of(*a, at), (const double *)d_dirs.h, (const double *)d_weights.h, n_weights, m, (const rt_hit *)d[0], nullptr,
                        dout, call.stream, st);
  });
}
