// rt_launch.hip — the launches of a resident scene (include/rt_hip.h: rt_render_*_device).  A colour launch is render_batch_impl: the
// argument checks, the launch record (fill_launch, bind_kernel), then the strict launch or the product launch with its launch table and
// the list-driven strict launch behind it (rt_retrace), then the stats; every launch works out its kernel variant once
// (rt_device.h: rt_trace_variant) and hands that value to the LDS size, the scratch guard and the launcher.  Also here: 3x3 / 4x4
// supersampling with a box filter, compact bands, primary hits and picking, caller-supplied rays (rt_trace_rays) in the list's or a
// given order and their ordering, occlusion queries, and the test build's per-sample probe.

#include "rt_api_internal.h"

// ------------------------------------------------------------------------------------ launch
extern "C" int rt_render_tiles_device(rt_scene_dev *s, uint32_t w, uint32_t h, const rt_tiles *tiles, void *d_out, void *hip_stream,
                                      uint32_t flags, rt_stats *stats) {
  return rt_render_batch_device(s, w, h, tiles, 1u, d_out, 0u, hip_stream, flags, stats);
}

namespace {
int render_batch_impl(rt_scene_dev *s, uint32_t w, uint32_t h, const rt_tiles *tiles, uint32_t n_frames, void *d_out, uint64_t frame_stride_bytes,
                      void *const *d_frames, void *hip_stream, uint32_t flags, rt_stats *stats, uint32_t ss_override = 0u);
#ifdef RT_TESTING
thread_local struct { double *d_buf; uint32_t x, y; } g_probe = {nullptr, 0u, 0u};
#endif

// The scene in its own order, every sphere in the loops, the reference's own miss colour: what the strict kernels, the counting
// variant, rt_retrace and rt_trace_rays walk (the rest of a frame launch's binding: bind_kernel).  Under launch_mu where an edit may run.
void bind_scene_order(const rt_scene_dev *s, rt_launch &K) {
  const uint8_t *ob = obj_block(s);                   // this generation's spheres, in blob order
  K.objects = (const rt_sphere *)(ob + s->o_objs);
  K.geom = (const rt_geom *)(ob + s->o_geom);
  K.lds_image = lds_image_of(s);                      // its materials and texture descriptors
  K.n_loop = s->hd.n_objects;
  K.enclosing = ~0u;
  memcpy(K.miss_color, s->hd.miss_color, sizeof K.miss_color);
}
}  // namespace

#ifdef RT_TESTING
// Test build only: the ray tree of ONE sample (sample-grid coordinates sx, sy) as RT_PROBE_NODES records of RT_PROBE_WORDS
// doubles {path, hcode, t, hit point, normal, direction, sampled colour, diffuse, specular, segs left, light intensity after
// the scans, ray origin, children mask, valid}; the row that holds the sample is rendered into scratch memory.
extern "C" int rt_test_probe(rt_scene_dev *s, uint32_t w, uint32_t h, uint32_t sx, uint32_t sy, uint32_t flags, double *out_records) {
  if (!s || !out_records) return fail(RT_ERR_INVALID, "rt_test_probe: NULL argument");
  int rc = ensure_device(s->device);
  if (rc) return rc;
  const size_t bytes = (size_t)RT_PROBE_NODES * RT_PROBE_WORDS * sizeof(double);
  double *d_probe = nullptr;
  void *d_row = nullptr;
  HIP_TRY(hipMalloc((void **)&d_probe, bytes));
  hipError_t e = hipMemset(d_probe, 0, bytes);
  if (e == hipSuccess) e = hipMalloc(&d_row, (size_t)w * 4u);
  if (e != hipSuccess) { (void)hipFree(d_probe); return fail(RT_ERR_DEVICE, "rt_test_probe: %s", hipGetErrorString(e)); }
  const uint32_t ss = s->hd.supersample;
  rt_tiles t = {1u, sy / ss, 1u, 1u};
  rt_stats st;
  g_probe.d_buf = d_probe; g_probe.x = sx; g_probe.y = sy;
  rc = rt_render_tiles_device(s, w, h, &t, d_row, nullptr, flags & ~(uint32_t)RT_FLAG_RGB24, &st);
  g_probe.d_buf = nullptr;
  if (!rc) { e = hipMemcpy(out_records, d_probe, bytes, hipMemcpyDeviceToHost); if (e != hipSuccess) rc = fail(RT_ERR_DEVICE, "rt_test_probe: %s", hipGetErrorString(e)); }
  (void)hipFree(d_probe); (void)hipFree(d_row);
  return rc;
}

// Test build only: how many waves of the device's product launches have taken the uniform-material path (rt_kernel.hip: trace_pixel,
// UNI) since the last call; the device is drained first, and the counter starts again at zero.
extern "C" int rt_test_uniform_waves(int device, unsigned long long *out_waves) {
  if (!out_waves) return fail(RT_ERR_INVALID, "rt_test_uniform_waves: NULL argument");
  int rc = ensure_device(device);
  if (rc) return rc;
  device_state &D = G.dev[device];
  HIP_TRY(hipSetDevice(D.hip_id));                    // (ensure_device has, too: said here because the next call drains THIS device)
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out_waves, D.d_counters + 3, sizeof *out_waves, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(D.d_counters + 3, 0, sizeof *out_waves));
  return RT_OK;
}
// ... and how many of the waves that took it had their checker cell from the launch table (rt_block.h: rt_column_cell) instead of working
// it out per sample; a counter of its own, read and cleared the same way
extern "C" int rt_test_cell_waves(int device, unsigned long long *out_waves) {
  if (!out_waves) return fail(RT_ERR_INVALID, "rt_test_cell_waves: NULL argument");
  int rc = ensure_device(device);
  if (rc) return rc;
  device_state &D = G.dev[device];
  HIP_TRY(hipSetDevice(D.hip_id));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out_waves, D.d_counters + 4, sizeof *out_waves, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(D.d_counters + 4, 0, sizeof *out_waves));
  return RT_OK;
}
// ... and how many waves of the general path walked the first-bounce set of their launch-table entry (rt_block.h: rt_first_bounce_set)
// instead of every loop sphere at the node after the primary; a counter of its own, read and cleared the same way
extern "C" int rt_test_first_bounce_waves(int device, unsigned long long *out_waves) {
  if (!out_waves) return fail(RT_ERR_INVALID, "rt_test_first_bounce_waves: NULL argument");
  int rc = ensure_device(device);
  if (rc) return rc;
  device_state &D = G.dev[device];
  HIP_TRY(hipSetDevice(D.hip_id));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out_waves, D.d_counters + 5, sizeof *out_waves, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(D.d_counters + 5, 0, sizeof *out_waves));
  return RT_OK;
}
// ... and how many of those waves left a candidate out of their walk, as the second-node bits of their entry allow (rt_block.h:
// rt_second_node_bits); a counter of its own, read and cleared the same way
extern "C" int rt_test_second_node_waves(int device, unsigned long long *out_waves) {
  if (!out_waves) return fail(RT_ERR_INVALID, "rt_test_second_node_waves: NULL argument");
  int rc = ensure_device(device);
  if (rc) return rc;
  device_state &D = G.dev[device];
  HIP_TRY(hipSetDevice(D.hip_id));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out_waves, D.d_counters + 6, sizeof *out_waves, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(D.d_counters + 6, 0, sizeof *out_waves));
  return RT_OK;
}
#endif

extern "C" int rt_render_batch_device(rt_scene_dev *s, uint32_t w, uint32_t h, const rt_tiles *tiles, uint32_t n_frames, void *d_out,
                                      uint64_t frame_stride_bytes, void *hip_stream, uint32_t flags, rt_stats *stats) {
  if (!d_out) return fail(RT_ERR_INVALID, "NULL scene, tiles or output");
  return render_batch_impl(s, w, h, tiles, n_frames, d_out, frame_stride_bytes, nullptr, hip_stream, flags, stats);
}

extern "C" int rt_render_scatter_device(rt_scene_dev *s, uint32_t w, uint32_t h, const rt_tiles *tiles, uint32_t n_frames, void *const *d_frames,
                                        void *hip_stream, uint32_t flags, rt_stats *stats) {
  if (!d_frames) return fail(RT_ERR_INVALID, "NULL frame pointer array");
  if (n_frames == 0 || n_frames > RT_MAX_SCATTER) return fail(RT_ERR_INVALID, "scatter: n_frames %u not in 1..%u", n_frames, RT_MAX_SCATTER);
  if (flags & RT_FLAG_RGB24) return fail(RT_ERR_INVALID, "scatter writes whole RGBA8 frames: RT_FLAG_RGB24 does not apply");
  for (uint32_t f = 0; f < n_frames; f++) if (!d_frames[f] || ((uintptr_t)d_frames[f] & 3u)) return fail(RT_ERR_INVALID, "scatter: frame pointer %u is NULL or unaligned", f);
  return render_batch_impl(s, w, h, tiles, n_frames, nullptr, 0u, d_frames, hip_stream, flags, stats);
}

namespace {
// k x k box filter of the two-pass supersampling (k = 3, 4): `src` holds the rendered SAMPLES of this call's tiles as a band
// (rows of k*w RGBA8 samples, k sample rows per output row, tiles contiguous), the output pixel is (sum + k*k/2) / (k*k) per
// channel, alpha 255, stored where the trace kernel would have stored it: in the band (`out`, frame f at f*frame_stride) or,
// scatter mode, at its row of the whole frame out_frames[f].  One work-item per output pixel; rows walked by grid y.
struct rt_box_launch {
  const uint32_t *src; uint64_t src_frame_stride;      // in samples (words)
  uint32_t *out; uint64_t frame_stride; uint32_t *out_frames[RT_MAX_SCATTER]; uint32_t scatter;
  uint32_t w, h, band_rows, tile_rows, tile_first, tile_stride;
};
template <uint32_t K>
__global__ void __launch_bounds__(256) rt_box_filter_kernel(const rt_box_launch B) {
  const uint32_t x = blockIdx.x * 256u + threadIdx.x, f = blockIdx.z;
  if (x >= B.w) return;
  const uint32_t *__restrict__ src = B.src + (size_t)f * B.src_frame_stride;
  for (uint32_t lrow = blockIdx.y; lrow < B.band_rows; lrow += gridDim.y) {
    const uint32_t tile_i = lrow / B.tile_rows, trow = lrow - tile_i * B.tile_rows;
    const uint32_t frow = (B.tile_first + tile_i * B.tile_stride) * B.tile_rows + trow;
    if (frow >= B.h) continue;
    uint32_t r = 0, g = 0, b = 0;
#pragma unroll
    for (uint32_t j = 0; j < K; j++) {
      const uint32_t *__restrict__ p = src + ((size_t)lrow * K + j) * ((size_t)B.w * K) + (size_t)x * K;
#pragma unroll
      for (uint32_t i = 0; i < K; i++) { const uint32_t v = p[i]; r += v & 255u; g += (v >> 8) & 255u; b += (v >> 16) & 255u; }
    }
    const uint32_t px = ((r + K * K / 2u) / (K * K)) | (((g + K * K / 2u) / (K * K)) << 8) | (((b + K * K / 2u) / (K * K)) << 16) | 0xff000000u;
    if (B.scatter) B.out_frames[f][(size_t)frow * B.w + x] = px;
    else B.out[(size_t)f * B.frame_stride + (size_t)lrow * B.w + x] = px;
  }
}

// supersample 3 and 4: the k*w x k*h sample frame of this call's tiles is rendered by the ordinary launch
// (supersample 1 on the sample grid: same kernels, same centre-row/column rule, same tiles with k times the rows) into
// scratch memory, in pieces of at most ~512 MiB, and box-filtered into the caller's output.
int render_supersampled(rt_scene_dev *s, uint32_t k, uint32_t w, uint32_t h, const rt_tiles *tiles, uint32_t n_frames, void *d_out, uint64_t frame_stride_bytes,
                        void *const *d_frames, hipStream_t stream, uint32_t flags, rt_stats *stats) {
  if (flags & RT_FLAG_RGB24) return fail(RT_ERR_INVALID, "RT_FLAG_RGB24 needs supersample 1 or 2 (the %ux%u box filter stores RGBA8)", k, k);
  if ((uint64_t)w * k > 65536u || (uint64_t)h * k > 65536u) return fail(RT_ERR_INVALID, "supersample %u: the %llu x %llu sample grid exceeds 65536", k, (unsigned long long)w * k, (unsigned long long)h * k);
  const auto t_begin = std::chrono::steady_clock::now();
  const size_t row_bytes = (size_t)w * k * 4u * k;                      // the k sample rows of one output row
  const size_t budget = (size_t)512u << 20;
  // pieces: whole tiles while they fit, else (one tile per call, starting on a multiple of the piece height) row pieces of a tile
  uint32_t tiles_per_piece = (uint32_t)(budget / (row_bytes * tiles->tile_rows * (size_t)n_frames));
  uint32_t piece_rows = tiles->tile_rows;
  if (tiles_per_piece == 0) {
    tiles_per_piece = 1;
    piece_rows = (uint32_t)(budget / (row_bytes * n_frames)) / RT_TILE_H * RT_TILE_H;
    if (piece_rows == 0) piece_rows = RT_TILE_H;
    if (piece_rows >= tiles->tile_rows) piece_rows = tiles->tile_rows;
    else if (tiles->n_tiles != 1 || ((uint64_t)tiles->tile_first * tiles->tile_rows) % piece_rows != 0)
      return fail(RT_ERR_NOMEM, "supersample %u: a tile of %u rows needs more than 512 MiB of sample scratch; render smaller tiles", k, tiles->tile_rows);
  }
  rt_stats agg;
  memset(&agg, 0, sizeof agg);
  for (uint32_t t0 = 0; t0 < tiles->n_tiles; t0 += tiles_per_piece) {
    const uint32_t nt = (tiles->n_tiles - t0 < tiles_per_piece) ? tiles->n_tiles - t0 : tiles_per_piece;
    for (uint32_t r0 = 0; r0 < tiles->tile_rows; r0 += piece_rows) {
      // this piece as a tile set of the OUTPUT frame ...
      rt_tiles po;
      if (piece_rows == tiles->tile_rows) po = rt_tiles{tiles->tile_rows, tiles->tile_first + t0 * tiles->tile_stride, tiles->tile_stride, nt};
      else po = rt_tiles{piece_rows, (uint32_t)(((uint64_t)tiles->tile_first * tiles->tile_rows + r0) / piece_rows), 1u, 1u};
      if ((uint64_t)po.tile_first * po.tile_rows >= h) continue;
      // ... and of the sample frame
      const rt_tiles ps = {po.tile_rows * k, po.tile_first, po.tile_stride, po.n_tiles};
      const uint32_t band_rows = po.n_tiles * po.tile_rows;
      const size_t frame_words = (size_t)band_rows * k * w * k;
      void *scratch = nullptr;
      hipError_t e = hipMalloc(&scratch, frame_words * 4u * n_frames);
      if (e != hipSuccess) return fail(RT_ERR_NOMEM, "supersample scratch (%zu bytes): %s", frame_words * 4u * n_frames, hipGetErrorString(e));
#ifdef RT_TESTING
      (void)hipMemsetAsync(scratch, 0xA5, frame_words * 4u * n_frames, stream);      // test build: a sample nobody writes shows up as 0xA5, not as stale data
#endif
      rt_stats st;
      int rc = render_batch_impl(s, w * k, h * k, &ps, n_frames, scratch, frame_words * 4u, nullptr, stream, flags, stats ? &st : nullptr, 1u);
      if (!rc) {
        rt_box_launch B;
        memset(&B, 0, sizeof B);
        B.src = (const uint32_t *)scratch; B.src_frame_stride = frame_words;
        B.w = w; B.h = h; B.band_rows = band_rows; B.tile_rows = po.tile_rows; B.tile_first = po.tile_first; B.tile_stride = po.tile_stride;
        const size_t out_row0 = (size_t)t0 * tiles->tile_rows + r0;            // this piece's first row in the caller's band
        B.out = d_out ? (uint32_t *)d_out + out_row0 * w : nullptr; B.frame_stride = frame_stride_bytes / 4u;
        B.scatter = d_frames ? 1u : 0u;
        if (d_frames) for (uint32_t f = 0; f < n_frames; f++) B.out_frames[f] = (uint32_t *)d_frames[f];
        const dim3 grid((w + 255u) / 256u, band_rows < 65535u ? band_rows : 65535u, n_frames), block(256);
        if (k == 3u) hipLaunchKernelGGL(rt_box_filter_kernel<3u>, grid, block, 0, stream, B);
        else hipLaunchKernelGGL(rt_box_filter_kernel<4u>, grid, block, 0, stream, B);
        e = hipGetLastError();
        if (e != hipSuccess) rc = fail(RT_ERR_DEVICE, "box filter launch: %s", hipGetErrorString(e));
      }
      (void)hipStreamSynchronize(stream);            // (a 9x / 16x render: the allocation and this wait are noise beside it)
      e = hipFree(scratch);
      if (rc) return rc;
      if (e != hipSuccess) return fail(RT_ERR_DEVICE, "supersample scratch release: %s", hipGetErrorString(e));
      if (stats) { agg.kernel_ms += st.kernel_ms; agg.rays += st.rays; agg.shadow_rays += st.shadow_rays; agg.sphere_tests += st.sphere_tests; }
    }
  }
  if (stats) {
    HIP_TRY(hipStreamSynchronize(stream));
    agg.pixels = tile_set_pixels(w, h, tiles) * n_frames;
    agg.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    *stats = agg;
  }
  return RT_OK;
}

// ---- one colour launch (supersample 1 or 2), as steps: what they share, the launch record, the strict launch, the product launch
//      with its mark list and the list-driven strict launch behind it (rt_retrace), the stats ----
// The test build's switches of a colour launch, read at ONE place.  The product build reads no environment variable: every switch is off.
struct test_switches {
  bool no_grid, no_bounce; unsigned lds_pad; long count_wait_us;                 // once per process (A/B runs)
  bool no_fixup, mark_all, exact_all, mark_stripes, no_uniform, no_cells, no_first_bounce, no_second_node, no_wide;      // per call: tests set these between calls
  int wide_form;                                                                 // (RT_WIDE_FORM; 0: not set)
  double flag_scale;                                                             // (RT_FLAG_SCALE; 1: not set)
  bool uncached_marks;                   // a switch that changes what is marked or re-traced is on - nothing is cached then
};
test_switches read_test_switches() {
  static const bool no_grid = RT_TEST_ENV("RT_NO_SHADOW_GRID") != nullptr, no_bounce = RT_TEST_ENV("RT_NO_BOUNCE_TABLE") != nullptr;     // A/B switches
  // RT_LDS_PAD (bytes): occupancy experiments only — extra dynamic LDS per workgroup caps the workgroups per CU
  static const unsigned lds_pad = RT_TEST_ENV("RT_LDS_PAD") ? (unsigned)atoi(RT_TEST_ENV("RT_LDS_PAD")) : 0u;
  static const long count_wait_us = RT_TEST_ENV("RT_COUNT_WAIT_US") ? atol(RT_TEST_ENV("RT_COUNT_WAIT_US")) : -1;
  test_switches t = {no_grid, no_bounce, lds_pad, count_wait_us};
  t.no_fixup = RT_TEST_ENV("RT_NO_FIXUP") != nullptr;                           // the product kernel's own pixels everywhere
  t.mark_all = RT_TEST_ENV("RT_MARK_ALL") != nullptr; t.exact_all = RT_TEST_ENV("RT_EXACT_ALL") != nullptr; t.mark_stripes = RT_TEST_ENV("RT_TEST_MARK_STRIPES") != nullptr;
  t.no_uniform = RT_TEST_ENV("RT_NO_UNIFORM_BLOCKS") != nullptr;                // every wave on the general path (rt_kernel.hip: trace_pixel, UNI)
  t.no_cells = RT_TEST_ENV("RT_NO_CHECKER_CELLS") != nullptr;                   // the table's checker cells are ignored (rt_kernel.hip: trace_pixel, one_cell)
  t.no_first_bounce = RT_TEST_ENV("RT_NO_FIRST_BOUNCE") != nullptr;             // the table's first-bounce sets are ignored (rt_kernel_trace.h: the node after the primary)
  t.no_second_node = RT_TEST_ENV("RT_NO_SECOND_NODE") != nullptr;               // the table's second-node bits are ignored (rt_kernel_trace.h: the first-bounce walk)
  t.no_wide = RT_TEST_ENV("RT_NO_WIDE_STORES") != nullptr;                      // every launch keeps one 4-byte store per pixel (rt_kernel.hip, A10)
  // RT_WIDE_FORM (A/B runs): 1 - the 16-byte stores plain, 2 - write-through everywhere (the product's form), 3 - write-through for the sky runs only
  t.wide_form = RT_TEST_ENV("RT_WIDE_FORM") ? atoi(RT_TEST_ENV("RT_WIDE_FORM")) : 0;
  const char *fs = RT_TEST_ENV("RT_FLAG_SCALE");                                // a wider boundary band, to exercise the second launch
  t.flag_scale = fs ? atof(fs) : 1.0;
  t.uncached_marks = fs || t.mark_all || t.exact_all || t.no_fixup;
  return t;
}

// what the steps of one colour launch share
struct colour_call {
  rt_scene_dev *s; device_state &D; hipStream_t stream;
  uint32_t w, h, ss; const rt_tiles *tiles; uint32_t n_frames, flags;
  bool ss2, count, compact;
  test_switches t;
};
// what the product launch leaves for the stats
struct retrace_result {
  const uint32_t *marks_read = nullptr; uint32_t marks_read_slot = 0;    // where this launch's mark count can be read afterwards
  uint64_t centre_items = 0;
  bool retraced_all = false, strict_rendered = false;
};
struct marks_guard {                                     // a per-call mark state: its list is released on every way out, after the stream has drained
  rt_scene_dev::mark_state temp = {~0u, nullptr, device_mem(), nullptr, 0u};
  ~marks_guard() { if (temp.d_marks.h) (void)hipStreamSynchronize(temp.stream); }
};

int launched(int err) { return err != 0 ? fail(RT_ERR_DEVICE, "kernel launch: %s", hipGetErrorString((hipError_t)err)) : RT_OK; }

// Dynamic LDS of a variant's workgroup: the scene's LDS image and the fold state (10 doubles per lane, the general kernel 13; the strict
// kernels one slot, the scatter store's tile).  The reflection-only many-sphere variants keep only the fold state in LDS (rt_kernel.hip:
// IMAGE_IN_LDS); one-wave workgroups have 64 lanes, and the few-sphere ones stage the image's materials alone (rt_kernel.hip: MTL_ONLY):
// 8 spheres are 1 280 + 5 120 = 6 400 bytes, 24 workgroups in a CU's 160 KiB (DESIGN section 4 has the count per scene size).
unsigned lds_for(const rt_scene_dev *s, rt_trace_variant v, unsigned lds_pad) {
  if (v.strict) return s->lds_bytes + lds_pad + RT_WG_THREADS * 8u;
  const unsigned fold = (v.refract ? 13u : 10u) * (v.one_wave ? 64u : RT_WG_THREADS) * 8u;
  if (v.one_wave && !v.grid) return s->hd.n_objects * (unsigned)sizeof(rt_mtl) + lds_pad + fold;
  return ((v.grid && !v.refract) ? 0u : s->lds_bytes) + lds_pad + fold;
}

// The part of the launch record that depends on the kernel: ordering B (enclosing sphere last, outside the loops) and the shadow grids /
// bounce table for the product kernel; `plain` - the strict kernels, rt_retrace and the counting variant - walks the scene in its own
// order (bind_scene_order) so that it stays literal / counts what the reference counts.
void bind_kernel(const rt_scene_dev *s, rt_launch &K, bool plain, const test_switches &t) {
  const rt_scene_header &hd = s->hd;
  const bool order_b = s->has_b && !plain;
  const uint8_t *ob = obj_block(s);                   // this generation's spheres
  if (order_b) {
    K.objects = (const rt_sphere *)(ob + s->o_objs_b);
    K.geom = (const rt_geom *)(ob + s->o_geom) + (size_t)hd.n_objects * (1 + hd.n_lights);      // [plain N | anchored at light k: NL x N]
    K.lds_image = lds_image_of(s) + s->lds_image_bytes;
    K.n_loop = K.enclosing = hd.n_objects - 1;
    memcpy(K.miss_color, hd.miss_color, sizeof K.miss_color);
  } else bind_scene_order(s, K);
  const rt_geom *gc = (const rt_geom *)cam_block(s) + (order_b ? 2 * (size_t)hd.n_objects : 0);     // this camera's block: [anchored at the camera N | cull rectangles N]
  K.geom_cam = gc;
  K.cull = gc + hd.n_objects;
  K.geom_light = K.geom + hd.n_objects;
  K.shadow_grid = (!plain && !t.no_grid && s->has_sg) ? ob + s->o_sg : nullptr;
  K.bounce_table = (!plain && !t.no_bounce && s->has_bt) ? ob + s->o_bt : nullptr;
  K.enclosing_flat = (order_b && s->enclosing_flat) ? 1u : 0u;
  K.cull_in_lds = s->cull_in_lds ? 1u : 0u;
  K.sky_fast = (!plain && sky_fast(s)) ? 1u : 0u;
  for (int c = 0; c < 3; c++) K.sky_rgb[c] = s->sky_rgb[c];
  if (K.sky_fast && s->enclosing == ~0u) {
    // no enclosing sphere at all: a primary ray that meets nothing is the miss colour (main.js:231), a constant as well
    memcpy(K.sky_rgb, hd.miss_color, sizeof K.sky_rgb);
  } else if (K.sky_fast) {
    // A flat sky of constant colour needs no hit record at all: "met nothing in the loops" IS "met the sky", whose pixel term
    // is the constant the host evaluated - so for the product kernel that constant takes the place of the miss colour
    // (main.js:231 is unreachable in such a scene: the sky encloses every ray) and the sphere leaves the kernel's view.
    // Lanes that end on the sky then take the two-instruction miss branch, at every level of the ray tree.
    K.enclosing = ~0u;
    memcpy(K.miss_color, s->sky_rgb, sizeof K.miss_color);
  }
}

// Step 2: the launch record of the call, bound to the strict kernel (`strict_main`) or to the product kernel.  The launch table, the
// mark list and the grid are the product launch's to add.
int fill_launch(const colour_call &c, bool strict_main, uint32_t stars_seed, void *d_out, uint64_t frame_stride_bytes, void *const *d_frames, rt_launch &L) {
  const rt_scene_dev *s = c.s;
  const rt_scene_header &hd = s->hd;
  const rt_tiles *tiles = c.tiles;
  memset(&L, 0, sizeof L);
  bind_kernel(s, L, strict_main || c.count, c.t);
  // the boundary test of the product kernel's samplers (rt_device.h)
  L.flag_tol = s->flag_tol * c.t.flag_scale;
  L.mark_flags = (c.t.mark_all ? RT_MARK_ALL : 0u) | (c.t.no_fixup ? RT_MARK_NEVER : 0u) | (c.t.mark_stripes ? RT_MARK_ZERO : 0u) | (s->unit_weights ? RT_MARK_WEIGHT : 0u);
  L.marks_cap = RT_MARKS_CAP;
  L.stars_seed = stars_seed;
  L.stars_step = (c.flags & RT_FLAG_STARS_PER_FRAME) ? 1u : 0u;
  L.textures = s->d_texdesc;
  L.texel_base = (const uint8_t *)s->d_blob;
  L.out = (uint32_t *)d_out;
  L.counters = c.D.d_counters;
  memcpy(L.cam_origin, hd.cam_origin, 12 * sizeof(double));   // origin, axisX, axisY, axisZ are contiguous
  const launch_geom geom = launch_geometry(hd.fov_deg, c.w, c.h, c.ss, tiles->tile_rows);
  L.proj_w = geom.proj_w; L.proj_h = geom.proj_h; L.proj_d = geom.proj_d;
  L.epsilon = hd.epsilon; L.light_intensity = hd.light_intensity;
  L.n_objects = hd.n_objects; L.n_lights = hd.n_lights; L.segs = hd.segs;
  L.w = c.w; L.h = c.h;
  L.tile_rows = tiles->tile_rows; L.tile_first = tiles->tile_first; L.tile_stride = tiles->tile_stride; L.n_tiles = tiles->n_tiles;
  L.tiles_x = geom.tiles_x;
  memcpy(L.lights, s->lights, sizeof L.lights);
  L.rb_per_tile = geom.rb_per_tile;
  L.rb_shift = ~0u;
  for (uint32_t b = 0; b < 31; b++) if (L.rb_per_tile == (1u << b)) L.rb_shift = b;
  if ((uint64_t)tiles->n_tiles * L.rb_per_tile > 65535u) return fail(RT_ERR_INVALID, "%u tiles x %u row blocks exceed the grid's y limit (65535)", tiles->n_tiles, L.rb_per_tile);
  L.n_frames = c.n_frames;
  L.frame_stride = frame_stride_bytes / 4u;
  L.rgb24 = (c.flags & RT_FLAG_RGB24) ? 1u : 0u;
  L.compact = c.compact ? 1u : 0u;
  L.scatter = d_frames ? 1u : 0u;
  if (d_frames) for (uint32_t f = 0; f < c.n_frames; f++) L.out_frames[f] = (uint32_t *)d_frames[f];
  for (int k = 0; k < 3; k++) L.cam_axis_sum[k] = hd.cam_axis_x[k] + hd.cam_axis_y[k] + hd.cam_axis_z[k];
  L.ray_bias[0] = 0.5 - L.proj_w; L.ray_bias[1] = L.proj_h - 0.5; L.ray_bias[2] = L.cam_axis_sum[2] * L.proj_d;
#ifdef RT_TESTING
  L.probe = g_probe.d_buf; L.probe_x = g_probe.x; L.probe_y = g_probe.y;
  L.no_uniform = c.t.no_uniform ? 1u : 0u;
  L.uniform_waves = c.D.d_counters + 3;
  L.no_cells = c.t.no_cells ? 1u : 0u;
  L.no_first_bounce = c.t.no_first_bounce ? 1u : 0u;
  L.no_second_node = (c.t.no_second_node || c.t.no_first_bounce) ? 1u : 0u;
#endif
  return RT_OK;
}

// Step 3, strict: the strict kernel renders the whole call on the plain grid - a strict call or scene, and a frame known to overflow
// the mark list.  Under launch_mu.
int strict_launch(const colour_call &c, const rt_launch &L, bool count) {
  const rt_trace_variant v = rt_trace_variant_of(true, false, c.s->refract, count, c.ss2, L.cull_in_lds != 0u, L.scatter != 0u, false);
  if (int rc = guard_kernel_scratch(c.D, c.stream, v, (uint64_t)L.tiles_x * L.n_tiles * L.rb_per_tile * c.n_frames * (RT_WG_THREADS / 64u), "the strict trace kernel")) return rc;
  return launched(launch_variant(L, v, 0u, nullptr, lds_for(c.s, v, c.t.lds_pad), c.stream));
}

// How many entries the launch table has, if the host knows (0: not yet).  One workgroup per table entry is launched (runs of sky blocks
// share one).  How many there are is known on the device; until the build's count has reached the host, one workgroup per BLOCK is
// launched: those behind the last entry read a zero slot and leave.
uint32_t table_entries_known(const rt_scene_dev *s, const rt_scene_dev::order_entry &oe, const test_switches &t) {
  uint32_t n_known = known_value(oe.known, s->cam_gen);
  // A table that rt_scene_set_camera is rebuilding on the side stream - beside the previous frame's trace - publishes its count
  // while that trace is still running.  A caller that issues frames back to back arrives here earlier than that: it is given a
  // short, BOUNDED wait for the word (it is ahead of the GPU anyway, and stays one frame ahead: the trace in flight has tens of
  // microseconds left when the word arrives); one workgroup per block costs a 4K frame 80 us instead of 68.  A caller that comes
  // later (a frame per display refresh) finds the word there; a word that does not come in time: one workgroup per block.
  if (!n_known && oe.built_on == s->sync.side.h && oe.cam_gen == s->cam_gen) {
    // (the bound grows with the table: a 4K frame's build takes ~50 us beside a trace, an 8K frame's four times that)
    const long wait_us = t.count_wait_us >= 0 ? t.count_wait_us : 100 + (long)(oe.n_blocks / 256u);
    const auto t0 = std::chrono::steady_clock::now();
    while (!n_known && std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() < wait_us) {
      __builtin_ia32_pause();
      n_known = known_value(oe.known, s->cam_gen);
    }
  }
  return n_known;
}

// The mark state of a (launch table, stream) pair, found or made.  The first launch of a pair gets a list of its own; beyond
// RT_KNOWN_WORDS pairs: one per call (`temp_marks`), nothing cached.
int mark_state_for(rt_scene_dev *s, uint32_t order_index, hipStream_t stream, marks_guard &temp_marks, rt_scene_dev::mark_state **out) {
  for (rt_scene_dev::mark_state &m : s->mark_states) if (m.order_index == order_index && m.stream == stream) { *out = &m; return RT_OK; }
  const size_t bytes = 16u + (size_t)RT_MARKS_CAP * 8u;
  device_mem d;
  hipError_t e = hipMalloc(&d.h, bytes);
  if (e == hipSuccess) e = hipMemsetAsync(d.h, 0, 16u, stream);
  if (e != hipSuccess) return fail(RT_ERR_DEVICE, "mark list: %s", hipGetErrorString(e));
  if (s->mark_states.size() >= RT_KNOWN_WORDS) { temp_marks.temp.stream = stream; temp_marks.temp.d_marks = std::move(d); *out = &temp_marks.temp; }
  else {
    s->mark_states.push_back(rt_scene_dev::mark_state{order_index, stream, std::move(d), known_word(s, s->mark_states.size()), 0u});
    *out = &s->mark_states.back();
  }
  return RT_OK;
}

// Step 3, behind the product launch `L`: the list-driven strict launch (rt_retrace) over the samples the product kernel marked and the
// centre lines - unless this frame is KNOWN to have nothing for it.  `known`: 0 not known (yet), else the frame's mark count + 1.
// Centre row / centre column of a sample grid with an ODD number of rows / columns (supersample 2 makes it even).  The primary
// rays there have a direction component that is EXACTLY zero (main.js:186: x - w/2 + 0.5 == 0), so they - and every ray they
// spawn that stays in that plane - live in a coordinate plane through the camera, and a sphere centred on that plane (the
// reference's own scene has several) is met with a normal component of exactly 0: u or v lands exactly ON a texel / checker
// boundary (main.js:127-130, 344-347), and on which side the reference falls is decided by whether ITS OWN rounding noise
// (e.g. main.js:257-259 at refract_index 1, where q is 0 or 1e-16 depending on the last bit of cosi) pushed the ray off the
// plane.  No arithmetic but the reference's own reproduces such coin flips: rt_retrace traces those samples too.
int retrace_launch(const colour_call &c, const rt_launch &L, const rt_scene_dev::order_entry &oe, rt_scene_dev::mark_state &ms, uint32_t known, retrace_result &o) {
  const rt_scene_dev *s = c.s;
  const rt_tiles *tiles = c.tiles;
  rt_launch F = L;
  F.order = nullptr; F.grid_x = F.grid_y = 0u;
  F.centre_row = F.centre_col = ~0u;
  if (!c.ss2 && (c.h & 1u)) {
    const uint32_t crow = (c.h - 1u) / 2u, tc = crow / tiles->tile_rows;
    if (tc >= tiles->tile_first && (tc - tiles->tile_first) % tiles->tile_stride == 0 && (tc - tiles->tile_first) / tiles->tile_stride < tiles->n_tiles) { F.centre_row = crow; o.centre_items += (uint64_t)c.w * c.n_frames; }
  }
  if (!c.ss2 && (c.w & 1u)) { F.centre_col = (c.w - 1u) / 2u; o.centre_items += (uint64_t)tiles->n_tiles * tiles->tile_rows * c.n_frames; }
  const bool retrace_all = c.t.exact_all && !c.t.no_fixup;
  // (a sky-only launch traces nothing; the centre lines belong to the calls that trace)
  if (c.t.no_fixup || (c.flags & RT_FLAG_SKY_ONLY) || !(known != 1u || o.centre_items != 0 || retrace_all)) return RT_OK;
  bind_kernel(s, F, true, c.t);                         // the scene in its own order, every sphere in the loops, the reference's own miss colour
  if (c.compact) {                                      // where a sample's block sits in the compact band: from the table's own arrays
    const rt_table_dev &T = oe.Tb[s->cam_gen & 1u];
    F.tb_item = T.item; F.tb_rank_in_row = T.rank_in_row; F.tb_row_hist = T.row_hist; F.tb_bin_start = T.bin_start; F.tb_bins = oe.cost_bins;
  }
  F.marks_known = c.t.uncached_marks ? nullptr : (unsigned long long *)ms.h_known;
  F.known_tag = (uint32_t)s->cam_gen;
  F.retrace_all = retrace_all ? 1u : 0u;
  o.retraced_all = retrace_all;
  // The grid.  Count known: its items and the centre lines.  Not known yet (the first frame from a camera): the list may hold up
  // to RT_MARKS_CAP items or have overflowed - 256 workgroups (idle ones leave at once) walk an overflowed 3840x2160 frame at
  // ~130 samples per lane, once; from the next frame on the count is known (and an overflow takes the strict kernel instead).
  uint64_t n_wg = (((known ? known - 1u : 0u) + o.centre_items) * (c.ss2 ? 4u : 1u) + RT_WG_THREADS - 1) / RT_WG_THREADS + 2u;      // (supersample 2: a lane per sample)
  if (!known && n_wg < 256u) n_wg = 256u;
  if (retrace_all) n_wg = ((uint64_t)tiles->n_tiles * tiles->tile_rows * c.w * c.n_frames + RT_WG_THREADS - 1) / RT_WG_THREADS;
  if (n_wg > 8192u) n_wg = 8192u;
  const rt_trace_variant v = rt_trace_variant_of(true, true, s->refract, false, c.ss2, L.cull_in_lds != 0u, L.scatter != 0u, false);
  if (int rc = guard_kernel_scratch(c.D, c.stream, v, n_wg * (RT_WG_THREADS / 64u), "the list-driven strict launch (rt_retrace)")) return rc;
  if (int rc = launched(launch_variant(F, v, (unsigned)n_wg, nullptr, 0u, c.stream))) return rc;
  o.marks_read = (const uint32_t *)ms.d_marks.h; o.marks_read_slot = ms.slot;
  ms.slot ^= 1u;                                        // rt_retrace cleared the other counter: the next launch's
  return RT_OK;
}

// Step 3, product: the launch table (found, or built on the GPU for this camera), the trace, and the list-driven strict launch behind
// it; one step for the threads of this process (under launch_mu).
int product_launch(const colour_call &c, rt_launch &L, marks_guard &temp_marks, retrace_result &o) {
  rt_scene_dev *s = c.s;
  const frame_kind kind = {c.w, c.h, c.ss, *c.tiles, sky_part_of(c.flags)};
  const uint32_t uses_before = c.count ? 0u : count_use(s, kind);
  // the first frame from a camera that has moved: a caller that moves the camera every frame has the next camera's table built
  // beside this launch (rt_scene_set_camera), and that build needs the trace's workgroups to be as wide as its own (rt_launch::four_waves)
  L.four_waves = (!c.count && uses_before == 0u && s->cam_gen != 0u) ? 1u : 0u;
  const int oi = dispatch_order(s, kind, choose_table(s, c.flags, uses_before), c.stream);
  if (oi < 0) return RT_ERR_DEVICE;
  rt_scene_dev::order_entry &oe = s->orders[oi];
  L.order = oe.Tb[s->cam_gen & 1u].entries;
  const uint32_t n_known = table_entries_known(s, oe, c.t);
  L.order_n8 = (oe.n_blocks + 7u) / 8u;
  L.grid_x = n_known ? n_known - 1u : oe.n_blocks;
  L.grid_y = 1u;
  rt_scene_dev::mark_state *ms = nullptr;
  if (int rc = mark_state_for(s, (uint32_t)oi, c.stream, temp_marks, &ms)) return rc;
  L.marks = (uint32_t *)ms->d_marks.h; L.marks_slot = ms->slot;
  const uint32_t known = c.t.uncached_marks ? 0u : known_value(ms->h_known, s->cam_gen);        // 0: not known (yet); else the frame's mark count + 1
  // A frame KNOWN to mark more samples than the list holds (a legal scene can: every hit of a sphere whose sampler coordinate is
  // an exact integer everywhere) would be traced twice in full, product kernel then rt_retrace over every sample: the strict
  // kernel renders it once instead, the same bytes (the count stays known: nothing republishes it for this camera).
  if (known != 0u && known - 1u > RT_MARKS_CAP && !c.count && !c.compact) {
    if (c.flags & RT_FLAG_SKY_ONLY) return RT_OK;       // (as every strict launch: a NO_SKY call stores every pixel, a SKY_ONLY call none)
    rt_launch S = L;
    S.order = nullptr; S.grid_x = S.grid_y = 0u;
    bind_kernel(s, S, true, c.t);
    o.strict_rendered = true;
    return strict_launch(c, S, false);
  }
  // how the trace stores the frame (rt_device.h: rt_wide_stores_of): 16 bytes per lane, write-through, where the launch's shape allows it
  const uint64_t out_bytes = (uint64_t)c.tiles->n_tiles * c.tiles->tile_rows * c.w * 4u * c.n_frames;
  L.wide_stores = c.t.no_wide ? 0u : rt_wide_stores_of(false, L.rgb24 != 0u, L.scatter != 0u, c.w, (uint64_t)(uintptr_t)L.out, c.n_frames, L.frame_stride, c.t.wide_form ? 0u : out_bytes);
  if (L.wide_stores && c.t.wide_form) L.wide_stores = RT_WIDE_STORES | (c.t.wide_form == 2 ? RT_WIDE_THROUGH_SKY | RT_WIDE_THROUGH_TRACED : (c.t.wide_form == 3 ? RT_WIDE_THROUGH_SKY : 0u));
  const rt_trace_variant v = rt_trace_variant_of(false, false, s->refract, c.count, c.ss2, L.cull_in_lds != 0u, L.scatter != 0u, L.four_waves != 0u);
  if (int rc = guard_kernel_scratch(c.D, c.stream, v, (uint64_t)L.grid_x * c.n_frames * (RT_WG_THREADS / 64u), "the trace kernel")) return rc;
#ifdef RT_WAVE_LOG
  // measurement build: RT_WAVE_LOG_FILE=<path> - every wave's entry / exit time and place of THIS launch, written after it has finished
  unsigned long long *d_wave_log = nullptr;
  const size_t wave_log_words = (size_t)((L.grid_x + 7u) / 8u * 8u) * c.n_frames * (RT_WG_THREADS / 64u) * 4u;
  if (getenv("RT_WAVE_LOG_FILE")) {
    if (hipMalloc((void **)&d_wave_log, wave_log_words * 8u) == hipSuccess) (void)hipMemsetAsync(d_wave_log, 0, wave_log_words * 8u, c.stream);
    L.wave_log = d_wave_log;
  }
#endif
  const int err = launch_variant(L, v, 0u, nullptr, lds_for(s, v, c.t.lds_pad), c.stream);
#ifdef RT_WAVE_LOG
  if (d_wave_log) {
    std::vector<unsigned long long> hostlog(wave_log_words);
    (void)hipStreamSynchronize(c.stream);
    (void)hipMemcpy(hostlog.data(), d_wave_log, wave_log_words * 8u, hipMemcpyDeviceToHost);
    (void)hipFree(d_wave_log);
    if (FILE *fp = fopen(getenv("RT_WAVE_LOG_FILE"), "wb")) { fwrite(hostlog.data(), 8u, wave_log_words, fp); fclose(fp); }
    L.wave_log = nullptr;
  }
#endif
  if (int rc = launched(err)) return rc;
  return retrace_launch(c, L, oe, *ms, known, o);
}

int render_batch_impl(rt_scene_dev *s, uint32_t w, uint32_t h, const rt_tiles *tiles, uint32_t n_frames, void *d_out, uint64_t frame_stride_bytes,
                      void *const *d_frames, void *hip_stream, uint32_t flags, rt_stats *stats, uint32_t ss_override) {
  // ---- 1. the arguments ----
  if (!s || !tiles) return fail(RT_ERR_INVALID, "NULL scene, tiles or output");
  if (n_frames == 0 || n_frames > 65535u) return fail(RT_ERR_INVALID, "n_frames %u not in 1..65535", n_frames);
  if ((frame_stride_bytes & 3u) != 0) return fail(RT_ERR_INVALID, "frame stride must be a multiple of 4 bytes");
  int rc = check_frame("render", w, h, tiles, flags);
  if (rc) return rc;
  if ((uint64_t)tiles->n_tiles * tiles->tile_rows * w >= (1ull << 32)) return fail(RT_ERR_INVALID, "a call may cover at most 2^32 - 1 pixels per frame");
  if ((flags & (RT_FLAG_NO_SKY | RT_FLAG_SKY_ONLY)) == (RT_FLAG_NO_SKY | RT_FLAG_SKY_ONLY) || ((flags & (RT_FLAG_NO_SKY | RT_FLAG_SKY_ONLY)) && (flags & RT_FLAG_COUNT)))
    return fail(RT_ERR_INVALID, "RT_FLAG_NO_SKY and RT_FLAG_SKY_ONLY exclude each other and RT_FLAG_COUNT");
  if ((flags & RT_FLAG_COMPACT) && ((flags & (RT_FLAG_RGB24 | RT_FLAG_NO_SKY | RT_FLAG_COUNT | RT_FLAG_STRICT_FP)) != (RT_FLAG_RGB24 | RT_FLAG_NO_SKY) || d_frames))
    return fail(RT_ERR_INVALID, "RT_FLAG_COMPACT goes with RT_FLAG_RGB24 | RT_FLAG_NO_SKY into a band (no counting, no strict kernel, no scatter)");
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  device_state &D = G.dev[s->device];
  stats_clock clock;
  uint32_t stars_seed;
  {
    // which streams the scene's launches run on (rt_scene_set_camera, dispatch_order), and: behind the last write of the camera block
    std::lock_guard<std::mutex> lk(s->launch_mu);
    stars_seed = s->hd.stars_seed;                     // (rt_scene_set_stars_seed: this launch's, whatever the next call sets)
    if ((rc = enter_launch(s, stream))) return rc;
  }
  const uint32_t ss = ss_override ? ss_override : s->hd.supersample;
  if (ss > 2u) {
    // (3x3 / 4x4 supersampling filters whole blocks of samples: a NO_SKY call stores every pixel, a SKY_ONLY call none)
    if (flags & RT_FLAG_SKY_ONLY) { if (stats) memset(stats, 0, sizeof *stats); return RT_OK; }
    return render_supersampled(s, ss, w, h, tiles, n_frames, d_out, frame_stride_bytes, d_frames, stream, flags & ~(uint32_t)RT_FLAG_NO_SKY, stats);
  }
  const colour_call c = {s, D, stream, w, h, ss, tiles, n_frames, flags, ss == 2u, (flags & RT_FLAG_COUNT) != 0, (flags & RT_FLAG_COMPACT) != 0, read_test_switches()};
  const bool strict_main = (flags & RT_FLAG_STRICT_FP) != 0 || strict_scene(s);
  if (c.compact && strict_main) return fail(RT_ERR_UNSUPPORTED, "RT_FLAG_COMPACT: this scene is rendered by the strict kernel (or supersampled 3x3 / 4x4), which knows no launch table: send plain bands");

  // ---- 2. the launch record ----
  rt_launch L;
  if ((rc = fill_launch(c, strict_main, stars_seed, d_out, frame_stride_bytes, d_frames, L))) return rc;
  if (c.count) HIP_TRY(hipMemsetAsync(D.d_counters, 0, 3 * sizeof(unsigned long long), stream));
  if ((rc = clock.start(stats, stream))) return rc;

  // ---- 3. the strict launch, or the product launch and the list-driven strict launch behind it ----
  marks_guard temp_marks;
  retrace_result o;
  // (the strict kernels know no sky blocks: the RT_FLAG_NO_SKY calls of a strict launch store every pixel, its RT_FLAG_SKY_ONLY call none)
  if (!(strict_main && (flags & RT_FLAG_SKY_ONLY))) {
    std::lock_guard<std::mutex> lk(s->launch_mu);
    rc = strict_main ? strict_launch(c, L, c.count) : product_launch(c, L, temp_marks, o);
  }
  if (rc) return rc;

  // ---- 4. the stats ----
  if ((rc = clock.finish(stats, stats ? tile_set_pixels(w, h, tiles) * n_frames : 0u))) return rc;
  if (stats) {
    if (c.count) {
      unsigned long long n[3];
      HIP_TRY(hipMemcpy(n, D.d_counters, sizeof n, hipMemcpyDeviceToHost));
      stats->rays = n[0]; stats->shadow_rays = n[1]; stats->sphere_tests = n[2];
    }
    // samples the second launch traced again: the marked ones (read back from the list's counter) and the odd grid's centre lines
    if (o.strict_rendered) stats->exact_samples = stats->pixels;      // the strict kernel rendered the call
    if (o.marks_read) {
      uint32_t n_marked = 0;
      HIP_TRY(hipMemcpy(&n_marked, o.marks_read + o.marks_read_slot, sizeof n_marked, hipMemcpyDeviceToHost));
      stats->exact_samples = (n_marked > RT_MARKS_CAP || o.retraced_all) ? stats->pixels : n_marked + o.centre_items;   // (list overflow / test build: every pixel of the call)
    }
    stats->total_ms = clock.host_ms();                  // (with the read-backs)
  }
  return RT_OK;
}
}  // namespace

// How many workgroups of its trace kernel a CU holds at once for a colour launch of this resident scene, by the runtime's own count
// (hipOccupancyMaxActiveBlocksPerMultiprocessor: the kernel's registers and the launch's dynamic LDS), and that LDS size.  The variant
// and the LDS size are worked out as product_launch does: `four_waves` - the first frame from a moved camera (rt_launch::four_waves).
// Nothing is launched.  (tests/test_gpu_occupancy.py: six waves per SIMD are 24 one-wave workgroups.)
extern "C" int rt_scene_trace_occupancy(rt_scene_dev *s, int four_waves, int *out_workgroups_per_cu, uint32_t *out_lds_bytes) {
  if (!s || !out_workgroups_per_cu) return fail(RT_ERR_INVALID, "rt_scene_trace_occupancy: NULL argument");
  if (int rc = ensure_device(s->device)) return rc;
  HIP_TRY(hipSetDevice(G.dev[s->device].hip_id));
  const uint32_t ss = s->hd.supersample;
  if (ss > 2u) return fail(RT_ERR_UNSUPPORTED, "rt_scene_trace_occupancy: supersample %u renders on the sample grid", ss);
  const rt_trace_variant v = rt_trace_variant_of(strict_scene(s), false, s->refract, false, ss == 2u, s->cull_in_lds, false, four_waves != 0);
  const void *f = (v.strict ? rt_kernel_trace_strict : rt_kernel_trace_fast)(v);
  if (!f) return fail(RT_ERR_DEVICE, "rt_scene_trace_occupancy: no kernel for the variant");
  const unsigned lds = lds_for(s, v, 0u);
  int n = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, f, v.one_wave ? 64 : (int)RT_WG_THREADS, lds));
  *out_workgroups_per_cu = n;
  if (out_lds_bytes) *out_lds_bytes = lds;
  return RT_OK;
}

// ------------------------------------------------------------------------------------ adaptive supersampling (rt_adaptive.hip)
// k x k samples only where the frame has edges (include/rt_hip.h: rt_render_adaptive_device).  Three launches follow each other on the
// caller's stream, with no allocation and no host wait between them: the ordinary colour launch of the supersample-1 frame
// (render_batch_impl, unchanged: the same tables, marks and rt_retrace, the same bytes), rt_adaptive_mark - the criterion on that frame,
// the list of pixels to refine in the caller's workspace - and rt_adaptive_refine<refract, k>, which traces the listed pixels' samples
// on a launch record of the k w x k h sample grid bound as rt_retrace's (fill_launch with the plain binding) and stores their box-filtered
// bytes over the base frame's.  The refine kernel keeps a recursion stack: its scratch figure goes through scratch_guard like every other.
extern "C" size_t rt_adaptive_work_bytes(uint32_t w, uint32_t h) {
  return (w == 0 || h == 0 || w > 65536u / 2u || h > 65536u / 2u) ? 0 : (size_t)rt_adaptive_bytes(w, h);      // (k >= 2: a side above 32768 is refused for every k)
}

#ifdef RT_TESTING
// Test build only: the criterion and the box rule of rt_adaptive.h as plain host code, without a GPU.  mask_out: w * h bytes, 1 = refined.
extern "C" int rt_test_adaptive_mask(const uint8_t *rgba, uint32_t w, uint32_t h, uint32_t threshold, uint8_t *mask_out) {
  if (!rgba || !mask_out || w == 0 || h == 0 || threshold > 256u) return fail(RT_ERR_INVALID, "rt_test_adaptive_mask: NULL argument, empty frame or threshold above 256");
  const auto at = [&](uint32_t x, uint32_t y) { uint32_t v; memcpy(&v, rgba + ((size_t)y * w + x) * 4u, 4u); return v; };
  for (uint32_t y = 0; y < h; y++)
    for (uint32_t x = 0; x < w; x++) {
      const uint32_t c = at(x, y);
      mask_out[(size_t)y * w + x] = rt_adaptive_refines(c, x > 0u ? at(x - 1u, y) : c, x + 1u < w ? at(x + 1u, y) : c, y > 0u ? at(x, y - 1u) : c,
                                                        y + 1u < h ? at(x, y + 1u) : c, threshold) ? 1u : 0u;
    }
  return RT_OK;
}
extern "C" uint32_t rt_test_adaptive_box(uint32_t sum, uint32_t k) { return rt_adaptive_box(sum, k); }
// ... and the refine launch's grid, so that a test knows whether a frame's list can outrun one turn of the kernel's loop
extern "C" uint32_t rt_test_adaptive_refine_grid(uint32_t w, uint32_t h, uint32_t k) { return rt_adaptive_refine_grid(w, h, k); }
#endif

namespace {
// the scratch bytes per lane of rt_adaptive_refine<refract, k>, asked once per kernel
int adaptive_scratch(bool refract, uint32_t k, size_t *out) {
  static std::mutex mu;
  static size_t cache[2][5];
  static bool have[2][5];
  std::lock_guard<std::mutex> lk(mu);
  if (!have[refract][k]) {
    size_t b = 0;
    const int e = rt_scratch_adaptive_refine(refract, k, &b);
    if (e != 0) return fail(RT_ERR_DEVICE, "hipFuncGetAttributes: %s", hipGetErrorString((hipError_t)e));
    cache[refract][k] = b; have[refract][k] = true;
  }
  *out = cache[refract][k];
  return RT_OK;
}
}  // namespace

// (the arguments first: they are judged without a scene, and before a device is touched)
extern "C" int rt_render_adaptive_device(rt_scene_dev *s, uint32_t w, uint32_t h, uint32_t k, uint32_t threshold, void *d_out, uint8_t *d_mask,
                                         void *d_work, size_t work_bytes, void *hip_stream, uint32_t flags, rt_stats *stats) {
  const char *const what = "rt_render_adaptive_device";
  if (k < 2u || k > 4u) return fail(RT_ERR_INVALID, "%s: k %u not in 2..4", what, k);
  if (threshold > 256u) return fail(RT_ERR_INVALID, "%s: threshold %u not in 0..256", what, threshold);
  if (w == 0 || h == 0 || (uint64_t)w * k > 65536u || (uint64_t)h * k > 65536u)
    return fail(RT_ERR_INVALID, "%s: frame size %ux%u: the %llu x %llu sample grid is not in 1..65536", what, w, h, (unsigned long long)w * k, (unsigned long long)h * k);
  if (!d_out || !d_work) return fail(RT_ERR_INVALID, "%s: NULL output or workspace", what);
  if (((uintptr_t)d_out & 3u) || ((uintptr_t)d_work & 3u)) return fail(RT_ERR_INVALID, "%s: misaligned output or workspace (4 bytes)", what);
  if (work_bytes < rt_adaptive_work_bytes(w, h))
    return fail(RT_ERR_INVALID, "%s: work_bytes %llu below rt_adaptive_work_bytes(%u, %u) = %llu", what, (unsigned long long)work_bytes, w, h, (unsigned long long)rt_adaptive_work_bytes(w, h));
  if (flags & ~(uint32_t)RT_FLAG_STRICT_FP) return fail(RT_ERR_INVALID, "%s: flags 0x%x: only RT_FLAG_STRICT_FP applies (to the base launch)", what, flags);
  if (!s) return fail(RT_ERR_STATE, "%s: NULL scene handle", what);
  if (s->hd.supersample != 1u) return fail(RT_ERR_INVALID, "%s: the scene's header supersample is %u: the base frame is a supersample-1 frame", what, s->hd.supersample);
  hipStream_t stream = nullptr;
  int rc = scene_stream(s, hip_stream, &stream);
  if (rc) return rc;
  device_state &D = G.dev[s->device];
  // the refine launch's grid (rt_adaptive.h): the count is only known on the device
  static_assert(RT_ADAPTIVE_REFINE_WAVES == RT_WG_THREADS / 64u, "rt_adaptive_refine_grid counts the waves of a trace workgroup");
  const unsigned n_wg = rt_adaptive_refine_grid(w, h, k);
  size_t per_lane = 0;
  if ((rc = adaptive_scratch(s->refract, k, &per_lane))) return rc;
  if ((rc = scratch_guard(D, stream, per_lane, (uint64_t)n_wg * (RT_WG_THREADS / 64u), "the adaptive refine kernel (rt_adaptive_refine)"))) return rc;
  stats_clock clock;
  if ((rc = clock.start(stats, stream))) return rc;

  // 1. the base frame
  const rt_tiles whole = {h, 0u, 1u, 1u};
  if ((rc = render_batch_impl(s, w, h, &whole, 1u, d_out, 0u, nullptr, hip_stream, flags, nullptr))) return rc;

  // 2. the criterion
  HIP_TRY(hipMemsetAsync(d_work, 0, RT_ADAPTIVE_HEADER_BYTES, stream));
  const rt_adaptive_mark_launch M = {(const uint32_t *)d_out, d_mask, (uint32_t *)d_work, w, h, threshold};
  if ((rc = launched(rt_launch_adaptive_mark(&M, stream)))) return rc;

  // 3. the listed pixels, from the k w x k h sample grid (a whole frame of it, one sample per "pixel" of the record: supersample 1)
  const rt_tiles grid_tiles = {h * k, 0u, 1u, 1u};
  const colour_call c = {s, D, stream, w * k, h * k, 1u, &grid_tiles, 1u, 0u, false, false, false, read_test_switches()};
  rt_launch F;
  {
    std::lock_guard<std::mutex> lk(s->launch_mu);
    if ((rc = enter_launch(s, stream))) return rc;
    if ((rc = fill_launch(c, true, s->hd.stars_seed, nullptr, 0u, nullptr, F))) return rc;      // (strict: the scene in its own order, as rt_retrace is bound)
  }
  const rt_adaptive_refine_launch A = {(const uint32_t *)d_work, (uint32_t *)d_out, w};
  if ((rc = launched(rt_launch_adaptive_refine(&F, &A, s->refract ? 1 : 0, k, n_wg, stream)))) return rc;
  return clock.finish(stats, (uint64_t)w * h);
}

// ------------------------------------------------------------------------------------ compact bands (RT_FLAG_COMPACT)
namespace {
// The launch table a compact launch over `tiles` uses (found, or built now on `stream`), under launch_mu: its index in *oi, the rows
// of a block in *rows_per_wg.  The product launch's own choice (choose_table) for a camera's first frame: masks do not matter for the
// ORDER of the blocks - a table with and one without them list the same blocks at the same places.
int compact_table(rt_scene_dev *s, uint32_t w, uint32_t h, const rt_tiles *tiles, hipStream_t stream, int *oi, uint32_t *rows_per_wg) {
  const uint32_t flags = RT_FLAG_RGB24 | RT_FLAG_NO_SKY | RT_FLAG_COMPACT;
  if (!tiles) return fail(RT_ERR_INVALID, "compact band: NULL tiles");
  if (int rc = check_frame("compact band", w, h, tiles, flags)) return rc;
  const uint32_t ss = s->hd.supersample;
  if (ss > 2u || strict_scene(s)) return fail(RT_ERR_UNSUPPORTED, "compact bands: this scene is rendered by the strict kernel (or supersampled 3x3 / 4x4): send plain bands");
  HIP_TRY(s->sync.before_launch(stream, s->cam_gen));
  *rows_per_wg = launch_geometry(s->hd.fov_deg, w, h, ss, tiles->tile_rows).rows_per_wg;
  *oi = dispatch_order(s, frame_kind{w, h, ss, *tiles, sky_part_of(flags)}, choose_table(s, flags, 0u), stream);
  return *oi < 0 ? RT_ERR_DEVICE : RT_OK;
}

struct rt_expand_launch { const uint32_t *entries; uint32_t n8, n_blocks, w, rows_per_wg; const uint8_t *src; uint32_t *dst; };
// one workgroup of 256 per entry: the block's 32 x RH pixels (RGB24, row by row) to their place in the RGBA8 frame
__global__ void __launch_bounds__(256) rt_compact_expand_kernel(const rt_expand_launch E) {
  const uint32_t b = blockIdx.x;
  const uint4 e = ((const uint4 *)E.entries)[(size_t)(b & 7u) * E.n8 + (b >> 3)];
  const uint32_t tile_x = e.x & 2047u, rows_valid = (e.x >> 11) & 15u, frow0 = e.x >> 15;
  if (rows_valid == 0u || (e.y >> 31)) return;                     // (no entry, or a sky run: not part of a compact band)
  const uint32_t r = threadIdx.x >> 5, i = threadIdx.x & 31u, px = tile_x * RT_TILE_W + i;
  if (r >= rows_valid || r >= E.rows_per_wg || px >= E.w) return;
  const uint8_t *p = E.src + (size_t)b * (RT_TILE_W * 3u * E.rows_per_wg) + ((size_t)r * RT_TILE_W + i) * 3u;
  E.dst[(size_t)(frow0 + r) * E.w + px] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | 0xff000000u;
}
}  // namespace

extern "C" int rt_compact_count(rt_scene_dev *s, uint32_t w, uint32_t h, const rt_tiles *tiles, void *hip_stream, uint32_t *n_blocks, uint32_t *block_bytes) {
  if (!n_blocks || !block_bytes) return fail(RT_ERR_INVALID, "rt_compact_count: NULL argument");
  hipStream_t stream = nullptr;
  int rc = s ? scene_stream(s, hip_stream, &stream) : RT_ERR_INVALID;
  if (rc) return rc == RT_ERR_INVALID ? fail(RT_ERR_INVALID, "NULL scene") : rc;
  uint32_t rows_per_wg = 0, header[4];
  const uint32_t *d_header = nullptr;
  {
    std::lock_guard<std::mutex> lk(s->launch_mu);
    int oi = -1;
    if ((rc = compact_table(s, w, h, tiles, stream, &oi, &rows_per_wg))) return rc;
    d_header = s->orders[oi].Tb[s->cam_gen & 1u].header;
  }
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipMemcpy(header, d_header, sizeof header, hipMemcpyDeviceToHost));
  *n_blocks = header[2];                                             // the entries in front of the sky runs' class: a ranked table's non-sky blocks
  *block_bytes = RT_TILE_W * 3u * rows_per_wg;
  return RT_OK;
}

extern "C" int rt_compact_expand_device(rt_scene_dev *s, uint32_t w, uint32_t h, const rt_tiles *tiles, const void *d_compact, void *d_frame, void *hip_stream) {
  if (!d_compact || !d_frame || ((uintptr_t)d_frame & 3u)) return fail(RT_ERR_INVALID, "rt_compact_expand_device: NULL or unaligned buffer");
  hipStream_t stream = nullptr;
  int rc = s ? scene_stream(s, hip_stream, &stream) : RT_ERR_INVALID;
  if (rc) return rc == RT_ERR_INVALID ? fail(RT_ERR_INVALID, "NULL scene") : rc;
  rt_expand_launch E;
  uint32_t grid = 0;
  {
    std::lock_guard<std::mutex> lk(s->launch_mu);
    uint32_t rows_per_wg = 0;
    int oi = -1;
    if ((rc = compact_table(s, w, h, tiles, stream, &oi, &rows_per_wg))) return rc;
    const rt_scene_dev::order_entry &oe = s->orders[oi];
    E.entries = oe.Tb[s->cam_gen & 1u].entries; E.n8 = (oe.n_blocks + 7u) / 8u; E.n_blocks = oe.n_blocks; E.w = w; E.rows_per_wg = rows_per_wg;
    E.src = (const uint8_t *)d_compact; E.dst = (uint32_t *)d_frame;
    const uint32_t n_known = known_value(oe.known, s->cam_gen);
    grid = n_known ? n_known - 1u : oe.n_blocks;                     // (workgroups behind the last entry read a zero slot and leave)
    s->sync.note_launch(stream);
  }
  if (grid) hipLaunchKernelGGL(rt_compact_expand_kernel, dim3(grid), dim3(256), 0, stream, E);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

// ------------------------------------------------------------------------------------ primary hits (rt_hits.hip)
// What is under a sample: the hit kernels read the sphere records of the scene's current generation (its object block: an object move
// writes the other one, rt_scene_set_objects) and take the camera from the scene's host state at the call.  So they come behind the
// generation's preparation on the side stream, like a colour launch, and count as launches of the scene for the next move's events.
namespace rt_api {
int hits_frame_check(uint32_t w, uint32_t h, uint32_t k, const char *what) {
  if (int rc = check_frame(what, w, h, nullptr, 0u)) return rc;
  if ((uint64_t)k * w * k * h >= (1ull << 32)) return fail(RT_ERR_INVALID, "%s: a sample grid of %ux%u exceeds 2^32 - 1 samples", what, k * w, k * h);
  return RT_OK;
}

int pick_points_check(uint32_t w, uint32_t h, uint32_t k, uint32_t n, const uint32_t *xy, const void *out, const char *what) {
  if (!xy || !out) return fail(RT_ERR_INVALID, "%s: NULL points or output", what);
  if (n == 0 || n > 65536u) return fail(RT_ERR_INVALID, "%s: n %u not in 1..65536", what, n);
  int rc = hits_frame_check(w, h, k, what);
  if (rc) return rc;
  for (uint32_t j = 0; j < n; j++)
    if (xy[2 * j] >= k * w || xy[2 * j + 1] >= k * h)
      return fail(RT_ERR_INVALID, "%s: point %u (%u, %u) lies outside the %ux%u sample grid", what, j, xy[2 * j], xy[2 * j + 1], k * w, k * h);
  return RT_OK;
}

// the launch record's scene part: blob-order spheres, the CURRENT camera, the projection of the k w x k h sample grid
int hits_bind(rt_scene_dev *s, uint32_t w, uint32_t h, rt_hits_launch &L, hipStream_t stream) {
  memset(&L, 0, sizeof L);
  std::lock_guard<std::mutex> lk(s->launch_mu);
  if (int rc = enter_launch(s, stream)) return rc;
  const rt_scene_header &hd = s->hd;
  L.objects = (const rt_sphere *)(obj_block(s) + s->o_objs);
  memcpy(L.cam, hd.cam_origin, 12 * sizeof(double));   // origin, axisX, axisY, axisZ are contiguous
  L.k = hd.supersample;
  L.sw = L.k * w; L.sh = L.k * h;
  const launch_geom g = launch_geometry(hd.fov_deg, w, h, L.k, 0u);
  L.proj_w = g.proj_w; L.proj_h = g.proj_h; L.proj_d = g.proj_d;
  L.epsilon = hd.epsilon;
  L.n_objects = hd.n_objects;
  return RT_OK;
}
}  // namespace rt_api

extern "C" int rt_render_hits_device(rt_scene_dev *s, uint32_t w, uint32_t h, const rt_tiles *tiles, const rt_hit_buffers *b, void *hip_stream,
                                     rt_stats *stats) {
  if (!s) return fail(RT_ERR_STATE, "rt_render_hits_device: NULL scene handle");
  if (!tiles || !b) return fail(RT_ERR_INVALID, "rt_render_hits_device: NULL tiles or buffers");
  int rc = hits_frame_check(w, h, s->hd.supersample, "rt_render_hits_device");
  if (rc) return rc;
  if ((rc = check_frame("rt_render_hits_device", w, h, tiles, 0u))) return rc;
  if (((uintptr_t)b->id & 3u) || ((uintptr_t)b->depth & 7u) || ((uintptr_t)b->normal & 3u))
    return fail(RT_ERR_INVALID, "rt_render_hits_device: misaligned buffer (id and normal need 4 bytes, depth 8)");
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  stats_clock clock;
  rt_hits_launch L;
  if ((rc = hits_bind(s, w, h, L, stream))) return rc;
  L.id = b->id; L.depth = b->depth; L.normal = b->normal;
  L.tile_rows = tiles->tile_rows; L.tile_first = tiles->tile_first; L.tile_stride = tiles->tile_stride;
  L.band_rows = tiles->n_tiles * L.k * tiles->tile_rows;
  if ((rc = clock.start(stats, stream))) return rc;
  if (L.id || L.depth || L.normal) {
    const int e = rt_launch_hits(&L, stream);
    if (e != 0) return fail(RT_ERR_DEVICE, "hits kernel launch: %s", hipGetErrorString((hipError_t)e));
  }
  return clock.finish(stats, stats ? tile_set_pixels(w, h, tiles) : 0u);
}

extern "C" int rt_scene_pick(rt_scene_dev *s, uint32_t w, uint32_t h, uint32_t n, const uint32_t *xy, rt_hit *out) {
  if (!s) return fail(RT_ERR_STATE, "rt_scene_pick: NULL scene handle");
  int rc = pick_points_check(w, h, s->hd.supersample, n, xy, out, "rt_scene_pick");
  if (rc) return rc;
  if ((rc = ensure_device(s->device))) return rc;
  device_state &D = G.dev[s->device];
  rt_hits_launch L;
  if ((rc = hits_bind(s, w, h, L, D.stream))) return rc;
  L.n_points = n;
  device_mem mem;
  HIP_TRY(hipMalloc(&mem.h, (size_t)n * (sizeof(rt_hit) + 2u * sizeof(uint32_t))));
  L.hits = (rt_hit *)mem.h;
  L.points = (const uint32_t *)((uint8_t *)mem.h + (size_t)n * sizeof(rt_hit));
  HIP_TRY(hipMemcpyAsync((void *)L.points, xy, (size_t)n * 2u * sizeof(uint32_t), hipMemcpyHostToDevice, D.stream));
  const int e = rt_launch_pick(&L, D.stream);
  if (e != 0) return fail(RT_ERR_DEVICE, "pick kernel launch: %s", hipGetErrorString((hipError_t)e));
  HIP_TRY(hipMemcpyAsync(out, L.hits, (size_t)n * sizeof(rt_hit), hipMemcpyDeviceToHost, D.stream));
  HIP_TRY(hipStreamSynchronize(D.stream));
  return RT_OK;
}

// ------------------------------------------------------------------------------------ caller-supplied rays (rt_kernel.hip: rt_trace_rays)
// intersectWorld for a list of rays (include/rt_hip.h: rt_scene_trace_rays_device).  One launch decision: the strict build's
// rt_trace_rays<refract> for the colours - the scene in its own order, every sphere in the loops, the reference's own miss colour
// (bind_scene_order, as rt_retrace is bound); camera, launch tables and flags play no part - and rt_hits.hip's rt_ray_hit_kernel for the hit records.  Both
// read the scene's current generation, so they come behind its preparation like every other launch of the scene.
// With an order (rt_scene_trace_rays_ordered_device) the same two kernels take their rays through it: the same launch, one more pointer.
// The ordering itself (rt_scene_order_rays_device -> rt_rays_order.hip) reads the rays and nothing of the scene: it waits for no edit.
namespace rt_api {
// what every list of rays or segments must be, once it is known not to be NULL: its count, and (each check at its own place) its alignment
int ray_list_count_check(uint64_t n, const char *what) { return (n == 0 || n >= (1ull << 31)) ? fail(RT_ERR_INVALID, "%s: n %llu not in 1..2^31 - 1", what, (unsigned long long)n) : RT_OK; }
int ray_list_align_check(const double *rays, const char *what) { return ((uintptr_t)rays & 15u) ? fail(RT_ERR_INVALID, "%s: the ray list must be 16-byte aligned", what) : RT_OK; }

int rays_check(uint64_t n, const double *rays, uint32_t segs, const rt_ray_outputs *out, const char *what) {
  if (!rays || !out) return fail(RT_ERR_INVALID, "%s: NULL rays or outputs", what);
  if (int rc = ray_list_count_check(n, what)) return rc;
  if (segs > RT_MAX_SEGS) return fail(RT_ERR_INVALID, "%s: segs %u not in 0..%u (0 = the scene's depth)", what, segs, RT_MAX_SEGS);
  if (!out->rgb && !out->rgba && !out->hits) return fail(RT_ERR_INVALID, "%s: every output is NULL", what);
  if (int rc = ray_list_align_check(rays, what)) return rc;
  if (((uintptr_t)out->rgb & 7u) || ((uintptr_t)out->rgba & 3u) || ((uintptr_t)out->hits & 7u))
    return fail(RT_ERR_INVALID, "%s: misaligned output (rgb and hits need 8 bytes, rgba 4)", what);
  return RT_OK;
}

int rays_order_check(uint64_t n, const double *rays, const uint32_t *order, const void *work, size_t work_bytes, const char *what) {
  if (!rays || !order || !work) return fail(RT_ERR_INVALID, "%s: NULL rays, order or workspace", what);
  if (int rc = ray_list_count_check(n, what)) return rc;
  if (int rc = ray_list_align_check(rays, what)) return rc;
  if (((uintptr_t)order & 3u) || ((uintptr_t)work & 3u)) return fail(RT_ERR_INVALID, "%s: misaligned order or workspace (4 bytes)", what);
  if (work_bytes < rt_rays_order_work_bytes(n))
    return fail(RT_ERR_INVALID, "%s: work_bytes %llu below rt_rays_order_work_bytes(%llu) = %llu", what, (unsigned long long)work_bytes,
                (unsigned long long)n, (unsigned long long)rt_rays_order_work_bytes(n));
  return RT_OK;
}

int order_rays_launch(uint32_t n, const double *d_rays, uint32_t *d_order, void *d_work, hipStream_t stream) {
  const int err = rt_launch_order_rays(n, d_rays, d_order, d_work, stream);
  if (err != 0) return fail(RT_ERR_DEVICE, "ray ordering launch: %s", hipGetErrorString((hipError_t)err));
  return RT_OK;
}

int trace_rays_launch(rt_scene_dev *s, uint32_t n, uint32_t base, const double *d_rays, const uint32_t *d_order, uint32_t segs, const rt_ray_outputs &out,
                      hipStream_t stream, rt_stats *stats) {
  stats_clock clock;
  const rt_scene_header &hd = s->hd;
  rt_launch L;
  memset(&L, 0, sizeof L);
  {
    std::lock_guard<std::mutex> lk(s->launch_mu);
    if (int rc = enter_launch(s, stream)) return rc;
    L.stars_seed = hd.stars_seed;                      // (rt_scene_set_stars_seed: this launch's, whatever the next call sets)
    bind_scene_order(s, L);                            // (materials and texture descriptors are read from HBM)
  }
  L.textures = s->d_texdesc;
  L.texel_base = (const uint8_t *)s->d_blob;
  L.n_objects = hd.n_objects; L.n_lights = hd.n_lights;
  memcpy(L.lights, s->lights, sizeof L.lights);
  L.epsilon = hd.epsilon; L.light_intensity = hd.light_intensity;
  L.segs = segs ? segs : hd.segs;                      // the CALL's depth
  L.n_frames = 1u;
  L.rays = d_rays; L.ray_rgb = out.rgb; L.ray_rgba = (uint32_t *)out.rgba; L.n_rays = n; L.ray_base = base;
  if (int rc = clock.start(stats, stream)) return rc;
  if (out.rgb || out.rgba) {
    // one work-item per ray; the grid-stride loop takes over beyond 2^20 workgroups
    const uint32_t wgs = (n + RT_WG_THREADS - 1u) / RT_WG_THREADS, n_wg = wgs < (1u << 20) ? wgs : (1u << 20);
    const rt_trace_variant v = rt_trace_variant_of_rays(s->refract);
    if (int rc = guard_kernel_scratch(G.dev[s->device], stream, v, (uint64_t)n_wg * (RT_WG_THREADS / 64u), "the ray-list kernel (rt_trace_rays)")) return rc;
    const int err = launch_variant(L, v, n_wg, d_order, 0u, stream);
    if (err != 0) return fail(RT_ERR_DEVICE, "ray kernel launch: %s", hipGetErrorString((hipError_t)err));
  }
  if (out.hits) {
    rt_hits_launch H;
    memset(&H, 0, sizeof H);
    H.objects = L.objects;
    H.epsilon = hd.epsilon;
    H.n_objects = hd.n_objects;
    H.rays = d_rays; H.n_rays = n; H.hits = out.hits; H.ray_order = d_order;
    const int err = rt_launch_ray_hits(&H, stream);
    if (err != 0) return fail(RT_ERR_DEVICE, "ray hit kernel launch: %s", hipGetErrorString((hipError_t)err));
  }
  return clock.finish(stats, n);
}
}  // namespace rt_api

extern "C" int rt_scene_trace_rays_device(rt_scene_dev *s, uint64_t n, const double *d_rays, uint32_t segs, const rt_ray_outputs *d_out, void *hip_stream,
                                          rt_stats *stats) {
  if (!s) return fail(RT_ERR_STATE, "rt_scene_trace_rays_device: NULL scene handle");
  int rc = rays_check(n, d_rays, segs, d_out, "rt_scene_trace_rays_device");
  if (rc) return rc;
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return trace_rays_launch(s, (uint32_t)n, 0u, d_rays, nullptr, segs, *d_out, stream, stats);
}

extern "C" size_t rt_rays_order_work_bytes(uint64_t n) { return (n == 0 || n >= (1ull << 31)) ? 0 : rt_order_layout_of(n).bytes; }
#ifdef RT_TESTING
// Test build only: the grid of the bounds and key kernels and the sort's tile count for n rays (rt_rays_order.h), so that a test knows
// whether a list reaches the second turn of their loops and the second chunk of rt_order_scan.  Host arithmetic, no GPU.
extern "C" uint32_t rt_test_order_grid(uint32_t n) { return rt_order_grid(n); }
extern "C" uint32_t rt_test_order_tiles(uint64_t n) { return rt_order_layout_of(n).tiles; }
#endif

// (the arguments first: they are judged without a scene, and before a device is touched)
extern "C" int rt_scene_order_rays_device(rt_scene_dev *s, uint64_t n, const double *d_rays, uint32_t *d_order, void *d_work, size_t work_bytes,
                                          void *hip_stream) {
  int rc = rays_order_check(n, d_rays, d_order, d_work, work_bytes, "rt_scene_order_rays_device");
  if (rc) return rc;
  if (!s) return fail(RT_ERR_STATE, "rt_scene_order_rays_device: NULL scene handle");
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return order_rays_launch((uint32_t)n, d_rays, d_order, d_work, stream);
}

extern "C" int rt_scene_trace_rays_ordered_device(rt_scene_dev *s, uint64_t n, const double *d_rays, const uint32_t *d_order, uint32_t segs,
                                                  const rt_ray_outputs *d_out, void *hip_stream, rt_stats *stats) {
  int rc = rays_check(n, d_rays, segs, d_out, "rt_scene_trace_rays_ordered_device");
  if (rc) return rc;
  if (!d_order || ((uintptr_t)d_order & 3u)) return fail(RT_ERR_INVALID, "rt_scene_trace_rays_ordered_device: NULL or misaligned order (4 bytes)");
  if (!s) return fail(RT_ERR_STATE, "rt_scene_trace_rays_ordered_device: NULL scene handle");
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  return trace_rays_launch(s, (uint32_t)n, 0u, d_rays, d_order, segs, *d_out, stream, stats);
}

// ------------------------------------------------------------------------------------ occlusion queries (rt_occlusion.hip)
// The reference's shadow scan (main.js:293-304) for a list of segments (include/rt_hip.h: rt_scene_occlusion_device).  One kernel, no
// launch decision: it reads the current generation's spheres in blob order, epsilon and the light intensity - camera, launch tables,
// flags, textures and the lights' positions play no part - so it comes behind the scene's preparation like every other launch.
namespace rt_api {
int occlusion_check(uint64_t n, const double *rays, const rt_occlusion_inputs *in, const rt_occlusion_outputs *out, const char *what) {
  if (!rays || !out) return fail(RT_ERR_INVALID, "%s: NULL rays or outputs", what);
  if (int rc = ray_list_count_check(n, what)) return rc;
  if (!out->intensity && !out->blocker) return fail(RT_ERR_INVALID, "%s: every output is NULL", what);
  if (int rc = ray_list_align_check(rays, what)) return rc;
  if (in && (((uintptr_t)in->length & 7u) || ((uintptr_t)in->intensity & 7u) || ((uintptr_t)in->skip & 3u)))
    return fail(RT_ERR_INVALID, "%s: misaligned input (length and intensity need 8 bytes, skip 4)", what);
  if (((uintptr_t)out->intensity & 7u) || ((uintptr_t)out->blocker & 3u))
    return fail(RT_ERR_INVALID, "%s: misaligned output (intensity needs 8 bytes, blocker 4)", what);
  return RT_OK;
}

int occlusion_launch(rt_scene_dev *s, uint32_t n, const double *d_rays, const uint32_t *d_order, const rt_occlusion_inputs &in,
                     const rt_occlusion_outputs &out, hipStream_t stream, rt_stats *stats) {
  stats_clock clock;
  const rt_scene_header &hd = s->hd;
  rt_occlusion_launch L;
  memset(&L, 0, sizeof L);
  {
    std::lock_guard<std::mutex> lk(s->launch_mu);
    if (int rc = enter_launch(s, stream)) return rc;
    L.objects = (const rt_sphere *)(obj_block(s) + s->o_objs);   // this generation's spheres, in blob order
    L.light_intensity = hd.light_intensity;                      // (rt_scene_set_light_intensity: this launch's)
  }
  L.epsilon = hd.epsilon;
  L.n_objects = hd.n_objects;
  L.rays = d_rays; L.n_rays = n; L.order = d_order;
  L.length = in.length; L.intensity_in = in.intensity; L.skip = in.skip;
  L.intensity = out.intensity; L.blocker = out.blocker;
  if (int rc = clock.start(stats, stream)) return rc;
  const int err = rt_launch_occlusion(&L, stream);
  if (err != 0) return fail(RT_ERR_DEVICE, "occlusion kernel launch: %s", hipGetErrorString((hipError_t)err));
  return clock.finish(stats, n);
}
}  // namespace rt_api

// (the arguments first: they are judged without a scene, and before a device is touched)
extern "C" int rt_scene_occlusion_device(rt_scene_dev *s, uint64_t n, const double *d_rays, const uint32_t *d_order, const rt_occlusion_inputs *d_in,
                                         const rt_occlusion_outputs *d_out, void *hip_stream, rt_stats *stats) {
  int rc = occlusion_check(n, d_rays, d_in, d_out, "rt_scene_occlusion_device");
  if (rc) return rc;
  if ((uintptr_t)d_order & 3u) return fail(RT_ERR_INVALID, "rt_scene_occlusion_device: misaligned order (4 bytes)");
  if (!s) return fail(RT_ERR_STATE, "rt_scene_occlusion_device: NULL scene handle");
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  const rt_occlusion_inputs none = {nullptr, nullptr, nullptr};
  return occlusion_launch(s, (uint32_t)n, d_rays, d_order, d_in ? *d_in : none, *d_out, stream, stats);
}
