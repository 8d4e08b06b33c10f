// rt_api.hip — the C ABI of include/rt_hip.h (its other units: rt_api_internal.h): library and device lifetime, errors, the scratch
// guard and the per-variant scratch figures, scene validation and the host-logic probes (bounce candidates, cull rectangles, the
// host-built launch table; test build: the variant of a launch), pinned framebuffers and device memory, IPC.
//
// Host-side counterpart of the reference's driver code: main() sets up what a frame needs
// (main.js:77-105), redraw()/spanish() walks the rows (:180-201).  Here a frame is one kernel
// launch per GPU.  There is no CPU rendering path in this library: without a GPU every render
// entry point fails with RT_ERR_DEVICE.

#include "rt_api_internal.h"
#include "rt_wide.h"          // the test build's probe of the 16-byte frame stores (rt_test_wide_stores)

// ------------------------------------------------------------------------------------ state
namespace rt_api {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

lib_state G;

int ensure_device(int d) {
  if (!G.inited) return fail(RT_ERR_STATE, "rt_init has not been called");
  if (d < 0 || d >= (int)G.dev.size()) return fail(RT_ERR_INVALID, "device %d out of range (0..%d)", d, (int)G.dev.size() - 1);
  device_state &s = G.dev[d];
  HIP_TRY(hipSetDevice(s.hip_id));
  std::lock_guard<std::mutex> lk(G.dev_mu);
  if (!s.stream) {
    hipStream_t st = nullptr;
    HIP_TRY(hipMalloc(&s.d_counters, 7 * sizeof(unsigned long long)));      // RT_FLAG_COUNT's three; [3] .. [6]: the test build's uniform-path waves, checker-cell waves, first-bounce-set waves and second-node waves (rt_test_uniform_waves, rt_test_cell_waves, rt_test_first_bounce_waves, rt_test_second_node_waves) - the product build never touches them
    HIP_TRY(hipMemset(s.d_counters, 0, 7 * sizeof(unsigned long long)));
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    s.stream = st;                         // published last: a non-NULL stream means the device state is complete
  }
  return RT_OK;
}

int device_stream(int device, void *hip_stream, hipStream_t *stream) {
  if (int rc = ensure_device(device)) return rc;
  *stream = hip_stream ? (hipStream_t)hip_stream : G.dev[device].stream;
  return RT_OK;
}

// Kernels with a private segment (the general kernel's park stack: 3472 B per lane; the strict kernels' recursion stack) make the
// runtime reserve scratch memory: bytes per lane x 64 lanes x the wave slots the dispatch can occupy (at most CUs x waves per CU =
// 8192 on MI355X: 1.8 GB for the general kernel).  When that reservation cannot be met the HIP runtime does not return an error from
// the launch: the queue's error callback ABORTS the process (profiles/r04_scratch_refusal.log).  So every launch path of a kernel that
// needs scratch holds the figure against the free device memory first - once per (stream, larger figure): later launches reuse the
// queue's scratch - and the library returns RT_ERR_NOMEM with the numbers instead of reaching that abort.
int scratch_guard(device_state &D, hipStream_t stream, size_t per_lane, uint64_t waves_in_grid, const char *what) {
#ifdef RT_TESTING
  bool pretend = false;
  if (const char *q = getenv("RT_TEST_SCRATCH_PER_LANE")) { per_lane = (size_t)strtoull(q, nullptr, 10); pretend = true; }    // as if the kernel asked for this much
#else
  const bool pretend = false;
#endif
  if (per_lane == 0) return RT_OK;
  std::lock_guard<std::mutex> lk(G.dev_mu);
  if (!pretend) for (const device_state::scratch_seen &c : D.scratch_checked) if (c.stream == stream && c.per_lane >= per_lane) return RT_OK;
  if (!D.wave_slots) {
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, D.hip_id));
    D.wave_slots = (size_t)p.multiProcessorCount * (size_t)(p.maxThreadsPerMultiProcessor / 64);
    if (!D.wave_slots) D.wave_slots = 8192;
  }
  const uint64_t slots = waves_in_grid < D.wave_slots ? waves_in_grid : D.wave_slots;
  const uint64_t reservation = (uint64_t)per_lane * 64u * slots;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const uint64_t margin = (uint64_t)64 << 20;
  if (reservation + margin > free_b)
    return fail(RT_ERR_NOMEM, "%s needs %zu bytes of scratch per lane: the runtime reserves that for %llu wave slots = %llu bytes, and %zu of %zu bytes of device memory are free",
                what, per_lane, (unsigned long long)slots, (unsigned long long)reservation, free_b, total_b);
  if (!pretend) {
    bool found = false;
    for (device_state::scratch_seen &c : D.scratch_checked) if (c.stream == stream) { c.per_lane = per_lane; found = true; }
    if (!found) { if (D.scratch_checked.size() >= 64u) D.scratch_checked.clear(); D.scratch_checked.push_back(device_state::scratch_seen{stream, per_lane}); }
  }
  return RT_OK;
}

// Scratch (private segment) bytes per lane of the variant's kernel, from the code object: what the runtime reserves for every wave
// slot of the device before the first launch.  Returns a hipError_t as int.
static int variant_scratch(rt_trace_variant v, size_t *bytes_per_lane) {
  const void *f = (v.strict ? rt_kernel_trace_strict : rt_kernel_trace_fast)(v);
  if (!f) return (int)hipErrorInvalidDeviceFunction;
  hipFuncAttributes fa;
  const hipError_t e = hipFuncGetAttributes(&fa, f);
  if (e == hipSuccess) *bytes_per_lane = (size_t)fa.localSizeBytes;
  return (int)e;
}

// ... asked once per variant
int kernel_scratch(rt_trace_variant v, size_t *out) {
  static std::mutex mu;
  static size_t cache[256];
  static bool have[256];
  const uint32_t k = rt_variant_bits(v);
  std::lock_guard<std::mutex> lk(mu);
  if (!have[k]) {
    size_t b = 0;
    const int e = variant_scratch(v, &b);
    if (e != 0) return fail(RT_ERR_DEVICE, "hipFuncGetAttributes: %s", hipGetErrorString((hipError_t)e));
    cache[k] = b; have[k] = true;
  }
  *out = cache[k];
  return RT_OK;
}

// the per-lane scratch of a variant's kernel (kernel_scratch), held against the free device memory (scratch_guard) before its launch
int guard_kernel_scratch(device_state &D, hipStream_t stream, rt_trace_variant v, uint64_t waves_in_grid, const char *what) {
  size_t per_lane = 0;
  if (int rc = kernel_scratch(v, &per_lane)) return rc;
  return scratch_guard(D, stream, per_lane, waves_in_grid, what);
}

// A w x h frame and, if given, a tile set of it: what every launch path asks of both (`what`: the entry point).  flags: RT_FLAG_RGB24
// stores 4 pixels as 3 words, so the width is a multiple of 4.
int check_frame(const char *what, uint32_t w, uint32_t h, const rt_tiles *tiles, uint32_t flags) {
  if (w == 0 || h == 0 || w > 65536 || h > 65536) return fail(RT_ERR_INVALID, "%s: frame size %ux%u not in 1..65536", what, w, h);
  if ((flags & RT_FLAG_RGB24) && (w & 3u)) return fail(RT_ERR_INVALID, "%s: RT_FLAG_RGB24 needs a frame width that is a multiple of 4 (got %u)", what, w);
  if (!tiles) return RT_OK;
  if (tiles->tile_rows == 0 || tiles->tile_stride == 0 || tiles->n_tiles == 0) return fail(RT_ERR_INVALID, "%s: empty tile set", what);
  if ((uint64_t)tiles->n_tiles * tiles->tile_rows > (1ull << 24)) return fail(RT_ERR_INVALID, "%s: too many rows in one call", what);
  return RT_OK;
}

// the pixels of a w x h frame that `tiles` covers (rt_stats::pixels of one frame)
uint64_t tile_set_pixels(uint32_t w, uint32_t h, const rt_tiles *tiles) {
  uint64_t px = 0;
  for (uint32_t i = 0; i < tiles->n_tiles; i++) {
    const uint64_t r0 = (uint64_t)(tiles->tile_first + (uint64_t)i * tiles->tile_stride) * tiles->tile_rows;
    if (r0 < h) px += ((r0 + tiles->tile_rows <= h) ? tiles->tile_rows : (h - r0)) * (uint64_t)w;
  }
  return px;
}

launch_geom launch_geometry(double fov_deg, uint32_t w, uint32_t h, uint32_t ss, uint32_t tile_rows) {
  launch_geom g;
  g.tiles_x = (w + RT_TILE_W - 1) / RT_TILE_W;
  g.rows_per_wg = ss == 2u ? 2u : RT_TILE_H;
  g.rb_per_tile = (tile_rows + g.rows_per_wg - 1) / g.rows_per_wg;
  const double projA = fov_deg * M_PI / 180.0;
  g.proj_w = (double)w * ss / 2.0; g.proj_h = (double)h * ss / 2.0; g.proj_d = g.proj_w / tan(projA / 2.0);
  return g;
}

}  // namespace rt_api

// The product kernels' scratch figure as the tests ask for it: the variant's template arguments (many spheres: GRID; one-wave
// workgroups: W1), uncached.  Returns a hipError_t as int.
extern "C" int rt_scratch_trace_fast(int refract, int count, int ss2, int grid_variant, int one_wave, size_t *bytes_per_lane) {
  const rt_trace_variant v = {false, false, false, refract != 0, count != 0, ss2 != 0, grid_variant != 0, one_wave != 0};
  return rt_api::variant_scratch(v, bytes_per_lane);
}

// ------------------------------------------------------------------------------------ lifetime
extern "C" uint32_t rt_abi_version(void) { return RT_ABI_VERSION; }
extern "C" const char *rt_build_id(void) { return RT_REFERENCE_BUILD "." RT_LIBRARY_REVISION; }

// main.js:204-205: 'build #' + build + ' (' + elapsed + 'ms)', elapsed a whole number of milliseconds (Date.now() difference)
extern "C" int rt_elapsed_report(const rt_stats *stats, char *out, size_t cap) {
  if (!stats || (!out && cap)) return fail(RT_ERR_INVALID, "rt_elapsed_report: NULL argument");
  const double ms = (stats->total_ms >= 0.0 && stats->total_ms < 1e15) ? stats->total_ms : 0.0;
  return snprintf(out, cap, "build #%s (%lldms)", rt_build_id(), (long long)llround(ms));
}
extern "C" const char *rt_last_error(void) { return g_err; }

extern "C" int rt_init(int max_devices) {
  std::lock_guard<std::mutex> lk(G.mu);
  if (G.inited) {
    // a second rt_init must not silently change how rt_render shards a frame: asking for a different number of GPUs than
    // the library already uses is an error (0 = "whatever is in use" is fine); rt_shutdown first to change it
    if (max_devices > 0 && max_devices != (int)G.dev.size() && !(max_devices > (int)G.dev.size() && G.all_visible))
      return fail(RT_ERR_STATE, "rt_init(%d): the library is already initialised with %d device(s); call rt_shutdown first", max_devices, (int)G.dev.size());
    return RT_OK;
  }
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(RT_ERR_DEVICE, "no HIP device visible (%s); this library has no CPU path", e == hipSuccess ? "count 0" : hipGetErrorString(e));
  const char *emu = RT_TEST_ENV("RT_EMULATE_DEVICES");
  G.emulated = emu && atoi(emu) > 1;
  if (G.emulated) n = atoi(emu);
  G.all_visible = !(max_devices > 0 && n > max_devices);   // every visible GPU is in use: a later request for "up to more" changes nothing
  if (max_devices > 0 && n > max_devices) n = max_devices;
  if (n > 16) n = 16;
  G.dev.resize(n);
  for (int i = 0; i < n; i++) G.dev[i].hip_id = G.emulated ? 0 : i;
  G.inited = true;
  return RT_OK;
}

extern "C" int rt_device_count(void) {
  if (!G.inited) return fail(RT_ERR_STATE, "rt_init has not been called");
  return (int)G.dev.size();
}

// ------------------------------------------------------------------------------------ validation (host logic only)
namespace rt_api {
// one sphere record of a scene with `n_textures` textures (rt_scene_validate, rt_scene_set_objects)
int check_sphere(const rt_sphere &o, uint32_t i, uint32_t n_textures) {
  const int k = o.sampler_kind;
  if (k != RT_SAMPLER_COLOR && k != RT_SAMPLER_TEXTURE && k != RT_SAMPLER_CHECKER && k != RT_SAMPLER_STARS)
    return fail(RT_ERR_UNSUPPORTED, "object %u: sampler kind %d is not supported (0 colour, 1 texture, 2 checker, 3 hashed stars)", i, k);
  if (k == RT_SAMPLER_TEXTURE && (o.texture < 0 || (uint32_t)o.texture >= n_textures))
    return fail(RT_ERR_INVALID, "object %u: texture index %d out of range", i, o.texture);
  return RT_OK;
}
}  // namespace rt_api

extern "C" int rt_scene_validate(const void *blob, size_t bytes) {
  if (!blob || bytes < sizeof(rt_scene_header)) return fail(RT_ERR_INVALID, "scene blob shorter than its header");
  if (((uintptr_t)blob & 7u) != 0) return fail(RT_ERR_INVALID, "scene blob must be 8-byte aligned");
  const rt_scene_header *hd = (const rt_scene_header *)blob;
  if (hd->magic != RT_SCENE_MAGIC) return fail(RT_ERR_INVALID, "bad scene magic 0x%08x", hd->magic);
  if (hd->abi_version != RT_ABI_VERSION) return fail(RT_ERR_INVALID, "scene ABI version %u, library speaks %u", hd->abi_version, RT_ABI_VERSION);
  if (hd->total_bytes != bytes) return fail(RT_ERR_INVALID, "total_bytes %llu != blob size %zu", (unsigned long long)hd->total_bytes, bytes);
  if (hd->n_objects < 1 || hd->n_objects > RT_MAX_OBJECTS) return fail(RT_ERR_INVALID, "n_objects %u not in 1..%u", hd->n_objects, RT_MAX_OBJECTS);
  if (hd->n_lights > RT_MAX_LIGHTS) return fail(RT_ERR_INVALID, "n_lights %u > %u", hd->n_lights, RT_MAX_LIGHTS);
  if (hd->n_textures > RT_MAX_TEXTURES) return fail(RT_ERR_INVALID, "n_textures %u > %u", hd->n_textures, RT_MAX_TEXTURES);
  if (hd->segs > RT_MAX_SEGS) return fail(RT_ERR_INVALID, "segs %u > %u", hd->segs, RT_MAX_SEGS);
  if (hd->supersample < 1 || hd->supersample > 4) return fail(RT_ERR_INVALID, "supersample must be 1, 2, 3 or 4");
  if (!(hd->fov_deg > 0.0 && hd->fov_deg < 180.0)) return fail(RT_ERR_INVALID, "fov_deg must be in (0,180)");
  auto in_range = [&](uint64_t off, uint64_t len) { return (off & 7u) == 0 && off >= sizeof(rt_scene_header) && off <= bytes && len <= bytes - off; };
  if (!in_range(hd->objects_offset, (uint64_t)hd->n_objects * sizeof(rt_sphere))) return fail(RT_ERR_INVALID, "object table out of bounds");
  if (!in_range(hd->lights_offset, (uint64_t)hd->n_lights * 24u)) return fail(RT_ERR_INVALID, "light table out of bounds");
  if (!in_range(hd->textures_offset, (uint64_t)hd->n_textures * sizeof(rt_texture_desc))) return fail(RT_ERR_INVALID, "texture table out of bounds");
  const uint8_t *base = (const uint8_t *)blob;
  const rt_texture_desc *td = (const rt_texture_desc *)(base + hd->textures_offset);
  for (uint32_t t = 0; t < hd->n_textures; t++) {
    if (td[t].width == 0 || td[t].height == 0 || td[t].width > 16384 || td[t].height > 16384) return fail(RT_ERR_INVALID, "texture %u: bad size", t);
    if ((td[t].texels_offset & 3u) != 0 || td[t].texels_offset > bytes || (uint64_t)td[t].width * td[t].height * 4u > bytes - td[t].texels_offset)
      return fail(RT_ERR_INVALID, "texture %u: texels out of bounds", t);
  }
  const rt_sphere *ob = (const rt_sphere *)(base + hd->objects_offset);
  for (uint32_t i = 0; i < hd->n_objects; i++)
    if (int rc = check_sphere(ob[i], i, hd->n_textures)) return rc;
  return RT_OK;
}

#ifdef RT_TESTING
// Host-logic probe (test build, no GPU): the variant of a launch with the facts in `facts` - bit 0 strict, 1 retrace, 2 refract, 3 count,
// 4 supersample 2, 5 cull_in_lds, 6 scatter, 7 four_waves; bit 8: a ray-list launch instead (refract alone counts) - as rt_variant_bits
// packs it, and whether the build it belongs to has a kernel for it.
extern "C" int rt_test_trace_variant(uint32_t facts, uint32_t *out_bits, int *out_has_kernel) {
  if (!out_bits || !out_has_kernel) return fail(RT_ERR_INVALID, "rt_test_trace_variant: NULL argument");
  const rt_trace_variant v = (facts & 256u) ? rt_trace_variant_of_rays((facts & 4u) != 0)
                                            : rt_trace_variant_of((facts & 1u) != 0, (facts & 2u) != 0, (facts & 4u) != 0, (facts & 8u) != 0, (facts & 16u) != 0,
                                                                  (facts & 32u) != 0, (facts & 64u) != 0, (facts & 128u) != 0);
  *out_bits = rt_variant_bits(v);
  *out_has_kernel = (v.strict ? rt_kernel_trace_strict : rt_kernel_trace_fast)(v) != nullptr;
  return RT_OK;
}

// Host-logic probe (test build, no GPU): how a launch with these facts stores the frame (rt_device.h: rt_wide_stores_of) - bit 0 strict,
// 1 rgb24, 2 scatter of `facts`; out_bytes: what the launch writes, all frames - as RT_WIDE_* flags, 0: one 4-byte store per pixel.
extern "C" int rt_test_wide_rule(uint32_t facts, uint32_t w, uint64_t out_address, uint32_t n_frames, uint64_t frame_stride_words, uint64_t out_bytes, uint32_t *out_flags) {
  if (!out_flags) return fail(RT_ERR_INVALID, "rt_test_wide_rule: NULL argument");
  *out_flags = rt_wide_stores_of((facts & 1u) != 0, (facts & 2u) != 0, (facts & 4u) != 0, w, out_address, n_frames, frame_stride_words, out_bytes);
  return RT_OK;
}

// Host-logic probe (test build, no GPU): the 16-byte stores of ONE launch-table entry (its words 0 and 1, as rt_scene_launch_table returns
// them) of a frame `w` pixels wide, enumerated by the header the kernel's epilogue is written from (rt_wide.h: rt_wide_entry_stores):
// out receives {wave of the entry, row in the call's output band, first pixel} per store, at most `cap` of them; *n_stores = how many
// there are.
extern "C" int rt_test_wide_stores(uint32_t e0, uint32_t e1, int ss2, uint32_t w, uint32_t *out, uint32_t cap, uint32_t *n_stores) {
  if (!n_stores || (!out && cap)) return fail(RT_ERR_INVALID, "rt_test_wide_stores: NULL argument");
  uint32_t n = 0;
  rt_wide_entry_stores(e0, e1, ss2 != 0, w, [&](uint32_t wave, uint32_t lrow, uint32_t px) {
    if (n < cap) { out[3u * n] = wave; out[3u * n + 1u] = lrow; out[3u * n + 2u] = px; }
    n++;
  });
  *n_stores = n;
  return RT_OK;
}
#endif

// Host-logic probe for tests: the bounce table's answer for one ray, with the kernel's own direction -> cell mapping
// (an exact division where the kernel uses a 2^-24 reciprocal: the cells overlap by 1e-6 rad for that).
extern "C" int rt_scene_bounce_candidates(const void *blob, size_t bytes, uint32_t from, const double dir[3], uint64_t *out_words) {
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  const rt_scene_header *hd = (const rt_scene_header *)blob;
  if (!dir || !out_words || from >= hd->n_objects) return fail(RT_ERR_INVALID, "bad bounce probe arguments");
  const rt_sphere *ob = (const rt_sphere *)((const uint8_t *)blob + hd->objects_offset);
  const uint32_t n = hd->n_objects, words = (n + 63u) / 64u;
  const std::vector<uint64_t> tab = build_bounce_table(ob, n, n);
  const double ax = fabs(dir[0]), ay = fabs(dir[1]), az = fabs(dir[2]);
  const bool bx = (ax >= ay) && (ax >= az), by = !bx && (ay >= az);
  const double dm = bx ? dir[0] : (by ? dir[1] : dir[2]);
  const double du = bx ? dir[1] : dir[0], dv = (bx || by) ? dir[2] : dir[1];
  const double sc = (0.5 * RT_BGRID) / fabs(dm);
  const double fu = fmin(fmax(du * sc + 0.5 * RT_BGRID, 0.0), (double)(RT_BGRID - 1u)), fv = fmin(fmax(dv * sc + 0.5 * RT_BGRID, 0.0), (double)(RT_BGRID - 1u));
  const uint32_t face = (bx ? 0u : (by ? 2u : 4u)) + ((dm < 0.0) ? 1u : 0u);
  const uint32_t cell = face * (RT_BGRID * RT_BGRID) + (uint32_t)fv * RT_BGRID + (uint32_t)fu;
  memcpy(out_words, tab.data() + ((size_t)from * RT_BCELLS + cell) * words, words * sizeof(uint64_t));
  return RT_OK;
}

// Host-logic probe for tests: the cull rectangle of every sphere, scene order, 4 doubles each.
extern "C" int rt_scene_cull_rects(const void *blob, size_t bytes, double *out) {
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if (!out) return fail(RT_ERR_INVALID, "out is NULL");
  const rt_scene_header *hd = (const rt_scene_header *)blob;
  const rt_sphere *ob = (const rt_sphere *)((const uint8_t *)blob + hd->objects_offset);
  for (uint32_t i = 0; i < hd->n_objects; i++) {
    const rt_geom r = cull_rect(hd, ob[i]);
    out[4 * i] = r.ox; out[4 * i + 1] = r.oy; out[4 * i + 2] = r.oz; out[4 * i + 3] = r.r2;
  }
  return RT_OK;
}

// Host-logic probe (no GPU): the product kernel's launch table for `tiles` of the w x h frame as the HOST builds it (rt_tables.cpp;
// the library builds the same table on the GPU, rt_tables_gpu.hip): out_entries receives 4 words per slot, 8 * ceil(blocks / 8) slots
// with workgroup b's entry in slot (b % 8) * ceil(blocks / 8) + b / 8; *n_workgroups = the number of entries, *n_blocks = the number
// of blocks.  Pass out_entries = NULL to ask for the two numbers only.
extern "C" int rt_scene_launch_table(const void *blob, size_t bytes, uint32_t w, uint32_t h, const rt_tiles *tiles, int ranked,
                                     uint32_t *out_entries, uint32_t *n_workgroups, uint32_t *n_blocks) {
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if (!tiles || !n_workgroups) return fail(RT_ERR_INVALID, "rt_scene_launch_table: NULL argument");
  if ((rc = check_frame("rt_scene_launch_table", w, h, tiles, 0u))) return rc;
  const rt_scene_header *hd = (const rt_scene_header *)blob;
  if (hd->supersample > 2) return fail(RT_ERR_INVALID, "supersample 3 and 4 launch on the sample grid: probe that size with a supersample-1 scene");
  const rt_sphere *ob = (const rt_sphere *)((const uint8_t *)blob + hd->objects_offset);
  std::vector<rt_geom> cull;
  std::vector<uint32_t> weight;
  scene_tile_weights(hd, ob, &cull, &weight);
  const uint32_t ss = hd->supersample;
  const launch_geom g = launch_geometry(hd->fov_deg, w, h, ss, tiles->tile_rows);
  if ((uint64_t)tiles->n_tiles * g.rb_per_tile > 65535u) return fail(RT_ERR_INVALID, "too many row blocks");
  // (bit 5 of `ranked`, with bit 2: word 3 also carries the checker cells of one-candidate blocks, as a product frame's table does;
  // bit 6, with bit 5: and the per-axis statements of the columns that are not inside one cell, rt_block.h: rt_cells_word;
  // bit 7, with bit 2: and the first-bounce sets of the blocks that show a mirror, rt_block.h: rt_first_bounce_set;
  // bit 8, with bit 7: and in word 1 of those entries what the node after the primary may skip, rt_block.h: rt_second_node_bits;
  // bit 9, with bit 8: and the two bits about that node's shadow scans, rt_block.h: rt_cand_second_dark - no launch's table has them)
  // (bit 1 of `ranked`: also mark the workgroups no sphere but the enclosing one can show in, as a launch of a constant-background scene does)
  double lights[RT_MAX_LIGHTS][3];
  memset(lights, 0, sizeof lights);
  if (hd->n_lights) memcpy(lights, (const uint8_t *)blob + hd->lights_offset, hd->n_lights * 24u);
  const uint32_t sky_sphere = enclosing_sphere(hd, ob, lights);
  uint32_t n_entries = 0;
  const std::vector<uint32_t> table = build_launch_table(hd, ob, cull, weight, w, h, ss, tiles, g.tiles_x, g.rb_per_tile, g.proj_w, g.proj_h, g.proj_d, (ranked & 1) != 0, (ranked & 2) != 0, sky_sphere,
                                                         (ranked & 4) != 0, (ranked & 4) != 0, (ranked & 32) ? ((ranked & 64) ? 2 : 1) : 0, (ranked & 128) != 0, (ranked & 256) ? ((ranked & 512) ? 2 : 1) : 0, lights, &n_entries, (ranked & 8) ? 1u : ((ranked & 16) ? 2u : 0u));
  if (table.empty()) return fail(RT_ERR_INVALID, "a launch of this size is beyond the launch table");
  *n_workgroups = n_entries;
  if (n_blocks) *n_blocks = g.tiles_x * tiles->n_tiles * g.rb_per_tile;
  if (out_entries) memcpy(out_entries, table.data(), table.size() * sizeof(uint32_t));
  return RT_OK;
}

// ------------------------------------------------------------------------------------ sharing memory between the ranks of a node
extern "C" int rt_ipc_export(int device, const void *d_ptr, void *handle_out) {
  static_assert(sizeof(hipIpcMemHandle_t) == RT_IPC_HANDLE_BYTES, "hipIpcMemHandle_t is expected to be 64 bytes");
  if (!d_ptr || !handle_out) return fail(RT_ERR_INVALID, "rt_ipc_export: NULL argument");
  int rc = ensure_device(device);
  if (rc) return rc;
  hipIpcMemHandle_t hnd;
  HIP_TRY(hipIpcGetMemHandle(&hnd, const_cast<void *>(d_ptr)));
  memcpy(handle_out, &hnd, sizeof hnd);
  return RT_OK;
}

extern "C" int rt_ipc_open(int device, const void *handle, void **d_ptr_out) {
  if (!handle || !d_ptr_out) return fail(RT_ERR_INVALID, "rt_ipc_open: NULL argument");
  int rc = ensure_device(device);
  if (rc) return rc;
  hipIpcMemHandle_t hnd;
  memcpy(&hnd, handle, sizeof hnd);
  void *p = nullptr;
  HIP_TRY(hipIpcOpenMemHandle(&p, hnd, hipIpcMemLazyEnablePeerAccess));
  *d_ptr_out = p;
  return RT_OK;
}

extern "C" int rt_ipc_close(int device, void *d_ptr) {
  if (!d_ptr) return RT_OK;
  int rc = ensure_device(device);
  if (rc) return rc;
  HIP_TRY(hipIpcCloseMemHandle(d_ptr));
  return RT_OK;
}

// ------------------------------------------------------------------------------------ memory helpers
// Pinned framebuffers are recycled: hipHostMalloc of a 33 MB frame costs ~15 ms, ten times the render.
// A freed buffer goes to a small pool (same-size reuse); at most 4 buffers / 1 GiB are kept.
namespace {
struct pinned_buf { void *p; size_t bytes; };
std::mutex g_pin_mu;
std::vector<pinned_buf> g_pin_live, g_pin_free;
}  // namespace

extern "C" void *rt_alloc_pinned(size_t bytes) {
  if (!bytes) bytes = 1;
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (size_t i = 0; i < g_pin_free.size(); i++)
      if (g_pin_free[i].bytes == bytes) {
        pinned_buf b = g_pin_free[i];
        g_pin_free.erase(g_pin_free.begin() + i);
        g_pin_live.push_back(b);
        return b.p;
      }
  }
  void *p = nullptr;
  hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
  if (e != hipSuccess) { fail(RT_ERR_NOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e)); return nullptr; }
  std::lock_guard<std::mutex> lk(g_pin_mu);
  g_pin_live.push_back({p, bytes});
  return p;
}

extern "C" void rt_free_pinned(void *p) {
  if (!p) return;
  pinned_buf b = {p, 0};
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (size_t i = 0; i < g_pin_live.size(); i++)
      if (g_pin_live[i].p == p) { b = g_pin_live[i]; g_pin_live.erase(g_pin_live.begin() + i); break; }
    size_t pooled = 0;
    for (const pinned_buf &f : g_pin_free) pooled += f.bytes;
    if (b.bytes && g_pin_free.size() < 4 && pooled + b.bytes <= ((size_t)1 << 30)) { g_pin_free.push_back(b); return; }
  }
  (void)hipHostFree(p);
}

extern "C" void *rt_alloc_device(int device, size_t bytes) {
  if (ensure_device(device)) return nullptr;
  void *p = nullptr;
  hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
  if (e != hipSuccess) { fail(RT_ERR_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); return nullptr; }
  return p;
}
extern "C" void rt_free_device(int device, void *p) {
  if (!p || ensure_device(device)) return;
  (void)hipFree(p);
}
extern "C" int rt_copy_to_host(int device, void *dst, const void *src, size_t bytes) {
  int rc = ensure_device(device);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(G.dev[device].stream));
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}

extern "C" int rt_memset_device(int device, void *dst, int value, size_t bytes) {
  if (!dst) return fail(RT_ERR_INVALID, "rt_memset_device: NULL destination");
  int rc = ensure_device(device);
  if (rc) return rc;
  HIP_TRY(hipMemset(dst, value, bytes));
  HIP_TRY(hipDeviceSynchronize());
  return RT_OK;
}

extern "C" void rt_shutdown(void) {
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (const pinned_buf &f : g_pin_free) (void)hipHostFree(f.p);
    g_pin_free.clear();
  }
  std::lock_guard<std::mutex> lk(G.mu);
  if (!G.inited) return;
  release_rccl();
  for (device_state &D : G.dev) {
    if (!D.stream) continue;
    (void)hipSetDevice(D.hip_id);
    (void)hipStreamSynchronize(D.stream);
    if (D.cached_scene) rt_scene_free(D.cached_scene);
    if (D.d_frame) (void)hipFree(D.d_frame);
    if (D.d_gather) (void)hipFree(D.d_gather);
    if (D.d_counters) (void)hipFree(D.d_counters);
    (void)hipStreamDestroy(D.stream);
    if (D.copy_stream) (void)hipStreamDestroy(D.copy_stream);
    D = device_state();
  }
  G.dev.clear();
  G.inited = false;
}
