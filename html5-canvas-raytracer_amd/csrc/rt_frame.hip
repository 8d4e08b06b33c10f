// rt_frame.hip — rt_render(width, height, scene) and its kin (rt_render_progressive, rt_render_hits, rt_pick; rt_trace_rays, rt_occlusion
// and their binned forms, rt_shade_rays and rt_relight_rays, which are rows and a step for the chunked list call of rt_api_internal.h;
// rt_trace_rays_wavefront and rt_trace_rays_soft, which share one level loop): the resident scene
// per device (scene_for), the prologue and epilogue of every host form (host_call), the one-GPU plans (banded copy-out, stores straight into a pinned frame) and the single-process multi-GPU
// frame (interleaved row tiles stored straight into GPU 0's frame over xGMI; fallback: RGB24 bands + one RCCL gather + de-interleave).

#include "rt_api_internal.h"
#include "rt_literal.h"       // lit_finite6

// ------------------------------------------------------------------------------------ de-interleave
// src: for rank g, its tiles (g, g+R, g+2R, ...) stored contiguously, ranks `rank_stride` bytes apart.
// dst: the frame in row order.  One workgroup row per frame row (grid y), so the tile/rank arithmetic is
// wave-uniform scalar work done once; a work-item moves 16 bytes (T = uint4) or, for ragged widths, 4 (T = uint32_t).
template <typename T>
__global__ void __launch_bounds__(256) rt_deinterleave_kernel(const T *__restrict__ src, T *__restrict__ dst, uint32_t row_elems, uint32_t tile_rows,
                                                              uint32_t n_ranks, uint64_t rank_stride_elems) {
  const uint32_t row = blockIdx.y;
  const uint32_t tile = row / tile_rows, r = row - tile * tile_rows;
  const uint32_t rank = tile % n_ranks, local_tile = tile / n_ranks;
  const T *__restrict__ s = src + rank * rank_stride_elems + ((uint64_t)local_tile * tile_rows + r) * row_elems;
  T *__restrict__ d = dst + (uint64_t)row * row_elems;
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < row_elems; x += gridDim.x * blockDim.x) d[x] = s[x];
}

extern "C" int rt_deinterleave_device(int device, const void *d_src, void *d_dst, uint32_t w, uint32_t h, uint32_t tile_rows, uint32_t n_ranks,
                                      uint64_t rank_stride_bytes, void *hip_stream) {
  if (!d_src || !d_dst || !w || !h || !tile_rows || !n_ranks || (rank_stride_bytes & 3u) || h > 65535u * 16u) return fail(RT_ERR_INVALID, "bad de-interleave arguments");
  hipStream_t stream = nullptr;
  int rc = device_stream(device, hip_stream, &stream);
  if (rc) return rc;
  if (h > 65535u) return fail(RT_ERR_INVALID, "de-interleave: more than 65535 rows");
  const bool wide = (w % 4u == 0) && (rank_stride_bytes % 16u == 0) && (((uintptr_t)d_src | (uintptr_t)d_dst) % 16u == 0);
  const uint32_t row_elems = wide ? w / 4u : w;
  const dim3 grid((row_elems + 255u) / 256u, h), block(256);
  if (wide)
    hipLaunchKernelGGL(rt_deinterleave_kernel<uint4>, grid, block, 0, stream, (const uint4 *)d_src, (uint4 *)d_dst, row_elems, tile_rows, n_ranks,
                       rank_stride_bytes / 16u);
  else
    hipLaunchKernelGGL(rt_deinterleave_kernel<uint32_t>, grid, block, 0, stream, (const uint32_t *)d_src, (uint32_t *)d_dst, row_elems, tile_rows,
                       n_ranks, rank_stride_bytes / 4u);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

// RGB24 bands -> RGBA8 frame.  A work-item turns 3 source words (4 pixels x 3 bytes) into one uint4 (4 pixels x RGBA);
// w % 4 == 0, so rows of both sides start word-aligned.
__global__ void __launch_bounds__(256) rt_deinterleave_rgb24_kernel(const uint32_t *__restrict__ src, uint4 *__restrict__ dst, uint32_t row_quads,
                                                                    uint32_t tile_rows, uint32_t n_ranks, uint64_t rank_stride_words) {
  const uint32_t row = blockIdx.y;
  const uint32_t tile = row / tile_rows, r = row - tile * tile_rows;
  const uint32_t rank = tile % n_ranks, local_tile = tile / n_ranks;
  const uint32_t *__restrict__ s = src + rank * rank_stride_words + ((uint64_t)local_tile * tile_rows + r) * row_quads * 3u;
  uint4 *__restrict__ d = dst + (uint64_t)row * row_quads;
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < row_quads; x += gridDim.x * blockDim.x) {
    const uint32_t a = s[3u * x], b = s[3u * x + 1u], c = s[3u * x + 2u];
    uint4 o;
    o.x = a | 0xff000000u;
    o.y = (a >> 24) | (b << 8) | 0xff000000u;
    o.z = (b >> 16) | (c << 16) | 0xff000000u;
    o.w = (c >> 8) | 0xff000000u;
    d[x] = o;
  }
}

extern "C" int rt_deinterleave_rgb24_device(int device, const void *d_src, void *d_dst, uint32_t w, uint32_t h, uint32_t tile_rows, uint32_t n_ranks,
                                            uint64_t rank_stride_bytes, void *hip_stream) {
  if (!d_src || !d_dst || !w || !h || !tile_rows || !n_ranks || (rank_stride_bytes & 3u) || (w & 3u) || (((uintptr_t)d_src) & 3u) || (((uintptr_t)d_dst) & 15u))
    return fail(RT_ERR_INVALID, "bad RGB24 de-interleave arguments (w must be a multiple of 4, dst 16-byte aligned)");
  if (h > 65535u) return fail(RT_ERR_INVALID, "de-interleave: more than 65535 rows");
  hipStream_t stream = nullptr;
  int rc = device_stream(device, hip_stream, &stream);
  if (rc) return rc;
  const uint32_t row_quads = w / 4u;
  const dim3 grid((row_quads + 255u) / 256u, h), block(256);
  hipLaunchKernelGGL(rt_deinterleave_rgb24_kernel, grid, block, 0, stream, (const uint32_t *)d_src, (uint4 *)d_dst, row_quads, tile_rows, n_ranks,
                     rank_stride_bytes / 4u);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

// ------------------------------------------------------------------------------------ the blob diff of scene_for
namespace rt_api {
// What scene_for does with a blob of the resident one's size (rt_api_internal.h).  The header but for camera, intensity and seed, the
// descriptors, and every byte outside the sphere table, the light table and the textures' texel ranges must be equal: a byte of the
// padding between two textures that differs is -1, like any other byte no edit call reaches (a flattener writes zeros there).
int texel_edits(const uint8_t *a, const uint8_t *b, size_t bytes, std::vector<texel_edit> *out) {
  out->clear();
  const size_t c0 = offsetof(rt_scene_header, cam_origin), c1 = c0 + 12 * sizeof(double);
  const size_t i0 = offsetof(rt_scene_header, light_intensity), i1 = i0 + sizeof(double);
  const size_t s0 = offsetof(rt_scene_header, stars_seed), s1 = s0 + sizeof(uint32_t);
  static_assert(c1 <= i0 && i1 <= s0, "the camera lies in front of the light intensity, and that in front of the stars seed in rt_scene_header");
  if (bytes < sizeof(rt_scene_header)) return -1;
  // the header's other fields equal (the places and sizes of the three tables included: the resident blob's, which rt_scene_validate has seen)
  if (memcmp(a, b, c0) != 0 || memcmp(a + c1, b + c1, i0 - c1) != 0 || memcmp(a + i1, b + i1, s0 - i1) != 0 || memcmp(a + s1, b + s1, sizeof(rt_scene_header) - s1) != 0) return -1;
  const rt_scene_header *hd = (const rt_scene_header *)a;
  // the ranges an edit reaches, in blob order: [begin, end, texture or -1)
  struct range { size_t begin, end; int texture; };
  std::vector<range> r;
  r.push_back(range{(size_t)hd->objects_offset, (size_t)hd->objects_offset + (size_t)hd->n_objects * sizeof(rt_sphere), -1});
  r.push_back(range{(size_t)hd->lights_offset, (size_t)hd->lights_offset + (size_t)hd->n_lights * 24u, -1});
  const size_t d0 = hd->textures_offset, d1 = d0 + (size_t)hd->n_textures * sizeof(rt_texture_desc);
  if (hd->n_textures > RT_MAX_TEXTURES || d1 > bytes) return -1;
  rt_texture_desc td[RT_MAX_TEXTURES];                   // (the blob's own bytes may be unaligned)
  if (hd->n_textures) memcpy(td, a + d0, d1 - d0);
  for (uint32_t t = 0; t < hd->n_textures; t++) r.push_back(range{(size_t)td[t].texels_offset, (size_t)td[t].texels_offset + (size_t)td[t].width * td[t].height * 4u, (int)t});
  for (size_t i = 1; i < r.size(); i++)                  // (at most 18 entries)
    for (size_t j = i; j > 0 && r[j].begin < r[j - 1].begin; j--) std::swap(r[j], r[j - 1]);
  // everything between them is equal - the descriptors too, wherever they lie; ranges that overlap (two descriptors of the same texels,
  // a table inside a texture: nothing a flattener writes) are left to the upload
  size_t at = sizeof(rt_scene_header);
  for (const range &q : r) {
    if (q.begin == q.end) continue;
    if (q.begin < at || q.end > bytes) return -1;
    if (memcmp(a + at, b + at, q.begin - at) != 0) return -1;
    at = q.end;
  }
  if (memcmp(a + at, b + at, bytes - at) != 0) return -1;
  for (const range &q : r) if (q.begin < d1 && d0 < q.end && q.begin != q.end) return -1;      // (the descriptors lie in none of them)
  for (uint32_t t = 0; t < hd->n_textures; t++) {
    const size_t row = (size_t)td[t].width * 4u;
    const uint8_t *ta = a + td[t].texels_offset, *tb = b + td[t].texels_offset;
    uint32_t first = 0, end = td[t].height;
    while (first < end && memcmp(ta + first * row, tb + first * row, row) == 0) first++;
    while (end > first && memcmp(ta + (end - 1u) * row, tb + (end - 1u) * row, row) == 0) end--;
    if (first < end) out->push_back(texel_edit{t, first, end - first});
  }
  return 0;
}
}  // namespace rt_api

#ifdef RT_TESTING
// Test build only: texel_edits as scene_for calls it, without a GPU: {texture, first_row, rows} per changed texture into out_triples (at
// most `cap` of them).  Returns their number, or -1 (blob_a is no valid scene, or the blobs differ in what no edit reaches).
extern "C" int rt_test_texel_edits(const void *blob_a, const void *blob_b, size_t bytes, uint32_t *out_triples, uint32_t cap) {
  if (!blob_a || !blob_b || rt_scene_validate(blob_a, bytes) != RT_OK) return -1;
  std::vector<texel_edit> edits;
  if (texel_edits((const uint8_t *)blob_a, (const uint8_t *)blob_b, bytes, &edits) != 0) return -1;
  for (size_t i = 0; i < edits.size() && i < cap && out_triples; i++) { out_triples[3 * i] = edits[i].texture; out_triples[3 * i + 1] = edits[i].first_row; out_triples[3 * i + 2] = edits[i].rows; }
  return (int)edits.size();
}
#endif

namespace {
typedef int (*nccl_comm_init_all_t)(void **comms, int ndev, const int *devlist);
typedef int (*nccl_gather_t)(const void *send, void *recv, size_t count, int dtype, int root, void *comm, hipStream_t stream);
typedef int (*nccl_group_t)(void);
typedef int (*nccl_comm_destroy_t)(void *comm);
typedef const char *(*nccl_errstr_t)(int);
struct { nccl_comm_init_all_t init_all; nccl_gather_t gather; nccl_group_t group_start, group_end; nccl_comm_destroy_t destroy; nccl_errstr_t errstr; } NCCL;
const int NCCL_UINT8 = 1;   // ncclUint8 (rccl.h ncclDataType_t)

int ensure_rccl(int ndev) {
  if (G.comms_ready) return RT_OK;
  if (!G.rccl) {
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    for (const char *n : names) if ((G.rccl = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!G.rccl) return fail(RT_ERR_DEVICE, "cannot load RCCL: %s", dlerror());
    NCCL.init_all = (nccl_comm_init_all_t)dlsym(G.rccl, "ncclCommInitAll");
    NCCL.gather = (nccl_gather_t)dlsym(G.rccl, "ncclGather");
    NCCL.group_start = (nccl_group_t)dlsym(G.rccl, "ncclGroupStart");
    NCCL.group_end = (nccl_group_t)dlsym(G.rccl, "ncclGroupEnd");
    NCCL.destroy = (nccl_comm_destroy_t)dlsym(G.rccl, "ncclCommDestroy");
    NCCL.errstr = (nccl_errstr_t)dlsym(G.rccl, "ncclGetErrorString");
    if (!NCCL.init_all || !NCCL.gather || !NCCL.group_start || !NCCL.group_end || !NCCL.destroy || !NCCL.errstr)
      return fail(RT_ERR_DEVICE, "RCCL is missing ncclCommInitAll/ncclGather/ncclGroup*");
  }
  int ids[16];
  for (int i = 0; i < ndev; i++) ids[i] = G.dev[i].hip_id;
  const int r = NCCL.init_all(G.comms, ndev, ids);
  if (r != 0) return fail(RT_ERR_DEVICE, "ncclCommInitAll: %s", NCCL.errstr(r));
  G.comms_ready = true;
  return RT_OK;
}

// rt_render's scene for `device`: the resident one if the blob is the same bytes, else a fresh upload that replaces it.
int scene_for(int device, const void *blob, size_t bytes, rt_scene_dev **out) {
  device_state &D = G.dev[device];
  if (D.cached_scene && D.cached_blob.size() == bytes && memcmp(D.cached_blob.data(), blob, bytes) == 0) { *out = D.cached_scene; return RT_OK; }
  // the same scene with other texels in its textures, from another camera, with another stars seed, with moved or restyled spheres
  // and / or with moved or dimmed lights (an animation: a video on a sphere, main.js:339-395, lookAt per frame, main.js:92-100, a new
  // sky per redraw, main.js:135-139, 180, objects and lights a page changes between redraws, main.js:283-284): the resident scene
  // takes, per texture whose texels differ, the rows of the smallest range that covers the differences, then the spheres of the
  // smallest range that covers theirs, then the lights of theirs, then the intensity, then the camera, then the seed
  std::vector<texel_edit> edits;
  if (D.cached_scene && D.cached_blob.size() == bytes && texel_edits(D.cached_blob.data(), (const uint8_t *)blob, bytes, &edits) == 0) {
    const uint8_t *a = D.cached_blob.data(), *b = (const uint8_t *)blob;
    const rt_scene_header *nh = (const rt_scene_header *)blob;
    const size_t o0 = nh->objects_offset, l0 = nh->lights_offset;
    bool ok = true;
    for (const texel_edit &e : edits) {
      rt_texture_desc d;
      memcpy(&d, a + nh->textures_offset + e.texture * sizeof(rt_texture_desc), sizeof d);
      ok = ok && rt_scene_set_texels(D.cached_scene, e.texture, 0u, e.first_row, d.width, e.rows, b + d.texels_offset + (size_t)e.first_row * d.width * 4u, 0u, nullptr) == RT_OK;
    }
    const rt_sphere *na = (const rt_sphere *)(a + o0), *nb = (const rt_sphere *)(b + o0);
    uint32_t first = nh->n_objects, last = 0;
    for (uint32_t i = 0; i < nh->n_objects; i++)
      if (memcmp(&na[i], &nb[i], sizeof(rt_sphere)) != 0) { if (first == nh->n_objects) first = i; last = i + 1; }
    uint32_t lfirst = nh->n_lights, llast = 0;
    for (uint32_t k = 0; k < nh->n_lights; k++)
      if (memcmp(a + l0 + 24u * k, b + l0 + 24u * k, 24u) != 0) { if (lfirst == nh->n_lights) lfirst = k; llast = k + 1; }
    double xyz[RT_MAX_LIGHTS][3];                    // (the blob's own bytes may be unaligned)
    if (lfirst < llast && llast - lfirst <= RT_MAX_LIGHTS) memcpy(xyz, b + l0 + 24u * lfirst, (size_t)(llast - lfirst) * 24u);
    if (ok && (first == nh->n_objects || rt_scene_set_objects(D.cached_scene, first, last - first, nb + first, nullptr) == RT_OK) &&
        (lfirst == nh->n_lights || rt_scene_set_lights(D.cached_scene, lfirst, llast - lfirst, &xyz[0][0], nullptr) == RT_OK) &&
        rt_scene_set_light_intensity(D.cached_scene, nh->light_intensity) == RT_OK &&
        rt_scene_set_camera(D.cached_scene, nh->cam_origin, nh->cam_axis_x, nh->cam_axis_y, nh->cam_axis_z, nullptr) == RT_OK &&
        rt_scene_set_stars_seed(D.cached_scene, nh->stars_seed) == RT_OK) {
      memcpy(D.cached_blob.data(), b, bytes);
      *out = D.cached_scene;
      return RT_OK;
    }
  }
  if (D.cached_scene) { rt_scene_free(D.cached_scene); D.cached_scene = nullptr; D.cached_blob.clear(); }
  rt_scene_dev *s = nullptr;
  const int rc = rt_scene_upload(device, blob, bytes, &s);
  if (rc) return rc;
  D.cached_scene = s;
  D.cached_blob.assign((const uint8_t *)blob, (const uint8_t *)blob + bytes);
  *out = s;
  return RT_OK;
}

// A device allocation must live on the device it was made for: every hipMalloc of the multi-GPU path is checked against
// hipPointerGetAttributes (a wrong current device would otherwise only show as a fault, or as silent xGMI traffic, on a real
// multi-GPU node - nothing a one-GPU box can catch).
int check_on_device(const void *p, const device_state &D, const char *what) {
  hipPointerAttribute_t attr;
  HIP_TRY(hipPointerGetAttributes(&attr, p));
  if (attr.device != D.hip_id) return fail(RT_ERR_DEVICE, "%s was allocated on HIP device %d, expected %d", what, attr.device, D.hip_id);
  return RT_OK;
}

// rt_render's per-device scratch frame, allocated with THAT device current (ensure_device does the hipSetDevice)
int ensure_frame(int device, size_t bytes) {
  int rc = ensure_device(device);
  if (rc) return rc;
  device_state &D = G.dev[device];
  if (D.frame_bytes >= bytes) return RT_OK;
  if (D.d_frame) (void)hipFree(D.d_frame);
  D.d_frame = nullptr; D.frame_bytes = 0;
  HIP_TRY(hipMalloc(&D.d_frame, bytes));
  D.frame_bytes = bytes;
  return check_on_device(D.d_frame, D, "rt_render's frame buffer");
}
}  // namespace

void rt_api::release_rccl() {
  if (G.comms_ready) { for (size_t g = 0; g < G.dev.size(); g++) if (G.comms[g]) NCCL.destroy(G.comms[g]); G.comms_ready = false; }
}

// ------------------------------------------------------------------------------------ a host form's prologue and epilogue
int rt_api::host_call::begin(const void *blob, size_t bytes) {
  if (!G.inited) return fail(RT_ERR_STATE, "rt_init has not been called");
  lock = std::unique_lock<std::mutex>(G.mu);
  t_begin = std::chrono::steady_clock::now();
  if (int rc = scene_for(0, blob, bytes, &s)) return rc;
  if (int rc = ensure_device(0)) return rc;
  stream = G.dev[0].stream;
  return RT_OK;
}

void rt_api::host_call::end(rt_stats *stats, double kernel_ms, uint64_t pixels) const {
  if (!stats) return;
  memset(stats, 0, sizeof *stats);
  stats->kernel_ms = kernel_ms;
  stats->pixels = pixels;
  stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
}

// ------------------------------------------------------------------------------------ render(width,height,scene)
namespace {
int render_to_host(const void *blob, size_t bytes, uint32_t w, uint32_t h, uint8_t *out_rgba, uint32_t flags, rt_stats *stats,
                   uint32_t want_bands, rt_band_callback on_band, void *user);
int g_last_plan = 0;      // how the last rt_render put its frame together: 0 one GPU (banded copy-out), 1 peer stores, 2 ncclGather (or its emulation), 3 one GPU storing into the pinned frame
int g_direct_stores = 1;  // one GPU: store straight into a pinned (mapped) caller buffer: 0 never, 1 frames below 8 MiB, 2 always (rt_render_options)
int g_copy_bands = 4;     // one GPU, copy-out plan: bands whose copy-out overlaps the next band's render (rt_render_options)
}  // namespace

#ifdef RT_TESTING
extern "C" int rt_test_last_plan(void) { return g_last_plan; }
#endif

extern "C" int rt_render_options(int direct_stores, uint32_t copy_bands) {
  if (copy_bands == 0 || copy_bands > 64u) return fail(RT_ERR_INVALID, "copy_bands %u not in 1..64", copy_bands);
  if (direct_stores < 0 || direct_stores > 2) return fail(RT_ERR_INVALID, "direct_stores %d not in 0..2", direct_stores);
  std::lock_guard<std::mutex> lk(G.mu);
  g_direct_stores = direct_stores;
  g_copy_bands = (int)copy_bands;
  return RT_OK;
}

extern "C" int rt_render(const void *blob, size_t bytes, uint32_t w, uint32_t h, uint8_t *out_rgba, uint32_t flags, rt_stats *stats) {
  return render_to_host(blob, bytes, w, h, out_rgba, flags, stats, 0u, nullptr, nullptr);
}

extern "C" int rt_render_progressive(const void *blob, size_t bytes, uint32_t w, uint32_t h, uint8_t *out_rgba, uint32_t n_bands,
                                     rt_band_callback on_band, void *user, uint32_t flags, rt_stats *stats) {
  if (n_bands == 0 || n_bands > 64u) return fail(RT_ERR_INVALID, "n_bands %u not in 1..64", n_bands);
  if (!on_band) return fail(RT_ERR_INVALID, "on_band is NULL");
  return render_to_host(blob, bytes, w, h, out_rgba, flags, stats, n_bands, on_band, user);
}

extern "C" int rt_render_hits(const void *blob, size_t bytes, uint32_t w, uint32_t h, const rt_hit_buffers *hb, rt_stats *stats) {
  if (!hb) return fail(RT_ERR_INVALID, "rt_render_hits: NULL buffers");
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  const uint32_t k = ((const rt_scene_header *)blob)->supersample;
  if ((rc = hits_frame_check(w, h, k, "rt_render_hits"))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  const size_t samples = (size_t)k * w * k * h;
  device_bufs<3> mem;
  const size_t each[3] = {sizeof(int32_t), sizeof(double), 3u * sizeof(float)};
  void *const host[3] = {hb->id, hb->depth, hb->normal};
  for (int i = 0; i < 3; i++) if (host[i]) HIP_TRY(hipMalloc(&mem.p[i], samples * each[i]));
  const rt_hit_buffers db = {(int32_t *)mem.p[0], (double *)mem.p[1], (float *)mem.p[2]};
  const rt_tiles whole = {h, 0u, 1u, 1u};
  rt_stats st;
  if ((rc = rt_render_hits_device(call.s, w, h, &whole, &db, call.stream, &st))) return rc;
  for (int i = 0; i < 3; i++) if (host[i]) HIP_TRY(hipMemcpyAsync(host[i], mem.p[i], samples * each[i], hipMemcpyDeviceToHost, call.stream));
  HIP_TRY(hipStreamSynchronize(call.stream));
  call.end(stats, st.kernel_ms, st.pixels);
  return RT_OK;
}

// Adaptive supersampling of a whole frame on the resident scene (rt_launch.hip: rt_render_adaptive_device), outputs in HOST memory.
extern "C" int rt_render_adaptive(const void *blob, size_t bytes, uint32_t w, uint32_t h, uint32_t k, uint32_t threshold, uint8_t *out_rgba, uint8_t *out_mask,
                                  uint32_t flags, rt_stats *stats, uint64_t *refined) {
  if (!out_rgba) return fail(RT_ERR_INVALID, "rt_render_adaptive: NULL output");
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  const size_t work_bytes = rt_adaptive_work_bytes(w, h);
  if (!work_bytes) return fail(RT_ERR_INVALID, "rt_render_adaptive: frame size %ux%u not in 1..32768", w, h);
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  const size_t pixels = (size_t)w * h;
  device_bufs<3> mem;                                  // the frame, the workspace, the mask
  HIP_TRY(hipMalloc(&mem.p[0], pixels * 4u));
  HIP_TRY(hipMalloc(&mem.p[1], work_bytes));
  if (out_mask) HIP_TRY(hipMalloc(&mem.p[2], pixels));
  rt_stats st;
  if ((rc = rt_render_adaptive_device(call.s, w, h, k, threshold, mem.p[0], (uint8_t *)mem.p[2], mem.p[1], work_bytes, call.stream, flags, &st))) return rc;
  uint32_t n_refined = 0;
  HIP_TRY(hipMemcpyAsync(out_rgba, mem.p[0], pixels * 4u, hipMemcpyDeviceToHost, call.stream));
  HIP_TRY(hipMemcpyAsync(&n_refined, mem.p[1], sizeof n_refined, hipMemcpyDeviceToHost, call.stream));
  if (out_mask) HIP_TRY(hipMemcpyAsync(out_mask, mem.p[2], pixels, hipMemcpyDeviceToHost, call.stream));
  HIP_TRY(hipStreamSynchronize(call.stream));
  if (refined) *refined = n_refined;
  call.end(stats, st.kernel_ms, st.pixels);
  return RT_OK;
}

extern "C" int rt_pick(const void *blob, size_t bytes, uint32_t w, uint32_t h, uint32_t n, const uint32_t *xy, rt_hit *out) {
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = pick_points_check(w, h, ((const rt_scene_header *)blob)->supersample, n, xy, out, "rt_pick"))) return rc;
  if (!G.inited) return fail(RT_ERR_STATE, "rt_init has not been called");
  std::lock_guard<std::mutex> lk(G.mu);
  rt_scene_dev *s = nullptr;
  if ((rc = scene_for(0, blob, bytes, &s))) return rc;
  return rt_scene_pick(s, w, h, n, xy, out);
}

// A list in host memory - rays (rt_trace_rays) or segments (rt_occlusion) - goes through rt_render's resident scene in chunks of
// RT_RAY_CHUNK elements and one set of device buffers (rt_api_internal.h: chunked_list_call).  A row without a host pointer gets no
// buffer.  `binned`: each chunk is ordered on the GPU first (rt_rays_order.hip).  Synchronous.
namespace {
// intersectWorld for a list of rays in host memory (`binned`: rt_trace_rays_binned)
int trace_rays_to_host(const void *blob, size_t bytes, uint64_t n, const double *rays, uint32_t segs, const rt_ray_outputs *ho, rt_stats *stats,
                       bool binned, const char *what) {
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = rays_check(n, rays, segs, ho, what))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  const chunk_row rows[4] = {row_in(rays, 6u * sizeof(double)), row_out(ho->rgb, 3u * sizeof(double)), row_out(ho->rgba, 4u), row_out(ho->hits, sizeof(rt_hit))};
  return chunked_list_call(call, n, rows, 4, binned, stats, [&](uint32_t m, uint64_t base, void *const *d, const uint32_t *d_order, rt_stats *st) {
    const rt_ray_outputs dout = {(double *)d[1], (uint8_t *)d[2], (rt_hit *)d[3]};
    return trace_rays_launch(call.s, m, (uint32_t)base, (const double *)d[0], d_order, segs, dout, call.stream, st);
  });
}

// the arrays of a list of rays that is shaded into nodes
void shade_rows(const double *rays, const uint32_t *pix, const uint32_t *path, rt_node *nodes, chunk_row rows[4]) {
  rows[0] = row_in(rays, 6u * sizeof(double)); rows[1] = row_in(pix, sizeof(uint32_t)); rows[2] = row_in(path, sizeof(uint32_t)); rows[3] = row_out(nodes, sizeof(rt_node));
}
}  // namespace

extern "C" int rt_trace_rays(const void *blob, size_t bytes, uint64_t n, const double *rays, uint32_t segs, const rt_ray_outputs *ho, rt_stats *stats) {
  return trace_rays_to_host(blob, bytes, n, rays, segs, ho, stats, false, "rt_trace_rays");
}

extern "C" int rt_trace_rays_binned(const void *blob, size_t bytes, uint64_t n, const double *rays, uint32_t segs, const rt_ray_outputs *ho,
                                    rt_stats *stats) {
  return trace_rays_to_host(blob, bytes, n, rays, segs, ho, stats, true, "rt_trace_rays_binned");
}

// One level of intersectWorld for a list of rays in host memory (rt_nodes.hip: the shade kernel)
extern "C" int rt_shade_rays(const void *blob, size_t bytes, uint64_t n, const double *rays, const uint32_t *pix, const uint32_t *path, int binned,
                             rt_node *nodes, rt_stats *stats) {
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = shade_check(n, rays, nullptr, pix, path, nodes, "rt_shade_rays"))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  chunk_row rows[4];
  shade_rows(rays, pix, path, nodes, rows);
  return chunked_list_call(call, n, rows, 4, binned != 0, stats, [&](uint32_t m, uint64_t base, void *const *d, const uint32_t *d_order, rt_stats *st) {
    return shade_launch(call.s, m, (uint32_t)base, (const double *)d[0], d_order, (const uint32_t *)d[1], (const uint32_t *)d[2], (rt_node *)d[3], call.stream, st);
  });
}

// rt_shade_rays followed by the relight of each chunk (rt_relight.hip): the table goes up once, and a chunk's base is added to the
// description's where no pix travels, so a list gives the bytes of one launch however it is cut
extern "C" int rt_relight_rays(const void *blob, size_t bytes, const struct rt_lighting *a, const double *offs, uint64_t n, const double *rays,
                               const uint32_t *pix, const uint32_t *path, int binned, rt_node *nodes, rt_stats *stats) {
  const char *what = "rt_relight_rays";
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = rt_lighting_validate(a, offs))) return rc;
  if ((rc = shade_check(n, rays, nullptr, pix, path, nodes, what))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  device_mem d_offs;                                     // (released behind the call, whose every chunk has been waited for)
  if ((rc = lighting_upload_offs(*a, offs, &d_offs, call.stream))) return rc;
  chunk_row rows[4];
  shade_rows(rays, pix, path, nodes, rows);
  return chunked_list_call(call, n, rows, 4, binned != 0, stats, [&](uint32_t m, uint64_t base, void *const *d, const uint32_t *d_order, rt_stats *st) {
    const uint32_t *d_pix = (const uint32_t *)d[1];
    if (int e = shade_launch(call.s, m, (uint32_t)base, (const double *)d[0], d_order, d_pix, (const uint32_t *)d[2], (rt_node *)d[3], call.stream, st)) return e;
    struct rt_lighting ac = *a;
    if (!d_pix) ac.base = a->base + base;                // node i of this chunk is node base + i of the list
    rt_stats relit;
    if (int e = relight_launch(call.s, ac, (const double *)d_offs.h, m, (const double *)d[0], d_order, d_pix, (rt_node *)d[3], call.stream, st ? &relit : nullptr)) return e;
    if (st) st->kernel_ms += relit.kernel_ms;
    return (int)RT_OK;
  });
}

// rt_trace_rays through the wavefront form (include/rt_hip.h: rt_trace_rays_wavefront): per chunk of the list, level after level is
// shaded (rt_nodes.hip) and its children spawned - a level's buffers are sized from the count read back after the spawn that made it -
// down to the call's depth or an empty level, then the levels are folded back up and level 1's colours copied out.  A chunk keeps the
// nodes and links of all its levels until the fold: RT_WAVEFRONT_NODES bounds them, a chunk that would exceed it is halved and started
// again.  Everything else of a level (rays, pix, path, order, workspace, the children's buffers, rgb) lives for that level only.
#define RT_WAVEFRONT_NODES (1u << 21)
namespace {
// the device allocations of one chunk: released one by one as the levels are done with them, and all on every way out
struct device_pool {
  std::vector<void *> held;
  ~device_pool() { for (void *q : held) if (q) (void)hipFree(q); }
  hipError_t get(void **out, size_t bytes) {
    *out = nullptr;
    const hipError_t e = hipMalloc(out, bytes ? bytes : 1u);
    if (e == hipSuccess) held.push_back(*out);
    return e;
  }
  void release(void *q) {
    if (!q) return;
    for (void *&h : held) if (h == q) { (void)hipFree(q); h = nullptr; return; }
  }
};
struct wave_level { rt_node *nodes; int32_t *links; uint32_t count; };
// rt_trace_rays_soft's step behind the shade of every level below `levels` (rt_relight.hip); d_offs: the table, in device memory
struct relight_step { const struct rt_lighting *a; const double *d_offs; uint32_t levels; };

// rays [base, base + m) of the list.  *overflow: the chunk's trees hold more than RT_WAVEFRONT_NODES nodes (and m > 1): nothing was written.
// relight: NULL, or the step that follows a level's shade; without it the launches are rt_trace_rays_wavefront's, one for one
int wavefront_chunk(rt_scene_dev *s, hipStream_t stream, const double *rays, uint64_t base, uint32_t m, uint32_t segs, bool order_levels,
                    const relight_step *relight, const rt_ray_outputs *ho, bool timed, double *kernel_ms, uint64_t *level_counts, bool *overflow) {
  device_pool mem;
  std::vector<wave_level> levels;
  int rc;
  *overflow = false;
  event_timer timer;                                     // one pair of events, used again for every stretch between two host waits
  if (timed) { HIP_TRY(hipEventCreate(&timer.a)); HIP_TRY(hipEventCreate(&timer.b)); }
  auto lap_start = [&]() -> hipError_t { return timed ? hipEventRecord(timer.a, stream) : hipSuccess; };
  auto lap_stop = [&]() -> hipError_t {                  // (the stream has been waited for)
    if (!timed) return hipSuccess;
    hipError_t e = hipEventRecord(timer.b, stream);
    if (e == hipSuccess) e = hipEventSynchronize(timer.b);
    float ms = 0.f;
    if (e == hipSuccess) e = timer.elapsed(&ms);
    *kernel_ms += ms;
    return e;
  };
  void *d_rays = nullptr, *d_pix = nullptr, *d_path = nullptr, *d_count = nullptr;
  HIP_TRY(mem.get(&d_rays, (size_t)m * 48u));
  HIP_TRY(mem.get(&d_count, sizeof(uint32_t)));
  HIP_TRY(hipMemcpyAsync(d_rays, rays + 6u * base, (size_t)m * 48u, hipMemcpyHostToDevice, stream));
  uint32_t c = m;
  uint64_t total = 0;
  for (uint32_t lv = 0; lv < segs && c != 0u; lv++) {
    const uint32_t pix_base = lv == 0u ? (uint32_t)base : 0u;  // (below the first level pix travels in d_pix)
    wave_level L = {nullptr, nullptr, c};
    void *d_order = nullptr, *d_owork = nullptr, *d_swork = nullptr, *d_crays = nullptr, *d_cpix = nullptr, *d_cpath = nullptr;
    HIP_TRY(mem.get((void **)&L.nodes, (size_t)c * sizeof(rt_node)));
    levels.push_back(L);
    total += c;
    HIP_TRY(lap_start());
    if (order_levels && lv != 0u) {
      HIP_TRY(mem.get(&d_order, (size_t)c * sizeof(uint32_t)));
      HIP_TRY(mem.get(&d_owork, rt_rays_order_work_bytes(c)));
      if ((rc = order_rays_launch(c, (const double *)d_rays, (uint32_t *)d_order, d_owork, stream))) return rc;
    }
    if ((rc = shade_launch(s, c, pix_base, (const double *)d_rays, (const uint32_t *)d_order, (const uint32_t *)d_pix, (const uint32_t *)d_path, L.nodes, stream,
                           nullptr)))
      return rc;
    if (relight && lv < relight->levels) {
      // pix is the root ray's index at every level: it travels in d_pix below the first, where the chunk's base stands in for it
      struct rt_lighting ac = *relight->a;
      if (lv == 0u) ac.base = relight->a->base + base;
      if ((rc = relight_launch(s, ac, relight->d_offs, c, (const double *)d_rays, (const uint32_t *)d_order, (const uint32_t *)d_pix, L.nodes, stream, nullptr)))
        return rc;
    }
    uint32_t next = 0u;
    if (lv + 1u < segs) {
      HIP_TRY(mem.get((void **)&levels.back().links, (size_t)c * 2u * sizeof(int32_t)));
      HIP_TRY(mem.get(&d_swork, rt_nodes_spawn_work_bytes(c)));
      HIP_TRY(mem.get(&d_crays, (size_t)c * 2u * 48u));
      HIP_TRY(mem.get(&d_cpix, (size_t)c * 2u * sizeof(uint32_t)));
      HIP_TRY(mem.get(&d_cpath, (size_t)c * 2u * sizeof(uint32_t)));
      if ((rc = spawn_launch(c, pix_base, L.nodes, (const uint32_t *)d_pix, (const uint32_t *)d_path, (double *)d_crays, (uint32_t *)d_cpix, (uint32_t *)d_cpath,
                             levels.back().links, (uint32_t *)d_count, d_swork, stream)))
        return rc;
      HIP_TRY(hipMemcpyAsync(&next, d_count, sizeof next, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(lap_stop());
    mem.release(d_rays); mem.release(d_pix); mem.release(d_path); mem.release(d_order); mem.release(d_owork); mem.release(d_swork);
    d_rays = d_crays; d_pix = d_cpix; d_path = d_cpath;
    if (total + next > RT_WAVEFRONT_NODES && m > 1u) { *overflow = true; return RT_OK; }
    c = next;
  }
  // the fold, from the deepest level up; level 1 writes the call's outputs
  void *d_child_rgb = nullptr, *d_rgba = nullptr;
  if (ho->rgba) HIP_TRY(mem.get(&d_rgba, (size_t)m * 4u));
  HIP_TRY(lap_start());
  for (size_t lv = levels.size(); lv-- > 0;) {
    const wave_level &L = levels[lv];
    void *d_rgb = nullptr;
    if (lv != 0 || ho->rgb) HIP_TRY(mem.get(&d_rgb, (size_t)L.count * 24u));
    if ((rc = fold_launch(L.count, L.nodes, lv + 1 < levels.size() ? L.links : nullptr, (const double *)d_child_rgb, (double *)d_rgb,
                          lv == 0 ? (uint8_t *)d_rgba : nullptr, stream)))
      return rc;
    HIP_TRY(hipStreamSynchronize(stream));               // (the level below is released next: hipFree waits anyway)
    mem.release(d_child_rgb); mem.release(L.nodes); mem.release(L.links);
    d_child_rgb = d_rgb;
  }
  HIP_TRY(lap_stop());
  if (ho->rgb) HIP_TRY(hipMemcpyAsync(ho->rgb + 3u * base, d_child_rgb, (size_t)m * 24u, hipMemcpyDeviceToHost, stream));
  if (ho->rgba) HIP_TRY(hipMemcpyAsync(ho->rgba + 4u * base, d_rgba, (size_t)m * 4u, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (level_counts) for (size_t lv = 0; lv < levels.size(); lv++) level_counts[lv] += levels[lv].count;
  return RT_OK;
}
}  // namespace

namespace {
// the wavefront loop over a list in host memory; a: NULL, or the lights of rt_trace_rays_soft for the first `levels` levels
int wavefront_to_host(const void *blob, size_t bytes, const struct rt_lighting *a, const double *offs, uint32_t levels, uint64_t n, const double *rays,
                      uint32_t segs, int order_levels, const rt_ray_outputs *ho, rt_stats *stats, uint64_t *level_counts, const char *what) {
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if (a && (rc = rt_lighting_validate(a, offs))) return rc;
  if ((rc = rays_check(n, rays, segs, ho, what))) return rc;
  if (ho->hits) return fail(RT_ERR_INVALID, "%s: no hit records (level 1 of rt_scene_shade_rays_device holds them)", what);
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  const uint32_t depth = segs ? segs : call.s->hd.segs;
  device_mem d_offs;                                     // the table goes up once per call
  relight_step step = {a, nullptr, levels};
  const bool relit = a && levels != 0u && depth != 0u;
  if (relit) {
    if ((rc = lighting_upload_offs(*a, offs, &d_offs, call.stream))) return rc;
    step.d_offs = (const double *)d_offs.h;
  }
  if (level_counts) memset(level_counts, 0, RT_MAX_SEGS * sizeof(uint64_t));
  double kernel_ms = 0.0;
  uint32_t chunk = n < RT_RAY_CHUNK ? (uint32_t)n : RT_RAY_CHUNK;
  if (depth == 0u) {
    // intersectWorld(0, ...) is [0,0,0] (main.js:221): no level is shaded, so there is nothing to fold and nothing to launch.  What is
    // left of rt_trace_rays is its guard: a ray with a non-finite component gives NaN x 3, which the store rule makes 0, 0, 0, 255 too
    for (uint64_t i = 0; i < n; i++) {
      const double *q = rays + 6u * i;
      const bool finite = lit_finite6(q[0], q[1], q[2], q[3], q[4], q[5]);
      if (ho->rgb) ho->rgb[3u * i] = ho->rgb[3u * i + 1u] = ho->rgb[3u * i + 2u] = finite ? 0.0 : __builtin_nan("");
      if (ho->rgba) { uint8_t *o = ho->rgba + 4u * i; o[0] = o[1] = o[2] = 0u; o[3] = 255u; }
    }
  }
  for (uint64_t base = 0; depth != 0u && base < n;) {
    const uint32_t m = n - base < chunk ? (uint32_t)(n - base) : chunk;
    bool overflow = false;
    if ((rc = wavefront_chunk(call.s, call.stream, rays, base, m, depth, order_levels != 0, relit ? &step : nullptr, ho, stats != nullptr, &kernel_ms, level_counts, &overflow))) return rc;
    if (overflow) { chunk = m / 2u; continue; }            // (m > 1; a chunk of one ray always fits)
    base += m;
  }
  call.end(stats, kernel_ms, n);
  return RT_OK;
}
}  // namespace

extern "C" int rt_trace_rays_wavefront(const void *blob, size_t bytes, uint64_t n, const double *rays, uint32_t segs, int order_levels,
                                       const rt_ray_outputs *ho, rt_stats *stats, uint64_t *level_counts) {
  return wavefront_to_host(blob, bytes, nullptr, nullptr, 0u, n, rays, segs, order_levels, ho, stats, level_counts, "rt_trace_rays_wavefront");
}

// rt_trace_rays_wavefront with the nodes of the first `levels` levels relit (rt_relight.hip) between their shade and their spawn
extern "C" int rt_trace_rays_soft(const void *blob, size_t bytes, const struct rt_lighting *a, const double *offs, uint32_t levels, uint64_t n,
                                  const double *rays, uint32_t segs, int order_levels, const rt_ray_outputs *ho, rt_stats *stats, uint64_t *level_counts) {
  if (!a) return fail(RT_ERR_INVALID, "rt_trace_rays_soft: NULL lighting description");
  return wavefront_to_host(blob, bytes, a, offs, levels, n, rays, segs, order_levels, ho, stats, level_counts, "rt_trace_rays_soft");
}

// The shadow scan for a list of segments in host memory (`binned`: rt_occlusion_binned)
namespace {
int occlusion_to_host(const void *blob, size_t bytes, uint64_t n, const double *rays, const rt_occlusion_inputs *hi, const rt_occlusion_outputs *ho,
                      rt_stats *stats, bool binned, const char *what) {
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = occlusion_check(n, rays, hi, ho, what))) return rc;
  host_call call;
  if ((rc = call.begin(blob, bytes))) return rc;
  const chunk_row rows[6] = {row_in(rays, 6u * sizeof(double)), row_in(hi ? hi->length : nullptr, sizeof(double)), row_in(hi ? hi->intensity : nullptr, sizeof(double)),
                             row_in(hi ? hi->skip : nullptr, sizeof(int32_t)), row_out(ho->intensity, sizeof(double)), row_out(ho->blocker, sizeof(int32_t))};
  return chunked_list_call(call, n, rows, 6, binned, stats, [&](uint32_t m, uint64_t, void *const *d, const uint32_t *d_order, rt_stats *st) {
    const rt_occlusion_inputs din = {(const double *)d[1], (const double *)d[2], (const int32_t *)d[3]};
    const rt_occlusion_outputs dout = {(double *)d[4], (int32_t *)d[5]};
    return occlusion_launch(call.s, m, (const double *)d[0], d_order, din, dout, call.stream, st);
  });
}
}  // namespace

extern "C" int rt_occlusion(const void *blob, size_t bytes, uint64_t n, const double *rays, const rt_occlusion_inputs *hi, const rt_occlusion_outputs *ho,
                            rt_stats *stats) {
  return occlusion_to_host(blob, bytes, n, rays, hi, ho, stats, false, "rt_occlusion");
}

extern "C" int rt_occlusion_binned(const void *blob, size_t bytes, uint64_t n, const double *rays, const rt_occlusion_inputs *hi,
                                   const rt_occlusion_outputs *ho, rt_stats *stats) {
  return occlusion_to_host(blob, bytes, n, rays, hi, ho, stats, true, "rt_occlusion_binned");
}

namespace {
int render_to_host(const void *blob, size_t bytes, uint32_t w, uint32_t h, uint8_t *out_rgba, uint32_t flags, rt_stats *stats,
                   uint32_t want_bands, rt_band_callback on_band, void *user) {
  if (!out_rgba) return fail(RT_ERR_INVALID, "out_rgba is NULL");
  if (flags & RT_FLAG_RGB24) return fail(RT_ERR_INVALID, "RT_FLAG_RGB24 applies to the device entry points only; rt_render returns ImageData.data (RGBA8)");
  if (!G.inited) return fail(RT_ERR_STATE, "rt_init has not been called");
  std::lock_guard<std::mutex> lk(G.mu);
  const auto t_begin = std::chrono::steady_clock::now();
  const int ndev = (int)G.dev.size();
  const size_t frame_bytes = (size_t)w * h * 4u;
  int rc;
  rt_stats agg;
  memset(&agg, 0, sizeof agg);

  // test build: RT_FORCE_GATHER=1 takes the ncclGather plan - also with ONE device, which runs the real RCCL symbols
  // (ncclCommInitAll, ncclGroupStart/End, ncclGather with one rank) on a one-GPU box
  const bool force_gather = RT_TEST_ENV("RT_FORCE_GATHER") != nullptr;
  g_last_plan = 0;
  if ((ndev == 1 && !force_gather) || h < (uint32_t)ndev * RT_TILE_H) {
    // ---- one GPU.  Large frames are rendered as a few row bands so that the PCIe copy-out of band i (copy
    //      stream) runs while band i+1 renders (render stream): the frame costs ~max(render, copy), not the sum ----
    rt_scene_dev *s = nullptr;
    if ((rc = scene_for(0, blob, bytes, &s))) return rc;
    device_state &D = G.dev[0];
    rc = ensure_device(0);                                          // (makes device 0 current: a previous multi-GPU call may have left another one)
    const bool count = (flags & RT_FLAG_COUNT) != 0;
    // Where the frame goes.  A buffer from rt_alloc_pinned (what the N-API layer hands in: the ImageData.data of main.js:83,
    // 195-200) is mapped into the GPU's address space: the kernel can store its pixels STRAIGHT into it over PCIe - 128-byte lines,
    // posted writes - with no staging frame in HBM, no copy engine and no band bookkeeping; the call then takes
    // ~max(kernel, frame bytes / PCIe).  Measured (r03_ab_log.md section 4) that is what the banded copy-out below takes as well -
    // the link, ~50-55 GB/s here, is the bound either way - and the copy engine is 2-7 % ahead for frames of 8 MiB and more, the
    // direct stores 3 % for smaller ones: the default follows the measurement.  Pageable memory always takes the copy-out.
    void *d_direct = nullptr;
    if (!rc && (g_direct_stores == 2 || (g_direct_stores == 1 && frame_bytes < (8u << 20)))) {
      hipPointerAttribute_t attr;
      if (hipPointerGetAttributes(&attr, out_rgba) == hipSuccess && attr.type == hipMemoryTypeHost && attr.devicePointer) d_direct = attr.devicePointer;
      else (void)hipGetLastError();
    }
    if (rc) return rc;
    const bool copy_out = d_direct == nullptr;
    if (copy_out && (rc = ensure_frame(0, frame_bytes))) return rc;
    if (copy_out && !D.copy_stream) {
      const hipError_t e = hipStreamCreateWithFlags(&D.copy_stream, hipStreamNonBlocking);
      if (e != hipSuccess) return fail(RT_ERR_DEVICE, "copy stream: %s", hipGetErrorString(e));
    }
    uint8_t *const d_dst = copy_out ? (uint8_t *)D.d_frame : (uint8_t *)d_direct;
    // The bands.  Counters come from one instrumented launch; a caller that asked for bands (rt_render_progressive) gets that many.
    // Direct stores: one band.  Copy-out frames of 8 MiB and more: g_copy_bands (4) - measured against 1, 2, 8, 16 equal bands,
    // growing bands and the direct stores above in profiles/r03_ab_log.md section 4: every plan ends within a few percent of frame
    // bytes / PCIe rate.
    const uint32_t nb = count ? 1u : (want_bands ? want_bands : ((!copy_out || frame_bytes < (8u << 20)) ? 1u : (uint32_t)g_copy_bands));
    const uint32_t rows_per = ((h + nb - 1) / nb + RT_TILE_H - 1) / RT_TILE_H * RT_TILE_H;
    const uint32_t n_bands = (h + rows_per - 1) / rows_per;
    rt_stats st;
    memset(&st, 0, sizeof st);
    // one launch over the whole frame, which times itself: direct stores when one band was asked for, a copy-out when the frame makes one
    if (copy_out ? n_bands == 1u : nb == 1u) {
      rt_tiles whole = {h, 0, 1, 1};
      rc = rt_render_tiles_device(s, w, h, &whole, d_dst, nullptr, flags, &st);       // (waits: stats)
      if (!rc && copy_out) {
        hipError_t e = hipMemcpyAsync(out_rgba, D.d_frame, frame_bytes, hipMemcpyDeviceToHost, D.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(D.stream);
        if (e != hipSuccess) rc = fail(RT_ERR_DEVICE, "copy-out: %s", hipGetErrorString(e));
      }
      if (!rc && on_band) on_band(user, 0u, h);
    } else {
      // one launch per band; a copy-out copies each band on the copy stream behind its render, while the next band renders
      event_timer timer;
      std::vector<hipEvent_t> rendered(n_bands, nullptr), ready(n_bands, nullptr);
      hipError_t e = timer.start(D.stream);
      for (uint32_t b = 0; b < n_bands && !rc && e == hipSuccess; b++) {
        const uint32_t r0 = b * rows_per, rows = (r0 + rows_per <= h) ? rows_per : h - r0;
        rt_tiles band = {rows_per, b, 1, 1};
        uint8_t *d_band = d_dst + (size_t)r0 * w * 4u;
        rc = rt_render_tiles_device(s, w, h, &band, d_band, nullptr, flags, nullptr);
        if (rc) break;
        hipStream_t ready_on = D.stream;
        if (copy_out) {
          e = hipEventCreateWithFlags(&rendered[b], hipEventDisableTiming);
          if (e == hipSuccess) e = hipEventRecord(rendered[b], D.stream);
          if (e == hipSuccess) e = hipStreamWaitEvent(D.copy_stream, rendered[b], 0);
          if (e == hipSuccess) e = hipMemcpyAsync(out_rgba + (size_t)r0 * w * 4u, d_band, (size_t)rows * w * 4u, hipMemcpyDeviceToHost, D.copy_stream);
          ready_on = D.copy_stream;
        }
        if (e == hipSuccess && on_band) e = hipEventCreateWithFlags(&ready[b], hipEventDisableTiming);
        if (e == hipSuccess && on_band) e = hipEventRecord(ready[b], ready_on);
      }
      if (e == hipSuccess && !rc) e = timer.stop(D.stream);
      // progressive delivery: every band is announced as soon as its rows are in the caller's buffer (behind its render, or its
      // copy), while the later bands are still rendering or on the PCIe link (the reference shows its frame row by row, main.js:201)
      for (uint32_t b = 0; on_band && b < n_bands && e == hipSuccess && !rc && ready[b]; b++) {
        e = hipEventSynchronize(ready[b]);
        const uint32_t r0 = b * rows_per;
        if (e == hipSuccess) on_band(user, r0, (r0 + rows_per <= h) ? rows_per : h - r0);
      }
      // on EVERY way out nothing may still be storing or copying into the caller's buffer: the caller may hand that (pinned) buffer
      // back to the pool as soon as this returns
      {
        const hipError_t e1 = hipStreamSynchronize(D.stream), e2 = copy_out ? hipStreamSynchronize(D.copy_stream) : hipSuccess;
        if (e == hipSuccess) e = (e1 != hipSuccess) ? e1 : e2;
      }
      if (e == hipSuccess && !rc) { float ms = 0.f; e = timer.elapsed(&ms); st.kernel_ms = ms; }
      if (e != hipSuccess && !rc) rc = fail(RT_ERR_DEVICE, copy_out ? "banded render/copy-out: %s" : "banded render into the pinned frame: %s", hipGetErrorString(e));
      st.pixels = (uint64_t)w * h;
      for (hipEvent_t ev : rendered) if (ev) (void)hipEventDestroy(ev);
      for (hipEvent_t ev : ready) if (ev) (void)hipEventDestroy(ev);
    }
    if (rc) return rc;
    agg = st;
    g_last_plan = copy_out ? 0 : 3;
  } else {
    // ---- G GPUs of one node (one process): interleaved row tiles (sky rows are cheap, floor rows are not), reassembled
    //      on GPU 0.  Primary plan: PEER STORES - every GPU's kernel writes its tiles straight into GPU 0's frame buffer over
    //      xGMI (hipDeviceEnablePeerAccess; rows at their place in the frame, whole 128-byte lines: the scatter store), so
    //      there is no gather buffer, no collective and no de-interleave pass.  Fallback (no peer access between some pair,
    //      or the test build's RT_FORCE_GATHER): RGB24 bands, ONE ncclGather to GPU 0, one de-interleave pass. ----
    const uint32_t tile_rows = (h >= (uint32_t)ndev * 64u) ? 16u : RT_TILE_H;
    const uint32_t n_tiles_total = (h + tile_rows - 1) / tile_rows;
    const uint32_t tiles_per_rank = (n_tiles_total + ndev - 1) / ndev;
    bool peer_plan = !force_gather;
    for (int g = 1; g < ndev && peer_plan && !G.emulated; g++) {
      device_state &D = G.dev[g];
      if (D.peer_to_root == 0) {
        int can = 0;
        hipError_t e = hipDeviceCanAccessPeer(&can, D.hip_id, G.dev[0].hip_id);
        if (e == hipSuccess && can) {
          e = hipSetDevice(D.hip_id);
          if (e == hipSuccess) e = hipDeviceEnablePeerAccess(G.dev[0].hip_id, 0);
          if (e == hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); e = hipSuccess; }
        }
        D.peer_to_root = (e == hipSuccess && can) ? 1 : -1;
      }
      if (D.peer_to_root < 0) peer_plan = false;
    }
    std::vector<rt_scene_dev *> scenes(ndev, nullptr);
    std::vector<event_timer> timers(ndev);
    // device g's share of the frame (`launch`), timed on its stream
    auto launch_timed = [&](int g, auto launch) {
      int r = ensure_device(g);
      if (r) return r;
      hipError_t e = timers[g].start(G.dev[g].stream);
      if (e == hipSuccess) {
        if ((r = launch())) return r;
        e = timers[g].stop(G.dev[g].stream);
      }
      return e == hipSuccess ? RT_OK : fail(RT_ERR_DEVICE, "timing events on device %d: %s", g, hipGetErrorString(e));
    };
    const uint32_t kflags = flags & ~(uint32_t)RT_FLAG_COUNT;
    rc = RT_OK;
    if (peer_plan) {
      for (int g = 0; g < ndev && !rc; g++) rc = scene_for(g, blob, bytes, &scenes[g]);     // (the scenes stay cached on their devices)
      if (!rc) rc = ensure_frame(0, frame_bytes);
      void *root_frame[1] = {G.dev[0].d_frame};
      for (int g = 0; g < ndev && !rc; g++)
        rc = launch_timed(g, [&] {
          rt_tiles t = {tile_rows, (uint32_t)g, (uint32_t)ndev, tiles_per_rank};
          // (the sky blocks of the whole frame are GPU 0's own work, below: the other GPUs do not send theirs over the links)
          int r = rt_render_scatter_device(scenes[g], w, h, &t, 1u, root_frame, nullptr, kflags | (g ? RT_FLAG_NO_SKY : 0u), nullptr);
          if (!r && g == 0) {
            rt_tiles whole = {h, 0u, 1u, 1u};
            r = rt_render_scatter_device(scenes[0], w, h, &whole, 1u, root_frame, nullptr, kflags | RT_FLAG_SKY_ONLY, nullptr);
          }
          return r;
        });
      // every GPU's stores have landed in GPU 0's frame once its stream is drained; then the copy-out
      for (int g = 0; g < ndev; g++) {
        if (!G.dev[g].stream) continue;
        hipError_t e = hipSetDevice(G.dev[g].hip_id);
        if (e == hipSuccess) e = hipStreamSynchronize(G.dev[g].stream);
        if (e != hipSuccess && !rc) rc = fail(RT_ERR_DEVICE, "peer-store plan, device %d: %s", g, hipGetErrorString(e));
      }
      if (!rc) {
        device_state &R = G.dev[0];
        hipError_t e = hipSetDevice(R.hip_id);
        if (e == hipSuccess) e = hipMemcpyAsync(out_rgba, R.d_frame, frame_bytes, hipMemcpyDeviceToHost, R.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(R.stream);
        if (e != hipSuccess) rc = fail(RT_ERR_DEVICE, "copy-out: %s", hipGetErrorString(e));
      }
    } else {
      if (!G.emulated && (rc = ensure_rccl(ndev))) return rc;      // nothing allocated yet
      // bands cross xGMI as RGB24 when the width allows it (the alpha byte is the constant 255, main.js:198; the
      // de-interleave restores it); tile_rows >= 8, so a band is a multiple of 96 bytes and d_final stays 16-byte aligned
      // (the 3x3 / 4x4 box filter of the two-pass supersampling stores RGBA8: those scenes gather RGBA8 bands)
      for (int g = 0; g < ndev && !rc; g++) rc = scene_for(g, blob, bytes, &scenes[g]);
      const bool rgb24 = (w & 3u) == 0 && !rc && scenes[0]->hd.supersample <= 2u;
      const size_t band_bytes = (size_t)tiles_per_rank * tile_rows * w * (rgb24 ? 3u : 4u);
      for (int g = 0; g < ndev && !rc; g++) rc = ensure_frame(g, band_bytes);
      if (!rc && !(rc = ensure_device(0))) {
        device_state &R = G.dev[0];
        if (R.gather_bytes < band_bytes * ndev + frame_bytes) {
          if (R.d_gather) (void)hipFree(R.d_gather);
          R.d_gather = nullptr; R.gather_bytes = 0;
          hipError_t e = hipMalloc(&R.d_gather, band_bytes * ndev + frame_bytes);
          if (e != hipSuccess) rc = fail(RT_ERR_DEVICE, "gather buffer: %s", hipGetErrorString(e));
          else { R.gather_bytes = band_bytes * ndev + frame_bytes; rc = check_on_device(R.d_gather, R, "rt_render's gather buffer"); }
        }
      }
      for (int g = 0; g < ndev && !rc; g++)
        rc = launch_timed(g, [&] {
          rt_tiles t = {tile_rows, (uint32_t)g, (uint32_t)ndev, tiles_per_rank};
          return rt_render_tiles_device(scenes[g], w, h, &t, G.dev[g].d_frame, nullptr, kflags | (rgb24 ? RT_FLAG_RGB24 : 0u), nullptr);
        });
      if (!rc && G.emulated) {                      // one physical GPU: the gather is a set of device-to-device copies
        for (int g = 0; g < ndev; g++) {
          hipError_t e = hipMemcpyAsync((uint8_t *)G.dev[0].d_gather + band_bytes * g, G.dev[g].d_frame, band_bytes, hipMemcpyDeviceToDevice, G.dev[g].stream);
          if (e == hipSuccess) e = hipStreamSynchronize(G.dev[g].stream);
          if (e != hipSuccess && !rc) rc = fail(RT_ERR_DEVICE, "emulated gather: %s", hipGetErrorString(e));
        }
      } else if (!rc) {
        // one ncclGather per device inside one group; a group that was opened is always closed, and every return code counts
        int r = NCCL.group_start();
        if (r != 0) rc = fail(RT_ERR_DEVICE, "ncclGroupStart: %s", NCCL.errstr(r));
        else {
          for (int g = 0; g < ndev && !rc; g++) {
            hipError_t e = hipSetDevice(G.dev[g].hip_id);
            if (e != hipSuccess) { rc = fail(RT_ERR_DEVICE, "hipSetDevice(%d): %s", G.dev[g].hip_id, hipGetErrorString(e)); break; }
            r = NCCL.gather(G.dev[g].d_frame, g == 0 ? G.dev[0].d_gather : nullptr, band_bytes, NCCL_UINT8, 0, G.comms[g], G.dev[g].stream);
            if (r != 0) rc = fail(RT_ERR_DEVICE, "ncclGather on device %d: %s", g, NCCL.errstr(r));
          }
          r = NCCL.group_end();
          if (r != 0 && !rc) rc = fail(RT_ERR_DEVICE, "ncclGroupEnd: %s", NCCL.errstr(r));
        }
      }
      if (!rc) {
        device_state &R = G.dev[0];
        uint8_t *d_final = (uint8_t *)R.d_gather + band_bytes * ndev;
        rc = (rgb24 ? rt_deinterleave_rgb24_device : rt_deinterleave_device)(0, R.d_gather, d_final, w, h, tile_rows, (uint32_t)ndev, band_bytes, nullptr);
        if (!rc) {
          hipError_t e = hipSetDevice(R.hip_id);
          if (e == hipSuccess) e = hipMemcpyAsync(out_rgba, d_final, frame_bytes, hipMemcpyDeviceToHost, R.stream);
          if (e == hipSuccess) e = hipStreamSynchronize(R.stream);
          if (e != hipSuccess) rc = fail(RT_ERR_DEVICE, "copy-out: %s", hipGetErrorString(e));
        }
      }
    }
    for (int g = 0; g < ndev; g++) {
      (void)hipSetDevice(G.dev[g].hip_id);
      if (G.dev[g].stream) (void)hipStreamSynchronize(G.dev[g].stream);
      float ms = 0.f;
      if (timers[g].a && timers[g].b && timers[g].elapsed(&ms) == hipSuccess && ms > agg.kernel_ms) agg.kernel_ms = ms;   // slowest GPU
      timers[g].release();
    }
    (void)hipSetDevice(G.dev[0].hip_id);
    if (rc) return rc;
    agg.pixels = (uint64_t)w * h;
    g_last_plan = peer_plan ? 1 : 2;
    if (on_band) on_band(user, 0u, h);           // several GPUs: the frame arrives whole
  }
  agg.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  if (stats) *stats = agg;
  return RT_OK;
}
}  // namespace
