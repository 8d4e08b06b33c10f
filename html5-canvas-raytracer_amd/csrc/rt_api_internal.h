// rt_api_internal.h — what the host units of the C ABI share: errors and test switches, the library and device state, the resident
// scene (rt_scene_dev) and the few functions that cross units.  Not part of the ABI.
//   rt_scene_sync.h  the stream ordering of a resident scene's launches, moves and texel edits (rules R1-R6) and the events, side stream
//                  and pinned rings it owns for it: header-only, HIP's API and nothing of the project
//   rt_chunked.h   how a host form pushes its work through one set of device buffers in chunks (lists: elements, views: whole rows): the
//                  driver, the device buffers of a call, the clocks of a call that reports rt_stats: header-only, HIP's API, rt_stats, the error codes
//   rt_api.hip     lifetime, errors, device state, the scratch guard and the per-variant scratch figures, the host-logic probes, memory helpers, IPC
//   rt_scene.hip   upload and moves of a resident scene (the generation pipeline), its texel edits (rt_texels.hip), its launch decisions and launch
//                  tables, and the launch prologue (enter_launch)
//   rt_launch.hip  the launches: colour (the launch record, then the strict launch or the product launch and rt_retrace), supersampling,
//                  compact bands, adaptive supersampling (rt_adaptive.hip), primary hits and picking, ray lists, occlusion queries
//   rt_frame.hip   rt_render and its one-GPU and multi-GPU plans, RCCL, de-interleave, the prologue and epilogue of every host form (host_call),
//                  rt_render_hits / rt_pick, and the host lists that go through device buffers in chunks (rt_trace_rays, rt_occlusion and
//                  their binned forms, rt_shade_rays, rt_relight_rays), rt_trace_rays_wavefront / rt_trace_rays_soft
//   rt_nodes_api.hip  the wavefront form's device entry points: one level of nodes, the next level's ray list, the fold (rt_nodes.hip)
//   rt_views_api.hip  views: validation, the panorama's tables, the host probe, the generator's launch (rt_views.hip), the traces of a whole view,
//                  and what every unit that traces a view shares: the size test, the workspace check, the upload of the panorama's tables
//   rt_ambient_api.hip  ambient occlusion: validation, the cosine table, the host probe, the launches of rt_ambient.hip, the host forms
//   rt_lighting_api.hip  sampled lights: validation, the offset table, the host probe, the launch of rt_lighting.hip, the host forms
//   rt_relight_api.hip  relit nodes: the argument check, the launch of rt_relight.hip and its device entry point (the host forms are rt_frame.hip's)
//   rt_soft_api.hip  the soft trace in one launch: the argument check, the launch of rt_soft.hip, its device entry points (a list, a view) and host forms
//   rt_gather_api.hip  gathered light: the argument checks, the launch of rt_gather.hip, its device entry points (a list, a view) and host forms
//   rt_probe_api.hip  probes: the weights' checks, the launch of rt_probe.hip on rt_gather_api.hip's launch record, the device entry point, the
//                  host form, the spherical-harmonics weights
// A host form is its argument checks, host_call::begin, rows for the chunk driver (chunked_list_call, chunked_view_call below) and a
// step of launches; the band loop of a view is for_bands.
// Which kernel a launch runs is one value (rt_device.h: rt_trace_variant), worked out once per launch; the two builds of rt_kernel.hip map
// it to a kernel (rt_kernel_trace_fast / rt_kernel_trace_strict), and the declarations below are all the host sees of them.
#ifndef RT_API_INTERNAL_H
#define RT_API_INTERNAL_H

#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "rt_device.h"
#include "rt_tables.h"
#include "rt_tables_gpu.h"
#include "rt_hits.h"
#include "rt_objects_gpu.h"
#include "rt_rays_order.h"
#include "rt_occlusion.h"
#include "rt_nodes.h"
#include "rt_texels.h"
#include "rt_adaptive.h"
#include "rt_scene_sync.h"
#include "rt_chunked.h"

// per build of rt_kernel.hip (product, strict): the variant's kernel (NULL: not this build's) and its launch
extern "C" const void *rt_kernel_trace_fast(rt_trace_variant);
extern "C" const void *rt_kernel_trace_strict(rt_trace_variant);
extern "C" int rt_launch_trace_fast(const rt_launch *, rt_trace_variant, unsigned n_wg, const uint32_t *order, unsigned lds_bytes, hipStream_t);
extern "C" int rt_launch_trace_strict(const rt_launch *, rt_trace_variant, unsigned n_wg, const uint32_t *order, unsigned lds_bytes, hipStream_t);

using namespace rt_tables;   // the host-built tables (pure host logic, rt_tables.cpp)

namespace rt_api {

extern thread_local char g_err[512];

// A/B and test switches exist only in the TEST build of this library (csrc/Makefile: librt_hip_test.so, -DRT_TESTING,
// selected by the tests with RT_HIP_LIB).  The product library reads no environment variable on the render path.
#ifdef RT_TESTING
#define RT_TEST_ENV(name) getenv(name)
#else
#define RT_TEST_ENV(name) ((const char *)nullptr)
#endif

struct device_state {
  int hip_id = -1;
  hipStream_t stream = nullptr;          // created on first use
  hipStream_t copy_stream = nullptr;     // rt_render: PCIe copy-out overlapped with rendering
  unsigned long long *d_counters = nullptr;
  void *d_frame = nullptr;               // rt_render scratch: this device's tiles (or the whole frame)
  size_t frame_bytes = 0;
  void *d_gather = nullptr;              // device 0 only: gather target (fallback plan of rt_render on several GPUs)
  size_t gather_bytes = 0;
  int peer_to_root = 0;                  // rt_render on several GPUs: 1 = this device may store into device 0's memory, -1 = it may not, 0 = not asked yet
  // rt_render: the scene of the previous call stays resident; a call with the same blob (byte for byte) reuses it
  // (upload + table builds cost 0.1 ms for 8 spheres and 1.8 ms for 64, against a 0.7 ms frame)
  struct rt_scene_dev *cached_scene = nullptr;
  std::vector<uint8_t> cached_blob;
  // scratch_guard: wave slots of the device (CUs x waves per CU) and, per stream, the largest per-lane scratch figure whose reservation
  // has been held against the free device memory
  size_t wave_slots = 0;
  struct scratch_seen { hipStream_t stream; size_t per_lane; };
  std::vector<scratch_seen> scratch_checked;
};

struct lib_state {
  bool inited = false;
  std::vector<device_state> dev;
  std::mutex mu;
  std::mutex dev_mu;                     // lazy per-device stream creation (ensure_device may run inside rt_render, which holds `mu`)
  // RCCL, resolved lazily with dlopen so that single-GPU users never load it
  void *rccl = nullptr;
  void *comms[16] = {nullptr};
  bool comms_ready = false;
  // RT_EMULATE_DEVICES=N (test aid for 1-GPU boxes): rt_init reports N devices that all map to HIP device 0, and
  // rt_render's gather becomes device-to-device copies instead of ncclGather (RCCL refuses two ranks on one GPU).
  // Everything else of the multi-GPU frame - tile plan, per-device scenes and streams, RGB24 bands, de-interleave -
  // runs as on a real node.
  bool emulated = false;
  bool all_visible = false;
};
extern lib_state G;

int ensure_device(int d);
// an entry point's prologue: the device is ready and current, and the launch's stream is the caller's or the device's own
int device_stream(int device, void *hip_stream, hipStream_t *stream);
int scratch_guard(device_state &D, hipStream_t stream, size_t per_lane, uint64_t waves_in_grid, const char *what);
int kernel_scratch(rt_trace_variant v, size_t *out);
int guard_kernel_scratch(device_state &D, hipStream_t stream, rt_trace_variant v, uint64_t waves_in_grid, const char *what);
// the variant's launch, by the build that has its kernel (n_wg, order: the list-driven kernels'; lds_bytes: rt_trace's)
inline int launch_variant(const rt_launch &L, rt_trace_variant v, unsigned n_wg, const uint32_t *order, unsigned lds_bytes, hipStream_t stream) {
  return (v.strict ? rt_launch_trace_strict : rt_launch_trace_fast)(&L, v, n_wg, order, lds_bytes, stream);
}
int check_frame(const char *what, uint32_t w, uint32_t h, const rt_tiles *tiles, uint32_t flags);
uint64_t tile_set_pixels(uint32_t w, uint32_t h, const rt_tiles *tiles);

// The sample grid of a launch over a w x h frame at supersample ss (1 or 2; the hit kernels: 1..4): workgroups per tile row, rows
// per workgroup, row blocks per tile, and the projection constants (main.js:102-105) in binary64 on the host.
struct launch_geom { uint32_t tiles_x, rows_per_wg, rb_per_tile; double proj_w, proj_h, proj_d; };
launch_geom launch_geometry(double fov_deg, uint32_t w, uint32_t h, uint32_t ss, uint32_t tile_rows);

using device_mem = owned<void *, hipFree>;   // (rt_scene_sync.h; pinned_mem: hipHostFree)

}  // namespace rt_api

using namespace rt_api;

// One kind of frame: size, sample grid (1 or 2), tile set and sky part (0 everything, 1 RT_FLAG_NO_SKY, 2 RT_FLAG_SKY_ONLY).  A scene
// keeps a launch table and a use count per kind.
struct frame_kind {
  uint32_t w, h, ss;
  rt_tiles tiles;
  uint32_t part;
  bool operator==(const frame_kind &o) const {
    return w == o.w && h == o.h && ss == o.ss && tiles.tile_rows == o.tiles.tile_rows && tiles.tile_first == o.tiles.tile_first &&
           tiles.tile_stride == o.tiles.tile_stride && tiles.n_tiles == o.tiles.n_tiles && part == o.part;
  }
};

struct rt_scene_dev {
  int device;
  // Everything the scene keeps in HBM is ONE allocation (`arena`), filled by one copy at upload; the pointers below point into it.
  // Its last part is the CAMERA BLOCK - what depends on the camera: per ordering the camera-anchored geometry and the cull
  // rectangles, and (few spheres) the LDS images, whose tails are the cull rectangles - rewritten with one small asynchronous copy
  // when the camera moves (rt_scene_set_camera).
  device_mem arena;
  size_t arena_bytes = 0;
  void *d_blob;                  // the uploaded scene blob (its texels; its sphere records are the OBJECT BLOCK's, its lights travel by value from `lights`)
  rt_texture_desc *d_texdesc;    // RT_MAX_TEXTURES descriptors (zero padded)
  double *d_cones;               // the bounce table's cell cones (rt_tables.cpp: bounce_cell_cones), or NULL (no bounce table)
  // The OBJECT BLOCK: what depends on the spheres but not on the camera, at offsets o_* inside it:
  //   o_objs     the sphere records in blob order (1/r in `reserved`)
  //   o_geom     camera-independent geometry tables, per ordering [plain N | anchored at light k: NL x N]
  //   o_objs_b   object records with the enclosing sphere moved last (ordering B); none without one
  //   o_img      many spheres: per ordering [materials (rt_mtl) | 16 texture descriptors], the LDS image (few spheres: it holds the
  //              cull rectangles and lives in the camera block)
  //   o_sg       light grids for the product kernel's loop order (has_sg: more than RT_SGRID_MIN_LOOP loop spheres)
  //   o_bt       bounce table for the same order (has_bt: more than RT_BTABLE_MIN_LOOP loop spheres and depth >= 2)
  // Everything up to the shadow grids' masks (obj_host_bytes) is written by the host; the masks and the bounce table are built from it
  // (rt_objects_gpu.hip after a move; rt_tables.cpp at upload).  Of these the anchored records and the light grids depend on the lights:
  // a light move rewrites them alone, for the lights that moved.  TWO blocks, like the camera blocks: generation g reads block g & 1,
  // so that rt_scene_set_objects can write the next one while launches with the current spheres are still running.
  uint8_t *d_obj_buf[2];
  size_t obj_bytes, obj_host_bytes;
  size_t o_objs, o_geom, o_objs_b, o_img, o_sg, o_bt, sg_bytes, bt_bytes;
  bool has_sg, has_bt;
  uint64_t obj_version = 0;      // bumped by every object move; slot_version[b]: the version object block b holds
  uint64_t slot_version[2] = {0, 0};
  double slot_lights[2][RT_MAX_LIGHTS][3];   // the light positions object block b's anchored records and shadow grids were made for (rt_scene_set_lights)
  // The camera block: per ordering [anchored at the camera N | cull rectangles N], then (few spheres) the LDS images.  TWO of them:
  // camera generation g lives in block g & 1, so that the block of the NEXT camera can be written - on the scene's own side stream,
  // by rt_scene_set_camera - while launches with the current one are still running.
  uint8_t *d_cam_buf[2];
  size_t cam_lds_offset;         // of the LDS images inside a camera block
  size_t cam_bytes;              // (with the padding the many-sphere staging may read over)
  size_t cam_bytes_used;         // what a camera move has to copy
  bool has_b;                    // two orderings (an enclosing sphere)
  bool cull_in_lds;
  size_t lds_image_bytes;        // of one ordering
  uint64_t cam_gen = 1;          // bumped when the camera moves: launch tables and mark counts of an older camera are stale
  // product launches per frame kind since the camera last moved: many-sphere scenes get their shadow masks with the SECOND frame of a kind
  struct camera_use { frame_kind kind; uint64_t cam_gen; uint32_t uses; };
  std::vector<camera_use> camera_uses;
  scene_sync sync;               // the stream ordering of launches, moves and texel edits, and what it owns (rt_scene_sync.h)
  // Texels live once, in d_blob, and every kernel reads them through texel_base + texels_offset; no table, host decision or mark count
  // reads a texel's VALUE (flag_tol and the strict routing read widths and heights; a texture sampler is never a constant sky).  So a
  // texel edit is no generation (rt_scene_sync.h: R4).  host_blob keeps the texels of the upload: nothing reads them.
  std::vector<uint8_t> host_blob;        // the scene as uploaded (patched: 1/r per sphere), for rebuilding the camera block
  std::vector<rt_sphere> host_objects_b; // ordering B of its sphere records
  rt_scene_header hd;            // host copy
  bool refract;                  // any albedo[4] > 0  -> general (binary-tree) kernel variant
  unsigned lds_bytes;
  double lights[RT_MAX_LIGHTS][3];   // host copy: lights travel in the kernarg segment
  uint32_t enclosing;            // sphere that strictly contains everything else (a skybox), or ~0u
  bool enclosing_flat;           // ... and it has no lighting, no children and a sampler that ignores the hit point (colour / stars)
  bool sky_const;                // ... a plain colour: the pixel of a ray that meets nothing else is the constant sky_rgb
  double sky_rgb[3];
  // cost-ordered dispatch (dispatch_order below): per sphere its screen rectangle (X/D, Y/D bounds, scene order) and a weight,
  // and the order tables built so far, one per (frame size, tile set), kept on the device
  std::vector<rt_sphere> host_objects;   // the scene's sphere records (scene order), for the launch table's sky marking
  std::vector<rt_geom> host_cull;
  std::vector<uint32_t> tile_weight;
  // One launch table per (frame size, tile set, flags), built on the GPU (rt_tables_gpu.hip) on the stream of the launch that needs
  // it first and again when the camera has moved since (cam_gen).  `Tb` = its device memory; `d_blockb` = ONE allocation
  // behind all of T's arrays; `n_blocks` workgroups are launched until the host has seen the number of entries the build published
  // (`known`: generation << 32 | entries + 1, a pinned host word), from then on exactly that many.
  struct order_entry {
    frame_kind kind; int ranked; bool sky, masks, cands; int cells; bool first_bounce; int second_node;     // ranked: 0 grid order, 1 ranked when large enough, 2 always (a compact band's launch)
    uint64_t cam_gen; uint32_t n_blocks; volatile unsigned long long *known; hipStream_t built_on; event built;
    bool shared;                   // launched with on a stream other than the one it was built on
    // two tables, like the camera blocks: generation g's is Tb[g & 1] (the next camera's is built while this one's is still read)
    rt_table_dev Tb[2]; device_mem d_blockb[2]; size_t hist_wordsb[2];
    uint32_t cost_bins;            // of the current build (rt_retrace of a compact launch)
    uint64_t used_gen;             // the last camera generation a launch used it with: a move rebuilds the tables in use ahead of the next render
  };
  std::vector<order_entry> orders;
  uint32_t order_evict = 0;
  rt_texture_desc descs[RT_MAX_TEXTURES];
  // Marked samples (rt_device.h, rt_kernel.hip: rt_retrace).  One state per (launch table, stream): the device list the product
  // launch appends to and rt_retrace reads, which of its two counters the next launch uses, and a pinned host word in which
  // rt_retrace publishes how many samples a frame of this scene, camera, size and tile set marks - the same every time, so once it
  // says "none" (and the sample grid has no odd centre) the second launch is skipped.  Launches that share a state share a
  // stream, i.e. they are ordered; mark_mu makes a launch pair one step for the threads of this process.
  struct mark_state { uint32_t order_index; hipStream_t stream; device_mem d_marks; volatile unsigned long long *h_known; uint32_t slot; };   // *h_known: camera generation << 32 | marks + 1
  std::vector<mark_state> mark_states;
  pinned_mem h_known_pool;       // 2 x RT_KNOWN_WORDS pinned words: the mark states', then the launch tables'
  std::mutex launch_mu;          // a product launch - its table (found or built), the trace launch, rt_retrace - is one step for the threads of this process
  bool needs_strict;             // the scene sits on an exact coincidence (below): every launch uses the strict kernel
  bool needs_strict_scene;       // ... whatever the camera (a light on a surface, a sphere without a radius, exotic checker frequencies)
  bool unit_weights;             // every albedo and colour in [0, 1] (RT_MARK_WEIGHT)
  double flag_tol;               // RT_FLAG_T1 x the largest sampler frequency of the scene (texture width / height, checker frequencies): rt_device.h
};

// units per chunk of every host form that goes through device buffers (rt_chunked.h): elements of a list, pixels of a view's whole rows
#define RT_RAY_CHUNK (1u << 18)

namespace rt_api {
constexpr size_t RT_KNOWN_WORDS = 256;
inline uint8_t *cam_block(const rt_scene_dev *s) { return s->d_cam_buf[s->cam_gen & 1u]; }
inline uint8_t *obj_block(const rt_scene_dev *s) { return s->d_obj_buf[s->cam_gen & 1u]; }
inline uint8_t *lds_image_of(const rt_scene_dev *s) { return s->cull_in_lds ? cam_block(s) + s->cam_lds_offset : obj_block(s) + s->o_img; }
inline int scene_stream(const rt_scene_dev *s, void *hip_stream, hipStream_t *stream) { return device_stream(s->device, hip_stream, stream); }

// rt_api.hip
int check_sphere(const rt_sphere &o, uint32_t i, uint32_t n_textures);

// rt_scene.hip: the launch decisions of a resident scene, its launch tables
int enter_launch(rt_scene_dev *s, hipStream_t stream);
bool strict_scene(const rt_scene_dev *s);
bool sky_fast(const rt_scene_dev *s);
bool masks_pay(const rt_scene_dev *s, uint32_t uses_before);
uint32_t sky_part_of(uint32_t flags);
struct table_choice { int ranked; bool mark_sky, shadow_masks, name_candidates; int checker_cells; bool first_bounce; int second_node; };      // checker_cells: 0 none, 1 whole cells, 2 and single axes; first_bounce: first-bounce sets, second_node: 1 and what the node after the primary may skip; 2 (the HOST probe's host-built table only, never a launch's) and its shadow bits (rt_block.h)
table_choice choose_table(const rt_scene_dev *s, uint32_t flags, uint32_t uses_before);
uint32_t count_use(rt_scene_dev *s, const frame_kind &kind);
volatile unsigned long long *known_word(rt_scene_dev *s, size_t index);
uint32_t known_value(const volatile unsigned long long *p, uint64_t gen);
int dispatch_order(rt_scene_dev *s, const frame_kind &kind, const table_choice &c, hipStream_t stream);

// rt_launch.hip: argument checks of the hit entry points
int hits_frame_check(uint32_t w, uint32_t h, uint32_t k, const char *what);
int pick_points_check(uint32_t w, uint32_t h, uint32_t k, uint32_t n, const uint32_t *xy, const void *out, const char *what);
// ... those of the ray entry points; the launch of rays [base, base + n) of a caller's list (device pointers to THOSE rays and their outputs),
// in the list's order (d_order NULL) or in the order of n entries; the ordering of n rays (rt_rays_order.hip) with its argument check
int rays_check(uint64_t n, const double *rays, uint32_t segs, const rt_ray_outputs *out, const char *what);
int rays_order_check(uint64_t n, const double *rays, const uint32_t *order, const void *work, size_t work_bytes, const char *what);
int trace_rays_launch(rt_scene_dev *s, uint32_t n, uint32_t base, const double *d_rays, const uint32_t *d_order, uint32_t segs, const rt_ray_outputs &out,
                      hipStream_t stream, rt_stats *stats);
int order_rays_launch(uint32_t n, const double *d_rays, uint32_t *d_order, void *d_work, hipStream_t stream);
// ... and of the occlusion entry points (`in` may be NULL); the launch of n segments (device pointers), in the list's order or a given one
int occlusion_check(uint64_t n, const double *rays, const rt_occlusion_inputs *in, const rt_occlusion_outputs *out, const char *what);
int occlusion_launch(rt_scene_dev *s, uint32_t n, const double *d_rays, const uint32_t *d_order, const rt_occlusion_inputs &in,
                     const rt_occlusion_outputs &out, hipStream_t stream, rt_stats *stats);

// rt_nodes_api.hip: the wavefront form's argument checks and launches (device pointers): one level of nodes for rays [base, base + n) of
// a caller's list, the next level's ray list, and the fold of a level
int shade_check(uint64_t n, const double *rays, const uint32_t *order, const uint32_t *pix, const uint32_t *path, const rt_node *nodes, const char *what);
int shade_launch(rt_scene_dev *s, uint32_t n, uint32_t base, const double *d_rays, const uint32_t *d_order, const uint32_t *d_pix, const uint32_t *d_path,
                 rt_node *d_nodes, hipStream_t stream, rt_stats *stats);
int spawn_launch(uint32_t n, uint32_t base, const rt_node *d_nodes, const uint32_t *d_pix, const uint32_t *d_path, double *d_child_rays, uint32_t *d_child_pix,
                 uint32_t *d_child_path, int32_t *d_links, uint32_t *d_count, void *d_work, hipStream_t stream);
int fold_launch(uint32_t n, const rt_node *d_nodes, const int32_t *d_links, const double *d_child_rgb, double *d_rgb, uint8_t *d_rgba, hipStream_t stream);

// rt_ambient_api.hip: the number of receivers of a device list (ambient occlusion, sampled lights)
int receiver_count_check(uint64_t n, const char *what);
// rt_lighting_api.hip: the checks of a lighting description whose table is DEVICE memory (NULL only at light_radius 0), and the table of a
// host form going up (nothing is allocated at light_radius 0)
int lighting_device_check(const struct rt_lighting *a, const double *d_offs, const char *what);
int lighting_upload_offs(const struct rt_lighting &a, const double *offs, device_mem *d_offs, hipStream_t stream);
// rt_relight_api.hip: the relight of a level's nodes (device pointers; a.base as given): argument check and launch
int relight_check(const struct rt_lighting *a, const double *d_offs, uint64_t n, const double *rays, const uint32_t *order, const uint32_t *pix,
                  const rt_node *nodes, const char *what);
int relight_launch(rt_scene_dev *s, const struct rt_lighting &a, const double *d_offs, uint32_t n, const double *d_rays, const uint32_t *d_order,
                   const uint32_t *d_pix, rt_node *d_nodes, hipStream_t stream, rt_stats *stats);

// rt_frame.hip: what scene_for does with a blob that differs from the resident one: per texture whose texels differ the smallest row
// range that covers the differences, in texture order.  -1: the blobs differ in something no edit of a resident scene reaches (anything
// outside the camera, light intensity and stars seed of the header, the sphere and light tables and the textures' texels: a
// descriptor, the padding between two textures).  `a` is a blob rt_scene_validate has accepted, `b` any `bytes` bytes.
struct texel_edit { uint32_t texture, first_row, rows; };
int texel_edits(const uint8_t *a, const uint8_t *b, size_t bytes, std::vector<texel_edit> *out);
// rt_frame.hip: RCCL's communicators are destroyed (rt_shutdown)
void release_rccl();

// rt_frame.hip: the prologue and epilogue of a host form, behind its argument checks.  begin: rt_init has run, G.mu is held until the
// call object goes, the clock runs, the blob is device 0's resident scene `s` (scene_for: rt_render's resident one, edited where the
// blob differs only in what an edit reaches, else a fresh upload), and device 0 is current with its stream `stream`.
// end: *stats (if any) = {kernel_ms, pixels, total_ms since begin}, every other field zero.
struct host_call {
  std::unique_lock<std::mutex> lock;
  std::chrono::steady_clock::time_point t_begin;
  rt_scene_dev *s = nullptr;
  hipStream_t stream = nullptr;
  int begin(const void *blob, size_t bytes);
  void end(rt_stats *stats, double kernel_ms, uint64_t pixels) const;
};

// launches on `stream` between the two events of a clock: *st (if any) = {their GPU time, pixels, the host's time}
template <typename Launches> int timed(hipStream_t stream, rt_stats *st, uint64_t pixels, Launches launches) {
  stats_clock clock;
  if (int rc = clock.start(st, stream)) return rc;
  if (int rc = launches()) return rc;
  return clock.finish(st, pixels);
}

// A binned chunk (rt_rays_order.hip): the two SCRATCH rows of a call over n elements - the chunk's order and the ordering's workspace;
// none when not binned - and the step: the timed ordering of m rays into d_order (NULL: not binned), then launch(d_order, st), whose
// GPU time the ordering's is added to.
inline void order_rows(bool binned, uint64_t n, chunk_row out[2]) {
  out[0] = row_scratch(binned ? sizeof(uint32_t) : 0u);
  out[1] = row_scratch(0u, binned ? rt_rays_order_work_bytes(units_per_chunk(n, RT_RAY_CHUNK)) : 0u);
}
template <typename Launch>
int ordered_step(uint32_t m, const double *d_rays, void *d_order, void *d_work, hipStream_t stream, rt_stats *st, Launch launch) {
  double order_ms = 0.0;
  if (d_order) {
    stats_clock clock;
    if (int rc = clock.start(st, stream)) return rc;
    if (int rc = order_rays_launch(m, d_rays, (uint32_t *)d_order, d_work, stream)) return rc;
    if (int rc = clock.finish(st, m)) return rc;
    if (st) order_ms = st->kernel_ms;
  }
  if (int rc = launch((const uint32_t *)d_order, st)) return rc;
  if (st) st->kernel_ms += order_ms;
  return RT_OK;
}

// A list's host form: the chunk driver with unit = element, so element i of the list keeps pix = i (the chunk's base travels to the
// launch).  `list`: the list's arrays, first the one a binned call orders (the ray records).  launch(m, base, d_rows, d_order, st):
// elements [base, base + m), in the list's order (d_order NULL) or in that of m entries; kernel_ms is the sum over the chunks, the
// orderings included.  Behind call.begin; ends the call.
template <typename Launch>
int chunked_list_call(const host_call &call, uint64_t n, const chunk_row *list, int n_rows, bool binned, rt_stats *stats, Launch launch) {
  chunk_row rows[RT_CHUNK_ROWS];
  if (n_rows + 2 > RT_CHUNK_ROWS) return fail(RT_ERR_INVALID, "a list call has at most %d arrays", RT_CHUNK_ROWS - 2);
  for (int i = 0; i < n_rows; i++) rows[i] = list[i];
  order_rows(binned, n, rows + n_rows);
  double kernel_ms = 0.0;
  const int rc = chunked_call(call.stream, n, RT_RAY_CHUNK, rows, n_rows + 2, stats ? &kernel_ms : nullptr,
                              [&](uint64_t base, uint64_t m, void *const *d, rt_stats *st) {
                                return ordered_step((uint32_t)m, (const double *)d[0], d[n_rows], d[n_rows + 1], call.stream, st,
                                                    [&](const uint32_t *d_order, rt_stats *st2) { return launch((uint32_t)m, base, d, d_order, st2); });
                              });
  if (rc) return rc;
  call.end(stats, kernel_ms, n);
  return RT_OK;
}

// ---- views (rt_views_api.hip), for every unit that traces one: the size a view may have; the workspace of a device entry point, which
// holds whole rows of pixel_bytes per pixel (`noun`: what a row is one of, in the entry point's own words) -> *band_rows, the rows of a
// band; the panorama's tables of a host form going up (n_tables of them back to back; nothing for another model) -> *dv, the view with
// device pointers, whose memory is `mem`'s; and the first half of a band of receivers: the rays of rows [y, y + m) into d_rays and their
// hit records into d_hits
bool view_size_ok(uint32_t w, uint32_t h);
int view_work_check(const void *d_work, size_t work_bytes, uint32_t w, uint32_t h, uint32_t pixel_bytes, const char *noun, const char *what, uint32_t *band_rows);
int view_upload_tables(const rt_view &v, uint32_t w, uint32_t h, uint32_t n_tables, hipStream_t stream, device_bufs<2> *mem, rt_view *dv);
int view_band_hits(rt_scene_dev *s, const rt_view *v, uint32_t w, uint32_t h, uint32_t y, uint32_t m, double *d_rays, rt_hit *d_hits, hipStream_t stream);
// rows [row0, row_end) in bands of at most band_rows: fn(y, m) -> an error code
template <typename Band> int for_bands(uint32_t row0, uint32_t row_end, uint32_t band_rows, Band fn) {
  for (uint32_t y = row0; y < row_end; y += band_rows)
    if (int rc = fn(y, row_end - y < band_rows ? row_end - y : band_rows)) return rc;
  return RT_OK;
}
// A view's host form: the chunk driver with unit = one row of w pixels (a row's `each`: w x its bytes per pixel).  bands(y, m, d_rows):
// the launches of rows [y, y + m), timed as one stretch.  Behind call.begin; ends the call.
template <typename Bands>
int chunked_view_call(const host_call &call, uint32_t w, uint32_t h, const chunk_row *rows, int n_rows, rt_stats *stats, Bands bands) {
  double kernel_ms = 0.0;
  const int rc = chunked_call(call.stream, h, rows_per_chunk(RT_RAY_CHUNK, w, h), rows, n_rows, stats ? &kernel_ms : nullptr,
                              [&](uint64_t y, uint64_t m, void *const *d, rt_stats *st) {
                                return timed(call.stream, st, m * w, [&] { return bands((uint32_t)y, (uint32_t)m, d); });
                              });
  if (rc) return rc;
  call.end(stats, kernel_ms, (uint64_t)w * h);
  return RT_OK;
}
}  // namespace rt_api

struct rt_gather_launch;     // (rt_gather.h)

namespace rt_api {
// ---- gathered light (rt_gather_api.hip), for the probe call (rt_probe_api.hip), which takes the same description and whose kernel reads
// the same launch record: the description's fields (and a table in HOST memory), the bound on n and pix, the record of one launch, and
// receivers [at, at + m) of a list or a view as one launch's - both indices advance with the piece
int gather_check(const struct rt_gather *a, const char *what);
int gather_table_check(const struct rt_gather *a, const double *dirs, const char *what);
int gather_count_check(const struct rt_gather &a, uint64_t n, const char *what);
int gather_record(rt_scene_dev *s, const struct rt_gather &a, const double *d_dirs, uint32_t n, const rt_hit *d_hits, const uint32_t *d_order, double *rgb,
                  uint32_t *rgba, hipStream_t stream, struct rt_gather_launch *out);
inline struct rt_gather gather_piece_of(const struct rt_gather &a, uint64_t at) {
  struct rt_gather p = a;
  p.base = a.base + at;
  p.pix_base = a.pix_base + (uint32_t)at;                          // (at + m <= n, and pix_base + ... + n <= 2^31 was checked)
  return p;
}
}  // namespace rt_api

#endif
