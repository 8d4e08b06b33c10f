/*
 * rt_hip.h — C ABI of the MI355X ray-sphere trace/shade path.
 *
 * This is the drop-in boundary for ONE path of termuxinator/html5-canvas-raytracer:
 * the per-pixel loop of main.js (primary-ray generation :184-193, intersectWorld
 * :220-337, intersectSphere :420-451, samplers :126-133/:343-351/:404, RGBA8 store
 * :195-198).  The reference has no FFI of its own; the entry points
 * below are what a Node N-API / Python ctypes binding for that path binds to.  Each
 * comment names the reference construct the entry point or field replaces.
 *
 * Plain C types only.  No torch, no C++ across the ABI.  All functions return 0 on
 * success and a negative rt_status on failure; rt_last_error() describes the failure
 * of the calling thread's last call.
 *
 * Threads: rt_init, rt_shutdown and rt_render serialise on an internal lock.  The device entry points
 * (rt_scene_upload, rt_render_tiles_device, rt_render_batch_device, rt_scene_trace_rays_device, rt_scene_order_rays_device, rt_scene_occlusion_device, rt_scene_ambient_device, rt_scene_ambient_view_device, rt_scene_gather_device, rt_scene_gather_view_device, rt_scene_shade_rays_device, rt_scene_spawn_rays_device, rt_scene_fold_nodes_device, rt_deinterleave_*) may be called from several
 * threads at once; work on one HIP stream is ordered by the stream.  Launches with RT_FLAG_COUNT share one counter
 * buffer per device: one at a time per device.
 *
 * The scene crosses the boundary as ONE contiguous, pointer-free blob
 * (rt_scene_header followed by the tables it gives offsets to), so any host language
 * can build it with typed arrays and the library can upload it with one copy.
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 2u
#define RT_SCENE_MAGIC 0x31535452u /* "RTS1" little endian */
/* `const build = '741'` (main.js:3): the reference build whose per-pixel path this library reproduces, and this library's own
 * revision of it; rt_build_id() returns "<reference build>.<revision>". */
#define RT_REFERENCE_BUILD "741"
#define RT_LIBRARY_REVISION "r4"

#define RT_MAX_OBJECTS  256u
#define RT_MAX_LIGHTS   16u
#define RT_MAX_TEXTURES 16u
#define RT_MAX_SEGS     16u

typedef enum rt_status {
  RT_OK = 0,
  RT_ERR_INVALID = -1,     /* malformed scene blob / bad argument */
  RT_ERR_UNSUPPORTED = -2, /* e.g. an unknown sampler kind */
  RT_ERR_DEVICE = -3,      /* HIP / RCCL failure, or no GPU */
  RT_ERR_NOMEM = -4,
  RT_ERR_STATE = -5        /* rt_init not called, bad handle */
} rt_status;

/* mtl.sampler closures of the reference, enumerated */
enum {
  RT_SAMPLER_COLOR = 0,   /* main.js:404       constant mtl.color                 */
  RT_SAMPLER_TEXTURE = 1, /* main.js:143-145   sampleTexture(tex, hit.u, hit.v)   */
  RT_SAMPLER_CHECKER = 2, /* main.js:126-133   sphere checker on its own u,v      */
  RT_SAMPLER_STARS = 3    /* main.js:135-139   night stars, with Math.random() replaced by a counter-based hash of
                           *                    (sample index in the frame, position in the ray tree, seed): deterministic, the same
                           *                    on every implementation here, NOT comparable with the (random) reference.
                           *                    checker_freq[0] = threshold (0.001), checker_freq[1] = scale (1000).
                           *                    With pix = sample y * sample-grid width + sample x (64 bits; pix_lo, pix_hi its
                           *                    words), path = the node's place in the ray tree (root 1, reflect child 2p, refract
                           *                    child 2p + 1) and seed = rt_scene_header.stars_seed (+ frame, RT_FLAG_STARS_PER_FRAME):
                           *                      mix = lowbias32(seed)                        (lowbias32(0) == 0)
                           *                      u   = lowbias32(pix_lo ^ lowbias32(path + 0x9e3779b9 * ((pix_hi ^ mix) + 1))) / 2^32
                           *                    (32-bit unsigned arithmetic; lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15;
                           *                    x *= 0x846ca68b; x ^= x >> 16), and the sample's grey is u * scale where u < threshold,
                           *                    else 0.  Seed 0 is the hash of ABI 2 before the seed existed, bit for bit.  The
                           *                    reference draws a new sky per redraw (main.js:180); a new seed per frame does that. */
};

/* One sphere + its material: createSphere (main.js:408-418) + createMaterial (:397-406).
 * 24 doubles = 192 bytes. */
typedef struct rt_sphere {
  double origin[3];           /* obj.origin            main.js:411 */
  double r2;                  /* obj.r2                main.js:413 */
  double color[3];            /* mtl.color             main.js:399 */
  double specular_exponent;   /* mtl.specular_exponent main.js:401 */
  double albedo[5];           /* ambient,diffuse,specular,reflect,refract  main.js:400 */
  double refract_index;       /* mtl.refract_index     main.js:402 */
  double checker_freq[2];     /* the literals 5000, 2500 of main.js:129-130 */
  double checker_color[2][3]; /* the table of main.js:131 */
  int32_t sampler_kind;       /* RT_SAMPLER_* */
  int32_t texture;            /* index into the texture table for RT_SAMPLER_TEXTURE, else -1 */
  double reserved;
} rt_sphere;

/* createTexture (main.js:339-341); texels are RGBA8 rows, top row first (getImageData layout, :388-391) */
typedef struct rt_texture_desc {
  uint32_t width;
  uint32_t height;
  uint64_t texels_offset; /* bytes from blob start to width*height*4 bytes */
} rt_texture_desc;

typedef struct rt_scene_header {
  uint32_t magic;          /* RT_SCENE_MAGIC */
  uint32_t abi_version;    /* RT_ABI_VERSION */
  uint64_t total_bytes;    /* size of the whole blob */
  double cam_origin[3];    /* origin  main.js:85,93 */
  double cam_axis_x[3];    /* axisX   main.js:86,97 */
  double cam_axis_y[3];    /* axisY   main.js:87,98 */
  double cam_axis_z[3];    /* axisZ   main.js:88,99 */
  double fov_deg;          /* 60      main.js:102 */
  double light_intensity;  /* 50      main.js:284 (shared across lights, quirk q2) */
  double epsilon;          /* 0.001   main.js:430-436,445 */
  double miss_color[3];    /* [1,0,0] main.js:231 */
  uint32_t segs;           /* 8       main.js:194 */
  uint32_t supersample;    /* 1, or k in {2,3,4} = render kw x kh by the reference's rule and box-average every k x k block of RGBA8
                            * samples with (sum + k*k/2) / (k*k), integer division: k = 2 is (a+b+c+d+2)>>2 (cfg5).  Not in the
                            * reference: defined so that the oracle stays "main.js + an integer post-step". */
  uint32_t n_objects;      /* objs.length, already in the reference's sorted order (main.js:159-163) */
  uint32_t n_lights;       /* lights.length main.js:283 */
  uint32_t n_textures;
  uint32_t stars_seed;     /* seed of the stars sampler's hash (RT_SAMPLER_STARS above); any value; 0 = the sky every host drew before
                            * the field existed.  Replaces the per-redraw Math.random() stream of main.js:135-139, 180. */
  uint64_t objects_offset;  /* rt_sphere[n_objects] */
  uint64_t lights_offset;   /* double[3*n_lights] */
  uint64_t textures_offset; /* rt_texture_desc[n_textures] */
} rt_scene_header;

/* Which rows of the w x h frame a call renders, as row tiles dealt round-robin:
 * tile t (t = tile_first + i*tile_stride, i in [0,n_tiles)) covers frame rows
 * [t*tile_rows, min(h,(t+1)*tile_rows)) and is stored at out + i*tile_rows*w*4.
 * The whole frame is {tile_rows=h, tile_first=0, tile_stride=1, n_tiles=1}.
 * Replaces the scanline scheduler spanish(y) (main.js:183-201). */
typedef struct rt_tiles {
  uint32_t tile_rows;
  uint32_t tile_first;
  uint32_t tile_stride;
  uint32_t n_tiles;
} rt_tiles;

/* Per-render counters and timings; counters are filled only when RT_FLAG_COUNT is set
 * (they come from an instrumented kernel variant, never from the timed one). */
typedef struct rt_stats {
  double kernel_ms;        /* hipEvent time of the trace kernel(s) on the render stream */
  double total_ms;         /* host wall time of the call */
  uint64_t pixels;         /* output pixels written */
  uint64_t rays;           /* intersectWorld invocations with segs>0 (main.js:220-221) */
  uint64_t shadow_rays;    /* lights tested for occlusion (main.js:293-304) */
  uint64_t sphere_tests;   /* intersectSphere calls (main.js:228,296) */
  uint64_t exact_samples;  /* samples the product kernel traced a second time with the reference's own operation sequence:
                            * a sampler coordinate on a texel / checker boundary (main.js:129-130, 344-347) up to rounding, or the
                            * centre row / column of an odd sample grid (main.js:186: x - w/2 + 0.5 == 0).  Every stats call. */
} rt_stats;

enum {
  RT_FLAG_NONE = 0,
  RT_FLAG_COUNT = 1,        /* run the counting variant and fill rays/shadow_rays/sphere_tests */
  RT_FLAG_STRICT_FP = 2,    /* no FMA contraction: operation-for-operation with the JS expression trees */
  RT_FLAG_RGB24 = 4,        /* device entry points only: store 3 bytes per pixel (R,G,B, rows packed, w*3 bytes each)
                             * instead of RGBA8.  The alpha byte is the constant 255 in the reference (main.js:198),
                             * so a band that is about to cross an xGMI link does not carry it; the receiving side
                             * restores it with rt_deinterleave_rgb24_device.  Needs w % 4 == 0. */
  RT_FLAG_NO_SKY = 8,       /* device entry points: blocks of 32 x 8 pixels in which nothing but a constant background can show (the
                             * reference's skybox with a plain colour, or the miss colour of main.js:231 - half of the headline frame) are
                             * NOT stored.  For a frame assembled from several GPUs' tiles in ONE buffer (rt_render_scatter_device into the
                             * owner's frame over xGMI): the senders leave the sky out ... */
  RT_FLAG_SKY_ONLY = 16,    /* ... and the frame's owner stores exactly those blocks, of whatever tiles the call names (the whole frame),
                             * from its own table: the two kinds of call together store every pixel once, and about half of the
                             * headline's pixels never cross a link.  Scenes without a constant background: RT_FLAG_NO_SKY leaves nothing
                             * out and RT_FLAG_SKY_ONLY stores nothing.  Not with RT_FLAG_COUNT. */
  RT_FLAG_COMPACT = 32,     /* rt_render_batch_device with RT_FLAG_RGB24 | RT_FLAG_NO_SKY: a COMPACT band for a collective - the blocks that
                             * are stored at all (everything but the sky) back to back, block b of the launch (32 pixels x 8 rows, x 2
                             * rows with supersample 2; RGB24, row by row: 768 / 192 bytes) at d_out + b * block_bytes, dearest block
                             * first.  rt_compact_count says how many there are; the receiver, which holds the same scene with the same
                             * camera, puts them back with rt_compact_expand_device and fills the sky itself (RT_FLAG_SKY_ONLY).  Not
                             * for scenes the strict kernel renders (RT_ERR_UNSUPPORTED: send plain bands), not with RT_FLAG_COUNT. */
  RT_FLAG_STARS_PER_FRAME = 64  /* rt_render_batch_device / rt_render_scatter_device: frame f of the batch draws its stars with seed
                                 * stars_seed + f (mod 2^32) - N different night skies, as N redraws of the reference give.  Without it
                                 * every frame of a batch is the same picture.  A no-op for one frame. */
};

typedef struct rt_scene_dev rt_scene_dev; /* opaque: a scene resident in one GPU's HBM */

/* Library lifetime.  rt_init(max_devices): use up to max_devices GPUs (0 = all visible). */
int rt_init(int max_devices);
void rt_shutdown(void);
int rt_device_count(void);            /* GPUs in use after rt_init, or a negative rt_status */
const char *rt_last_error(void);
uint32_t rt_abi_version(void);
const char *rt_build_id(void);        /* RT_REFERENCE_BUILD "." RT_LIBRARY_REVISION, e.g. "741.r4" (main.js:3) */

/* Validate a scene blob without touching a GPU (host logic; usable in CPU-only tests). */
int rt_scene_validate(const void *scene_blob, size_t blob_bytes);

/* Host-logic probe (no GPU): the conservative screen rectangle the product kernel uses to cull spheres for
 * primary rays, per sphere in scene order: {x_lo, x_hi, y_lo, y_hi} bounding X/D and Y/D of every pixel whose
 * line meets the sphere (X = x - w/2 + 0.5, Y = h/2 - y - 0.5, D = (w/2)/tan(fov/2); +-inf = unbounded). */
int rt_scene_cull_rects(const void *scene_blob, size_t blob_bytes, double *out_4n);

/* Host-logic probe (no GPU): the candidate set the product kernel's bounce table gives a reflected / refracted ray
 * that starts on sphere `from` (scene order) with direction `dir`: bit j of out_words (ceil(n_objects/64) words) is
 * set if sphere j is tested.  Conservative by construction: every sphere such a ray can meet is in the set. */
int rt_scene_bounce_candidates(const void *scene_blob, size_t blob_bytes, uint32_t from, const double dir[3], uint64_t *out_words);

/* Host-logic probe (no GPU): the launch table of the product kernel for `tiles` of the w x h frame (scene supersample 1 or 2), as
 * the HOST builds it; the library builds the same table on the GPU (same per-block source), per camera, frame size and tile set.
 * The kernel runs on a flat grid; workgroup b renders the 32-pixel-wide, 8-row (2 with supersample 2) block described by its
 * 16-byte entry {tile_x | rows_valid << 11 | first frame row << 15, first row in this call's output band | (run - 1) << 24 |
 * sky << 31, shadow masks, primary candidates}, stored in slot (b % 8) * ceil(blocks / 8) + b / 8.  `ranked` is a bit set:
 *   1  the blocks are listed dearest first (a cost estimate from the spheres' screen rectangles), which is the order the
 *      hardware then hands them out in;
 *   2  blocks none of whose primary rays can meet a sphere are marked (sky = 1) and consecutive ones of a row block share one
 *      entry (a run of blocks that does not cross a multiple of 32 blocks), as the launch of a scene with a constant background
 *      does: their workgroup stores the background;
 *   4  word 2 = per light (16 bits each) the loop-order spheres that can shadow a primary hit of the block at all (scenes of at
 *      most 16 loop spheres and 2 lights; 0xffffffff = no statement), word 3 = the at most two spheres the block can show.
 * out_entries: 32 * ceil(blocks / 8) words, or NULL to ask for *n_workgroups (the number of entries) and *n_blocks only. */
int rt_scene_launch_table(const void *scene_blob, size_t blob_bytes, uint32_t w, uint32_t h, const rt_tiles *tiles, int ranked,
                          uint32_t *out_entries, uint32_t *n_workgroups, uint32_t *n_blocks);

/* Upload a scene to `device` (index into the GPUs in use) and keep it resident. */
int rt_scene_upload(int device, const void *scene_blob, size_t blob_bytes, rt_scene_dev **out);
void rt_scene_free(rt_scene_dev *scene);

/* Move the camera of a resident scene (the reference's lookAt(), main.js:92-100: origin and the three axes; the reference
 * recomputes everything on every redraw, main.js:180-201).  Asynchronous: what depends on the camera - one small block of the
 * resident scene and, per frame size in use, the launch table - exists twice (even / odd camera generations); the move copies the
 * new block and rebuilds those tables ON THE GPU on a stream of the library's own, beside the previous camera's frames that are
 * still rendering, and the next render of the scene waits for them by event (no host wait).  A plain loop
 * `rt_scene_set_camera; rt_render_tiles_device; ...` on ONE stream therefore overlaps a frame's table build with its predecessor's
 * trace.  (The one host wait in that loop is bounded: the render that follows a move so closely that the rebuilt table's entry
 * count has not reached the host yet waits for it for at most 0.1 ms + 1 us per 256 blocks - the caller is ahead of the GPU
 * then - and launches for every block instead of every entry if it does not come.)  `hip_stream` is accepted for source compatibility and not used.  Renders of one scene belong on one stream (several
 * work: a move then drains the device first).  Camera moves and renders of ONE scene handle must not be issued concurrently from
 * different threads (renders among themselves may).  A camera that crosses the scene's enclosing sphere (a skybox) is
 * RT_ERR_UNSUPPORTED: upload the scene again. */
int rt_scene_set_camera(rt_scene_dev *scene, const double origin[3], const double axis_x[3], const double axis_y[3], const double axis_z[3],
                        void *hip_stream);

/* Set the stars seed of a resident scene (rt_scene_header.stars_seed; the reference's fresh Math.random() draws per redraw, main.js:180).
 * Host state only: it is copied into each later render's launch parameters - frames already enqueued keep the seed they were launched
 * with, nothing is uploaded and no launch table is rebuilt (a stars sky is never a constant background).  Thread rules as for
 * rt_scene_set_camera.  Any value is valid. */
int rt_scene_set_stars_seed(rt_scene_dev *scene, uint32_t seed);

/* How many workgroups of its trace kernel one compute unit holds at once for a colour launch of this resident scene, by the HIP
 * runtime's count for the kernel's registers and the launch's dynamic LDS (nothing is launched).  four_waves != 0: the first frame
 * from a moved camera, which runs four-wave workgroups.  out_lds_bytes (may be NULL): the launch's dynamic LDS per workgroup.
 * RT_ERR_UNSUPPORTED for supersample 3 / 4 (rendered on the sample grid). */
int rt_scene_trace_occupancy(rt_scene_dev *scene, int four_waves, int *out_workgroups_per_cu, uint32_t *out_lds_bytes);

/* Replace the sphere records [first, first + count) of a resident scene, in blob order (the reference's objects are plain arrays a
 * page may change between redraws, main.js:180-201): every field of a record may change - origin, r2, material, sampler, texture
 * index; n_objects, lights, textures, camera and seed stay.  Blob order stays the semantics (closest hit: strict <, the first wins).
 * Records are checked by rt_scene_validate's rules; a bad record or a range outside [0, n_objects) is RT_ERR_INVALID and leaves the
 * scene as it was.  Records equal to the current ones change nothing.  Asynchronous, like a camera move: what depends on the spheres
 * (records, geometry tables, LDS images, shadow grids, bounce table) exists twice, the move writes the next copy on the library's
 * own stream - the tables of many-sphere scenes are rebuilt ON THE GPU - beside frames still rendering with the old spheres, and
 * the next render of the scene on any stream waits for it by event.  An edit that changes the sphere that encloses everything (a
 * skybox) is RT_ERR_UNSUPPORTED: upload the scene again.  `hip_stream` and thread rules as for rt_scene_set_camera. */
int rt_scene_set_objects(rt_scene_dev *scene, uint32_t first, uint32_t count, const rt_sphere *records, void *hip_stream);

/* Replace the positions of lights [first, first + count) of a resident scene, three doubles per light, in the blob's light order (the
 * reference's lights are a literal array inside intersectWorld, main.js:283, with two more entries commented out: what a page author
 * changes first); n_lights, spheres, textures, camera and seed stay.  Positions are accepted by rt_scene_validate's rules for a
 * blob's light table (any value); a range outside [0, n_lights), or NULL `xyz` with a count, is RT_ERR_INVALID and leaves the scene
 * as it was.  Positions equal to the current ones change nothing.  Asynchronous, like an object move and cheaper: of the object
 * block only the records anchored at the moved lights and those lights' shadow grids depend on them, and the library rewrites just
 * these ON THE GPU on its own stream (the bounce table, the sphere records and the LDS images stay), beside frames still rendering
 * with the old lights - which keep them: lights travel in each launch's parameters - and rebuilds the launch tables in use (their
 * shadow masks); the next render of the scene on any stream (colour, strict, batch, scatter, hits, pick, ray list) waits for it by
 * event.  A light moved exactly onto a sphere's surface makes the scene a strict-kernel scene, as at upload.  A move that changes
 * the sphere that encloses everything (a light carried outside the skybox) is RT_ERR_UNSUPPORTED and leaves the scene as it was:
 * upload the scene again.  `hip_stream` and thread rules as for rt_scene_set_camera. */
int rt_scene_set_lights(rt_scene_dev *scene, uint32_t first, uint32_t count, const double *xyz, void *hip_stream);

/* Set the light intensity of a resident scene (rt_scene_header.light_intensity; the reference's one intensity shared by all lights,
 * "common (for now)", main.js:284).  Host state only, like the stars seed: it is copied into each later render's launch parameters -
 * frames already enqueued keep theirs, nothing is uploaded, and no table, launch decision or mark count depends on it.  Thread
 * rules as for rt_scene_set_camera.  Any value is valid, as in a blob. */
int rt_scene_set_light_intensity(rt_scene_dev *scene, double light_intensity);

/* Replace texels of one texture of a resident scene (the reference's textures are ImageData, createTexture / loadTexture,
 * main.js:339-395, which a page may draw into between two redraws; sampled one texel at a time, main.js:343-351): the rectangle
 * [x, x + w) x [y, y + h) of texture `texture` takes h source rows of w RGBA8 texels, top row first.  Source row j starts at
 * rgba + j * pitch_bytes; pitch_bytes 0 means 4 * w.  All four bytes of a texel are stored as given (the samplers never read alpha).
 * Widths, heights, descriptors, n_textures and everything else of the scene stay: a texture of another size is an upload.
 * ORDER is the contract: a launch of this scene issued before the call - colour, strict, batch, scatter, hits, pick, ray list,
 * occlusion, shade, on any stream, in the order the API was called - reads the old texels in full, a launch issued after it the new
 * ones in full, and nothing waits on the host.  Unlike the other edits this one USES `hip_stream` (NULL = the library's stream for the
 * scene's device): the write is enqueued there.  Launches of the scene in flight on another stream are covered by an event (on
 * several streams: the device is drained first, as for a camera move), and later launches on other streams wait for the write by
 * event, as they wait for a move.  Only stream and event order at kernel boundaries is relied on.  Texels need no generation: they
 * live once in the resident scene, and no table, launch decision or mark count depends on a texel's value.
 * rt_scene_set_texels: `rgba` is HOST memory (any alignment), free to be reused as soon as the call returns: the rows are staged in
 * pinned memory of the scene - 4 MiB, sixteen slots of 256 KiB, allocated by the scene's first host edit - and an edit of more than a
 * slot goes through in pieces of whole rows.  A piece waits on the host only for the slot it needs, i.e. for a piece sixteen pieces
 * before it (of this edit, or - a caller that many edits ahead of the GPU - of an earlier one).
 * rt_scene_set_texels_device: `d_rgba` is DEVICE memory, 4-byte aligned, that does not overlap the texture; the library's kernel
 * rt_texels_blit - one dword per work-item, grid ceil(w / 256) x h - copies it on `hip_stream`, behind whatever produced d_rgba there.
 * The renderer writes RGBA8 rows, top row first, so a frame or an equirectangular panorama traced on the GPU becomes a texture of this
 * or another scene without leaving the GPU: `render probe; rt_scene_set_texels_device; render frame` on one stream holds no runtime
 * copy and no host wait.
 * RT_ERR_INVALID, before a device is touched and with the scene left as it was: a NULL source with w * h > 0; pitch_bytes non-zero
 * and below 4 * w, or no multiple of 4; a device source that is not 4-byte aligned; then RT_ERR_STATE for a NULL scene; then
 * RT_ERR_INVALID for texture >= n_textures and for a rectangle that leaves the texture (computed in 64 bits: x = 2^32 - 1, w = 2 is
 * refused).  w == 0 or h == 0 with the rest valid is RT_OK and changes nothing.  Thread rules as for rt_scene_set_camera. */
int rt_scene_set_texels(rt_scene_dev *scene, uint32_t texture, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const void *rgba,
                        size_t pitch_bytes, void *hip_stream);
int rt_scene_set_texels_device(rt_scene_dev *scene, uint32_t texture, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const void *d_rgba,
                               size_t pitch_bytes, void *hip_stream);

/* Render tiles of the w x h frame into DEVICE memory `d_out_rgba` (at least
 * n_tiles*tile_rows*w*4 bytes) on `hip_stream` (a hipStream_t; NULL = the library's own
 * stream for that device).  Asynchronous unless `stats` is non-NULL (then it waits and
 * times).  This is the per-pixel loop main.js:185-199 for those rows. */
int rt_render_tiles_device(rt_scene_dev *scene, uint32_t w, uint32_t h, const rt_tiles *tiles,
                           void *d_out_rgba, void *hip_stream, uint32_t flags, rt_stats *stats);

/* The same for a BATCH of n_frames frames in one launch (grid z = frame): frame f's tiles go to
 * d_out_rgba + f*frame_stride_bytes.  All frames use `scene` and its camera (synthetic batches; a real animation moves the
 * camera per frame and calls rt_render_tiles_device per frame); with RT_FLAG_STARS_PER_FRAME frame f has a sky of its own.  Used by the multi-GPU plan, where a step
 * renders this rank's row tiles of N frames and one all-to-all reassembles frame f on rank f. */
int rt_render_batch_device(rt_scene_dev *scene, uint32_t w, uint32_t h, const rt_tiles *tiles, uint32_t n_frames,
                           void *d_out_rgba, uint64_t frame_stride_bytes, void *hip_stream, uint32_t flags, rt_stats *stats);

/* The same batch with one destination PER FRAME: frame f's tiles are written into d_frames[f], a whole w x h RGBA8
 * frame buffer, at their rows of the FRAME (not contiguously as a band).  d_frames is a HOST array of n_frames
 * (<= 16) device pointers; they may point into other GPUs' memory (peer-mapped, e.g. opened with rt_ipc_open): on an
 * xGMI node every rank then stores its tiles of frame f straight into the memory of the rank that owns frame f, and
 * no exchange or de-interleave pass is left - only a barrier.  RGBA8 only (no RT_FLAG_RGB24). */
int rt_render_scatter_device(rt_scene_dev *scene, uint32_t w, uint32_t h, const rt_tiles *tiles, uint32_t n_frames,
                             void *const *d_frames, void *hip_stream, uint32_t flags, rt_stats *stats);

/* Sharing a device allocation between the processes of one node (one process per GPU): rt_ipc_export fills a 64-byte
 * handle for memory obtained from rt_alloc_device (the pointer must be the allocation's base); rt_ipc_open maps it in
 * another process for `device` (with peer access over xGMI when it lives on another GPU) and rt_ipc_close unmaps it. */
#define RT_IPC_HANDLE_BYTES 64u
int rt_ipc_export(int device, const void *d_ptr, void *handle_out);
int rt_ipc_open(int device, const void *handle, void **d_ptr_out);
int rt_ipc_close(int device, void *d_ptr);

/* render(width,height,scene): whole frame into HOST memory (any host pointer; memory from rt_alloc_pinned is what the copy engine
 * and the GPU's own stores reach directly).  One GPU: frames of 8 MiB and more are rendered as 4 row bands whose copy-out overlaps
 * the next band's render; into smaller pinned frames the trace kernel stores directly, over PCIe.  Either way the call takes about
 * max(kernel, frame bytes / PCIe rate).  With more than one GPU in use the frame is sharded by interleaved row tiles and put
 * together on GPU 0 (peer stores, or one RCCL gather) before the copy-out.  The scene stays resident between calls: a blob that
 * differs from the previous call's only in the texels of its textures, the camera, stars_seed, sphere records, light positions and /
 * or light_intensity is not uploaded again (the resident scene takes, per texture whose texels differ, the full-width rows of the
 * smallest range that covers the differences, rt_scene_set_texels, then the spheres of the smallest range that covers theirs, rt_scene_set_objects, then
 * the lights of theirs, rt_scene_set_lights, then the intensity, rt_scene_set_light_intensity, then moves its camera,
 * rt_scene_set_camera, and takes the seed, rt_scene_set_stars_seed; an edit any of these refuses with RT_ERR_UNSUPPORTED is uploaded).  Replaces redraw()/spanish() + ImageData (main.js:83,180-201). */
int rt_render(const void *scene_blob, size_t blob_bytes, uint32_t w, uint32_t h,
              uint8_t *out_rgba, uint32_t flags, rt_stats *stats);

/* How the one-GPU rt_render / rt_render_progressive hand the frame over (process-wide; for measurements - the defaults (1, 4) follow
 * profiles/r03_ab_log.md section 4).  direct_stores: 0 never, 1 the kernel stores straight into a pinned caller buffer for frames
 * below 8 MiB, 2 for every pinned caller buffer.  copy_bands (1..64): the bands of the copy-out plan for frames of 8 MiB and more. */
int rt_render_options(int direct_stores, uint32_t copy_bands);

/* The same, delivered progressively: the frame is rendered as n_bands (1..64) row bands and on_band(user, first_row,
 * n_rows) is called - on the calling thread, in row order - as soon as a band's rows are in out_rgba, while later bands
 * are still rendering or crossing PCIe.  This is the reference's row-by-row display (spanish(y) per macrotask,
 * main.js:183-201) with bands for rows.  With several GPUs in use the frame arrives whole (one call).  on_band runs
 * inside the library's render lock: it must not call rt_render / rt_render_progressive itself. */
typedef void (*rt_band_callback)(void *user, uint32_t first_row, uint32_t n_rows);
int rt_render_progressive(const void *scene_blob, size_t blob_bytes, uint32_t w, uint32_t h, uint8_t *out_rgba,
                          uint32_t n_bands, rt_band_callback on_band, void *user, uint32_t flags, rt_stats *stats);

/* The reference's end-of-frame report (main.js:204-205: `'build #' + build + ' (' + elapsed + 'ms)'`, drawn over the canvas with
 * fillText): the same string for a finished render, with elapsed = stats->total_ms rounded to whole milliseconds as Date.now()
 * differences are.  Writes at most cap bytes including the terminator; returns the length the full string needs (snprintf rule),
 * or a negative rt_status. */
int rt_elapsed_report(const rt_stats *stats, char *out, size_t cap);

/* Pinned host framebuffers (the ImageData buffer of main.js:83 becomes one of these). */
void *rt_alloc_pinned(size_t bytes);
void rt_free_pinned(void *p);

/* Device scratch helpers for hosts without their own allocator (the Python/torch host
 * passes torch storage instead and never calls these). */
void *rt_alloc_device(int device, size_t bytes);
void rt_free_device(int device, void *p);
int rt_copy_to_host(int device, void *dst_host, const void *src_device, size_t bytes);
int rt_memset_device(int device, void *dst_device, int byte_value, size_t bytes);   /* synchronous */

/* De-interleave a gathered frame: src holds, for rank g in [0,n_ranks), that rank's tiles
 * (g, g+n_ranks, ...) contiguously with `rank_stride_bytes` between ranks; dst receives the
 * frame in row order.  One HBM->HBM pass on `hip_stream`. */
int rt_deinterleave_device(int device, const void *d_src, void *d_dst, uint32_t w, uint32_t h,
                           uint32_t tile_rows, uint32_t n_ranks, uint64_t rank_stride_bytes,
                           void *hip_stream);

/* The same for bands rendered with RT_FLAG_RGB24: src rows are w*3 bytes, dst is the RGBA8 frame
 * (ImageData.data layout) with the alpha byte set to 255.  Needs w % 4 == 0. */
int rt_deinterleave_rgb24_device(int device, const void *d_src, void *d_dst, uint32_t w, uint32_t h,
                                 uint32_t tile_rows, uint32_t n_ranks, uint64_t rank_stride_bytes,
                                 void *hip_stream);

/* Compact bands (RT_FLAG_COMPACT).  rt_compact_count: for `tiles` of the w x h frame of a resident scene and its current camera, the
 * number of blocks a compact launch stores and the bytes of one block; waits until the launch table behind the answer has been built
 * (one small synchronous read).  The collective then moves n_blocks * block_bytes bytes instead of the band. */
int rt_compact_count(rt_scene_dev *scene, uint32_t w, uint32_t h, const rt_tiles *tiles, void *hip_stream, uint32_t *n_blocks, uint32_t *block_bytes);

/* Put the blocks of a compact band back: `d_compact` holds what a launch with RT_FLAG_COMPACT over `tiles` stored - on this GPU or
 * on another rank that holds the same scene with the same camera -; every pixel of every block goes to its place in the RGBA8 frame
 * `d_frame` (w x h, alpha 255).  The sky blocks are not part of the band: the frame's owner stores them with RT_FLAG_SKY_ONLY. */
int rt_compact_expand_device(rt_scene_dev *scene, uint32_t w, uint32_t h, const rt_tiles *tiles, const void *d_compact, void *d_frame, void *hip_stream);

/* What is under a sample: primary hits.  The reference computes, per ray, the closest sphere and where and how it is met
 * (main.js:216-231, 440-449: hit_i, hit.t, hit.p, hit.n, the inside flag behind hit.l, hit.u / hit.v) and throws it away after
 * shading; these entry points return it - for picking (clicking on the canvas), depth compositing and object-id / normal views.
 *
 * For each sample of the sample grid (k w x k h when the scene supersamples by k, else w x h) the primary ray of main.js:184-193
 * (the reference's operation order, dist indexed by component: quirk q1) and then:
 *   id      the closest hit over the spheres in BLOB order (the host's sorted `objects`, main.js:159-163), strict <, first wins
 *           (main.js:223-231): the reference's hit_i, | inside << 16 with inside = (t0 < eps || t1 < eps) of main.js:445; -1 on a
 *           miss (main.js:231).  (Not the colour kernels' internal loop order, which moves an enclosing sphere last.)
 *   depth   hit.t as binary64; +Infinity on a miss.
 *   normal  hit.n = (hit.p - origin) * (1 / |hit.p - origin|) (quirk q7), as 3 float32 each rounded to nearest from binary64;
 *           0, 0, 0 on a miss.
 *   pick    (single samples, binary64 throughout) object, inside, t, point = hit.p, normal = hit.n, and u, v of main.js:446-447:
 *           atan2(-n[2], -n[0]) / pi / 2 + 0.5 and asin(-n[1]) / (pi / 2) / 2 + 0.5 - two successive divisions each (q6), with
 *           fdlibm's atan2 / asin as the JS engines have them.  A miss: object -1, inside 0, t +Infinity, everything else 0.
 * The arithmetic is the strict one (no FMA contraction; the reference's own discriminant r2 - d2), so t, p and n are the bits
 * of the reference's expressions.  The primary ray is traced whatever the scene's depth (segs). */
typedef struct rt_hit {
  int32_t object;     /* hit_i (blob order), or -1 */
  int32_t inside;     /* 1: the ray starts inside the sphere (main.js:445) */
  double t;
  double point[3];
  double normal[3];
  double u, v;
} rt_hit;             /* 80 bytes */

typedef struct rt_hit_buffers {
  int32_t *id;        /* one per sample, or NULL */
  double *depth;      /* one per sample, or NULL */
  float *normal;      /* three per sample, or NULL */
} rt_hit_buffers;

/* The primary hits of `tiles` (in OUTPUT rows, as rt_render_tiles_device) into DEVICE buffers: tile slot i holds its k*tile_rows
 * sample rows of k*w samples one after another (rows past the frame's last are not written).  Any buffer may be NULL and is then
 * not touched; id and normal must be 4-byte aligned, depth 8-byte aligned.  Uses the scene's CURRENT camera (the latest
 * rt_scene_set_camera).  Stream and thread rules as rt_render_tiles_device: asynchronous on `hip_stream` (NULL = the library's
 * stream for the scene's device) unless `stats` is non-NULL (then it waits and fills kernel_ms, total_ms and pixels). */
int rt_render_hits_device(rt_scene_dev *scene, uint32_t w, uint32_t h, const rt_tiles *tiles,
                          const rt_hit_buffers *d_bufs, void *hip_stream, rt_stats *stats);

/* The hit records of n (1..65536) samples, sample_xy = {x0, y0, x1, y1, ...} in sample-grid coordinates (x < k*w, y < k*h), into
 * the HOST array out[n], with the scene's current camera.  Synchronous. */
int rt_scene_pick(rt_scene_dev *scene, uint32_t w, uint32_t h, uint32_t n, const uint32_t *sample_xy, rt_hit *out);

/* The host forms: rt_render's resident scene (a blob that differs from the resident one only in the camera, stars_seed, sphere
 * records, light positions and / or light_intensity is not uploaded again: the resident scene takes the edits), outputs in HOST memory.  rt_render_hits fills the whole frame's
 * (k*w x k*h samples) non-NULL buffers of host_bufs; rt_pick is rt_scene_pick on that scene.  Both synchronous, on GPU 0. */
int rt_render_hits(const void *scene_blob, size_t blob_bytes, uint32_t w, uint32_t h, const rt_hit_buffers *host_bufs, rt_stats *stats);
int rt_pick(const void *scene_blob, size_t blob_bytes, uint32_t w, uint32_t h, uint32_t n, const uint32_t *sample_xy, rt_hit *out);

/* Adaptive supersampling: k x k samples only where the frame has edges.  `supersample` k renders every pixel k k times; Whitted's own
 * paper supersampled only where neighbouring samples disagree.  For a resident scene whose header supersample is 1, a frame size
 * w x h, a factor k in {2, 3, 4} and a threshold T in 0..256:
 *   base      B is the frame rt_render_tiles_device(scene, w, h, the whole frame, flags) stores: the same launches, the same bytes.
 *   criterion pixel (x, y) is refined iff it has a 4-neighbour (x +- 1, y) or (x, y +- 1) inside the frame whose stored byte differs from
 *             its own by at least T in R, G or B (integers; alpha plays no part).  T = 0 refines every pixel (a 1 x 1 frame's too),
 *             T = 256 none.  The criterion is evaluated entirely on B: no refined pixel is seen by it.
 *   refine    a refined pixel becomes the pixel of the k-supersampled strict frame: its samples (k x + i, k y + j) of the k w x k h sample
 *             grid - the primary ray of main.js:184-193 on that grid, the reference's own operation sequence without FMA contraction,
 *             the scene's own segs, stars drawn with pix = sy * (k w) + sx and the scene's current seed, stored with the rule of
 *             main.js:195-198 - averaged as (sum + k k / 2) / (k k) per channel, alpha 255: the bytes
 *             rt_render_tiles_device(..., RT_FLAG_STRICT_FP) stores for the same scene with header supersample = k.
 *   every other pixel keeps B's bytes.
 * The whole frame only: the criterion looks across rows, so a tile set would change the picture.
 *
 * rt_adaptive_work_bytes: the bytes of DEVICE workspace a w x h frame needs; host arithmetic, no GPU, no rt_init: 16 + 4 w h; 0 for
 * w == 0, h == 0 or a frame the call refuses for every k (a side above 32768). */
size_t rt_adaptive_work_bytes(uint32_t w, uint32_t h);

/* The adaptive frame into d_out_rgba (DEVICE memory, w * h RGBA8, 4-byte aligned).  d_mask (DEVICE, w * h bytes, or NULL) receives 1
 * for a refined pixel and 0 for every other; d_work is work_bytes >= rt_adaptive_work_bytes(w, h) bytes of DEVICE workspace, 4-byte
 * aligned: when the call's work is done its first uint32 holds the number of refined pixels (the words behind it are the list the
 * refine launch walked, x | y << 16 each, in no particular order).  d_out_rgba, d_mask and d_work must not overlap.
 * flags: 0 or RT_FLAG_STRICT_FP, which goes to the base launch.  Three launches follow each other on `hip_stream` (NULL = the library's
 * stream for the scene's device) - the base frame, the criterion, the refined pixels - with no allocation and no host wait between
 * them: asynchronous unless `stats` is non-NULL (then it waits and fills kernel_ms - all three -, total_ms and pixels = w h).  Pending
 * edits of the scene (camera, objects, lights, texels) are waited for by event, as by every other launch; thread rules as
 * rt_render_tiles_device.  The refine kernel keeps a recursion stack in scratch memory: a reservation the device cannot meet is
 * RT_ERR_NOMEM.
 * RT_ERR_INVALID, before a device is touched and with the scene left as it was: k outside 2..4, threshold above 256, w or h 0, k w or
 * k h above 65536, a NULL or misaligned d_out_rgba or d_work, work_bytes too small, flags other than RT_FLAG_STRICT_FP; then
 * RT_ERR_STATE: a NULL scene; then RT_ERR_INVALID: a scene whose header supersample is not 1. */
int rt_render_adaptive_device(rt_scene_dev *scene, uint32_t w, uint32_t h, uint32_t k, uint32_t threshold,
                              void *d_out_rgba, uint8_t *d_mask, void *d_work, size_t work_bytes, void *hip_stream, uint32_t flags, rt_stats *stats);

/* The host form: rt_render's resident scene (a blob that differs from the resident one only in what an edit reaches is not uploaded
 * again, as for rt_render_hits), outputs in HOST memory: out_rgba w * h * 4 bytes, out_mask w * h bytes or NULL, *refined (or NULL)
 * the number of refined pixels.  Synchronous, on GPU 0. */
int rt_render_adaptive(const void *scene_blob, size_t blob_bytes, uint32_t w, uint32_t h, uint32_t k, uint32_t threshold,
                       uint8_t *out_rgba, uint8_t *out_mask, uint32_t flags, rt_stats *stats, uint64_t *refined);

/* Caller-supplied rays.  The reference's unit of work is not the frame but intersectWorld(segs, objs, org, dir) (main.js:216-336), a
 * function of a ray; these entry points are that function for a LIST of rays - other projections (panoramas, cube faces, orthographic,
 * fisheye, stereo), depth of field and jittered sampling with the caller's own pattern, reflection / light probes at any point
 * (inside a glass sphere too), and the colour twin of rt_scene_pick.
 *
 * `rays` is n records of six doubles {org[3], dir[3]} (48 bytes each; the array 16-byte aligned).  Ray i is
 * intersectWorld(segs, objects, org, dir) over the scene's spheres in BLOB order, its lights, light_intensity, epsilon, miss_color and
 * textures.  `dir` is used AS GIVEN: the reference does not normalise inside intersectWorld either (main.js:192 normalises before the
 * call); the hosts offer the reference's normal3D for callers who want it.
 *   segs    1..RT_MAX_SEGS, or 0 = the scene's own depth: intersectWorld's first argument.  The hit record does not depend on it.
 *   rgb     the return value of intersectWorld, binary64, before any store rule.
 *   rgba    255 * rgb through the Uint8ClampedArray store of main.js:195-198 (NaN -> 0, clamp, round half to even), alpha 255.
 *   hits    the ray's first hit, rt_hit exactly as rt_scene_pick fills it: closest hit, strict <, first wins, inside, t, point, normal,
 *           u, v; a miss: object -1, inside 0, t +Infinity, everything else 0.
 * The arithmetic is the strict one everywhere (no FMA contraction, correctly rounded sqrt and division, fdlibm atan2 / asin), for any
 * origin: the scene's camera, its launch tables, RT_FLAG_* and `supersample` play no part.  The resident scene's CURRENT spheres do
 * (rt_scene_set_objects), and so do its lights (rt_scene_set_lights, rt_scene_set_light_intensity) and its stars seed
 * (rt_scene_set_stars_seed).
 * Stars sampler: pix = i (the ray's index in the list, 64 bits), path from the root 1, seed as for a frame.  So the list of a w x h
 * frame's primary rays in row order draws that frame's sky - and, every other sampler being a function of the ray alone, that list
 * gives the RT_FLAG_STRICT_FP frame byte for byte.
 * A ray with a non-finite component (NaN, +-Infinity in any of its six slots) is NOT traced: rgb = NaN x 3, rgba = 0, 0, 0, 255 (what
 * the store rule makes of NaN), hits = the miss record.  (A zero direction is finite and is traced; the reference's arithmetic stays
 * finite for it.)
 * Any output may be NULL and is then not touched; all three NULL is RT_ERR_INVALID, as are n == 0, n >= 2^31, segs > RT_MAX_SEGS and
 * a NULL or misaligned ray pointer (16 bytes; rgb and hits need 8, rgba 4).  Outputs are written for every i < n and nowhere else.
 * One work-item per ray, and the 64 rays of a wave run in lock step: neighbouring rays in the list should be neighbouring rays in
 * space.  These two calls take the list in its own order; for a list that is not coherent - probes at scattered points, collected
 * secondary rays, sampled directions - rt_scene_order_rays_device + rt_scene_trace_rays_ordered_device (rt_trace_rays_binned for host
 * memory) below bin it on the GPU first, with the same results. */
typedef struct rt_ray_outputs {
  double  *rgb;    /* 3 per ray: the return value of intersectWorld, binary64, before any store rule; or NULL */
  uint8_t *rgba;   /* 4 per ray: 255 * rgb through the Uint8ClampedArray store of main.js:195-198, alpha 255; or NULL */
  rt_hit  *hits;   /* the first hit of the ray, the record rt_scene_pick returns; or NULL */
} rt_ray_outputs;

/* Device form: `d_rays` and the buffers `d_out` names are DEVICE memory (d_out itself is a host struct).  Asynchronous on `hip_stream`
 * (NULL = the library's stream for the scene's device) unless `stats` is non-NULL (then it waits and fills kernel_ms, total_ms and
 * pixels = n).  Waits by event for a pending rt_scene_set_objects or rt_scene_set_lights like every other render.  The refracting scenes' kernel keeps its
 * frame stack in scratch memory: a reservation the device cannot meet is RT_ERR_NOMEM.  Thread rules as rt_render_tiles_device. */
int rt_scene_trace_rays_device(rt_scene_dev *scene, uint64_t n, const double *d_rays, uint32_t segs,
                               const rt_ray_outputs *d_out, void *hip_stream, rt_stats *stats);

/* Host form: rt_render's resident scene (a blob that differs from the resident one only in the camera, stars_seed, sphere records,
 * light positions and / or light_intensity is not uploaded again), rays and outputs in HOST memory, synchronous, on GPU 0.  The list is processed in chunks of 2^18
 * rays (ray i keeps pix = i), so the device memory the call allocates does not grow with n. */
int rt_trace_rays(const void *scene_blob, size_t blob_bytes, uint64_t n, const double *rays, uint32_t segs,
                  const rt_ray_outputs *host_out, rt_stats *stats);

/* Binning a ray list.  A wave of 64 unrelated rays walks 64 different ray trees in lock step (a shuffled 3840 x 2160 frame of primary
 * rays costs 4 - 11 times the frame in row order, docs/EVIDENCE.md); these entry points put a list into an order in which the rays
 * of a wave are neighbours, on the GPU, and trace it in that order.  No result depends on the order: every output of ray i is a
 * function of the ray, the scene and i, and is written at index i - a binned trace fills the buffers with exactly the bytes of
 * rt_scene_trace_rays_device.  Binning pays for lists whose neighbours in the list are NOT neighbours in space and whose trace is
 * dear (many spheres, deep trees); a list that is coherent already (a frame in row order), or a scene whose shuffled trace costs
 * about what the ordering does (docs/EVIDENCE.md, "Binned ray lists"), gains nothing.
 *
 * rt_rays_order_work_bytes: the bytes of DEVICE workspace an ordering of n rays needs; host arithmetic, no GPU, no rt_init.  0 for
 * n == 0 and n >= 2^31; non-decreasing in n (about 12 bytes per ray + 1 KiB per 4096 rays). */
size_t rt_rays_order_work_bytes(uint64_t n);

/* Writes into d_order[0..n) (DEVICE memory, 4-byte aligned) a permutation of 0..n-1 in which 64 consecutive entries name rays that are
 * close in origin and direction: the rays sorted by a 32-bit key that interleaves the bits of the origin's cell and of the direction's
 * cell (its place on its cube-map face) inside the list's own bounds, axes the list does not vary in left out - a list that shares
 * one origin is ordered by direction alone, one that shares a direction by origin alone.  Rays with a non-finite component come
 * after all finite ones.  The sort is stable and the key a function of the list: the same list gives the same order on every call.
 * The key reads NOTHING of the scene - `scene` names the device and its default stream, and the call waits for no pending
 * rt_scene_set_objects / rt_scene_set_lights; an order stays valid while the list does, whatever is done to the scene.
 * Asynchronous on `hip_stream` (NULL = the library's stream for the scene's device); no allocation and no host wait: `d_work` is
 * work_bytes >= rt_rays_order_work_bytes(n) bytes of device memory (4-byte aligned) the call may overwrite, and d_order is written
 * more than once on the way.  RT_ERR_INVALID: a NULL pointer, rays not 16-byte aligned, d_order or d_work not 4-byte aligned,
 * work_bytes too small, n outside 1..2^31 - 1; RT_ERR_STATE: a NULL scene; all of them before a device is touched. */
int rt_scene_order_rays_device(rt_scene_dev *scene, uint64_t n, const double *d_rays, uint32_t *d_order, void *d_work, size_t work_bytes,
                               void *hip_stream);

/* rt_scene_trace_rays_device in the order of `d_order` (n entries, DEVICE memory, 4-byte aligned): work-item j traces ray i = d_order[j],
 * reads record i, draws its stars with pix = i and writes its outputs at index i.  For a permutation of 0..n-1 - the library's or
 * the caller's own - the buffers hold exactly what rt_scene_trace_rays_device puts there: rgb bit for bit, rgba, hits.  An entry
 * >= n is skipped: nothing is read or written for it (a ray no entry names keeps what its outputs held; a ray named twice is
 * traced twice, with the same result).  Everything else - validation, non-finite rays, segs, stats, the scratch reservation, waiting for pending
 * edits - is the plain call's; a NULL or misaligned d_order is RT_ERR_INVALID. */
int rt_scene_trace_rays_ordered_device(rt_scene_dev *scene, uint64_t n, const double *d_rays, const uint32_t *d_order, uint32_t segs,
                                       const rt_ray_outputs *d_out, void *hip_stream, rt_stats *stats);

/* Host form: rt_trace_rays with each chunk of 2^18 rays ordered on the GPU before it is traced (chunks are binned one by one, not
 * across each other; ray i keeps pix = i over the whole list).  The order buffer and the workspace are the call's own device memory,
 * like the rest.  stats->kernel_ms includes the orderings.  The same bytes as rt_trace_rays in every output. */
int rt_trace_rays_binned(const void *scene_blob, size_t blob_bytes, uint64_t n, const double *rays, uint32_t segs,
                         const rt_ray_outputs *host_out, rt_stats *stats);

/* Occlusion queries: how much of a light reaches a point.  The other loop of the reference, the shadow scan of main.js:293-304, for a
 * LIST of segments - baked or per-vertex lighting, light probes, "is this point lit" for game logic, shadow and visibility views, a
 * caller's own shading on top of rt_render_hits.  It is not a closest-hit query (the `hits` of a ray list cannot answer it): the scan
 * stops at the first OPAQUE sphere in blob order, leaves one sphere out (the receiver, `j != hit_i`), compares against the light's
 * distance instead of infinity, and divides the intensity by albedo[4] for every transparent sphere it crosses (quirk q2).
 *
 * `rays` is the ray list of rt_scene_trace_rays_device: n records {org[3], dir[3]}, 48 bytes each, 16-byte aligned, `dir` used AS GIVEN
 * (the reference scans along unit(light - hit.p), main.js:287-290; the hosts' lightSegments / light_segments build exactly that).
 * The same list goes through rt_scene_order_rays_device unchanged.  Ray i, in the strict arithmetic (no FMA contraction, correctly
 * rounded sqrt and division):
 *     li = intensity[i]; blocker = -1
 *     for j in blob order, j != skip[i]:
 *       t = intersectSphere(obj j, org, dir, null)          main.js:420-439, the epsilon rule included
 *       if t < length[i]:
 *         if albedo[4] != 0: li = li / albedo[4]            one division per crossed sphere, in blob order
 *         else: li = 0; blocker = j; break
 * A NaN t or a NaN length occludes nothing (the reference's comparison is false).  A ray with a non-finite component in its six slots
 * is NOT traced: intensity NaN, blocker -1; length and intensity may hold any value.  The reference carries ONE intensity from light
 * to light (q2): feed the intensity a point's first light left into the segment to its second (the hosts' light_intensity_at).
 * It reads the scene's CURRENT spheres (rt_scene_set_objects), epsilon and light intensity (rt_scene_set_light_intensity); the camera,
 * launch tables, RT_FLAG_*, textures and the lights' positions play no part - the caller's segments say where the lights are. */
typedef struct rt_occlusion_inputs {   /* each one per ray, or NULL */
  const double  *length;     /* light_len of main.js:288; NULL = +Infinity for every ray */
  const double  *intensity;  /* the light_intensity the scan starts with; NULL = the scene's current one */
  const int32_t *skip;       /* hit_i of main.js:294: the sphere (blob order) left out; NULL or a value outside [0, n_objects) = none */
} rt_occlusion_inputs;
typedef struct rt_occlusion_outputs {  /* any may be NULL; both NULL is RT_ERR_INVALID */
  double  *intensity;        /* light_intensity after the scan */
  int32_t *blocker;          /* the opaque sphere that ended it (blob order), or -1 */
} rt_occlusion_outputs;

/* Device form: `d_rays`, `d_order` and the arrays `d_in` and `d_out` name are DEVICE memory (d_in and d_out themselves are host structs;
 * a NULL d_in means all three inputs are NULL).  d_order is NULL or an order as rt_scene_trace_rays_ordered_device takes it: work-item j
 * takes ray i = d_order[j], an entry >= n is skipped, and ray i reads and writes index i - the buffers hold the bytes of the call
 * without an order.  Outputs are written for every ray an entry names (every i < n without an order) and nowhere else; an output that
 * is NULL is not touched.  Asynchronous on `hip_stream` (NULL = the library's stream for the scene's device) unless `stats` is non-NULL
 * (then it waits and fills kernel_ms, total_ms and pixels = n).  Waits by event for a pending rt_scene_set_objects / rt_scene_set_lights
 * like every other launch.  One work-item per ray; a lane whose ray has met its opaque sphere goes idle and a wave leaves the scan as
 * soon as none of its 64 rays is live, so neighbours in the list should be neighbours in space here too.
 * RT_ERR_INVALID, before a device is touched: n outside 1..2^31 - 1, NULL or misaligned d_rays (16 bytes), a NULL d_out or both of its
 * outputs NULL, a misaligned length or intensity array (8 bytes), skip, blocker or d_order (4 bytes); then RT_ERR_STATE: a NULL scene.
 * Thread rules as rt_render_tiles_device. */
int rt_scene_occlusion_device(rt_scene_dev *scene, uint64_t n, const double *d_rays, const uint32_t *d_order,
                              const rt_occlusion_inputs *d_in, const rt_occlusion_outputs *d_out, void *hip_stream, rt_stats *stats);

/* Host form: rt_render's resident scene (a blob that differs from the resident one only in the camera, stars_seed, sphere records,
 * light positions and / or light_intensity is not uploaded again), every array in HOST memory, the list's own order, synchronous, on
 * GPU 0.  The list is processed in chunks of 2^18 rays, so the device memory the call allocates does not grow with n. */
int rt_occlusion(const void *scene_blob, size_t blob_bytes, uint64_t n, const double *rays,
                 const rt_occlusion_inputs *host_in, const rt_occlusion_outputs *host_out, rt_stats *stats);

/* The same with each chunk of 2^18 rays ordered on the GPU (rt_scene_order_rays_device's ordering) before it is scanned, as
 * rt_trace_rays_binned does; stats->kernel_ms includes the orderings.  The same bytes as rt_occlusion in both outputs. */
int rt_occlusion_binned(const void *scene_blob, size_t blob_bytes, uint64_t n, const double *rays,
                        const rt_occlusion_inputs *host_in, const rt_occlusion_outputs *host_out, rt_stats *stats);

/* Wavefront tracing of ray lists: ONE level of intersectWorld per call.  rt_scene_trace_rays_device runs the reference's recursion
 * (main.js:268-278) inside one kernel; these entry points open it: a node per ray (what intersectWorld computes WITHOUT its two
 * recursive calls), the child rays the nodes spawn as the next level's ray list, and the fold that puts the colours of a level's
 * children back into their parents (main.js:322-336).  A caller can put their own shading on the reference's geometry, look at bounce k
 * alone, keep per-bounce buffers, or bin each level (rt_scene_order_rays_device) before it is shaded.  Shading level 1, spawning,
 * shading again down to `segs` levels (or an empty level) and folding back up gives the rgb of rt_scene_trace_rays_device bit for bit.
 *
 * The arithmetic is the strict one (no FMA contraction, correctly rounded sqrt and division, fdlibm atan2 / asin, the strict build's
 * pow); spheres in blob order, strict <, first wins; the shadow scan is rt_scene_occlusion_device's loop per light with ONE intensity
 * carried from light to light (q2).  It reads the resident scene's current spheres, lights, light_intensity, epsilon, miss_color,
 * textures and stars seed; the camera, launch tables and RT_FLAG_* play no part.
 * A ray with a non-finite component is not traced: the miss record, sample = NaN x 3, children = 0, every other double 0. */
typedef struct rt_node {        /* intersectWorld(segs >= 1, objs, org, dir) WITHOUT its two recursive calls */
  rt_hit  hit;                  /* exactly the record `hits` of rt_scene_trace_rays_device holds for this ray */
  double  sample[3];            /* hit.m.sampler(hit), main.js:320;   a miss: miss_color (main.js:231) */
  double  diffuse, specular;    /* diffuse_intensity, specular_intensity AFTER main.js:316-317; 0 when neither albedo[1] nor [2] > 0, or a miss */
  double  ambient, reflect_weight, refract_weight;   /* albedo[0], albedo[3], albedo[4] of the hit sphere; a miss: 0 */
  double  reflect_dir[3];       /* the direction handed to the first recursive call (main.js:236-238, normalised); 0,0,0 when reflect_len == 0 */
  double  refract_dir[3];       /* the same for main.js:243-265, total internal reflection included */
  uint32_t children;            /* bit 0: reflect_len != 0, bit 1: refract_len != 0 - whatever the depth left */
  uint32_t reserved;            /* 0 */
} rt_node;                      /* 200 bytes; the child rays' origin is hit.point */

/* One level: node i of ray i into d_nodes[i] (DEVICE memory, 8-byte aligned, n records).  d_rays and d_order as for
 * rt_scene_trace_rays_ordered_device (d_order NULL or an order; an entry >= n is skipped and nothing is written for it).  d_pix and
 * d_path (uint32 per ray, 4-byte aligned, or NULL) are the stars sampler's pix and path of ray i; NULL means pix = i and path = 1, so a
 * root list behaves as rt_scene_trace_rays_device does.  Stream, thread, stats and pending-edit rules are rt_scene_occlusion_device's.
 * RT_ERR_INVALID, before a device is touched: n outside 1..2^31 - 1, NULL or misaligned d_rays (16 bytes), NULL or misaligned
 * d_nodes (8 bytes), misaligned d_order, d_pix or d_path (4 bytes); then RT_ERR_STATE: a NULL scene.
 * One work-item per ray; the kernel keeps no stack and uses no scratch memory. */
int rt_scene_shade_rays_device(rt_scene_dev *scene, uint64_t n, const double *d_rays, const uint32_t *d_order, const uint32_t *d_pix,
                               const uint32_t *d_path, rt_node *d_nodes, void *hip_stream, rt_stats *stats);

/* Host form of one level: rt_render's resident scene, every array in HOST memory (pix and path may be NULL: i and 1), the list's own
 * order or (binned != 0) each chunk ordered on the GPU first - the same nodes; synchronous, on GPU 0, in chunks of 2^18 rays like
 * rt_trace_rays (ray i keeps pix = i without d_pix).  host_nodes: n records, 8-byte aligned. */
int rt_shade_rays(const void *scene_blob, size_t blob_bytes, uint64_t n, const double *rays, const uint32_t *pix, const uint32_t *path,
                  int binned, rt_node *host_nodes, rt_stats *stats);

/* The bytes of DEVICE workspace rt_scene_spawn_rays_device needs for n nodes; host arithmetic.  0 for n == 0 and n >= 2^31;
 * non-decreasing in n (4 bytes per 256 nodes). */
size_t rt_nodes_spawn_work_bytes(uint64_t n);

/* Compacts the children of n nodes into the next level's ray list, in a stable order: by parent index, reflect before refract (the
 * reference's recursion order).  Child c: d_child_rays[c] = {hit.point, dir}, d_child_pix[c] = the parent's pix, d_child_path[c] =
 * 2p (reflect) or 2p + 1 (refract) for the parent's path p (d_pix / d_path NULL: i and 1, as above).  Parent i: d_links[2i] and
 * d_links[2i + 1] (int32) = the index of its reflect / refract child in the new list, or -1.  *d_count (a device uint32) = the number
 * of children.  The child buffers hold 2n entries; d_child_pix and d_child_path may be NULL.  No allocation and no host wait: the scan
 * lives in d_work (work_bytes >= rt_nodes_spawn_work_bytes(n), 4-byte aligned).  Reads nothing of the scene: `scene` names the device
 * and its default stream.  RT_ERR_INVALID, before a device is touched: n outside 1..2^31 - 1, a NULL d_nodes, d_child_rays, d_links,
 * d_count or d_work, misaligned pointers (nodes 8, child rays 16, the others 4), work_bytes too small; then RT_ERR_STATE: a NULL scene. */
int rt_scene_spawn_rays_device(rt_scene_dev *scene, uint64_t n, const rt_node *d_nodes, const uint32_t *d_pix, const uint32_t *d_path,
                               double *d_child_rays, uint32_t *d_child_pix, uint32_t *d_child_path, int32_t *d_links, uint32_t *d_count,
                               void *d_work, size_t work_bytes, void *hip_stream);

/* main.js:322-336 for node i: a miss gives rgb = sample; otherwise per channel
 *     max(sample * ambient, min(1, sample * diffuse + sample * specular + re + rf))
 * with re = d_child_rgb[3 * link] * reflect_weight when d_links[2i] >= 0, else +0.0, rf the same through d_links[2i + 1] and
 * refract_weight; the four terms added left to right; Math.min / Math.max with JavaScript's NaN rule.  d_links == NULL marks the
 * deepest level: every child is intersectWorld(0, ...) = [0,0,0].  d_rgb (3 doubles per node, 8-byte aligned) and d_rgba (the store
 * rule of main.js:195-198, alpha 255, 4-byte aligned): either may be NULL, not both.  Reads nothing of the scene.  RT_ERR_INVALID,
 * before a device is touched: n outside 1..2^31 - 1, NULL or misaligned d_nodes, both outputs NULL, d_links without d_child_rgb,
 * misaligned pointers; then RT_ERR_STATE: a NULL scene. */
int rt_scene_fold_nodes_device(rt_scene_dev *scene, uint64_t n, const rt_node *d_nodes, const int32_t *d_links, const double *d_child_rgb,
                               double *d_rgb, uint8_t *d_rgba, void *hip_stream);

/* Host form: rt_trace_rays' rgb and rgba through the wavefront loop, on rt_render's resident scene, synchronous, on GPU 0: level 1 is
 * shaded, its children spawned and shaded, down to `segs` levels (0 = the scene's depth) or an empty level, then the levels are folded
 * back up.  order_levels != 0: every level after the first goes through rt_scene_order_rays_device before it is shaded.  The list is
 * processed in chunks of at most 2^18 rays (ray i keeps pix = i); a level's buffers are sized from the count read back after the
 * spawn that made it, and the nodes of all levels of a chunk together are held to 2^21: a chunk whose trees would exceed that is
 * halved and started again (one ray's tree has at most 2^16 - 1 nodes), so the device memory of a call stays below 2^21 x 400 bytes
 * (node and links of every level, and the transient ray, pix, path, order, child and rgb records of one) = 800 MiB, whatever n.
 * level_counts (uint64[RT_MAX_SEGS], or NULL): the rays shaded at each level, summed over the chunks.  host_out->hits must be NULL.
 * At depth 0 (segs 0 on a scene whose own depth is 0) no level is shaded and nothing is launched: the outputs are rt_trace_rays' all
 * the same ([0,0,0] and 0,0,0,255 per finite ray), level_counts all zero.
 * The bytes are rt_trace_rays' in both outputs, for every list. */
int rt_trace_rays_wavefront(const void *scene_blob, size_t blob_bytes, uint64_t n, const double *rays, uint32_t segs, int order_levels,
                            const rt_ray_outputs *host_out, rt_stats *stats, uint64_t *level_counts);

/* Views: a camera's rays generated on the GPU.  The ray-list calls above render any projection, but the list has to be built on the
 * host and crosses the link at 48 bytes per ray (a 3840 x 2160 view: 398 MB per frame from a moving eye).  A view is the list's
 * description instead - a model, an origin, a basis - and the library generates the list on the device, band by band, in front of
 * the same rt_trace_rays launch.  No trace kernel knows about it.
 *
 * Pixel (x, y) of a w x h view, with X = ((double)x - w / 2.0) + 0.5 and Y = (h / 2.0 - (double)y) - 0.5 (main.js:186), o = origin,
 * ax, ay, az = the axes, per component c, every operation in binary64 without FMA contraction, in the order written:
 *   RT_VIEW_REFERENCE  org = o; main.js:186-193 operation for operation (quirk q1: dist is indexed by COMPONENT): with d = (X, Y, proj_d),
 *                      target[c] = ((o[c] + ax[c] * d[c]) + ay[c] * d[c]) + az[c] * d[c], dir[c] = target[c] - o[c].  A pinhole only
 *                      while the axes are the world's; the strict frame's own rays.
 *   RT_VIEW_PINHOLE    org = o; dir[c] = (ax[c] * X + ay[c] * Y) + az[c] * proj_d.  A true pinhole for any basis.
 *   RT_VIEW_ORTHO      org[c] = (o[c] + ax[c] * (X * scale)) + ay[c] * (Y * scale); dir = az.  `scale` is world units per pixel.
 *   RT_VIEW_EQUIRECT   org = o; with {sl, cl} = lon[2x], lon[2x + 1] and {sa, ca} = lat[2y], lat[2y + 1]: l0 = ca * sl, l1 = sa,
 *                      l2 = ca * cl, dir[c] = (ax[c] * l0 + ay[c] * l1) + az[c] * l2.
 * and dir then goes through the reference's normal3D (multiplied by 1 / |dir|, a zero vector left as it is).  proj_d is
 * (w / 2.0) / tan((fov_deg * M_PI / 180.0) / 2.0), the host's tan, as for a frame.  No transcendental function runs on the device: the
 * panorama's tables hold per column the sine and cosine of lon_x = 2.0 * M_PI * (x + 0.5) / w - M_PI and per row those of
 * lat_y = M_PI / 2.0 - M_PI * (y + 0.5) / h, made once per frame size (rt_view_equirect_tables, or the caller's own).  With axes
 * (1,0,0), (0,1,0), (0,0,-1) the centre of the panorama looks along -z. */
enum { RT_VIEW_REFERENCE = 0, RT_VIEW_PINHOLE = 1, RT_VIEW_ORTHO = 2, RT_VIEW_EQUIRECT = 3 };
typedef struct rt_view {
  uint32_t model, reserved;                 /* reserved = 0 */
  double origin[3], axis_x[3], axis_y[3], axis_z[3];
  double fov_deg;                            /* REFERENCE, PINHOLE: 0 < fov_deg < 180 */
  double scale;                              /* ORTHO: finite, > 0 */
  const double *lon, *lat;                   /* EQUIRECT: 2 w and 2 h doubles {sin, cos}, 16-byte aligned; else ignored */
} rt_view;

/* Host logic, no GPU, no rt_init.  RT_ERR_INVALID: NULL; an unknown model or reserved != 0; w == 0, h == 0 or w * h >= 2^31 (in 64
 * bits); a non-finite origin or axis component; fov_deg outside (0, 180) or NaN for the two perspective models; scale not finite or
 * <= 0 for ORTHO; NULL or misaligned (16 bytes) tables for EQUIRECT.  A zero axis is valid: the arithmetic stays finite for it. */
int rt_view_validate(const rt_view *v, uint32_t w, uint32_t h);

/* Host logic: the panorama's tables for a w x h view, lon_2w[2x], lon_2w[2x + 1] = sin, cos of lon_x and lat_2h[2y], lat_2h[2y + 1] =
 * sin, cos of lat_y (the host's libm).  RT_ERR_INVALID: a NULL pointer, w == 0 or h == 0. */
int rt_view_equirect_tables(uint32_t w, uint32_t h, double *lon_2w, double *lat_2h);

/* Host logic: rows [first_row, first_row + rows) of the view into out (rows * w records of six doubles, row order; the tables in HOST
 * memory).  The restatement the device is held to, bit for bit.  RT_ERR_INVALID: what rt_view_validate refuses, a NULL out,
 * first_row + rows > h; rows == 0 is RT_OK and writes nothing. */
int rt_view_rays(const rt_view *v, uint32_t w, uint32_t h, uint32_t first_row, uint32_t rows, double *out);

/* The same rows into d_rays (DEVICE memory, 16-byte aligned, rows * w * 6 doubles), asynchronous on `hip_stream` (NULL = the
 * library's stream of `device`); for EQUIRECT lon and lat are DEVICE pointers.  It needs no scene and waits for no edit.
 * RT_ERR_INVALID as rt_view_rays, and for a NULL or misaligned d_rays, before a device is touched. */
int rt_view_rays_device(int device, const rt_view *v, uint32_t w, uint32_t h, uint32_t first_row, uint32_t rows,
                        double *d_rays, void *hip_stream);

/* Host arithmetic: the workspace rt_scene_trace_view_device prefers for a w x h view: 48 w h bytes, the whole view in one band (smaller
 * bands measured slower, docs/EVIDENCE.md "Views"; a caller short of memory hands in fewer rows and gets the same bytes).  0 for w == 0, h == 0 or w * h >= 2^31. */
size_t rt_view_work_bytes(uint32_t w, uint32_t h);

/* intersectWorld for every ray of the view, outputs in frame order: ray i = y * w + x.  rgba is the w x h frame in ImageData.data's
 * layout; rgb and hits as for rt_scene_trace_rays_device, and so are segs, every-output-NULL, output alignment, the scratch
 * reservation, stats (kernel_ms covers generation and trace of all bands) and the thread rules.  The view is processed in bands of
 * whole rows: each band is generated into d_work (DEVICE memory, 16-byte aligned, work_bytes >= 48 w: one row is the smallest band)
 * and traced by the rt_trace_rays launch with its base, so ray i keeps pix = i - the stars of a REFERENCE view with the scene's camera
 * and fov are the RT_FLAG_STRICT_FP frame's, and so is every byte - and no result depends on the band size.  The scene's own camera,
 * fov_deg, supersample, launch tables and RT_FLAG_* play no part; its current spheres, lights and stars seed do.  For EQUIRECT lon
 * and lat are DEVICE pointers.  RT_ERR_STATE: a NULL scene; RT_ERR_INVALID: what rt_view_validate refuses, segs > RT_MAX_SEGS, NULL
 * d_out or every output NULL, misaligned outputs, a NULL or misaligned d_work, work_bytes below one row. */
int rt_scene_trace_view_device(rt_scene_dev *scene, const rt_view *v, uint32_t w, uint32_t h, uint32_t segs,
                               const rt_ray_outputs *d_out, void *d_work, size_t work_bytes, void *hip_stream, rt_stats *stats);

/* Host form: rt_render's resident scene (a blob that differs from the resident one only in what an edit reaches is not uploaded
 * again, as for rt_trace_rays), outputs in HOST memory, synchronous, on GPU 0, in chunks of whole rows of at most 2^18 rays (a single
 * row longer than that is its own chunk).  No ray crosses the link; for EQUIRECT lon and lat are HOST memory and the call uploads
 * them once, (w + h) * 16 bytes. */
int rt_trace_view(const void *scene_blob, size_t blob_bytes, const rt_view *v, uint32_t w, uint32_t h, uint32_t segs,
                  const rt_ray_outputs *host_out, rt_stats *stats);

/* Sampled views: n rays per pixel of a view - sub-pixel offsets for antialiasing, points of a thin lens for depth of field, in the
 * caller's own pattern - generated, traced and averaged on the GPU.  Every pixel uses the same n samples (the accumulation-buffer form:
 * each sample is a coherent view).  No trace kernel knows about it: a generator that takes a sample stands in front of the same
 * rt_trace_rays launch, an accumulator in binary64 and a resolve with the reference's store rule behind it.
 *
 * Sample s of pixel (x, y) of a w x h view; every operation in binary64 without FMA contraction, in the order written; proj_w = w / 2.0,
 * proj_h = h / 2.0 and proj_d as for a view:
 *   X = (((double)x - proj_w) + 0.5) + dx,  Y = ((proj_h - (double)y) - 0.5) - dy.  Offsets are in pixels, positive dy is DOWN like y;
 *   any finite value is valid, a pattern normally stays in [-0.5, 0.5].
 *   RT_VIEW_REFERENCE, RT_VIEW_ORTHO   the view's expressions (above) with this X and Y.
 *   RT_VIEW_PINHOLE    raw[c] = (ax[c] * X + ay[c] * Y) + az[c] * proj_d.  Without a lens (NULL or radius == 0): org = o, dir = raw, and
 *                      lu, lv are not read.  With a lens: f = focus / proj_d, lx = lu * radius, ly = lv * radius,
 *                      off[c] = ax[c] * lx + ay[c] * ly, org[c] = o[c] + off[c], dir[c] = raw[c] * f - off[c].  With orthonormal axes
 *                      every sample of a pixel passes through o + raw * f, on the plane at distance `focus` along az.
 *   RT_VIEW_EQUIRECT   no transcendental function runs on the device, as before: the offset lives in the tables.  lon and lat hold one
 *                      table per sample back to back - sample s reads lon + 2 w s and lat + 2 h s - made by
 *                      rt_view_equirect_sample_tables from the angles 2.0 * M_PI * ((x + 0.5) + dx) / w - M_PI and
 *                      M_PI / 2.0 - M_PI * ((y + 0.5) + dy) / h.  dx and dy are not read by the generator.
 * and dir then goes through the reference's normal3D, as for a view.  A lens with radius > 0 is RT_VIEW_PINHOLE only.  With dx = dy = 0
 * and no lens every model's sample ray is the view's ray bit for bit (X and Y are never -0, so adding 0.0 changes nothing).
 *
 * A sampled trace of n samples (1 <= n <= 1024, (uint64)n * w * h <= 2^32): ray i = y * w + x of sample s is intersectWorld(segs, ...)
 * exactly as rt_scene_trace_rays_device traces it, its stars drawn with pix = s * w * h + i - each sample draws its own sky, as each
 * redraw of the reference does.  Per channel acc = rgb_0, then acc = acc + rgb_s for s = 1 .. n - 1 in that order, then
 * mean = acc / (double)n, one correctly rounded division.  rgb receives mean; rgba receives 255 * mean through the store rule of
 * main.js:195-198 with alpha 255.  NaN propagates by IEEE rules and stores as 0.  n = 1 with the zero sample and no lens gives
 * rt_scene_trace_view_device's bytes in rgb and rgba. */
typedef struct rt_view_sample { double dx, dy, lu, lv; } rt_view_sample;   /* 32 bytes: the sub-pixel offset, the lens point on the unit disk */
typedef struct rt_view_lens   { double radius, focus; } rt_view_lens;      /* NULL or radius 0 = no lens */

/* Host logic, no GPU, no rt_init.  RT_ERR_INVALID: everything rt_view_validate refuses; n outside 1..1024 or n * w * h > 2^32 (in 64
 * bits); NULL samples or a non-finite sample component; radius negative or non-finite; radius > 0 with a model other than
 * RT_VIEW_PINHOLE, or with focus not finite or <= 0. */
int rt_view_samples_validate(const rt_view *v, uint32_t w, uint32_t h, const rt_view_lens *lens, uint32_t n, const rt_view_sample *samples);

/* Host logic: the k x k grid pattern, k in 1..32, into out[k * k]: sample j * k + i (row j, column i) has dx = (i + 0.5) / k - 0.5,
 * dy = (j + 0.5) / k - 0.5 and (lu, lv) = Shirley's concentric map of (a, b) = (2 dx, 2 dy) onto the unit disk (the host's libm): (0, 0)
 * at the centre; |a| > |b|: r = a, phi = (M_PI / 4.0) * (b / a); else r = b, phi = M_PI / 2.0 - (M_PI / 4.0) * (a / b); lu = r * cos(phi),
 * lv = r * sin(phi).  k = 1 gives the zero sample.  One pattern serves antialiasing and the lens.  RT_ERR_INVALID: k outside 1..32, NULL. */
int rt_view_samples_grid(uint32_t k, rt_view_sample *out);

/* Host logic: the panorama's tables of n samples, one table per sample back to back (lon: n * 2 w doubles, lat: n * 2 h doubles; the
 * layout of rt_view_equirect_tables each, whose bits the zero sample's table has).  RT_ERR_INVALID: a NULL pointer, w, h or n == 0. */
int rt_view_equirect_sample_tables(uint32_t w, uint32_t h, uint32_t n, const rt_view_sample *samples, double *lon, double *lat);

/* Host logic: rt_view_rays for ONE sample - the restatement the device is held to, bit for bit.  `table` is the index of the panorama
 * table to read (RT_VIEW_EQUIRECT: lon + 2 w table, lat + 2 h table, HOST memory; not read for the other models, pass 0).
 * RT_ERR_INVALID: what rt_view_samples_validate refuses for n = 1, a NULL out, first_row + rows > h; rows == 0 writes nothing. */
int rt_view_sample_rays(const rt_view *v, uint32_t w, uint32_t h, const rt_view_lens *lens, const rt_view_sample *sample, uint32_t table,
                        uint32_t first_row, uint32_t rows, double *out);

/* The same rows into d_rays (DEVICE memory, 16-byte aligned), asynchronous on `hip_stream` (NULL = the library's stream of `device`);
 * for RT_VIEW_EQUIRECT the tables are DEVICE pointers.  `sample` and `lens` are HOST memory, read before the call returns.  It needs no
 * scene and waits for no edit.  RT_ERR_INVALID as rt_view_sample_rays, and for a NULL or misaligned d_rays, before a device is touched. */
int rt_view_sample_rays_device(int device, const rt_view *v, uint32_t w, uint32_t h, const rt_view_lens *lens, const rt_view_sample *sample,
                               uint32_t table, uint32_t first_row, uint32_t rows, double *d_rays, void *hip_stream);

/* Host arithmetic: the workspace rt_scene_trace_view_samples_device prefers: 96 w h bytes - per pixel of a band the rays (48), one
 * sample's rgb (24) and the accumulator (24) -, the whole view in one band (docs/EVIDENCE.md "Sampled views").  0 where
 * rt_view_work_bytes is 0. */
size_t rt_view_samples_work_bytes(uint32_t w, uint32_t h);

/* The sampled trace of the view into d_out->rgb and / or d_out->rgba (DEVICE memory, frame order, as rt_scene_trace_view_device);
 * d_out->hits must be NULL: a mean of hit records means nothing.  `samples` (and `lens`) are HOST memory, read before the call returns:
 * each sample's 32 bytes travel in the generator's kernel arguments.  The view is processed in bands of whole rows (d_work: DEVICE
 * memory, 16-byte aligned, work_bytes >= 96 w: one row is the smallest band): per band and per sample in order the rays are generated
 * and traced with base = s * w * h + y0 * w; sample 0 goes straight into the accumulator, later samples into the rgb slab and are then
 * accumulated; the last sample's accumulation is fused with the resolve, which writes the band's pixels of the outputs and nothing else.
 * No result depends on the band size.  Stream, stats (kernel_ms covers every launch, pixels = w h), thread, scratch-reservation and
 * pending-edit rules are rt_scene_trace_view_device's; for RT_VIEW_EQUIRECT the tables are DEVICE pointers.  Before a device is
 * touched: RT_ERR_STATE for a NULL scene; then RT_ERR_INVALID for what rt_view_samples_validate refuses; then for segs > RT_MAX_SEGS,
 * NULL d_out, both rgb and rgba NULL, a non-NULL hits, misaligned outputs, a NULL or misaligned d_work, work_bytes below one row. */
int rt_scene_trace_view_samples_device(rt_scene_dev *scene, const rt_view *v, uint32_t w, uint32_t h, const rt_view_lens *lens, uint32_t n,
                                       const rt_view_sample *samples, uint32_t segs, const rt_ray_outputs *d_out, void *d_work,
                                       size_t work_bytes, void *hip_stream, rt_stats *stats);

/* Host form on rt_render's resident scene, as rt_trace_view: outputs in HOST memory, synchronous, on GPU 0, in chunks of whole rows of
 * at most 2^18 pixels (every sample of a chunk is traced before the next chunk).  No ray crosses the link; for RT_VIEW_EQUIRECT the
 * tables are HOST memory and the call uploads them once, (w + h) * 16 * n bytes. */
int rt_trace_view_samples(const void *scene_blob, size_t blob_bytes, const rt_view *v, uint32_t w, uint32_t h, const rt_view_lens *lens,
                          uint32_t n, const rt_view_sample *samples, uint32_t segs, const rt_ray_outputs *host_out, rt_stats *stats);

/* Ambient occlusion (sky visibility): n_samples shadow scans per RECEIVER over the hemisphere of its facing normal, counted and
 * averaged on the GPU.  A receiver is an rt_hit record - what `hits` of rt_scene_trace_rays_device / rt_scene_trace_view_device holds,
 * already in device memory - and a scan is rt_scene_occlusion_device's, bit for bit.  A fused kernel builds each segment in registers
 * (no segment exists in memory) and stores 8 to 20 bytes per receiver; a generator kernel writes the segments of one sample as a ray
 * list for callers who want to scan, order or trace them themselves (their trace and fold in one launch: rt_gather, below).  Whether the fused kernel is faster than those
 * parts is a matter of measurement: docs/EVIDENCE.md, "Ambient occlusion".
 *
 * Receiver i with record H and sample s; every operation in binary64 without FMA contraction, in the order written:
 *   l = H.inside ? -H.normal : H.normal              hit.l of main.js:445, the normal on the ray's side
 *   org = H.point;  skip = H.object                  the receiver is left out, as main.js:294 leaves hit_i out - which is also what
 *                                                    keeps a skybox from occluding everything seen from inside it
 *   the frame around l (Duff et al. 2017, branch-free):
 *     sg = copysign(1.0, l2);  a = -1.0 / (sg + l2);  b = (l0 * l1) * a
 *     t  = {1.0 + (sg * (l0 * l0)) * a,  sg * b,  -sg * l0}
 *     bt = {b,  sg + (l1 * l1) * a,  -l1}
 *   e = (((uint64)base + (uint64)i) * (uint64)stride + (uint64)s) % (uint64)n_dirs      unsigned 64-bit, wrapping at 2^64
 *   d = dirs[e]                                      a LOCAL direction {d0, d1, d2}, d2 along l; used as given
 *   dir[c] = (t[c] * d0 + bt[c] * d1) + l[c] * d2,   then the reference's normal3D (times 1 / |dir|, a zero vector left as it is)
 * stride == 0 gives every receiver the same n_samples directions (entries 0 .. n_samples - 1); stride >= 1 walks the table, so
 * neighbours use different directions (a table of whole n_samples-point sets with stride = n_samples gives each receiver one set;
 * n_samples consecutive entries of ONE long spiral all lie at nearly the same elevation).  A receiver is NOT SCANNED if it is a miss (object < 0) or has a non-finite word in point or
 * normal: its segment is six NaNs and its skip -1, which rt_scene_occlusion_device answers with intensity NaN and blocker -1.
 *
 * The n_samples segments of a receiver are scanned with length `radius` (any value > 0, +Infinity included), starting intensity 1.0,
 * the scene's CURRENT spheres and epsilon, in blob order, as rt_scene_occlusion_device scans them:
 *   open       (double)count / (double)n_samples, count = the scans that ended with blocker -1.  A receiver that is not scanned: 1.0 -
 *              a miss is open sky.
 *   intensity  acc = li_0; acc = acc + li_s for s = 1 .. n_samples - 1 in that order; acc / (double)n_samples - the fold of a sampled
 *              view.  A scan that crosses glass DIVIDES its intensity by albedo[4] (quirk q2), so intensity can exceed 1.  NaN for a
 *              receiver that is not scanned.
 *   rgba       `open` on all three channels through the store rule of main.js:195-198, alpha 255 - what rt_scene_set_texels_device takes. */
struct rt_ambient {            /* 32 bytes.  A struct tag only, as POSIX has struct stat beside stat(): rt_ambient() is the host form */
  uint32_t n_samples;          /* 1..1024 scans per receiver */
  uint32_t n_dirs;             /* n_samples..65536 entries of the direction table, 3 doubles each */
  uint32_t stride;             /* see e above */
  uint32_t reserved;           /* 0 */
  uint64_t base;               /* added to the receiver's index: a list processed in pieces passes each piece's first index */
  double radius;               /* > 0; +Infinity: sky visibility */
};
typedef struct rt_ambient_outputs {   /* one entry per receiver; any may be NULL; all three NULL is RT_ERR_INVALID */
  double   *open;
  double   *intensity;
  uint32_t *rgba;
} rt_ambient_outputs;

/* Host logic, no GPU, no rt_init.  RT_ERR_INVALID: a NULL pointer; n_samples outside 1..1024; n_dirs outside n_samples..65536;
 * reserved != 0; radius not > 0 (a NaN radius included); a table entry with a non-finite component (`dirs`: HOST memory). */
int rt_ambient_validate(const struct rt_ambient *a, const double *dirs);

/* Host logic: a cosine-weighted spiral of n directions (1..65536) into out_3n.  Entry k: u = (k + 0.5) / n,
 * phi = k * (M_PI * (3.0 - sqrt(5.0))), r = sqrt(u), {r * cos(phi), r * sin(phi), sqrt(1.0 - u)}, with fdlibm's cosine and sine
 * (csrc/rt_fdlibm.h), so that the table's bits do not depend on the host's libm.  Every z is above 0.  No transcendental function runs
 * on the device.  RT_ERR_INVALID: n outside 1..65536, NULL. */
int rt_ambient_cosine_dirs(uint32_t n, double *out_3n);

/* Host logic, the probe: the segments of sample `sample` of receivers 0 .. n - 1 (hits, dirs: HOST memory) into out_rays (n records
 * {org[3], dir[3]}) and out_skip (n entries, or NULL) - the restatement the device is held to, bit for bit.  RT_ERR_INVALID: what
 * rt_ambient_validate refuses, n outside 1..2^31 - 1, sample >= n_samples, NULL hits or out_rays. */
int rt_ambient_segments(const struct rt_ambient *a, const double *dirs, uint64_t n, const rt_hit *hits, uint32_t sample, double *out_rays,
                        int32_t *out_skip);

/* The same from a kernel: d_dirs, d_hits (8-byte aligned), d_rays (16-byte aligned) and d_skip (4-byte aligned, or NULL) are DEVICE
 * memory; asynchronous on `hip_stream` (NULL = the library's stream of `device`).  It needs no scene and waits for no edit.  The list
 * goes into rt_scene_occlusion_device (length = radius, intensity = 1.0, skip = d_skip), rt_scene_order_rays_device or
 * rt_scene_trace_rays_device as it is.  RT_ERR_INVALID as the probe (the table's entries are not looked at), and for a NULL or
 * misaligned pointer, before a device is touched. */
int rt_ambient_segments_device(int device, const struct rt_ambient *a, const double *d_dirs, uint64_t n, const rt_hit *d_hits,
                               uint32_t sample, double *d_rays, int32_t *d_skip, void *hip_stream);

/* The fused kernel: d_dirs, d_hits, d_order and the arrays d_out names are DEVICE memory (d_out itself is a host struct).  d_order is
 * NULL or an order as rt_scene_trace_rays_ordered_device takes it: work-item j takes receiver i = d_order[j], an entry >= n is skipped,
 * and receiver i reads record i, uses index i in e and writes index i - the buffers hold the bytes of the call without an order.
 * Outputs are written for every receiver an entry names (every i < n without an order) and nowhere else; an output that is NULL is not
 * touched.  A scan whose direction comes out non-finite is not traced (rt_scene_occlusion_device's rule: its intensity is NaN, it
 * counts as open).  Asynchronous on `hip_stream` (NULL = the library's stream for the scene's device) unless `stats` is non-NULL (then
 * it waits and fills kernel_ms, total_ms and pixels = n).  Waits by event for a pending rt_scene_set_objects like every other launch.
 * One work-item per receiver; a lane whose scan has met its opaque sphere goes idle and a wave leaves the scan as soon as none of its
 * 64 is live, so neighbours in the list should be neighbours in space.
 * RT_ERR_INVALID, before a device is touched: what rt_ambient_validate refuses of `a`, n outside 1..2^31 - 1, a NULL or misaligned
 * d_dirs or d_hits (8 bytes), a NULL d_out or all of its outputs NULL, a misaligned open or intensity (8 bytes), rgba or d_order
 * (4 bytes); then RT_ERR_STATE: a NULL scene.  Thread rules as rt_render_tiles_device. */
int rt_scene_ambient_device(rt_scene_dev *scene, const struct rt_ambient *a, const double *d_dirs, uint64_t n, const rt_hit *d_hits,
                            const uint32_t *d_order, const rt_ambient_outputs *d_out, void *hip_stream, rt_stats *stats);

/* Host form: rt_render's resident scene (as rt_occlusion), every array in HOST memory, the list's own order, synchronous, on GPU 0,
 * any n >= 1.  The list is processed in chunks of 2^18 receivers and chunk c passes base + c * 2^18: the call gives the bytes of one
 * launch over the whole list, and a caller who splits a list themselves passes base = the piece's first index for the same. */
int rt_ambient(const void *scene_blob, size_t blob_bytes, const struct rt_ambient *a, const double *dirs, uint64_t n, const rt_hit *hits,
               const rt_ambient_outputs *host_out, rt_stats *stats);

/* Host arithmetic: the workspace rt_scene_ambient_view_device prefers for a w x h view: 128 w h bytes - per pixel of a band its ray
 * (48) and its hit record (80) -, the whole view in one band.  0 where rt_view_work_bytes is 0. */
size_t rt_ambient_view_work_bytes(uint32_t w, uint32_t h);

/* Ambient occlusion of what a view sees: pixel i = y * w + x is receiver i, outputs in frame order (rgba is the w x h frame).  The view
 * is processed in bands of whole rows (d_work: DEVICE memory, 16-byte aligned, work_bytes >= 128 w: one row is the smallest band): per
 * band the view's rays, their hit records (the `hits` of rt_scene_trace_view_device) and the fused kernel with base + y0 * w.  No result
 * depends on the band size.  d_dirs is DEVICE memory; for RT_VIEW_EQUIRECT the view's tables are DEVICE pointers.  Stream, stats
 * (kernel_ms covers every launch, pixels = w h), thread and pending-edit rules are rt_scene_trace_view_device's.  RT_ERR_STATE: a NULL
 * scene; RT_ERR_INVALID: what rt_view_validate and rt_ambient_validate (of `a`) refuse, a NULL or misaligned d_dirs, d_out as for
 * rt_scene_ambient_device, a NULL or misaligned d_work, work_bytes below one row. */
int rt_scene_ambient_view_device(rt_scene_dev *scene, const rt_view *v, uint32_t w, uint32_t h, const struct rt_ambient *a,
                                 const double *d_dirs, const rt_ambient_outputs *d_out, void *d_work, size_t work_bytes, void *hip_stream,
                                 rt_stats *stats);

/* Host form on rt_render's resident scene, as rt_trace_view: `dirs` and the outputs in HOST memory, synchronous, on GPU 0, in chunks of
 * whole rows of at most 2^18 pixels.  No ray and no hit record crosses the link: the table goes up once (24 n_dirs bytes), 8 to 20
 * bytes per pixel come back. */
int rt_ambient_view(const void *scene_blob, size_t blob_bytes, const rt_view *v, uint32_t w, uint32_t h, const struct rt_ambient *a,
                    const double *dirs, const rt_ambient_outputs *host_out, rt_stats *stats);

/* Sampled lights ("how much light arrives here"): the reference's light loop (main.js:283-306, and :316 for the picture) per RECEIVER,
 * n_samples times, every light displaced by a table entry times light_radius in each sample, averaged on the GPU.  A receiver is an
 * rt_hit record as for rt_ambient; a scan is rt_scene_occlusion_device's, bit for bit, and the intensity is carried from light to
 * light (quirk q2).  With light_radius 0 and one sample it is the reference's own loop: `intensity` is what the hosts'
 * light_intensity_at returns, min(1, diffuse) * albedo[1] the reference's diffuse_intensity.  One fused kernel; no segment exists in
 * memory.  What it was measured at: docs/EVIDENCE.md, "Sampled lights".
 *
 * Receiver i with record H, sample s; every operation in binary64 without FMA contraction, in the order written:
 *   l = H.inside ? -H.normal : H.normal;  p = H.point;  skip = H.object          (as rt_ambient; no frame is built)
 *   NOT SCANNED: H.object < 0, or a non-finite word in point or normal
 *   e = (((uint64)base + (uint64)i) * (uint64)stride + (uint64)s) % (uint64)n_offs     unsigned 64-bit, wrapping at 2^64
 *   o = offs[e]                                       three doubles, used as given; the SAME entry for every light of the sample
 *   li = the scene's current light_intensity;  diffuse = 0;  contributed = 0
 *   for k = 0 .. n_lights - 1, the scene's current lights in blob order:
 *     pos = light_radius == 0 ? light_k : { light_k[c] + light_radius * o[c] }         (at radius 0 the table is not read)
 *     sv = pos - p;  mag = (sv0 * sv0 + sv1 * sv1) + sv2 * sv2;  len = sqrt(mag);  if (len != 0) sv = sv * (1 / len)
 *     sd = (sv0 * l0 + sv1 * l1) + sv2 * l2;  if (sd <= 0) continue                    (a NaN sd goes on, as in the reference)
 *     the scan of rt_scene_occlusion_device over the segment {p, sv}: length len, starting intensity li, sphere `skip` left out,
 *       the scene's current spheres in blob order and its epsilon -> li.  A segment with a non-finite word is not scanned: li = NaN.
 *     if (li == 0) continue
 *     diffuse = diffuse + (li * sd) / mag;  contributed++
 * (A light that is blocked leaves li 0 for the lights after it, whose scans still run, as the reference's do: a glass sphere then
 * divides 0 by its albedo[4], which is -0 for a negative and NaN for a NaN albedo[4], and rt_scene_validate admits both.)
 * Per receiver, over the samples (the fold of a sampled view: acc = x_0; acc = acc + x_s in order; acc / (double)n_samples):
 *   diffuse    the fold of the per-sample diffuse, raw: before min(1, .) and albedo[1]
 *   intensity  the fold of li after the last light
 *   lit        (double)contributed / (double)(n_samples * n_lights), all samples' count; 0.0 for a scene without lights
 *   rgba       jsmin(1, diffuse) on three channels through the store rule of main.js:195-198 (a NaN stores 0), alpha 255
 * A receiver that is not scanned: diffuse and intensity NaN, lit 0.0, rgba 0xff000000.  A scene without lights: diffuse 0.0 and
 * intensity the scene's light_intensity.
 * stride == 0 gives every receiver the same n_samples entries (0 .. n_samples - 1); stride >= 1 walks the table.  Consecutive entries
 * of rt_lighting_sphere_offsets lie on a ring, so a table of whole well-spread sets with stride = n_samples is the way to use it. */
struct rt_lighting {           /* 32 bytes.  A struct tag only, as struct rt_ambient: rt_lighting() is the host form */
  uint32_t n_samples;          /* 1..1024 runs of the light loop per receiver */
  uint32_t n_offs;             /* n_samples..65536 entries of the offset table, 3 doubles each */
  uint32_t stride;             /* see e above */
  uint32_t reserved;           /* 0 */
  uint64_t base;               /* added to the receiver's index: a list processed in pieces passes each piece's first index */
  double light_radius;         /* finite, >= 0; 0: point lights, the table is not read */
};
typedef struct rt_lighting_outputs {  /* one entry per receiver; any may be NULL; all four NULL is RT_ERR_INVALID */
  double   *diffuse;
  double   *intensity;
  double   *lit;
  uint32_t *rgba;
} rt_lighting_outputs;

/* Host logic, no GPU, no rt_init.  RT_ERR_INVALID: a NULL pointer; n_samples outside 1..1024; n_offs outside n_samples..65536;
 * reserved != 0; light_radius negative or not finite; a table entry with a non-finite component (`offs`: HOST memory). */
int rt_lighting_validate(const struct rt_lighting *a, const double *offs);

/* Host logic: n points (1..65536) on the unit sphere into out_3n, a spiral from pole to pole.  Entry k: z = 1 - (2 k + 1) / n,
 * r = sqrt(1 - z * z), phi = k * (M_PI * (3.0 - sqrt(5.0))), {r * cos(phi), r * sin(phi), z}, with fdlibm's cosine and sine
 * (csrc/rt_fdlibm.h): the same bits on every host.  Consecutive entries lie on a ring of nearly one z: give each receiver a whole
 * set (stride = n_samples over a table of sets), not n_samples neighbours of one long spiral.  RT_ERR_INVALID: n outside 1..65536, NULL. */
int rt_lighting_sphere_offsets(uint32_t n, double *out_3n);

/* Host logic, the probe: the segment of (`sample`, `light`) of receivers 0 .. n - 1 towards light `light` of lights_xyz (n_lights
 * positions, three doubles each; hits, offs: HOST memory) - out_rays n records {p[3], sv[3]} as rt_scene_occlusion_device takes
 * them, out_length len, out_mag mag, out_dot sd, out_skip the sphere left out; any but out_rays may be NULL.  A receiver that is not
 * scanned gives six NaNs, NaN length, mag and dot, and skip -1.  The restatement the device is held to, bit for bit.
 * RT_ERR_INVALID: what rt_lighting_validate refuses, n_lights outside 1..16, NULL lights_xyz, n outside 1..2^31 - 1,
 * sample >= n_samples, light >= n_lights, NULL hits or out_rays. */
int rt_lighting_segments(const struct rt_lighting *a, const double *offs, uint32_t n_lights, const double *lights_xyz, uint64_t n,
                         const rt_hit *hits, uint32_t sample, uint32_t light, double *out_rays, double *out_length, double *out_mag,
                         double *out_dot, int32_t *out_skip);

/* The fused kernel: d_offs, d_hits, d_order and the arrays d_out names are DEVICE memory (d_out itself is a host struct).  d_order,
 * the stream, stats (pixels = n), pending edits, threads and alignment are rt_scene_ambient_device's.  The lights and light_intensity
 * are the scene's current ones at the call (rt_scene_set_lights, rt_scene_set_light_intensity before it are seen); it waits by event
 * for a pending rt_scene_set_objects.  d_offs may be NULL where light_radius is 0.  One work-item per receiver; a lane that does not
 * face the light or whose scan has met its opaque sphere goes idle, and a wave leaves the scan as soon as none of its 64 is live.
 * RT_ERR_INVALID, before a device is touched: what rt_lighting_validate refuses of `a`, n outside 1..2^31 - 1, a NULL (light_radius
 * != 0) or misaligned d_offs, a NULL or misaligned d_hits (8 bytes), a NULL d_out or all of its outputs NULL, a misaligned diffuse,
 * intensity or lit (8 bytes), rgba or d_order (4 bytes); then RT_ERR_STATE: a NULL scene. */
int rt_scene_lighting_device(rt_scene_dev *scene, const struct rt_lighting *a, const double *d_offs, uint64_t n, const rt_hit *d_hits,
                             const uint32_t *d_order, const rt_lighting_outputs *d_out, void *hip_stream, rt_stats *stats);

/* Host form, as rt_ambient: rt_render's resident scene, every array in HOST memory, synchronous, on GPU 0, any n >= 1, in chunks of
 * 2^18 receivers; chunk c passes base + c * 2^18: the bytes of one launch over the whole list. */
int rt_lighting(const void *scene_blob, size_t blob_bytes, const struct rt_lighting *a, const double *offs, uint64_t n,
                const rt_hit *hits, const rt_lighting_outputs *host_out, rt_stats *stats);

/* Host arithmetic: the workspace rt_scene_lighting_view_device prefers for a w x h view, 128 w h bytes (rt_ambient_view_work_bytes). */
size_t rt_lighting_view_work_bytes(uint32_t w, uint32_t h);

/* Sampled lights on what a view sees: pixel i = y * w + x is receiver i, outputs in frame order.  Bands of whole rows in d_work
 * (DEVICE, 16-byte aligned, work_bytes >= 128 w): per band the view's rays, their hit records and the fused kernel with
 * base + y0 * w.  No result depends on the band size.  Everything else as rt_scene_ambient_view_device. */
int rt_scene_lighting_view_device(rt_scene_dev *scene, const rt_view *v, uint32_t w, uint32_t h, const struct rt_lighting *a,
                                  const double *d_offs, const rt_lighting_outputs *d_out, void *d_work, size_t work_bytes,
                                  void *hip_stream, rt_stats *stats);

/* Host form on rt_render's resident scene, as rt_ambient_view: `offs` and the outputs in HOST memory, chunks of whole rows of at
 * most 2^18 pixels.  The table goes up once (24 n_offs bytes), 8 to 28 bytes per pixel come back. */
int rt_lighting_view(const void *scene_blob, size_t blob_bytes, const rt_view *v, uint32_t w, uint32_t h, const struct rt_lighting *a,
                     const double *offs, const rt_lighting_outputs *host_out, rt_stats *stats);

/* Relit nodes: soft shadows in the picture.  rt_lighting returns the diffuse sum alone; a wavefront node (rt_node) holds BOTH numbers the
 * lights decide, diffuse and specular, and rt_scene_fold_nodes_device turns nodes into the picture.  This call computes the two again
 * over n_samples displaced copies of the lights and writes their mean back into the node: shade, relight, spawn and fold then draw the
 * reference's picture - colours, highlights, reflections, glass - with lights that have a size.  What it was measured at:
 * docs/EVIDENCE.md, "Relit nodes".
 *
 * Node i of ray i (d_rays: the list rt_scene_shade_rays_device shaded it from; d is its direction), with the parameters of a struct
 * rt_lighting; every operation in binary64 without FMA contraction, the strict arithmetic of rt_scene_shade_rays_device:
 *   shading = hit.object >= 0 && (albedo[1] > 0 || albedo[2] > 0) of the hit sphere;  l = hit.inside ? -hit.normal : hit.normal
 *   e = (((uint64)base + (uint64)pix_i) * (uint64)stride + (uint64)s) % (uint64)n_offs    pix_i = d_pix[i], or i where d_pix is NULL
 *   o = offs[e]                             the SAME entry for every light of the sample; at light_radius 0 the table is not read
 *   per sample s: the light loop of rt_scene_shade_rays_device (main.js:283-315) with light k standing at
 *     light_radius == 0 ? light_k : { light_k[c] + light_radius * o[c] }
 *   - ONE intensity carried from light to light, no scan for a light once it is 0 (the shade kernel's rule, where rt_lighting scans
 *   on: they differ for a negative or NaN albedo[4] only), the specular term with the strict build's pow - and then
 *     diffuse_s = min(1, diffuse) * albedo[1],  specular_s = min(1, specular) * albedo[2]            (main.js:316-317, PER SAMPLE)
 *   over the samples, the fold of a sampled view, once per term: acc = x_0; acc = acc + x_s in order; acc / (double)n_samples
 * The two means are stored at bytes 104 and 112 of the node; no other byte is written.  A miss and a node that is not shading get 0.0
 * and 0.0, which is what the shade wrote.  The terms are clamped per sample: a relit node is the mean of the nodes
 * rt_scene_shade_rays_device writes for the same ray in n_samples scenes whose lights were moved on the host - the accumulation of n
 * point-light pictures' light terms - and with n_samples 1 and light_radius 0 it is the shaded node itself.
 *
 * d_offs, d_rays, d_order, d_pix and d_nodes are DEVICE memory.  d_order works as for rt_scene_shade_rays_device (an entry >= n is
 * skipped, nothing is written for it).  Stream, stats (pixels = n), thread and pending-edit rules are rt_scene_lighting_device's: the
 * spheres, epsilon, lights and light_intensity are the scene's current ones at the call.  One work-item per node, no scratch memory.
 * RT_ERR_INVALID, before a device is touched: what rt_lighting_validate refuses of `a`, n outside 1..2^31 - 1, a NULL or misaligned
 * d_rays (16 bytes) or d_nodes (8 bytes), a NULL (light_radius != 0) or misaligned d_offs (8 bytes), a misaligned d_order or d_pix
 * (4 bytes); then RT_ERR_STATE: a NULL scene. */
int rt_scene_relight_nodes_device(rt_scene_dev *scene, const struct rt_lighting *a, const double *d_offs, uint64_t n, const double *d_rays,
                                  const uint32_t *d_order, const uint32_t *d_pix, rt_node *d_nodes, void *hip_stream, rt_stats *stats);

/* Host form: rt_shade_rays followed by the relight of each chunk of 2^18 rays; `offs` (HOST memory, n_offs entries, what
 * rt_lighting_validate accepts) goes up once.  Ray i keeps pix = i without `pix` (chunk c passes base + c * 2^18), so a list gives the
 * bytes of one launch however it is cut.  Everything else as rt_shade_rays. */
int rt_relight_rays(const void *scene_blob, size_t blob_bytes, const struct rt_lighting *a, const double *offs, uint64_t n,
                    const double *rays, const uint32_t *pix, const uint32_t *path, int binned, rt_node *host_nodes, rt_stats *stats);

/* Host form: rt_trace_rays_wavefront's loop with a relight behind the shade of every level lv < levels (level 0 holds the primary hits).
 * levels 0 gives rt_trace_rays_wavefront itself, launch for launch; levels >= the depth relights every bounce.  pix_i is the ROOT ray's
 * index in the list at every level (it travels with the children as the stars sampler's pix does), so the nodes of one tree share their
 * root's table entries and no result depends on how the list is chunked.  The table goes up once per call.  RT_ERR_INVALID: what
 * rt_lighting_validate and rt_trace_rays_wavefront refuse. */
int rt_trace_rays_soft(const void *scene_blob, size_t blob_bytes, const struct rt_lighting *a, const double *offs, uint32_t levels,
                       uint64_t n, const double *rays, uint32_t segs, int order_levels, const rt_ray_outputs *host_out, rt_stats *stats,
                       uint64_t *level_counts);

/* Soft trace in one launch: rt_trace_rays_soft's picture from a recursive kernel.  The wavefront loop above allocates device memory,
 * writes 200-byte nodes to HBM and waits on the host for the child count, per chunk and per level; this call is one launch per list
 * with no node in HBM and no host wait.  What it was measured at: docs/EVIDENCE.md, "Soft trace in one launch".
 *
 * Ray i (record i of d_rays; pix = pix_base + i) is intersectWorld(segs, objects, org, dir), walked depth-first over a per-lane stack.
 * Every operation is in binary64 without FMA contraction, and every step is one the calls above define:
 *   a node at tree level lv (root = 0, lv < segs)   what rt_scene_shade_rays_device computes for the ray: the closest hit in blob order,
 *     the sample (the stars sampler with pix and with path 1 at the root, 2 path for the reflect child, 2 path + 1 for the refract
 *     child), the material's weights and the two directions.  A ray with a non-finite word is a miss whose sample is NaN x 3.
 *   its light terms at lv < levels    rt_scene_relight_nodes_device's: n_samples passes of the light loop, sample s displacing every
 *     light by light_radius * offs[e], e = (((uint64)base + pix_base + i) * stride + s) % n_offs with the ROOT ray's i; clamped and
 *     weighted per sample; acc = x_0; acc = acc + x_s; acc / (double)n_samples; 0.0 and 0.0 for a node that is not shading
 *   its light terms at lv >= levels   rt_scene_shade_rays_device's own: one pass, the lights where they stand, no division
 *   children    as rt_scene_shade_rays_device marks them, reflect before refract; below the last level (lv + 1 == segs) none is visited
 *   its colour  rt_scene_fold_nodes_device's: rgb*diffuse + rgb*specular + re + rf in that order, re and rf 0.0 where a child was not
 *     visited (and added all the same), then max(rgb*albedo[0], min(1, .)); a miss returns its sample
 * So rgb and rgba are rt_trace_rays_soft's for the same list, bit for bit; with levels 0, or with n_samples 1 and light_radius 0,
 * they are rt_scene_trace_rays_device's.  segs 0 is the scene's depth; at depth 0 every finite ray gives 0, 0, 0.
 * d_out: rgb (3 doubles per ray) and / or rgba (the store rule of main.js:195-198, alpha 255) at index i; hits must be NULL (the
 * recursive rt_scene_trace_rays_device holds those).  d_order as for rt_scene_trace_rays_ordered_device, or NULL: work-item j takes ray
 * d_order[j], an entry >= n is skipped and nothing is written for it; no result depends on it.  pix_base: a list processed in pieces
 * passes each piece's first index, and gets the bytes of one call.
 * d_offs, d_rays, d_order and the arrays d_out names are DEVICE memory.  Stream, stats (pixels = n), thread and pending-edit rules are
 * rt_scene_relight_nodes_device's: the spheres, epsilon, lights, light_intensity and stars seed are the scene's current ones at the
 * call.  One work-item per ray, 256 per workgroup; the stack (14 doubles per frame, at most 15 frames) lives in scratch memory, less
 * per lane than rt_scene_trace_rays_device reserves; RT_ERR_NOMEM where the device cannot hold that reservation.
 * RT_ERR_INVALID, before a device is touched: what rt_lighting_validate refuses of `a`, a NULL (light_radius != 0) or misaligned
 * d_offs (8 bytes), n outside 1..2^31 - 1, pix_base + n > 2^31, a NULL or misaligned d_rays (16 bytes), a misaligned d_order
 * (4 bytes), a NULL d_out, segs > RT_MAX_SEGS, a non-NULL hits, rgb and rgba both NULL, a misaligned rgb (8 bytes) or rgba (4 bytes);
 * then RT_ERR_STATE: a NULL scene. */
int rt_scene_trace_rays_soft_device(rt_scene_dev *scene, const struct rt_lighting *a, const double *d_offs, uint32_t levels, uint64_t n,
                                    const double *d_rays, const uint32_t *d_order, uint32_t pix_base, uint32_t segs,
                                    const rt_ray_outputs *d_out, void *hip_stream, rt_stats *stats);

/* Host arithmetic: the workspace rt_scene_trace_view_soft_device prefers for a w x h view, 48 w h bytes - the whole view in one band.
 * 0 where rt_view_work_bytes is 0. */
size_t rt_soft_view_work_bytes(uint32_t w, uint32_t h);

/* The soft trace of what a view sees, device-resident: pixel i = y * w + x is ray i, outputs in frame order.  Bands of whole rows in
 * d_work (DEVICE, 16-byte aligned, work_bytes >= 48 w): per band the view's rays (rt_view_rays_device) and one launch of the kernel
 * above with pix_base = y0 * w.  No result depends on the band size.  A panorama's tables are DEVICE memory, as for
 * rt_scene_trace_view_device.  RT_ERR_INVALID, before a device is touched: what rt_view_validate refuses, what
 * rt_scene_trace_rays_soft_device refuses of a, d_offs, segs and d_out, a NULL or misaligned workspace or one below a row; then
 * RT_ERR_STATE: a NULL scene. */
int rt_scene_trace_view_soft_device(rt_scene_dev *scene, const rt_view *v, uint32_t w, uint32_t h, const struct rt_lighting *a,
                                    const double *d_offs, uint32_t levels, uint32_t segs, const rt_ray_outputs *d_out, void *d_work,
                                    size_t work_bytes, void *hip_stream, rt_stats *stats);

/* Host form of rt_scene_trace_rays_soft_device on rt_render's resident scene, as rt_trace_rays: `offs`, the rays and the outputs in
 * HOST memory, synchronous, on GPU 0, in chunks of 2^18 rays; chunk c passes pix_base = c * 2^18: the bytes of one launch over the
 * whole list.  The table goes up once.  binned != 0 orders each chunk on the GPU first (rt_trace_rays_binned), which changes no result. */
int rt_trace_rays_soft_recursive(const void *scene_blob, size_t blob_bytes, const struct rt_lighting *a, const double *offs,
                                 uint32_t levels, uint64_t n, const double *rays, uint32_t segs, int binned,
                                 const rt_ray_outputs *host_out, rt_stats *stats);

/* Host form of rt_scene_trace_view_soft_device, as rt_trace_view: the rays are generated on the GPU and never cross the link; `offs`,
 * a panorama's tables and the outputs in HOST memory, chunks of whole rows of at most 2^18 pixels.  The table goes up once (24 n_offs
 * bytes); 4 to 28 bytes per pixel come back. */
int rt_trace_view_soft(const void *scene_blob, size_t blob_bytes, const rt_view *v, uint32_t w, uint32_t h, const struct rt_lighting *a,
                       const double *offs, uint32_t levels, uint32_t segs, const rt_ray_outputs *host_out, rt_stats *stats);

/* Gathered light ("what colour arrives here from the rest of the scene"): n_samples rays per RECEIVER over the hemisphere of its facing
 * normal, each traced as rt_scene_trace_rays_device traces any ray, averaged on the GPU - colour bleeding, irradiance and light probes,
 * sky light from a textured skybox, a final gather for baked textures.  What rt_ambient_segments_device makes one launch per sample and
 * a 48-byte ray in HBM for, rt_scene_trace_rays_soft_device a second launch per sample, and a host a fold over 24 n n_samples bytes,
 * is ONE launch here: no segment and no per-sample colour exists in memory.  What it was measured at: docs/EVIDENCE.md, "Gathered light".
 *
 * Receiver i with record H (an rt_hit, as for rt_ambient) and sample s; binary64 without FMA contraction, in the order written:
 *   the ray     the segment rt_ambient_segments defines for (i, s), by rt_ambient's own source: org = H.point; the direction is
 *               dirs[e], e = (((uint64)base + (uint64)i) * (uint64)stride + (uint64)s) % (uint64)n_dirs, turned into the frame of the
 *               facing normal l and passed through normal3D.  NO sphere is left out (there is no skip): the scene's epsilon alone
 *               keeps the receiver's own sphere from the start, as the reference's reflected rays rely on (main.js:270, 430).
 *   c_s         intersectWorld(segs, objects, org, dir) over the scene's CURRENT spheres, lights (where they stand), light intensity,
 *               epsilon, miss colour, textures and stars seed; the stars sampler with pix = pix_base + s * pix_stride + i and the path
 *               from the root 1.  Bit for bit what rt_scene_trace_rays_soft_device(levels = 0, pix_base = pix_base + s * pix_stride)
 *               returns for that segment list.  segs 0 is the scene's depth.
 *   rgb         acc = c_0; acc = acc + c_s for s = 1 .. n_samples - 1 in that order; acc / (double)n_samples, per channel - the fold
 *               of a sampled view.  With a cosine-weighted table (rt_ambient_cosine_dirs) rgb is irradiance / pi.
 *   rgba        rgb through the store rule of main.js:195-198, alpha 255, packed as rt_ambient's rgba - what
 *               rt_scene_set_texels_device takes.
 * A receiver that is NOT SCANNED (a miss, or a non-finite word in point or normal) has six-NaN segments: rt_scene_trace_rays_device's
 * rule for a ray that is not finite gives every c_s NaN x 3, so rgb is NaN x 3 and rgba 0, 0, 0, 255.  A sample whose direction comes
 * out non-finite makes that receiver's mean NaN, by the same rule.  Neither is a special case of this call.
 * One work-item per receiver: neighbours in the list should be neighbours in space (stride 0 then gives a wave one local direction per
 * sample), and a list below a few thousand receivers under-fills the GPU: for short lists - light probes - the same result, and its
 * weighted sums, come from rt_scene_gather_probes_device below, which puts a receiver's samples on lanes. */
struct rt_gather {             /* 32 bytes, no padding.  A struct tag only, as struct rt_ambient: rt_gather() is the host form */
  uint32_t n_samples;          /* 1..1024 rays per receiver */
  uint32_t n_dirs;             /* n_samples..65536 entries of the direction table, 3 doubles each */
  uint32_t stride;             /* rt_ambient's: see e above */
  uint32_t segs;               /* 1..RT_MAX_SEGS, 0 = the scene's depth: intersectWorld's first argument for every gathered ray */
  uint64_t base;               /* added to the receiver's index in e */
  uint32_t pix_base;           /* stars: pix of sample s of receiver i = pix_base + s * pix_stride + i */
  uint32_t pix_stride;
};
typedef struct rt_gather_outputs {    /* rgb: 3 doubles per receiver; rgba: one word; either may be NULL; both NULL is RT_ERR_INVALID */
  double   *rgb;
  uint32_t *rgba;
} rt_gather_outputs;

/* Host logic, no GPU, no rt_init.  RT_ERR_INVALID: a NULL pointer; n_samples outside 1..1024; n_dirs outside n_samples..65536;
 * segs > RT_MAX_SEGS; a table entry with a non-finite component (`dirs`: HOST memory). */
int rt_gather_validate(const struct rt_gather *a, const double *dirs);

/* The fused kernel: d_dirs, d_hits, d_order and the arrays d_out names are DEVICE memory (d_out itself is a host struct).  d_order as
 * for rt_scene_ambient_device: work-item j takes receiver d_order[j], an entry >= n is skipped, receiver i reads record i, uses index
 * i in e and in pix and writes index i.  Outputs are written for every receiver an entry names (every i < n without an order) and
 * nowhere else; an output that is NULL is not touched.  Stream, stats (pixels = n), pending-edit (spheres, lights, texels) and thread
 * rules are rt_scene_trace_rays_soft_device's.  The kernel keeps that call's stack in scratch memory, the same bytes per lane;
 * RT_ERR_NOMEM where the device cannot hold the reservation.
 * RT_ERR_INVALID, before a device is touched: what rt_gather_validate refuses of `a` (the table's entries are not looked at),
 * n outside 1..2^31 - 1, pix_base + (n_samples - 1) * pix_stride + n > 2^31 (in 64 bits: the soft call's bound, for the last sample),
 * a NULL or misaligned d_dirs or d_hits (8 bytes), a NULL d_out or both of its outputs NULL, a misaligned rgb (8 bytes), rgba or
 * d_order (4 bytes); then RT_ERR_STATE: a NULL scene. */
int rt_scene_gather_device(rt_scene_dev *scene, const struct rt_gather *a, const double *d_dirs, uint64_t n, const rt_hit *d_hits,
                           const uint32_t *d_order, const rt_gather_outputs *d_out, void *hip_stream, rt_stats *stats);

/* Host form, as rt_ambient: rt_render's resident scene, every array in HOST memory, the list's own order, synchronous, on GPU 0.  The
 * list is processed in chunks of 2^18 receivers and chunk c adds c * 2^18 to both base and pix_base: the call gives the bytes of one
 * launch over the whole list.  RT_ERR_INVALID as above, with `dirs` judged by rt_gather_validate. */
int rt_gather(const void *scene_blob, size_t blob_bytes, const struct rt_gather *a, const double *dirs, uint64_t n, const rt_hit *hits,
              const rt_gather_outputs *host_out, rt_stats *stats);

/* Host arithmetic: the workspace rt_scene_gather_view_device prefers for a w x h view, 128 w h bytes (rt_ambient_view_work_bytes). */
size_t rt_gather_view_work_bytes(uint32_t w, uint32_t h);

/* Gathered light of what a view sees: pixel i = y * w + x is receiver i, outputs in frame order (rgba is the w x h frame).  Bands of
 * whole rows as rt_scene_ambient_view_device (d_work: DEVICE memory, 16-byte aligned, work_bytes >= 128 w): per band the view's rays,
 * their hit records and the fused kernel; a band that starts at row y0 adds y0 * w to base and pix_base.  No result depends on the
 * band size.  The bound on pix is taken with n = w h.  Everything else as rt_scene_ambient_view_device and rt_scene_gather_device. */
int rt_scene_gather_view_device(rt_scene_dev *scene, const rt_view *v, uint32_t w, uint32_t h, const struct rt_gather *a,
                                const double *d_dirs, const rt_gather_outputs *d_out, void *d_work, size_t work_bytes, void *hip_stream,
                                rt_stats *stats);

/* Host form on rt_render's resident scene, as rt_ambient_view: `dirs` and the outputs in HOST memory, synchronous, on GPU 0, in chunks
 * of whole rows of at most 2^18 pixels.  No ray and no hit record crosses the link: the table goes up once, 4 to 28 bytes per pixel
 * come back. */
int rt_gather_view(const void *scene_blob, size_t blob_bytes, const rt_view *v, uint32_t w, uint32_t h, const struct rt_gather *a,
                   const double *dirs, const rt_gather_outputs *host_out, rt_stats *stats);

/* Probes: gathered light for SHORT receiver lists, and its weighted sums.  The description is struct rt_gather, unchanged, and rgb and
 * rgba are rt_scene_gather_device's, BYTE FOR BYTE: the same ray, the same c_s, the same fold in the same order.  What differs is the
 * mapping - one workgroup per receiver, the receiver's samples on its lanes (up to 1024), the colours folded through LDS by one lane
 * per chain in list order - and the third output:
 *   coef        n x n_weights x 3 doubles.  With e_s the table entry sample s of receiver i took its direction from (e above: the SAME
 *               entry; d_weights has one row of n_weights contiguous doubles per table entry, n_dirs rows), binary64 without FMA
 *               contraction, in the order written:
 *                 acc = w[e_0][k] * c_0[ch];  acc = acc + (w[e_s][k] * c_s[ch]) for s = 1 .. n_samples - 1 in that order;
 *                 coef[i][k][ch] = acc / (double)n_samples.
 *               With rt_probe_sh9_weights of the table and a table of uniform sphere directions, coef is the projection of the arriving
 *               radiance on the nine real spherical harmonics of bands 0..2 up to the measure: the radiance coefficient is 4 pi * coef,
 *               which is the caller's multiplication.  A receiver that is not scanned has NaN in every coefficient (the sign of a NaN
 *               product is not stated).
 * n_weights 0: d_weights and coef must both be NULL, and the call is the plain mean.
 * Which call to choose (measured on one MI355X, default14, docs/EVIDENCE.md, "Probes"): this call below some 300 000 receivers - 120
 * times faster at 64 receivers x 256 samples, 5 times at 65 536 receivers -, rt_scene_gather_device above: it overtakes between 262 144
 * and 1 048 576 receivers at 64, 256 and 1024 samples alike.  Table directions are world directions where the receiver's normal is
 * (0, 0, 1): the frame of that normal is the world's axes. */
typedef struct rt_probe_outputs {     /* rgb, rgba: as rt_gather_outputs; coef: n x n_weights x 3 doubles; any may be NULL, not all */
  double   *rgb;
  uint32_t *rgba;
  double   *coef;
} rt_probe_outputs;

#define RT_PROBE_MAX_WEIGHTS 16u

/* Host logic, no GPU, no rt_init.  RT_ERR_INVALID: what rt_gather_validate refuses of `a` and `dirs`; n_weights > 16; n_weights > 0
 * with NULL `weights`, or n_weights 0 with `weights` given; a weight (`weights`: HOST memory, n_dirs x n_weights) that is not finite. */
int rt_probes_validate(const struct rt_gather *a, const double *dirs, const double *weights, uint32_t n_weights);

/* Nine real spherical-harmonics values per direction, for `n` directions (x, y, z) = dirs[3 i .. 3 i + 2] taken AS GIVEN (not
 * normalised), into out[9 i .. 9 i + 8].  Host arithmetic in binary64, only *, + and -, in exactly this order:
 *   out[0] = 0.28209479177387814
 *   out[1] = 0.4886025119029199 * y        out[2] = 0.4886025119029199 * z        out[3] = 0.4886025119029199 * x
 *   out[4] = 1.0925484305920792 * (x * y)  out[5] = 1.0925484305920792 * (y * z)  out[6] = 1.0925484305920792 * (x * z)
 *   out[7] = 0.31539156525252005 * ((3.0 * (z * z)) - 1.0)
 *   out[8] = 0.5462742152960396 * ((x * x) - (y * y))
 * RT_ERR_INVALID: a NULL pointer, n == 0 or n > 65536. */
int rt_probe_sh9_weights(uint32_t n, const double *dirs, double *out);

/* The probe kernel: d_dirs, d_weights, d_hits, d_order and the arrays d_out names are DEVICE memory (d_out itself is a host struct).
 * d_order, the outputs written, stream, stats (pixels = n), pending-edit and thread rules and RT_ERR_NOMEM are
 * rt_scene_gather_device's; one workgroup per entry of the list, 24 n_samples bytes of LDS each.
 * RT_ERR_INVALID, before a device is touched: everything rt_scene_gather_device refuses (with every output NULL in place of both),
 * n_weights > 16, d_weights and coef not both given or both absent, n_weights 0 with either given or > 0 with neither, a misaligned
 * coef or d_weights (8 bytes); then RT_ERR_STATE: a NULL scene.  The weights in DEVICE memory are not looked at. */
int rt_scene_gather_probes_device(rt_scene_dev *scene, const struct rt_gather *a, const double *d_dirs, const double *d_weights,
                                  uint32_t n_weights, uint64_t n, const rt_hit *d_hits, const uint32_t *d_order,
                                  const rt_probe_outputs *d_out, void *hip_stream, rt_stats *stats);

/* Host form, as rt_gather: every array in HOST memory, chunks of 2^18 receivers with base and pix_base advanced; `dirs` and `weights`
 * judged by rt_probes_validate. */
int rt_gather_probes(const void *scene_blob, size_t blob_bytes, const struct rt_gather *a, const double *dirs, const double *weights,
                     uint32_t n_weights, uint64_t n, const rt_hit *hits, const rt_probe_outputs *host_out, rt_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* RT_HIP_H */
