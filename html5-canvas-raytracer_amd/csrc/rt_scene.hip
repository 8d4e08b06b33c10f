// rt_scene.hip — a resident scene (include/rt_hip.h: rt_scene_*): upload and free, the host decisions that depend on its spheres and
// its camera, the blocks it keeps in HBM, the camera / object / light / stars-seed moves (the generation pipeline), the texel edits, the launch
// decisions of its product launches and its launch tables (built on the GPU, rt_tables_gpu.hip).

#include "rt_api_internal.h"
#include "rt_objects.h"

// ------------------------------------------------------------------------------------ launch decisions of a resident scene
namespace rt_api {
// The prologue of a launch of the scene on `stream` (launch_mu held): it comes behind the last texel edit and the current generation's
// preparation, and the next move or edit orders itself behind it (rt_scene_sync.h: R1)
int enter_launch(rt_scene_dev *s, hipStream_t stream) {
  HIP_TRY(s->sync.before_launch(stream, s->cam_gen));
  s->sync.note_launch(stream);
  return RT_OK;
}

// Which kernel.  The product (FMA) kernel unless the caller asks for the strict one - or the scene itself sits on an exact
// coincidence whose outcome in the reference is decided by the last bit of its own arithmetic (s->needs_strict, see
// object_decisions): only the operation-for-operation kernel reproduces those.  (Test build: RT_NO_FIXUP, read per call, keeps the
// product kernel's own pixels everywhere.)
bool strict_scene(const rt_scene_dev *s) { return s->needs_strict && RT_TEST_ENV("RT_NO_FIXUP") == nullptr; }

// The product kernel meets a constant where a primary ray meets nothing but the background: a flat sky of constant colour, or no
// enclosing sphere at all (the miss colour, main.js:231)
bool sky_fast(const rt_scene_dev *s) { return (s->enclosing_flat && s->sky_const) || (s->enclosing == ~0u && s->hd.segs > 0); }

// Many spheres (more than 16 in the loops: a light's set is "empty or not"): the masks cost the table build ten times what
// they save ONE frame (64 spheres at 3840x2160: 0.33 ms of a 0.36 ms build against 0.013 ms of a 0.11 ms trace; few spheres:
// 0.011 against 0.020: profiles/r03_ab_log.md section 3) - the first frame from a camera is rendered from a table without
// them, a camera that stays gets the full table with its second frame.  (The picture is the same either way: masks only prune.)
// ("second frame" is counted per frame kind: the bands of one rt_render frame and the owner's sky fill are several launches of
// ONE frame, and all of them are first launches from a new camera)
bool masks_pay(const rt_scene_dev *s, uint32_t uses_before) {
  const uint32_t n_loop = s->hd.n_objects - (s->enclosing != ~0u ? 1u : 0u);
  return n_loop <= 16u || uses_before >= 1u;
}

uint32_t sky_part_of(uint32_t flags) { return (flags & RT_FLAG_NO_SKY) ? 1u : ((flags & RT_FLAG_SKY_ONLY) ? 2u : 0u); }

// The launch table of a product launch (dispatch_order's key beside the frame kind), from its flags and the launches of its frame
// kind from the current camera before it.
//   sky marks: workgroups no sphere can show in store the background constant without tracing (rt_block.h); the counting
//     variant traces them like any other (its counters are what the caller wants)
//   shadow masks: per block and light, the spheres that can shadow a primary hit of the block at all; needs every lit primary
//     hit to lie on a loop sphere, i.e. no enclosing sphere or a flat one
//   candidates: the block's primary candidates
//   checker cells: which 8-pixel columns of a one-candidate block lie inside one cell of that sphere's checker (rt_block.h)
//   first-bounce sets: which spheres the rays reflected at a block's primary hits can meet (rt_block.h)
//   second node: which of a stating block's mirrors its reflected rays cannot meet again, and whether they meet nothing at all (rt_block.h)
//   (a table of nothing but sky runs is read by workgroups that store a constant: neither masks nor candidates)
table_choice choose_table(const rt_scene_dev *s, uint32_t flags, uint32_t uses_before) {
  static const bool no_order = RT_TEST_ENV("RT_NO_DISPATCH_ORDER") != nullptr;    // A/B switches (test build): the grid's own order,
  static const bool no_sky_tiles = RT_TEST_ENV("RT_NO_SKY_TILES") != nullptr;     //   no sky marks,
  static const bool no_shadow_masks = RT_TEST_ENV("RT_NO_SHADOW_MASKS") != nullptr;   //   neither masks nor candidates
  const bool count = (flags & RT_FLAG_COUNT) != 0;
  const uint32_t part = sky_part_of(flags);
  table_choice c;
  c.ranked = (flags & RT_FLAG_COMPACT) ? 2 : ((!count && !no_order) ? 1 : 0);
  c.mark_sky = !count && !no_sky_tiles && sky_fast(s);
  c.shadow_masks = !count && !no_shadow_masks && masks_pay(s, uses_before) && part != 2u && (s->enclosing == ~0u || s->enclosing_flat);
  c.name_candidates = !count && !no_shadow_masks && part != 2u;
  // (whole cells only: the trace kernels do not read the per-axis statements - docs/EVIDENCE.md, "Checker cells, per axis")
  c.checker_cells = c.name_candidates ? 1 : 0;        // (costs the build nothing unless the scene has a checker sphere: rt_tables.cpp)
  // first-bounce sets: read by the few-sphere reflection-only product kernels alone (rt_kernel_trace.h), at a depth that lets a mirror reflect,
  // in a scene whose enclosing sphere - outside the loops and the statement - spawns no reflected ray of its own (rt_tables.cpp: make_table_params)
  c.first_bounce = c.name_candidates && !s->refract && s->cull_in_lds && s->hd.segs >= 2u &&
                   (s->enclosing == ~0u || s->host_objects[s->enclosing].albedo[3] <= 0.0);
  // ... and beside them what the node after the primary may skip (rt_block.h: rt_second_node_bits), read by the same kernels
  // (always beside the sets in a product launch: the field of its own in the table cache's key differs only through rt_test_launch_table's flags)
  c.second_node = c.first_bounce ? 1 : 0;
  return c;
}

// Product launches of this frame kind from the scene's current camera before this one (which is counted); launch_mu held
uint32_t count_use(rt_scene_dev *s, const frame_kind &kind) {
  rt_scene_dev::camera_use *cu = nullptr;
  for (rt_scene_dev::camera_use &c : s->camera_uses) if (c.kind == kind) { cu = &c; break; }
  if (!cu) {
    if (s->camera_uses.size() >= 64u) s->camera_uses.erase(s->camera_uses.begin());
    s->camera_uses.push_back(rt_scene_dev::camera_use{kind, 0u, 0u});
    cu = &s->camera_uses.back();
  }
  if (cu->cam_gen != s->cam_gen) { cu->cam_gen = s->cam_gen; cu->uses = 0u; }
  return cu->uses++;
}
}  // namespace rt_api

// ------------------------------------------------------------------------------------ upload
namespace {

// [materials (rt_mtl) | 16 texture descriptors | cull rectangles (few spheres)] of ordering `ord`: the workgroup's LDS image
void fill_lds_image(const rt_scene_dev *s, uint8_t *dst, int ord) {
  const uint32_t NO = s->hd.n_objects;
  const rt_sphere *src = ord ? s->host_objects_b.data() : (const rt_sphere *)(s->host_blob.data() + s->hd.objects_offset);
  rt_mtl *mt = (rt_mtl *)dst;
  for (uint32_t i = 0; i < NO; i++) {
    const rt_sphere &o = src[i];
    rt_mtl &m = mt[i];
    memset(&m, 0, sizeof m);
    memcpy(m.origin, o.origin, sizeof m.origin);
    m.inv_r = o.reserved;                           // 1/r, patched at upload
    memcpy(m.albedo, o.albedo, sizeof m.albedo);
    m.specular_exponent = o.specular_exponent; m.refract_index = o.refract_index;
    m.spec_n = rt_spec_n(o.specular_exponent);
    m.sampler_kind = (int16_t)o.sampler_kind; m.texture = (int16_t)(o.sampler_kind == RT_SAMPLER_TEXTURE ? o.texture : -1);   // (check_sphere: 0..3, < RT_MAX_TEXTURES)
    if (o.sampler_kind == RT_SAMPLER_CHECKER) memcpy(m.c, o.checker_color, 6 * sizeof(double));
    else memcpy(m.c, o.color, 3 * sizeof(double));
    m.c[6] = o.checker_freq[0]; m.c[7] = o.checker_freq[1];
  }
  memcpy(dst + (size_t)NO * sizeof(rt_mtl), s->descs, sizeof s->descs);
  if (s->cull_in_lds) {
    rt_geom *cr = (rt_geom *)(dst + (size_t)NO * sizeof(rt_mtl) + sizeof s->descs);
    for (uint32_t i = 0; i < NO; i++) cr[i] = cull_rect(&s->hd, src[i]);
  }
}

// The camera block (rt_scene_dev): per ordering [anchored at the camera {o - cam, |o - cam|^2 - r2} N | primary-ray cull
// rectangles N], then the LDS images when they hold the rectangles.  `dst`: cam_bytes of host memory.
void fill_camera_block(const rt_scene_dev *s, uint8_t *dst) {
  const uint32_t NO = s->hd.n_objects;
  const int n_ord = s->has_b ? 2 : 1;
  for (int ord = 0; ord < n_ord; ord++) {
    const rt_sphere *src = ord ? s->host_objects_b.data() : (const rt_sphere *)(s->host_blob.data() + s->hd.objects_offset);
    rt_geom *g = (rt_geom *)dst + (size_t)ord * 2u * NO;
    for (uint32_t i = 0; i < NO; i++) {
      const double lx = src[i].origin[0] - s->hd.cam_origin[0], ly = src[i].origin[1] - s->hd.cam_origin[1], lz = src[i].origin[2] - s->hd.cam_origin[2];
      g[i] = rt_geom{lx, ly, lz, (lx * lx + ly * ly + lz * lz) - src[i].r2};
      g[NO + i] = cull_rect(&s->hd, src[i]);
    }
  }
  if (s->cull_in_lds) {
    uint8_t *img = dst + s->cam_lds_offset;
    for (int ord = 0; ord < n_ord; ord++) fill_lds_image(s, img + ord * s->lds_image_bytes, ord);
  }
}

// what of a resident scene depends on the camera and is decided on the host: is it a strict-kernel scene, which sphere encloses
// everything, the background constant, the cull rectangles and cost weights of the launch tables
void camera_decisions(rt_scene_dev *s) {
  const rt_scene_header *hd = &s->hd;
  const rt_sphere *ob = (const rt_sphere *)(s->host_blob.data() + hd->objects_offset);
  s->needs_strict = s->needs_strict_scene;
  for (int c = 0; c < 3; c++) if (hd->cam_axis_x[c] + hd->cam_axis_y[c] + hd->cam_axis_z[c] == 0.0) s->needs_strict = true;
  // cost-ordered dispatch: what a tile that shows sphere j is expected to cost, in rough units of one shaded hit - a guess
  // that only has to RANK tiles: lit hits 2, one more per bounce a reflective or refractive hit can spawn, and the binary tree
  // of a sphere that does both (main.js:268-278) its node count; pure-ambient spheres (the reference's skybox) nothing
  scene_tile_weights(hd, ob, &s->host_cull, &s->tile_weight);
}

// What of a resident scene depends on its spheres (and its lights: the coincidence below) and is decided on the host - in ONE place,
// for rt_scene_upload, rt_scene_set_objects and rt_scene_set_lights alike: the device copy of the records (host_blob's, with 1/r in `reserved`), ordering B, the kernel
// variant, the strict-kernel coincidences, the samplers' boundary tolerance, the mark weight rule and the enclosing sphere's
// background.  Reads host_objects (the records as given); `enclosing` is decided already.
void object_decisions(rt_scene_dev *s) {
  const rt_scene_header *hd = &s->hd;
  const uint8_t *base = s->host_blob.data();
  const rt_sphere *ob = s->host_objects.data();
  s->refract = false;
  for (uint32_t i = 0; i < hd->n_objects; i++) if (ob[i].albedo[4] > 0.0) s->refract = true;
  // Scenes whose picture hinges on exact coincidences are rendered by the strict kernel throughout (the product kernel's
  // short cuts - 1/r from the host, anchored discriminants, shadow rays walked from the light - assume a generic scene):
  //   * a light exactly ON a sphere's surface (the reference's own `t < light_len`, main.js:297, then compares two numbers
  //     that are equal up to rounding: a coin flip that only the reference's own arithmetic reproduces);
  //   * a sphere with r2 <= 0 or not finite (no 1/r);
  //   * a sphere-checker whose frequencies are negative, NaN or >= 2^31 (below);
  //   * a camera whose axis sums (main.js:187-191, quirk q1) have an exactly zero component: EVERY primary ray then lies in
  //     a coordinate plane through the camera (camera_decisions; rt_retrace traces the centre row / column of an odd sample grid
  //     for the same reason).
  s->needs_strict_scene = false;
  for (uint32_t i = 0; i < hd->n_objects; i++) {
    if (!(ob[i].r2 > 0.0) || !std::isfinite(ob[i].r2)) s->needs_strict_scene = true;
    for (uint32_t k = 0; k < hd->n_lights; k++) {
      const double x = s->lights[k][0] - ob[i].origin[0], y = s->lights[k][1] - ob[i].origin[1], z = s->lights[k][2] - ob[i].origin[2];
      if (fabs((x * x + y * y + z * z) - ob[i].r2) <= 1e-9 * fmax(ob[i].r2, 1.0)) s->needs_strict_scene = true;
    }
  }
  // the boundary test of the product kernel's samplers (rt_device.h: RT_FLAG_T1): a coordinate is u * frequency
  {
    double fmaxq = 1.0;
    const rt_texture_desc *td = (const rt_texture_desc *)(base + hd->textures_offset);
    for (uint32_t i = 0; i < hd->n_objects; i++) {
      if (ob[i].sampler_kind != RT_SAMPLER_TEXTURE && ob[i].sampler_kind != RT_SAMPLER_CHECKER) continue;
      if (ob[i].sampler_kind == RT_SAMPLER_TEXTURE) fmaxq = fmax(fmaxq, (double)(td[ob[i].texture].width > td[ob[i].texture].height ? td[ob[i].texture].width : td[ob[i].texture].height));
      if (ob[i].sampler_kind == RT_SAMPLER_CHECKER) {
        const double f0 = ob[i].checker_freq[0], f1 = ob[i].checker_freq[1];
        if (fabs(f0) > fmaxq) fmaxq = fabs(f0);                       // (NaN frequencies: every sample of such a sphere is NaN, and marked)
        if (fabs(f1) > fmaxq) fmaxq = fabs(f1);
        // the product kernel takes ToInt32(u * f) & 1 (main.js:129-130) from a fixed-point sum that holds it for products in [0, 2^31):
        // other frequencies (negative, huge, NaN) make the scene a strict-kernel scene
        if (!(f0 >= 0.0 && f0 < 2147483648.0 && f1 >= 0.0 && f1 < 2147483648.0)) s->needs_strict_scene = true;
      }
    }
    // The hot path's prefilter passes coordinates within 2^-20 of an integer to the precise test against flag_tol = RT_FLAG_T1 x this
    // frequency, scaled by the hit's magnification bound (rt_kernel.hip): the band has to leave that scaling room.  Up to 2^17 per unit u
    // it is 36 x the flat tolerance; the adversarial soak's second pixel (a checker at 1e6 per unit, two bounces: an error of 1.75e-6
    // squares, beyond the band) is what set the limit.  Scenes with finer samplers take the strict kernel.
    if (fmaxq > 131072.0) s->needs_strict_scene = true;
    s->flag_tol = RT_FLAG_T1 * fmaxq;
    // (boundary marks) every albedo and colour within [0, 1]: then a node's colour moves the pixel by at most its accumulated weight
    s->unit_weights = true;
    for (uint32_t i = 0; i < hd->n_objects; i++) {
      for (int c = 0; c < 5; c++) if (!(ob[i].albedo[c] >= 0.0 && ob[i].albedo[c] <= 1.0)) s->unit_weights = false;
      for (int c = 0; c < 3; c++) if (!(ob[i].color[c] >= 0.0 && ob[i].color[c] <= 1.0)) s->unit_weights = false;
      if (ob[i].sampler_kind == RT_SAMPLER_CHECKER) for (int c = 0; c < 6; c++) if (!(ob[i].checker_color[c / 3][c % 3] >= 0.0 && ob[i].checker_color[c / 3][c % 3] <= 1.0)) s->unit_weights = false;
    }
  }
  s->enclosing_flat = false;
  if (s->enclosing != ~0u) {
    const rt_sphere &sk = ob[s->enclosing];
    s->enclosing_flat = !(sk.albedo[1] > 0.0) && !(sk.albedo[2] > 0.0) && !(sk.albedo[3] > 0.0) && !(sk.albedo[4] > 0.0) &&
                        (sk.sampler_kind == RT_SAMPLER_COLOR || sk.sampler_kind == RT_SAMPLER_STARS);
  }
  s->sky_const = s->enclosing_flat && ob[s->enclosing].sampler_kind == RT_SAMPLER_COLOR && hd->segs > 0;
  for (int c = 0; c < 3; c++) {
    s->sky_rgb[c] = 0.0;
    if (s->sky_const) {
      // main.js:322-336 for a hit without light and without children: diffuse = specular = 0, reflect = refract = [0,0,0]
      const volatile double col = ob[s->enclosing].color[c], a0 = ob[s->enclosing].albedo[0], zero = 0.0;
      const volatile double amb = col * a0, d0 = col * zero, s0 = col * zero;
      const volatile double shade = d0 + s0;
      const double m1 = (shade > 1.0) ? 1.0 : shade;                    // Math.min(1, shade); NaN stays NaN
      s->sky_rgb[c] = (m1 < amb) ? (double)amb : m1;                    // Math.max(amb, .) as the kernel's maxa() evaluates it
    }
  }
  // device copy of the records: the `reserved` slot of each sphere record carries 1/r for the product kernel
  rt_sphere *pob = (rt_sphere *)(s->host_blob.data() + hd->objects_offset);
  memcpy(pob, ob, (size_t)hd->n_objects * sizeof(rt_sphere));
  for (uint32_t i = 0; i < hd->n_objects; i++) pob[i].reserved = 1.0 / sqrt(pob[i].r2);
  // Two orderings of the spheres.  A = the scene's own order (strict kernels, counting variant).  B = the enclosing sphere moved to
  // the end, so that the product kernel's loops run over [0, N-1) and never test it.
  s->host_objects_b.clear();
  if (s->enclosing != ~0u) {
    for (uint32_t i = 0; i < hd->n_objects; i++) if (i != s->enclosing) s->host_objects_b.push_back(pob[i]);
    s->host_objects_b.push_back(pob[s->enclosing]);
  }
}

// The host-written part of an object block (rt_scene_dev: obj_host_bytes of host memory at `dst`): the records, the geometry tables,
// ordering B, the LDS images of many-sphere scenes and the shadow grids' headers.  The masks and the bounce table behind it are built
// from these (rt_scene_upload: rt_tables.cpp on the host; rt_scene_set_objects: rt_objects_gpu.hip).
void fill_object_block(const rt_scene_dev *s, uint8_t *dst) {
  const rt_scene_header *hd = &s->hd;
  const uint32_t NO = hd->n_objects, NL = hd->n_lights;
  const int n_ord = s->has_b ? 2 : 1;
  memset(dst, 0, s->obj_host_bytes);
  const rt_sphere *pob_a = (const rt_sphere *)(s->host_blob.data() + hd->objects_offset);
  memcpy(dst + s->o_objs, pob_a, (size_t)NO * sizeof(rt_sphere));
  const size_t geom_per_order = (size_t)NO * (1 + NL);                 // [plain N | anchored at light k: NL x N]
  for (int ord = 0; ord < n_ord; ord++) {
    const rt_sphere *src = ord ? s->host_objects_b.data() : pob_a;
    rt_geom *g = (rt_geom *)(dst + s->o_geom) + ord * geom_per_order;
    for (uint32_t i = 0; i < NO; i++) {
      g[i] = rt_geom{src[i].origin[0], src[i].origin[1], src[i].origin[2], src[i].r2};
      for (uint32_t k = 0; k < NL; k++) g[(size_t)NO * (1 + k) + i] = rt_anchored(src[i].origin, src[i].r2, s->lights[k]);
    }
  }
  ((rt_geom *)(dst + s->o_geom))[geom_per_order * n_ord] = rt_geom{0.0, 0.0, 0.0, -1.0};   // one record of padding: the kernel's scans fetch a light's first two records at once, also when it has one
  if (s->has_b) memcpy(dst + s->o_objs_b, s->host_objects_b.data(), (size_t)NO * sizeof(rt_sphere));
  // the LDS images' camera-independent part: [materials | texture descriptors] (fill_camera_block writes them, with their cull
  // rectangles, when they live in the camera block)
  if (!s->cull_in_lds) for (int ord = 0; ord < n_ord; ord++) fill_lds_image(s, dst + s->o_img + ord * s->lds_image_bytes, ord);
  if (s->has_sg) {
    const rt_sphere *loop = s->has_b ? s->host_objects_b.data() : pob_a;
    for (uint32_t k = 0; k < NL; k++) shadow_grid_frame(loop, s->has_b ? NO - 1u : NO, s->lights[k], (double *)(dst + s->o_sg) + 16u * k);
  }
}

std::atomic<int> g_uploads{0};       // rt_scene_upload calls (test build: rt_test_upload_count)
constexpr size_t up256(size_t x) { return (x + 255u) & ~(size_t)255u; }
}  // namespace

#ifdef RT_TESTING
extern "C" int rt_test_upload_count(void) { return g_uploads.load(); }
#endif

extern "C" int rt_scene_upload(int device, const void *blob, size_t bytes, rt_scene_dev **out) {
  if (!out) return fail(RT_ERR_INVALID, "out handle is NULL");
  *out = nullptr;
  int rc = rt_scene_validate(blob, bytes);
  if (rc) return rc;
  if ((rc = ensure_device(device))) return rc;
  g_uploads++;
  const rt_scene_header *hd = (const rt_scene_header *)blob;
  rt_scene_dev *s = new rt_scene_dev();
  s->device = device; s->hd = *hd; s->d_blob = nullptr; s->d_texdesc = nullptr; s->d_cones = nullptr;
  s->d_cam_buf[0] = s->d_cam_buf[1] = nullptr; s->d_obj_buf[0] = s->d_obj_buf[1] = nullptr;
  const uint8_t *base = (const uint8_t *)blob;
  const rt_sphere *ob = (const rt_sphere *)(base + hd->objects_offset);
  memset(s->lights, 0, sizeof s->lights);
  if (hd->n_lights) memcpy(s->lights, base + hd->lights_offset, hd->n_lights * 24u);
  memcpy(s->slot_lights[0], s->lights, sizeof s->lights); memcpy(s->slot_lights[1], s->lights, sizeof s->lights);
  rt_texture_desc (&descs)[RT_MAX_TEXTURES] = s->descs;
  memset(descs, 0, sizeof descs);
  if (hd->n_textures) memcpy(descs, base + hd->textures_offset, hd->n_textures * sizeof(rt_texture_desc));
  s->enclosing = enclosing_sphere(hd, ob, s->lights);     // (rt_tables.cpp)
  s->host_objects.assign(ob, ob + hd->n_objects);
  s->host_blob.assign((const uint8_t *)blob, (const uint8_t *)blob + bytes);
  object_decisions(s);
  camera_decisions(s);
  const uint32_t NO = hd->n_objects, NL = hd->n_lights;
  s->has_b = s->enclosing != ~0u;
  const bool has_b = s->has_b;
  const int n_ord = has_b ? 2 : 1;
  const rt_sphere *pob_a = (const rt_sphere *)(s->host_blob.data() + hd->objects_offset);
  const uint32_t n_loop_b = has_b ? NO - 1 : NO;       // spheres in the product kernel's loops
  static const uint32_t sgrid_min = RT_TEST_ENV("RT_SGRID_MIN") ? (uint32_t)atoi(RT_TEST_ENV("RT_SGRID_MIN")) : RT_SGRID_MIN_LOOP;     // A/B switches (test build)
  static const uint32_t btable_min = RT_TEST_ENV("RT_BTABLE_MIN") ? (uint32_t)atoi(RT_TEST_ENV("RT_BTABLE_MIN")) : RT_BTABLE_MIN_LOOP;
  s->has_sg = n_loop_b > sgrid_min && NL > 0;
  s->has_bt = n_loop_b > btable_min && hd->segs > 1;      // rays bounce at all only from depth 2 on
  // few spheres: the cull rectangles ride in the LDS image; scenes that get a shadow grid or a bounce table run the many-sphere
  // kernel variant, which fetches them per lane (rt_kernel.hip: 64 spheres + the fold state then fit 32 KB of LDS, five workgroups
  // per CU instead of four)
  s->cull_in_lds = !(s->has_sg || s->has_bt);
  s->lds_image_bytes = (size_t)NO * (sizeof(rt_mtl) + (s->cull_in_lds ? sizeof(rt_geom) : 0u)) + sizeof descs;
  s->lds_bytes = (unsigned)s->lds_image_bytes;
  const size_t sg_words = s->has_sg ? (size_t)NL * 16u + (size_t)NL * (RT_SGRID * RT_SGRID + 1u) * ((n_loop_b + 63u) / 64u) : 0u;
  const size_t bt_words = s->has_bt ? (size_t)NO * RT_BCELLS * ((n_loop_b + 63u) / 64u) : 0u;
  // ---- an object block's layout (every part 256-byte aligned) ----
  size_t ot = 0;
  s->o_objs = ot; ot = up256(ot + (size_t)NO * sizeof(rt_sphere));
  s->o_geom = ot; ot = up256(ot + ((size_t)NO * (1 + NL) * n_ord + 1) * sizeof(rt_geom));
  s->o_objs_b = ot; ot = up256(ot + (has_b ? NO * sizeof(rt_sphere) : 0));
  s->o_img = ot; ot = up256(ot + (s->cull_in_lds ? 0 : s->lds_image_bytes * n_ord + 4096u));   // the many-sphere kernel reads whole 4 KB pieces (rt_kernel.hip staging)
  s->o_sg = ot; ot = up256(ot + sg_words * sizeof(uint64_t));
  s->obj_host_bytes = s->o_sg + (s->has_sg ? (size_t)NL * 16u * sizeof(double) : 0u);
  s->o_bt = ot; ot = up256(ot + bt_words * sizeof(uint64_t));
  s->obj_bytes = ot;
  s->sg_bytes = sg_words * sizeof(uint64_t); s->bt_bytes = bt_words * sizeof(uint64_t);
  // ---- the arena's layout ----
  size_t at = 0;
  const size_t off_blob = at; at = up256(at + bytes);
  const size_t off_tex = at; at = up256(at + sizeof descs);
  const size_t off_cones = at; at = up256(at + (s->has_bt ? 5u * RT_BCELLS * sizeof(double) : 0u));
  const size_t off_obj0 = at; at = up256(at + s->obj_bytes);
  const size_t off_obj1 = at; at = up256(at + s->obj_bytes);
  s->cam_lds_offset = up256((size_t)n_ord * 2u * NO * sizeof(rt_geom));
  s->cam_bytes_used = s->cam_lds_offset + (s->cull_in_lds ? s->lds_image_bytes * n_ord : 0);
  s->cam_bytes = s->cam_bytes_used + (s->cull_in_lds ? 4096u : 0);
  const size_t off_cam0 = at; at = up256(at + s->cam_bytes);
  const size_t off_cam1 = at; at = up256(at + s->cam_bytes);
  s->arena_bytes = at;
  std::vector<uint8_t> host(at, 0);
  memcpy(host.data() + off_blob, s->host_blob.data(), bytes);
  memcpy(host.data() + off_tex, descs, sizeof descs);
  if (s->has_bt) { const std::vector<double> cones = bounce_cell_cones(); memcpy(host.data() + off_cones, cones.data(), cones.size() * sizeof(double)); }
  fill_object_block(s, host.data() + off_obj0);
  if (s->has_sg) {
    const std::vector<uint64_t> sg = build_shadow_grid(has_b ? s->host_objects_b.data() : pob_a, n_loop_b, NL, s->lights);
    memcpy(host.data() + off_obj0 + s->o_sg, sg.data(), sg.size() * sizeof(uint64_t));
  }
  if (s->has_bt) {
    const std::vector<uint64_t> bt = build_bounce_table(has_b ? s->host_objects_b.data() : pob_a, NO, n_loop_b);
    memcpy(host.data() + off_obj0 + s->o_bt, bt.data(), bt.size() * sizeof(uint64_t));
  }
  memcpy(host.data() + off_obj1, host.data() + off_obj0, s->obj_bytes);
  fill_camera_block(s, host.data() + off_cam0);
  memcpy(host.data() + off_cam1, host.data() + off_cam0, s->cam_bytes_used);
  // ---- one allocation, one copy ----
  hipError_t e = hipMalloc(&s->arena.h, s->arena_bytes);
  if (e == hipSuccess) e = hipMemcpy(s->arena.h, host.data(), s->arena_bytes, hipMemcpyHostToDevice);
  // pinned staging for what follows a camera move (the camera block) or an object move (the camera block, then the host-written
  // part of the object block): the ring's slots hold either, or a launch table's parameters, cone-test spheres and cost rectangles
  const size_t table_dyn = 512u + (size_t)NO * (sizeof(rt_ball) + sizeof(rt_cost_rect)), move_bytes = up256(s->cam_bytes) + s->obj_host_bytes;
  if (e == hipSuccess) e = s->sync.moves.make(up256(move_bytes > table_dyn ? move_bytes : table_dyn));
  if (e != hipSuccess) {
    const std::string why = hipGetErrorString(e);
    rt_scene_free(s);
    return fail(RT_ERR_DEVICE, "scene upload: %s", why.c_str());
  }
  uint8_t *arena = (uint8_t *)s->arena.h;
  s->d_blob = arena + off_blob;
  s->d_texdesc = (rt_texture_desc *)(arena + off_tex);
  s->d_cones = s->has_bt ? (double *)(arena + off_cones) : nullptr;
  s->d_obj_buf[0] = arena + off_obj0; s->d_obj_buf[1] = arena + off_obj1;
  s->d_cam_buf[0] = arena + off_cam0; s->d_cam_buf[1] = arena + off_cam1;
  *out = s;
  return RT_OK;
}

extern "C" void rt_scene_free(rt_scene_dev *s) {
  if (!s) return;
  if (G.inited && s->device < (int)G.dev.size()) (void)hipSetDevice(G.dev[s->device].hip_id);
  (void)hipDeviceSynchronize();                    // nothing of this scene is in flight any more: its members release what they own
  delete s;
}

// The camera of a resident scene moves (lookAt, main.js:92-100; the reference recomputes everything per redraw, main.js:180-201).
// What depends on it - the camera-anchored geometry, the cull rectangles, the LDS images that hold them (ONE block of the scene's
// arena) and the launch tables of the frame sizes in use - exists twice, for even and odd camera generations.  The move stages the
// new block (pinned host memory) and, on the scene's OWN side stream, copies it and rebuilds the tables the previous camera's frames
// used: beside those frames' launches, which are still running on the caller's stream, and ordered against them by two events
// (rt_scene_sync.h: OLD, PREP).  A plain `set_camera; render; set_camera; render ...` loop on one stream thereby overlaps frame
// k + 1's table build with frame k's trace - what round 3 needed two scene handles on two streams for.  Nothing waits on the host
// unless launches of this scene are in flight on several caller streams (then the device is drained first).
namespace rt_api {
bool build_table(rt_scene_dev *s, int found, hipStream_t stream, pinned_ring::slot *cam);
}  // namespace rt_api

namespace {
// The host state of the scene has just changed - its camera (rt_scene_set_camera), its spheres (rt_scene_set_objects,
// `objects_moved`) or its lights (rt_scene_set_lights), host decisions included - and generation old_gen + 1 begins: on the side
// stream, behind the launches that read its blocks last (generation old_gen - 1), the camera block is copied and the object block
// brought up to date, and the launch tables the previous generation's frames used are rebuilt.  The object block, in two steps:
//   its spheres (slot_version)  an object move: the staged host part, then the masks of every light and the bounce table on the GPU;
//                               a move of another kind after an object move: a copy of the other block;
//   its lights (slot_lights)    the lights it holds at other positions than the scene's - the moved ones after a light move, and
//                               whatever the move before left behind in this block - get their anchored records, their grid
//                               headers (host-computed, staged) and their grids' masks from rt_objects_gpu.hip.  Nothing else of the
//                               block depends on a light: no bounce table, no staged object block for a light move.
// Lights reach the kernels by value (rt_light_list), from s->lights: the copy in d_blob is the upload's and is not read.
// Everything keyed to the generation - launch tables, mark counts, camera_uses - is stale from here on.  launch_mu held.
int next_generation(rt_scene_dev *s, uint64_t old_gen, bool objects_moved) {
  hipStream_t side = s->sync.side.h;
  const uint64_t G = ++s->cam_gen;
  const uint32_t b = (uint32_t)(G & 1u);
  // the side stream is behind the launches that read blocks and tables b last (generation G - 2)
  HIP_TRY(s->sync.begin_generation(G));
  pinned_ring::slot *slot = nullptr;
  HIP_TRY(s->sync.moves.acquire(&slot));
  uint8_t *st = slot->h;
  fill_camera_block(s, st);
  if (objects_moved) s->obj_version++;
  uint8_t *blk = s->d_obj_buf[b];
  const uint32_t NO = s->hd.n_objects, NL = s->hd.n_lights, n_loop = s->has_b ? NO - 1u : NO;
  const rt_sphere *loop = (const rt_sphere *)(blk + (s->has_b ? s->o_objs_b : s->o_objs));
  uint8_t *so = st + up256(s->cam_bytes);              // (the slot's second part: an object move's host part, or a light move's grid headers)
  if (s->slot_version[b] != s->obj_version) {
    hipError_t e = hipSuccess;
    if (objects_moved) {
      fill_object_block(s, so);
      rt_light_list all = {};
      all.n = NL;
      for (uint32_t k = 0; k < NL; k++) { all.k[k] = k; memcpy(all.xyz[k], s->lights[k], 24u); }
      e = (hipError_t)rt_launch_objects_copy(blk, so, s->obj_host_bytes, side);
      if (e == hipSuccess && s->has_sg) e = (hipError_t)rt_launch_sgrid_build(loop, n_loop, NL, &all, (uint64_t *)(blk + s->o_sg), side);
      if (e == hipSuccess && s->has_bt) e = (hipError_t)rt_launch_bounce_build(loop, NO, n_loop, s->d_cones, (uint64_t *)(blk + s->o_bt), side);
      memcpy(s->slot_lights[b], s->lights, sizeof s->lights);
    } else {
      e = hipMemcpyAsync(blk, s->d_obj_buf[b ^ 1u], s->obj_bytes, hipMemcpyDeviceToDevice, side);
      memcpy(s->slot_lights[b], s->slot_lights[b ^ 1u], sizeof s->lights);
    }
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "object block: %s", hipGetErrorString(e));
    s->slot_version[b] = s->obj_version;
  }
  rt_light_list moved = {};
  for (uint32_t k = 0; k < NL; k++)
    if (memcmp(s->slot_lights[b][k], s->lights[k], 24u) != 0) { moved.k[moved.n] = k; memcpy(moved.xyz[moved.n], s->lights[k], 24u); moved.n++; }
  if (moved.n) {
    double *headers = (double *)so;
    if (s->has_sg) {
      const rt_sphere *hloop = s->has_b ? s->host_objects_b.data() : (const rt_sphere *)(s->host_blob.data() + s->hd.objects_offset);
      for (uint32_t j = 0; j < moved.n; j++) shadow_grid_frame(hloop, n_loop, moved.xyz[j], headers + 16u * j);
    }
    hipError_t e = (hipError_t)rt_launch_light_anchor((const rt_sphere *)(blk + s->o_objs), s->has_b ? (const rt_sphere *)(blk + s->o_objs_b) : nullptr, s->has_b ? 2u : 1u, NO, NL, &moved,
                                                      (rt_geom *)(blk + s->o_geom), s->has_sg ? (double *)(blk + s->o_sg) : nullptr, headers, side);
    if (e == hipSuccess && s->has_sg) e = (hipError_t)rt_launch_sgrid_build(loop, n_loop, NL, &moved, (uint64_t *)(blk + s->o_sg), side);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "object block, lights: %s", hipGetErrorString(e));
    memcpy(s->slot_lights[b], s->lights, sizeof s->lights);
  }
  // the tables the previous generation's frames used are rebuilt now, on the side stream, beside those frames' launches: the next
  // render of such a frame finds its table (up to four; others are built by the launch that needs them, on its stream).  Many-sphere
  // scenes: the first frame from a camera takes the table without shadow masks (masks_pay).
  int built = 0;
  bool cam_sent = false;
  for (size_t i = 0; i < s->orders.size() && built < 4; i++) {
    rt_scene_dev::order_entry &e = s->orders[i];
    if (e.used_gen != old_gen || !e.built || (e.masks && !masks_pay(s, 0u))) continue;
    if (!build_table(s, (int)i, side, cam_sent ? nullptr : slot)) return RT_ERR_DEVICE;
    cam_sent = true;
    built++;
  }
  if (!cam_sent) {
    hipError_t e = (hipError_t)rt_launch_small_copy(cam_block(s), st, s->cam_bytes_used, nullptr, nullptr, 0u, side);
    if (e == hipSuccess) e = s->sync.moves.done(slot, side);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "camera block: %s", hipGetErrorString(e));
  }
  HIP_TRY(s->sync.end_generation(G));
  return RT_OK;
}
}  // namespace

extern "C" int rt_scene_set_camera(rt_scene_dev *s, const double origin[3], const double axis_x[3], const double axis_y[3], const double axis_z[3], void *hip_stream) {
  if (!s || !origin || !axis_x || !axis_y || !axis_z) return fail(RT_ERR_INVALID, "rt_scene_set_camera: NULL argument");
  int rc = ensure_device(s->device);
  if (rc) return rc;
  (void)hip_stream;                                  // (kept in the signature: the copy and the rebuilds run on the scene's own side stream)
  std::lock_guard<std::mutex> lk(s->launch_mu);
  rt_scene_header nh = s->hd;
  memcpy(nh.cam_origin, origin, 24); memcpy(nh.cam_axis_x, axis_x, 24); memcpy(nh.cam_axis_y, axis_y, 24); memcpy(nh.cam_axis_z, axis_z, 24);
  if (memcmp(&nh, &s->hd, sizeof nh) == 0) return RT_OK;
  // the two orderings of the scene's tables are built around the sphere that encloses everything INCLUDING the camera
  if (enclosing_sphere(&nh, s->host_objects.data(), s->lights) != s->enclosing)
    return fail(RT_ERR_UNSUPPORTED, "rt_scene_set_camera: the camera crossed the enclosing sphere (the scene's tables are laid out around it): upload the scene again");
  HIP_TRY(s->sync.ensure_side());
  const uint64_t old_gen = s->cam_gen;
  s->hd = nh;
  memcpy(s->host_blob.data(), &nh, sizeof nh);
  camera_decisions(s);
  return next_generation(s, old_gen, false);
}

// The spheres of a resident scene move or change their material (the reference's objects are plain arrays a page may change between
// two redraws, main.js:180-201).  What depends on them - the object block, the camera block, the launch tables, the host decisions -
// follows through the same generation pipeline as a camera move (next_generation): frames already enqueued keep the old spheres, the
// next launch of the scene on any stream waits (by event) for the new ones.
extern "C" int rt_scene_set_objects(rt_scene_dev *s, uint32_t first, uint32_t count, const rt_sphere *records, void *hip_stream) {
  if (!s) return fail(RT_ERR_INVALID, "rt_scene_set_objects: NULL scene");
  (void)hip_stream;                                  // (as rt_scene_set_camera: the copy and the builds run on the scene's side stream)
  const uint32_t NO = s->hd.n_objects;
  if (first > NO || count > NO - first) return fail(RT_ERR_INVALID, "rt_scene_set_objects: spheres [%u, %u + %u) outside [0, %u)", first, first, count, NO);
  if (count && !records) return fail(RT_ERR_INVALID, "rt_scene_set_objects: NULL records");
  for (uint32_t i = 0; i < count; i++)
    if (check_sphere(records[i], first + i, s->hd.n_textures) != RT_OK) { const std::string why = g_err; return fail(RT_ERR_INVALID, "rt_scene_set_objects: %s", why.c_str()); }
  int rc = ensure_device(s->device);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(s->launch_mu);
  std::vector<rt_sphere> next(s->host_objects);
  for (uint32_t i = 0; i < count; i++) {
    rt_sphere r = records[i];
    r.reserved = next[first + i].reserved;           // (the device copy's 1/r: derived, whatever the caller's record holds)
    next[first + i] = r;
  }
  if (memcmp(next.data(), s->host_objects.data(), (size_t)NO * sizeof(rt_sphere)) == 0) return RT_OK;
  if (enclosing_sphere(&s->hd, next.data(), s->lights) != s->enclosing)
    return fail(RT_ERR_UNSUPPORTED, "rt_scene_set_objects: the edit changes the sphere that encloses everything (the scene's tables are laid out around it): upload the scene again");
  HIP_TRY(s->sync.ensure_side());
  const uint64_t old_gen = s->cam_gen;
  s->host_objects.swap(next);
  object_decisions(s);
  camera_decisions(s);
  return next_generation(s, old_gen, true);
}

// The lights of a resident scene move (the reference's lights are a literal array inside intersectWorld, main.js:283, that a page
// edits in place).  What depends on them - the host copy every launch record takes, the light-anchored records and the shadow grids
// of the object block, the launch tables' shadow masks, the "light on a surface" decision - follows through the generation pipeline
// (next_generation): a move of its own kind, cheaper than an object move - no bounce table, no staged object block.
extern "C" int rt_scene_set_lights(rt_scene_dev *s, uint32_t first, uint32_t count, const double *xyz, void *hip_stream) {
  if (!s) return fail(RT_ERR_INVALID, "rt_scene_set_lights: NULL scene");
  (void)hip_stream;                                  // (as rt_scene_set_camera: the builds run on the scene's side stream)
  const uint32_t NL = s->hd.n_lights;
  if (first > NL || count > NL - first) return fail(RT_ERR_INVALID, "rt_scene_set_lights: lights [%u, %u + %u) outside [0, %u)", first, first, count, NL);
  if (count && !xyz) return fail(RT_ERR_INVALID, "rt_scene_set_lights: NULL positions");
  int rc = ensure_device(s->device);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(s->launch_mu);
  double next[RT_MAX_LIGHTS][3];
  memcpy(next, s->lights, sizeof next);
  if (count) memcpy(next[first], xyz, (size_t)count * 24u);
  if (memcmp(next, s->lights, sizeof next) == 0) return RT_OK;
  if (enclosing_sphere(&s->hd, s->host_objects.data(), next) != s->enclosing)
    return fail(RT_ERR_UNSUPPORTED, "rt_scene_set_lights: the move changes the sphere that encloses everything (the scene's tables are laid out around it): upload the scene again");
  HIP_TRY(s->sync.ensure_side());
  const uint64_t old_gen = s->cam_gen;
  memcpy(s->lights, next, sizeof next);
  memcpy(s->host_blob.data() + s->hd.lights_offset, next, (size_t)NL * 24u);
  object_decisions(s);
  camera_decisions(s);
  return next_generation(s, old_gen, false);
}

// The shared light intensity (main.js:284) is host state like the stars seed: the launch record carries it (rt_launch.hip), and
// neither a table, nor a host decision, nor a mark count depends on it (a sample is marked by its sampler coordinate and the product
// of the albedos above it, rt_kernel.hip: RT_XY_INDEX).  Frames already enqueued keep theirs.
extern "C" int rt_scene_set_light_intensity(rt_scene_dev *s, double light_intensity) {
  if (!s) return fail(RT_ERR_INVALID, "rt_scene_set_light_intensity: NULL scene");
  std::lock_guard<std::mutex> lk(s->launch_mu);
  s->hd.light_intensity = light_intensity;
  memcpy(s->host_blob.data() + offsetof(rt_scene_header, light_intensity), &light_intensity, sizeof light_intensity);
  return RT_OK;
}

// The stars seed (include/rt_hip.h: RT_SAMPLER_STARS) is host state: render_batch_impl copies it into each launch record, so frames
// already enqueued keep theirs.  Nothing on the device depends on it - a stars sky is never a constant background, so no launch
// table or sky block changes.
extern "C" int rt_scene_set_stars_seed(rt_scene_dev *s, uint32_t seed) {
  if (!s) return fail(RT_ERR_INVALID, "rt_scene_set_stars_seed: NULL scene");
  std::lock_guard<std::mutex> lk(s->launch_mu);
  s->hd.stars_seed = seed;
  memcpy(s->host_blob.data() + offsetof(rt_scene_header, stars_seed), &seed, sizeof seed);
  return RT_OK;
}

// ------------------------------------------------------------------------------------ texel edits
// The texels of a resident scene's textures are replaced (the reference's textures are ImageData a page may draw into between two
// redraws, main.js:339-395; sampled one texel at a time, main.js:343-351).  No generation, no table, no launch decision (rt_scene_dev:
// R4): one write by rt_texels_blit on the caller's stream - behind the scene's launches in flight (stream order, or TEXB;
// launches on several streams: the device is drained, as a move does) and in front of every later one (stream order, or TEXD in
// enter_launch).  Only kernel boundaries order it: nothing relies on caches being coherent inside a kernel.
namespace {
constexpr size_t RT_TEXEL_STAGE_SLOT = 256u * 1024u;    // of pinned_ring::n_slots = 16: 4 MiB of pinned memory (include/rt_hip.h says so)

// the checks of both forms that need no scene
int texels_args_check(const char *what, uint32_t w, uint32_t h, const void *src, size_t pitch_bytes, bool device) {
  if (!src && w && h) return fail(RT_ERR_INVALID, "%s: NULL source for a rectangle of %ux%u texels", what, w, h);
  if (pitch_bytes && (pitch_bytes < 4u * (size_t)w || (pitch_bytes & 3u))) return fail(RT_ERR_INVALID, "%s: a pitch of %zu bytes is below 4 x %u or no multiple of 4", what, pitch_bytes, w);
  if (device && ((uintptr_t)src & 3u)) return fail(RT_ERR_INVALID, "%s: the device source is not 4-byte aligned", what);
  return RT_OK;
}
// ... and those that need one
int texels_rect_check(const char *what, const rt_scene_dev *s, uint32_t texture, uint32_t x, uint32_t y, uint32_t w, uint32_t h) {
  if (texture >= s->hd.n_textures) return fail(RT_ERR_INVALID, "%s: texture %u of %u", what, texture, s->hd.n_textures);
  const rt_texture_desc &d = s->descs[texture];
  if ((uint64_t)x + w > d.width || (uint64_t)y + h > d.height)
    return fail(RT_ERR_INVALID, "%s: the rectangle [%u, %u + %u) x [%u, %u + %u) leaves texture %u (%ux%u): another size is an upload", what, x, x, w, y, y, h, texture, d.width, d.height);
  return RT_OK;
}

uint32_t *texel_at(const rt_scene_dev *s, uint32_t texture, uint32_t x, uint32_t y) {
  const rt_texture_desc &d = s->descs[texture];
  return (uint32_t *)((uint8_t *)s->d_blob + d.texels_offset) + (size_t)y * d.width + x;
}

int set_texels(rt_scene_dev *s, uint32_t texture, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const void *src, size_t pitch_bytes, void *hip_stream, bool device) {
  const char *what = device ? "rt_scene_set_texels_device" : "rt_scene_set_texels";
  int rc = texels_args_check(what, w, h, src, pitch_bytes, device);
  if (rc) return rc;
  if (!s) return fail(RT_ERR_STATE, "%s: NULL scene handle", what);
  if ((rc = texels_rect_check(what, s, texture, x, y, w, h))) return rc;
  if (w == 0u || h == 0u) return RT_OK;
  hipStream_t stream = nullptr;
  if ((rc = scene_stream(s, hip_stream, &stream))) return rc;
  const size_t pitch = pitch_bytes ? pitch_bytes : 4u * (size_t)w;
  const uint32_t tex_w = s->descs[texture].width;
  std::lock_guard<std::mutex> lk(s->launch_mu);
  if (!device) HIP_TRY(s->sync.texels.make(RT_TEXEL_STAGE_SLOT));
  HIP_TRY(s->sync.begin_edit(stream));
  auto write = [&]() -> int {
    if (device) {
      const rt_texels_launch L = {texel_at(s, texture, x, y), (const uint32_t *)src, tex_w, pitch / 4u, w};
      HIP_TRY((hipError_t)rt_launch_texels_blit(&L, h, stream));
      return RT_OK;
    }
    // the rows are packed into pinned slots, which the blit reads over the host link: pieces of whole rows (a texture row is at most
    // 64 KiB: four rows and more per slot).  A slot is written again only after the piece that read it (its event): the one host wait,
    // taken when the caller is sixteen pieces ahead of the GPU.
    const uint32_t rows_per = (uint32_t)(RT_TEXEL_STAGE_SLOT / (4u * (size_t)w));
    for (uint32_t j0 = 0; j0 < h; j0 += rows_per) {
      const uint32_t rows = h - j0 < rows_per ? h - j0 : rows_per;
      pinned_ring::slot *g = nullptr;
      HIP_TRY(s->sync.texels.acquire(&g));
      for (uint32_t j = 0; j < rows; j++) memcpy(g->h + (size_t)j * 4u * w, (const uint8_t *)src + (size_t)(j0 + j) * pitch, 4u * (size_t)w);
      const rt_texels_launch L = {texel_at(s, texture, x, y + j0), (const uint32_t *)g->h, tex_w, w, w};
      HIP_TRY((hipError_t)rt_launch_texels_blit(&L, rows, stream));
      HIP_TRY(s->sync.texels.done(g, stream));
    }
    return RT_OK;
  };
  rc = write();
  const hipError_t after = s->sync.end_edit(stream);         // (also behind pieces of an edit that failed half way)
  if (rc == RT_OK) HIP_TRY(after);
  return rc;
}
}  // namespace

extern "C" int rt_scene_set_texels(rt_scene_dev *s, uint32_t texture, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const void *rgba, size_t pitch_bytes, void *hip_stream) {
  return set_texels(s, texture, x, y, w, h, rgba, pitch_bytes, hip_stream, false);
}

extern "C" int rt_scene_set_texels_device(rt_scene_dev *s, uint32_t texture, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const void *d_rgba, size_t pitch_bytes, void *hip_stream) {
  return set_texels(s, texture, x, y, w, h, d_rgba, pitch_bytes, hip_stream, true);
}

namespace rt_api {
// a pinned host word of the scene's pool (generation << 32 | value + 1, written by a kernel): [0, RT_KNOWN_WORDS) the mark states',
// [RT_KNOWN_WORDS, 2 RT_KNOWN_WORDS) the launch tables'
volatile unsigned long long *known_word(rt_scene_dev *s, size_t index) {
  if (!s->h_known_pool.h) {
    if (hipHostMalloc(&s->h_known_pool.h, 2 * RT_KNOWN_WORDS * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); s->h_known_pool.h = nullptr; return nullptr; }
    memset(s->h_known_pool.h, 0, 2 * RT_KNOWN_WORDS * sizeof(unsigned long long));
  }
  return index < 2 * RT_KNOWN_WORDS ? (unsigned long long *)s->h_known_pool.h + index : nullptr;
}
// what a kernel published for camera generation `gen`: value + 1, or 0 (nothing yet, or an older camera's)
uint32_t known_value(const volatile unsigned long long *p, uint64_t gen) {
  if (!p) return 0u;
  const unsigned long long v = *p;
  return (uint32_t)(v >> 32) == (uint32_t)gen ? (uint32_t)v : 0u;
}

// Build the launch table of entry `found` for the scene's CURRENT camera (generation g, into the entry's table g & 1) on `stream`:
// one small copy of its parameters - which also carries the staged camera block `cam` of a move, if given - and three small launches
// (rt_tables_gpu.hip); nothing waits for them.  Called with the scene's launch_mu held.  false: rt_last_error says why.
bool build_table(rt_scene_dev *s, int found, hipStream_t stream, pinned_ring::slot *cam) {
  rt_scene_dev::order_entry &e = s->orders[found];
  const frame_kind &k = e.kind;
  const launch_geom g = launch_geometry(s->hd.fov_deg, k.w, k.h, k.ss, k.tiles.tile_rows);
  const uint32_t tb = (uint32_t)(s->cam_gen & 1u);
  rt_table_params P;
  std::vector<rt_ball> balls;
  std::vector<rt_cost_rect> rects;
  if (make_table_params(&s->hd, s->host_objects.data(), s->host_cull, s->tile_weight, k.w, k.h, k.ss, &k.tiles, g.tiles_x, g.rb_per_tile, g.proj_w, g.proj_h, g.proj_d, e.ranked,
                        e.sky, s->enclosing, e.masks, e.cands, e.cells, e.first_bounce, e.second_node, s->lights, &P, &balls, &rects)) {
    fail(RT_ERR_INVALID, "a launch of %llu workgroups is beyond the launch table", (unsigned long long)g.tiles_x * k.tiles.n_tiles * g.rb_per_tile);
    return false;
  }
  P.flags |= k.part == 1u ? RT_TABLE_NO_SKY : (k.part == 2u ? RT_TABLE_SKY_ONLY : 0u);
  const uint32_t n = P.tiles_x * P.ny;
  const size_t hist_words = (size_t)P.ny * P.cost_bins;
  rt_table_dev &T = e.Tb[tb];
  // the table's device memory: one allocation behind all its arrays; the per-row histograms grow with the camera's cost range
  if (!e.d_blockb[tb].h || e.hist_wordsb[tb] < hist_words) {
    if (e.d_blockb[tb].h) { (void)hipDeviceSynchronize(); e.d_blockb[tb].reset(); }
    auto up = [](size_t x) { return (x + 255u) & ~(size_t)255u; };
    const size_t cap_hist = hist_words > (size_t)P.ny * 128u ? hist_words : (size_t)P.ny * 128u;
    const size_t dyn_bytes = up(sizeof(rt_table_params)) + up((size_t)RT_MAX_OBJECTS * sizeof(rt_ball)) + up((size_t)RT_MAX_OBJECTS * sizeof(rt_cost_rect)) + 256u;
    size_t at = 0;
    const size_t o_dyn = at; at += dyn_bytes;
    const size_t o_blk = at; at = up(at + (size_t)n * 12u);
    const size_t o_item = at; at = up(at + (size_t)n * 4u);
    const size_t o_rank = at; at = up(at + (size_t)n * 4u);
    const size_t o_hist = at; at = up(at + cap_hist * 4u);
    const size_t o_bins = at; at = up(at + (size_t)(RT_COST_MAX + 1u) * 4u);
    const size_t o_head = at; at = up(at + 16u + ((size_t)(n + 7u) / 8u) * 8u * 16u);
    uint8_t *blk = nullptr;
    hipError_t er = hipMalloc((void **)&blk, at);
    if (er == hipSuccess) er = hipMemsetAsync(blk + o_dyn + dyn_bytes - 256u, 0, 256u, stream);     // the scan's ticket
    if (er == hipSuccess) er = e.built.make();
    if (er != hipSuccess) { if (blk) (void)hipFree(blk); fail(RT_ERR_DEVICE, "launch table (%zu bytes): %s", at, hipGetErrorString(er)); return false; }
    e.d_blockb[tb].h = blk;
    e.hist_wordsb[tb] = cap_hist;
    T.params = (const rt_table_params *)(blk + o_dyn);
    T.ticket = (uint32_t *)(blk + o_dyn + dyn_bytes - 256u);
    T.blk = (uint32_t *)(blk + o_blk); T.item = (uint32_t *)(blk + o_item); T.rank_in_row = (uint32_t *)(blk + o_rank);
    T.row_hist = (uint32_t *)(blk + o_hist); T.bin_start = (uint32_t *)(blk + o_bins);
    T.header = (uint32_t *)(blk + o_head); T.entries = T.header + 4;
    T.known = (unsigned long long *)e.known;
  } else if (e.shared && stream != s->sync.side.h) {
    // rebuilt lazily on a caller's stream while launches on ANOTHER caller's stream may still read this table's older contents: only
    // when nothing is in flight (rare; a move's own rebuilds, on the side stream, come behind OLD instead)
    (void)hipDeviceSynchronize();
  }
  e.n_blocks = n;
  e.cost_bins = P.cost_bins;
  e.cam_gen = s->cam_gen;
  T.known_tag = (uint32_t)s->cam_gen;
  e.built_on = stream; e.shared = false;
  // parameters, cone-test spheres and cost rectangles, packed: one staging slot, ONE small copy kernel - which also carries the
  // scene's camera block of a move (an SDMA copy in front of the build would cost two engine hand-overs, more than the copy)
  pinned_ring::slot *slot = nullptr;
  hipError_t er = s->sync.moves.acquire(&slot);
  uint8_t *st = slot->h;
  const size_t o_balls = (sizeof(rt_table_params) + 15u) & ~(size_t)15u, o_rects = o_balls + balls.size() * sizeof(rt_ball);
  const size_t copy_bytes = o_rects + rects.size() * sizeof(rt_cost_rect);
  T.balls = (const rt_ball *)((const uint8_t *)T.params + o_balls);
  T.rects = (const rt_cost_rect *)((const uint8_t *)T.params + o_rects);
  memcpy(st, &P, sizeof P);
  if (!balls.empty()) memcpy(st + o_balls, balls.data(), balls.size() * sizeof(rt_ball));
  if (!rects.empty()) memcpy(st + o_rects, rects.data(), rects.size() * sizeof(rt_cost_rect));
  if (er == hipSuccess) er = (hipError_t)rt_launch_small_copy((void *)T.params, st, copy_bytes, cam ? cam_block(s) : nullptr, cam ? cam->h : nullptr, cam ? s->cam_bytes_used : 0u, stream);
  if (er == hipSuccess) er = s->sync.moves.done(slot, stream);
  if (er == hipSuccess && cam) er = s->sync.moves.done(cam, stream);
  if (er == hipSuccess) er = (hipError_t)rt_launch_table_build(&T, P.tiles_x, P.ny, P.cost_bins, (uint32_t)copy_bytes, ((P.flags & RT_TABLE_WIDE) ? 1 : 0) | (stream == s->sync.side.h ? 2 : 0), stream);
  if (er == hipSuccess) er = hipEventRecord(e.built.h, stream);
  if (er != hipSuccess) { e.cam_gen = 0; fail(RT_ERR_DEVICE, "launch table build: %s", hipGetErrorString(er)); return false; }
  return true;
}

// The launch table of this (frame kind, table choice) for the scene's CURRENT camera: found - built by rt_scene_set_camera on the
// scene's side stream, or by an earlier launch - or built now on `stream`.  Called with the scene's launch_mu held.  Returns the
// entry's index, or -1 (rt_last_error says why).
int dispatch_order(rt_scene_dev *s, const frame_kind &kind, const table_choice &c, hipStream_t stream) {
  // kind.part: 0 every entry; 1 (RT_FLAG_NO_SKY) a table without the sky runs; 2 (RT_FLAG_SKY_ONLY) a table of nothing else - tables of
  // their own, so that the trace kernel knows nothing of it (a test of the launch record in its prologue cost the headline 1.5 %)
  int found = -1;
  for (size_t i = 0; i < s->orders.size(); i++) {
    const rt_scene_dev::order_entry &e = s->orders[i];
    if (e.kind == kind && e.ranked == c.ranked && e.sky == c.mark_sky && e.masks == c.shadow_masks && e.cands == c.name_candidates && e.cells == c.checker_cells && e.first_bounce == c.first_bounce && e.second_node == c.second_node) { found = (int)i; break; }
  }
  if (found >= 0 && s->orders[found].cam_gen == s->cam_gen) {
    rt_scene_dev::order_entry &e = s->orders[found];
    // built on another caller's stream: this stream's launches come behind the build (the side stream's builds: behind PREP,
    // which every stream waits for before its first launch with a camera)
    if (e.built_on != stream && e.built_on != s->sync.side.h) { if (hipStreamWaitEvent(stream, e.built.h, 0) != hipSuccess) { fail(RT_ERR_DEVICE, "launch table: hipStreamWaitEvent"); return -1; } e.shared = true; }
    e.used_gen = s->cam_gen;
    return found;
  }
  if (found < 0) {
    const launch_geom g = launch_geometry(s->hd.fov_deg, kind.w, kind.h, kind.ss, kind.tiles.tile_rows);
    if ((uint64_t)g.tiles_x * kind.tiles.n_tiles * g.rb_per_tile >= (1ull << 31) || g.tiles_x > 2048u) {
      fail(RT_ERR_INVALID, "a launch of %llu workgroups is beyond the launch table", (unsigned long long)g.tiles_x * kind.tiles.n_tiles * g.rb_per_tile);
      return -1;
    }
    // a scene that has been rendered with 64 different (frame size, tile set) pairs gives up its oldest table (nothing of it may be
    // in flight: the device is drained first; rare)
    if (s->orders.size() >= 64u) {
      (void)hipDeviceSynchronize();
      found = (int)(s->order_evict++ % 64u);
      for (rt_scene_dev::mark_state &m : s->mark_states) if (m.order_index == (uint32_t)found && m.h_known) *m.h_known = 0ull;     // its mark counts were another table's
    } else {
      s->orders.push_back(rt_scene_dev::order_entry());
      found = (int)s->orders.size() - 1;
    }
    rt_scene_dev::order_entry &e = s->orders[found];
    e = rt_scene_dev::order_entry();                     // (an evicted table's memory and event go with it)
    e.kind = kind;
    e.ranked = c.ranked; e.sky = c.mark_sky; e.masks = c.shadow_masks; e.cands = c.name_candidates; e.cells = c.checker_cells; e.first_bounce = c.first_bounce; e.second_node = c.second_node;
    e.known = known_word(s, RT_KNOWN_WORDS + (size_t)found);
    if (e.known) *e.known = 0ull;                        // (a table evicted from this slot may have published its count for the same camera)
  }
  if (!build_table(s, found, stream, nullptr)) return -1;
  s->orders[found].used_gen = s->cam_gen;
  return found;
}

}  // namespace rt_api

#ifdef RT_TESTING
// Test build only: a sphere-dependent region of the scene's CURRENT generation, read back (the device is drained first).  part: 0 the
// records in blob order (1/r in `reserved`), 1 the geometry tables, 2 ordering B, 3 the LDS images, 4 the shadow grids, 5 the bounce
// table, 6 the camera block.  Returns the region's size in bytes (0: the scene has no such region), copied to `out` when `bytes`
// holds it; < 0: an RT_ERR_* code.
extern "C" long long rt_test_scene_state(rt_scene_dev *s, int part, void *out, size_t bytes) {
  if (!s) return fail(RT_ERR_INVALID, "rt_test_scene_state: NULL scene");
  if (int rc = ensure_device(s->device)) return rc;
  std::lock_guard<std::mutex> lk(s->launch_mu);
  const uint32_t NO = s->hd.n_objects, NL = s->hd.n_lights;
  const int n_ord = s->has_b ? 2 : 1;
  const uint8_t *src = nullptr;
  size_t n = 0;
  switch (part) {
    case 0: src = obj_block(s) + s->o_objs; n = (size_t)NO * sizeof(rt_sphere); break;
    case 1: src = obj_block(s) + s->o_geom; n = ((size_t)NO * (1 + NL) * n_ord + 1) * sizeof(rt_geom); break;
    case 2: src = obj_block(s) + s->o_objs_b; n = s->has_b ? (size_t)NO * sizeof(rt_sphere) : 0u; break;
    case 3: src = lds_image_of(s); n = s->lds_image_bytes * n_ord; break;
    case 4: src = obj_block(s) + s->o_sg; n = s->sg_bytes; break;
    case 5: src = obj_block(s) + s->o_bt; n = s->bt_bytes; break;
    case 6: src = cam_block(s); n = s->cam_bytes_used; break;
    default: return fail(RT_ERR_INVALID, "rt_test_scene_state: part %d not in 0..6", part);
  }
  if (out && n && bytes >= n) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, src, n, hipMemcpyDeviceToHost));
  }
  return (long long)n;
}

// Test build only: the resident blob's bytes from its first texel to its end (the textures' texels and whatever lies between them), read
// back after a drain.  Returns their count (0: a scene without textures), copied to `out` when `bytes` holds it; < 0: an RT_ERR_* code.
extern "C" long long rt_test_scene_texels(rt_scene_dev *s, void *out, size_t bytes) {
  if (!s) return fail(RT_ERR_INVALID, "rt_test_scene_texels: NULL scene");
  if (int rc = ensure_device(s->device)) return rc;
  std::lock_guard<std::mutex> lk(s->launch_mu);
  size_t first = s->host_blob.size();
  for (uint32_t t = 0; t < s->hd.n_textures; t++) if (s->descs[t].texels_offset < first) first = s->descs[t].texels_offset;
  const size_t n = s->host_blob.size() - first;
  if (out && n && bytes >= n) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, (const uint8_t *)s->d_blob + first, n, hipMemcpyDeviceToHost));
  }
  return (long long)n;
}

// Test build only: the launch table as the library builds it ON THE GPU for `tiles` of the w x h frame of a resident scene (its
// current camera), read back: same arguments and layout as the host-logic probe rt_scene_launch_table below, whose table (the host
// build of the same rt_block.h) it must equal word for word.
extern "C" int rt_test_launch_table(rt_scene_dev *s, uint32_t w, uint32_t h, const rt_tiles *tiles, int ranked, uint32_t *out_entries, uint32_t *n_workgroups, uint32_t *n_blocks) {
  if (!s || !tiles || !n_workgroups) return fail(RT_ERR_INVALID, "rt_test_launch_table: NULL argument");
  int rc = ensure_device(s->device);
  if (rc) return rc;
  hipStream_t stream = G.dev[s->device].stream;
  const uint32_t ss = s->hd.supersample;
  if (ss > 2u) return fail(RT_ERR_INVALID, "supersample 3 and 4 launch on the sample grid");
  const frame_kind kind = {w, h, ss, *tiles, (ranked & 8) ? 1u : ((ranked & 16) ? 2u : 0u)};
  const table_choice c = {(ranked & 1) != 0, (ranked & 2) != 0, (ranked & 4) != 0, (ranked & 4) != 0, (ranked & 32) ? ((ranked & 64) ? 2 : 1) : 0, (ranked & 128) != 0, (ranked & 256) ? 1 : 0};
  std::lock_guard<std::mutex> lk(s->launch_mu);
  HIP_TRY(s->sync.before_launch(stream, s->cam_gen));
  const int oi = dispatch_order(s, kind, c, stream);
  if (oi < 0) return RT_ERR_DEVICE;
  HIP_TRY(hipStreamSynchronize(stream));
  const rt_scene_dev::order_entry &e = s->orders[oi];
  uint32_t header[4];
  const rt_table_dev &T = e.Tb[s->cam_gen & 1u];
  HIP_TRY(hipMemcpy(header, T.header, sizeof header, hipMemcpyDeviceToHost));
  if (known_value(e.known, s->cam_gen) != header[0] + 1u) return fail(RT_ERR_STATE, "the build published %u entries to the host, its header says %u", known_value(e.known, s->cam_gen), header[0] + 1u);
  *n_workgroups = header[0];
  if (n_blocks) *n_blocks = e.n_blocks;
  if (out_entries) HIP_TRY(hipMemcpy(out_entries, T.entries, (size_t)((e.n_blocks + 7u) / 8u) * 8u * 16u, hipMemcpyDeviceToHost));
  return RT_OK;
}
#endif
