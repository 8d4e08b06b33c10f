// rt_kernel.hip — the per-pixel ray-sphere trace/shade loop as ONE hand-written gfx950 kernel.
//
// What it computes, per output pixel (reference lines in /root/reference/main.js):
//   A1  primary ray                     :102-105, :186-193   (dist indexed by component, quirk q1)
//   A2  ray-sphere intersection         :420-451
//   A3  closest hit, strict <           :223-231
//   A4  reflection / A5 refraction      :233-266
//   A6  bounded recursion               :221, :268-278       (stackless forward fold, or explicit per-lane stack)
//   A7  lights, shadows, Phong          :280-318              (light_intensity shared across lights, q2)
//   A8  samplers (colour/texture/checker) :404, :343-351, :126-133
//   A9  combine + non-linear clamp      :320-336
//   A10 RGBA8 store                     :195-198              (Uint8ClampedArray: clamp, round-half-even)
//
// MI355X mapping (no MFMA: there is no dense contraction anywhere in this path; all arithmetic is
// binary64 VALU, which is what JS numbers are):
//   * one work-item per pixel (per SAMPLE when supersampling 2x2); a wave owns a compact 8x8 block so its
//     64 rays take the same branches; 4 waves side by side make a 32x8 workgroup tile = whole
//     128-byte framebuffer lines, each line written by exactly one workgroup (no cross-XCD sharing);
//     product kernel: a FLAT grid whose workgroups look their tile up in a launch table built on the GPU (one
//     s_load_dwordx4: no tile arithmetic, no division) that lists the tiles dearest first, so a launch ends
//     on cheap sky tiles (rt_scene.hip: dispatch_order); strict kernel: the plain 2-D grid;
//   * everything wave-uniform — camera, lights, loop bounds (kernarg) and the sphere tables walked by
//     the uniform object loops (typed address_space(4)) — is read with SCALAR loads into SGPRs: the
//     intersection loops issue no vector memory and no LDS instruction;
//   * the per-hit, per-lane data (material + sampler parameters of the sphere that lane hit, texture
//     descriptors), the primary-ray cull rectangles and the 10-double state of the stackless recursion
//     fold live in LDS; the LDS image is one contiguous block in HBM, loaded behind the ray generation (the few-sphere one-wave
//     kernels stage its materials alone and read descriptors and rectangles where they lie: six waves per SIMD, MTL_ONLY below);
//   * one-wave product kernels: a wave whose launch-table entry names ONE primary candidate and whose 64 rays all meet it (a floor
//     block) has ONE material record: it is read with scalar loads from the image in HBM and the wave shades on the uniform-material
//     path (trace_pixel, UNI) - no staging, no LDS access, no closest-hit selects, no node loop; the same statements otherwise;
//   * texels are plain global loads (gfx950 has no image/texture path); the two 128 KB textures stay
//     L2-resident;
//   * product kernel only: "anchored" line-sphere discriminants for primary rays (camera) and shadow
//     rays (walked from the light): 4 operations instead of 10; a wave-wide cull of primary-ray
//     candidates (__ballot over per-sphere screen rectangles); per-light shadow grids when the scene has
//     many spheres; an enclosing sphere (skybox) kept out of the loops; hardware rsq/rcp + Newton;
//   * divergent phases are exec-mask branches the compiler lowers to s_cbranch_execz; the bookkeeping of
//     a hit is pinned inside its branch, so a wave whose 64 rays all miss a sphere pays 4 FP64 operations
//     and one compare for it.
//
// The file is compiled twice (csrc/Makefile): RT_STRICT=0 with FMA contraction (the product kernels)
// and RT_STRICT=1 with -ffp-contract=off (operation for operation with the JS expression trees, IEEE
// sqrt/div, fdlibm atan2/asin, OCML pow, explicit recursion stack; RT_FLAG_STRICT_FP).  Both are held to <= 1 LSB on generic
// samples.  Samples whose outcome in the reference is decided by the last bit of its own arithmetic - a sampler coordinate
// within rounding of a texel / checker boundary, rays with an exactly-zero direction component (the centre row / column of an
// odd sample grid) that stay in a coordinate plane through sphere centres - can only be reproduced by the reference's own
// operation sequence.  The product kernels MARK the former while tracing (a list in HBM); the strict build has a second,
// list-driven kernel (rt_retrace) that traces the marked samples and the centre row / column again and stores over them
// (rt_launch.hip: render_batch_impl launches it unless it KNOWS that a frame of this scene, camera, size and tile set has neither).
// Scenes that sit on a coincidence as a whole (a light exactly on a surface, a camera with a zero axis sum:
// rt_scene_dev::needs_strict) take the strict kernels throughout.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rt_device.h"
#include "rt_block.h"      // the launch table's words (RT_CAND_MASK, RT_CELL_SHIFT)
#include "rt_wide.h"       // which lane stores which four pixels (the product kernels' 16-byte frame stores)

#ifndef RT_STRICT
#define RT_STRICT 0
#endif
#if RT_STRICT
#define RT_LAUNCH_NAME rt_launch_trace_strict
#define RT_SCRATCH_NAME rt_scratch_trace_strict
#else
#define RT_LAUNCH_NAME rt_launch_trace_fast
#define RT_SCRATCH_NAME rt_scratch_trace_fast
#endif

// Register budget: minimum waves per SIMD the kernel must fit (second __launch_bounds__ argument).
#ifndef RT_WAVES_PER_EU
#define RT_WAVES_PER_EU 2
#endif

// ... by instantiation, in ONE place.  The few-sphere one-wave kernels: 6 (80 VGPRs; with their 6 400 bytes of LDS, 24 workgroups
// per CU).  Measured on the headline by padding LDS (docs/EVIDENCE.md, "Six waves per SIMD"): 3 waves -27 %, 4 waves -11.5 %, 5 the
// parent, 6 waves +5 % spill-free (the compiler's own 6-wave build, 12 spilled registers: +3.4 % with the LDS budget, -1.6 % without).
// The reflection-only shadow-grid variants are held at 5 (96 VGPRs), the general kernel and the few-sphere four-wave forms are left
// free: they fit 96 on their own, and forcing the general kernel to 5 waves spills into its loops (-9 %).
constexpr unsigned rt_waves_per_eu(bool refract, bool grid, bool w1) {
  return (w1 && !grid && !refract) ? (RT_WAVES_PER_EU > 6 ? RT_WAVES_PER_EU : 6)
       : (refract || !grid)        ? RT_WAVES_PER_EU
                                   : (RT_WAVES_PER_EU > 5 ? RT_WAVES_PER_EU : 5);
}

#define RT_INF __builtin_inf()

namespace {

#include "rt_literal.h"          // the list head of rt_trace_rays: lit_ordered, lit_load_ray
#include "rt_kernel_math.h"      // v3, rt_sqrt / rt_rcp / rt_div / rt_pow*, rt_atan2_asin, to_byte, the stars hash
#include "rt_kernel_entry.h"     // rt_pixel_of, rt_entry_*, rt_cold_args, rt_mark_append
#include "rt_kernel_tables.h"    // rt_load_*, rt_mtl_*, rt_tex_desc, frame, park
#include "rt_kernel_trace.h"     // trace_pixel

#if !RT_STRICT
// The 16-byte frame stores of the product kernels (rt_wide.h says which lane stores what; rt_device.h: rt_wide_stores_of which launches
// take them).  `through`: write-through (sc1) - the line leaves L2 with the store instead of staying dirty until the end-of-kernel
// release writes the frame back while no SIMD has work.  A 16-byte sc1 store costs what a plain one does; a 4-byte one is a fabric
// write of its own, which is why the store's flavour comes with its shape.  (The asm ends in s_nop 1: the instruction behind it may
// not overwrite the data registers before the store has read them.)
typedef uint32_t __attribute__((ext_vector_type(4))) rt_px4;
__device__ __forceinline__ void rt_store16(uint32_t *p, rt_px4 v, bool through) {
  if (through) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(v) : "memory");
  else *(rt_px4 *)p = v;
}
// the value lane + N of this lane's 16-lane row holds (DPP row_shl:N)
template <int N>
__device__ __forceinline__ uint32_t rt_row_down(uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x100 + N, 0xf, 0xf, true); }
#endif

// W1: one-wave workgroups (rt_pixel_of), for the reflection-only variants.  A workgroup's waves are placed together: a 4-wave
// workgroup starts when its CU has room for all four, and where the waves of a launch differ in length freed slots wait for their
// neighbours - the dear two thirds of a 64-sphere frame kept 3 400 - 4 100 of the chip's 5 120 wave slots resident, the headline
// 4 550 - 4 720 (profiles/wave_timeline.py).  One wave per workgroup fills every slot as it frees.  The many-sphere variants stage
// nothing (64 spheres 2x2 -8.6 %, cfg5's frame -7.1 %); the few-sphere ones stage their image per wave, as 16-byte units - 8 spheres:
// two loads and two LDS stores per work-item, no barrier (headline -2.8 %, 8K -1.6 %; with the 8-byte staging loop of the four-wave
// form it was +0.5 %).  The general kernel keeps four waves (its 13-double fold state and image would leave a CU 16 one-wave
// workgroups), and so does the peer-store path (whole 128-byte lines across the workgroup's waves).  profiles/r04_ab_log.md section 8.
template <bool REFRACT, bool COUNT, bool SS2, bool GRID, bool W1 = false>
// Register budget: rt_waves_per_eu above.
__global__ void __launch_bounds__(W1 ? 64 : RT_WG_THREADS, rt_waves_per_eu(REFRACT, GRID, W1)) rt_trace(const rt_launch L) {
  static_assert(!W1 || (!REFRACT && !COUNT && !RT_STRICT), "one-wave workgroups: the reflection-only product variants");
  [[maybe_unused]] constexpr uint32_t WG_WAVES = W1 ? 1u : RT_WG_THREADS / 64u;
  constexpr uint32_t KT = W1 ? 64u : RT_WG_THREADS;            // work-items of this workgroup
  extern __shared__ double lds_raw[];
#if defined(RT_WAVE_LOG) && !RT_STRICT
  // measurement build: when this wave started, and where (nothing is kept in registers: the exit stamp recomputes its slot)
  if (unsigned long long *const wl = rt_cold_args()->wave_log; wl != nullptr && (threadIdx.x & 63u) == 0u) {
    unsigned long long *q = wl + ((size_t)(blockIdx.z * gridDim.x + blockIdx.x) * WG_WAVES + (threadIdx.x >> 6)) * 4u;
    q[0] = __builtin_amdgcn_s_memrealtime();
    q[2] = (unsigned long long)__builtin_amdgcn_s_getreg((4u) | (0u << 6) | (31u << 11)) | ((unsigned long long)__builtin_amdgcn_s_getreg((20u) | (0u << 6) | (31u << 11)) << 32);
    q[3] = rt_entry_index<W1>();
  }
#endif
  // ---- stage the per-workgroup tables into LDS: ONE contiguous image in HBM (materials | texture descriptors |
  //      cull rectangles, laid out exactly as the LDS copy), so a workgroup pays one memory latency, not three;
  //      the loads are issued first and land while the ray is being generated ----
  const uint32_t tid = threadIdx.x;
  const uint32_t mtl_words = L.n_objects * (uint32_t)(sizeof(rt_mtl) / 8);
  const uint32_t tex_words = 16u * 2u;               // RT_MAX_TEXTURES descriptors of 16 B
  const bool cull_lds_on = (!RT_STRICT && !COUNT) ? !GRID : (L.cull_in_lds != 0u);      // (see trace_pixel)
  const uint32_t cull_words = cull_lds_on ? L.n_objects * 4u : 0u;     // per-sphere screen rectangles of the primary-ray cull (few spheres)
  // The few-sphere one-wave kernels stage the MATERIALS alone (the image's first mtl_words): 8 spheres and the fold state are then
  // 6 400 bytes, so that 24 one-wave workgroups - six waves per SIMD - fit a CU's 160 KiB, where the whole image (6 912 bytes) admits 22
  // or 23.  Their texture descriptors are read where they lie in HBM (a textured hit's one 16-byte load, as in the many-sphere forms)
  // and the cull's rectangles from L.cull at their one use (trace_pixel: only a block whose entry names no candidate runs the cull).
  constexpr bool MTL_ONLY = W1 && !GRID;
  const uint32_t image_words = MTL_ONLY ? mtl_words : mtl_words + tex_words + cull_words;
  // The reflection-only many-sphere variants read materials and texture descriptors WHERE THEY ARE (HBM / L2 / L1: a 32-bit offset from
  // a uniform base) instead of staging 10 KB of them per workgroup: LDS is then the fold state alone, 20 KB instead of 30 - a
  // workgroup's LDS stays allocated until its slowest wave ends, and with 30 KB (five per CU) the dear two thirds of a launch kept
  // only 66-78 % of the wave slots resident - and there is no staging and no barrier.  64 spheres: -3.8 % (3840x2160), -2.1 % (2x2),
  // cfg5's full frame -2.6 % (profiles/r04_ab_log.md section 6).  (The general kernel keeps its image in LDS: it has no register to spare.)
  constexpr bool IMAGE_IN_LDS = RT_STRICT || COUNT || !(GRID && !REFRACT);
  const uint32_t lds_words = IMAGE_IN_LDS ? image_words : 0u;
  const double *__restrict__ image = (const double *)L.lds_image;
  // Few spheres (8: exactly one word per work-item): one 8-byte load each, a loop for the rest.  The many-sphere variant (64
  // spheres are 10.5 KB) moves 16 bytes per work-item and instruction, three 4 KB pieces unrolled with ALL their loads in flight
  // before the first is waited for, the loads themselves unconditional (the host pads the buffer to whole pieces, so a piece
  // that starts inside the image may be read to its end) behind a scalar test per piece: one memory latency per workgroup
  // and ~a tenth of the instructions of a word-by-word loop (profiles/r02_ab_log.md).
  typedef uint32_t __attribute__((ext_vector_type(4))) rt_u4;
  constexpr uint32_t RT_STAGE_PIECES = 3u;
  const uint32_t image_vec = image_words >> 1;                                     // 16-byte units (GRID: the image is whole units)
  [[maybe_unused]] rt_u4 piece[RT_STAGE_PIECES];
  [[maybe_unused]] double stage0 = 0.0;
  const auto stage_issue = [&](const uint32_t tid) __attribute__((always_inline)) {
    if constexpr (!IMAGE_IN_LDS) {
    } else if constexpr (GRID || W1) {           // (W1, few spheres: 8 spheres are 112 units - two loads per work-item of the one wave)
      const rt_u4 *__restrict__ image4 = (const rt_u4 *)L.lds_image;
#pragma unroll
      for (uint32_t i = 0; i < RT_STAGE_PIECES; i++) if (i * KT < image_vec) piece[i] = image4[tid + i * KT];
    } else {
      stage0 = (tid < image_words) ? image[tid] : 0.0;
    }
  };
  // The one-wave product kernels know a class of blocks whose waves need no LDS image at all (the uniform-material path below): they
  // read their launch-table entry first and issue the staging loads only for a wave that will use them.  Every other kernel
  // issues them here, ahead of everything.
  // (not the many-sphere 2x2 form, cfg5's: the path's scalar material costs that kernel a fifth spilled scalar register, one more
  // than tests/test_kernel_resources.py allows it)
  constexpr bool UNI_OK = W1 && !REFRACT && !COUNT && !RT_STRICT && !(GRID && SS2);
  if constexpr (!UNI_OK) stage_issue(tid);
  const rt_mtl *mtl = IMAGE_IN_LDS ? (const rt_mtl *)lds_raw : (const rt_mtl *)L.lds_image;
  const rt_texture_desc *tex = (IMAGE_IN_LDS && !MTL_ONLY) ? (const rt_texture_desc *)(lds_raw + mtl_words) : (const rt_texture_desc *)((const double *)L.lds_image + mtl_words);
  const rt_geom *cull_lds = (const rt_geom *)(lds_raw + mtl_words + tex_words);
  double *acc = lds_raw + lds_words + tid;   // fold state: 10 (general kernel: 13) x RT_WG_THREADS doubles, lane-major
  // Many spheres: the primary-ray cull's rectangle of sphere `lane` (the wave's first 64 spheres) comes straight from HBM / L2,
  // in flight while the ray is generated, and is no part of the LDS image: 64 spheres + the fold state then fit 32 KB, five
  // workgroups per CU instead of four (64-sphere scenes -12 %; with 8 spheres the extra vector load costs 3 %, so few
  // spheres keep their rectangles in the image)
  rt_geom cull0 = rt_geom{0.0, 0.0, 0.0, 0.0};
  if (!cull_lds_on) { const uint32_t lane0 = tid & 63u; cull0 = L.cull[lane0 < L.n_loop ? lane0 : 0u]; }

  // ---- which pixel / sample this work-item owns ----
  const uint32_t lane = tid & 63u;
  const rt_pixel P0 = rt_pixel_of<SS2, W1>(L, tid);
#if !RT_STRICT
  // (the few-sphere one-wave kernels: the launch-record fields of the prologue go out beside the entry's load - rt_kernel_entry.h)
  if constexpr (W1 && !REFRACT && !COUNT && !GRID) rt_head_batch(L);
  // workgroup-uniform: a block wholly past its tile's or the frame's last row - or no entry at all: while the host does not know how
  // many entries a table built on the GPU a moment ago has, it launches one workgroup per BLOCK, and the slots behind the last
  // entry are zero (rt_tables_gpu.hip)
  if (P0.rows_valid == 0u) return;
  // (RT_FLAG_NO_SKY / RT_FLAG_SKY_ONLY - a frame assembled from several GPUs' tiles: the OWNER fills the sky blocks of the whole frame,
  // the others do not send them over the links - are launch tables of their own, without the entries the launch leaves out: this
  // kernel knows nothing of it.  As a test of the launch record here it cost the headline 1.5 %.)
#endif
  // Blocks that show ONE sphere (word 3 of the entry: count 1 - a floor, a wall, a planet filling the view; nine in ten of the
  // headline's tracing waves): the wave tries the uniform-material path (trace_pixel, UNI) - that sphere's record in scalar registers,
  // no staging, no LDS access, no node loop.  A one-wave workgroup decides for itself: no barrier is involved.  The four-wave forms
  // (peer stores, a moved camera's first frame, the general kernel) do not take the path.
  [[maybe_unused]] bool uni_try = false;
  [[maybe_unused]] uint32_t cell = 0u;
  // The few-sphere one-wave kernels keep the wave's two decisions about its entry - a sky run; one candidate: try the path - as BITS of one
  // scalar word, set in nested branches and tested where each is used (s_bitcmp; s_cbranch_scc).  As booleans carried across the ray generation
  // they were lane masks: seven s_cselect_b64, two s_or_b64 and three branches through vcc in every wave (docs/EVIDENCE.md, "Scalar forms").
  // (The many-sphere one-wave kernel keeps the booleans: its code object is not part of this change.)
  constexpr bool WAVE_FLAGS = UNI_OK && !GRID;
  [[maybe_unused]] uint32_t wf = 0u;                      // bit 0: try the uniform-material path; bit 1: a sky run
  if constexpr (WAVE_FLAGS) {
    cell = (P0.cell >> rt_wave_of<W1>(tid)) & 0x11u;     // this wave's column of the block: bit 0 - inside one checker cell, bit 4 - the cell's parity
#ifdef RT_TESTING
    if (L.no_cells) cell = 0u;                          // test build (RT_NO_CHECKER_CELLS): every wave works its checker out per sample
#endif
    if (P0.sky) wf = 2u;
    else {
      if ((P0.cand >> 16) == 1u) wf = 1u;
#ifdef RT_TESTING
      if (L.no_uniform) wf = 0u;                        // test build (RT_NO_UNIFORM_BLOCKS): every wave on the general path
#endif
      if ((wf & 1u) == 0u) stage_issue(tid);
    }
    asm volatile("" : "+s"(wf));                        // opaque: a word in a scalar register, not two conditions
  } else
  if constexpr (UNI_OK) {
    uni_try = !P0.sky && (P0.cand >> 16) == 1u;
    if constexpr (!GRID) cell = (P0.cell >> rt_wave_of<W1>(tid)) & 0x11u;     // this wave's column of the block: bit 0 - inside one checker cell, bit 4 - the cell's parity
#ifdef RT_TESTING
    if (L.no_uniform) uni_try = false;                  // test build (RT_NO_UNIFORM_BLOCKS): every wave on the general path
    if (L.no_cells) cell = 0u;                          // test build (RT_NO_CHECKER_CELLS): every wave works its checker out per sample
#endif
    if (!uni_try && !P0.sky) stage_issue(tid);
  }
  // (tested at each use, through an opaque copy of the word: one condition shared by the uses would be carried between them as a lane mask again)
  const auto wf_bit0 = [&]() __attribute__((always_inline)) { uint32_t w_ = wf; asm volatile("" : "+s"(w_)); return (w_ & 1u) != 0u; };
#define RT_UNI_TRY() (WAVE_FLAGS ? wf_bit0() : uni_try)
  double rgb[3];
  uint32_t cnt[3] = {0u, 0u, 0u};
  // A workgroup the table build marked as showing no sphere (rt_block.h: the cone test, made once for the workgroup's
  // box) stores the background constant: no staging, no barrier, no ray, no cull.  (Staging loads issued above - the four-wave forms -
  // are simply never waited for.)  45 % of the headline's workgroups.
  // (WAVE_FLAGS: a sky run's wave skips the trace here and takes the constant in the epilogue, where its entry is read again - as a value that
  // meets the traced colour behind this block, the constant was copied into vector registers in front of it, by every wave)
  if (!WAVE_FLAGS && P0.sky) {
    rgb[0] = L.sky_rgb[0]; rgb[1] = L.sky_rgb[1]; rgb[2] = L.sky_rgb[2];
  } else if (!WAVE_FLAGS || (wf & 2u) == 0u) {
  const uint32_t px = P0.px, frow = P0.frow, sub = P0.sub;
  const uint32_t sx = SS2 ? 2u * px + (sub & 1u) : px;
  const uint32_t sy = SS2 ? 2u * frow + (sub >> 1) : frow;

  // ---- A1 primary ray (main.js:186-193); dist is indexed by component k, not by axis (q1) ----
#if RT_STRICT
  const double d0 = ((double)sx - L.proj_w) + 0.5, d1 = (L.proj_h - (double)sy) - 0.5, d2 = L.proj_d;
#else
  // the same numbers with one addition each: sx, sy are integers and proj_w, proj_h half-integers far below 2^52, so
  // sx + (0.5 - proj_w) and (proj_h - 0.5) - sy are exact, like the reference's two-step forms
  const double d0 = (double)sx + L.ray_bias[0], d1 = L.ray_bias[1] - (double)sy;
#endif
  const v3 o = mk(L.cam_origin[0], L.cam_origin[1], L.cam_origin[2]);
  double rl;
#if RT_STRICT
  const v3 target = mk(o.x + L.cam_axis_x[0] * d0 + L.cam_axis_y[0] * d0 + L.cam_axis_z[0] * d0,
                       o.y + L.cam_axis_x[1] * d1 + L.cam_axis_y[1] * d1 + L.cam_axis_z[1] * d1,
                       o.z + L.cam_axis_x[2] * d2 + L.cam_axis_y[2] * d2 + L.cam_axis_z[2] * d2);
  const v3 ray = unit(mk(target.x - o.x, target.y - o.y, target.z - o.z), &rl);
#else
  // target[k] - origin[k] = (axisX[k] + axisY[k] + axisZ[k]) * dist[k]; the sums come from the host
  // (its z component is axis_sum.z * projD: never the zero vector unless the camera is degenerate, and then the
  // reference divides by zero as well, so no zero-length select here)
  const v3 rawray = mk(L.cam_axis_sum[0] * d0, L.cam_axis_sum[1] * d1, L.ray_bias[2]);      // [2] = axis_sum.z * projD, from the host
  rl = rt_rsqrt_pos(dot(rawray, rawray));
  const v3 ray = mk(rawray.x * rl, rawray.y * rl, rawray.z * rl);
#endif

#ifdef RT_TESTING
  const bool is_probe = L.probe != nullptr && sx == L.probe_x && sy == L.probe_y && blockIdx.z == 0;
#else
  const bool is_probe = false;
#endif
  // finish the staging (first use of LDS: the cull table or the closest hit's material inside trace_pixel)
  const auto stage_finish = [&](const uint32_t tid) __attribute__((always_inline)) {
    if constexpr (!IMAGE_IN_LDS) {
    } else if constexpr (GRID || W1) {
      rt_u4 *lds4 = (rt_u4 *)lds_raw;
      const rt_u4 *__restrict__ image4 = (const rt_u4 *)L.lds_image;
#pragma unroll
      for (uint32_t i = 0; i < RT_STAGE_PIECES; i++) {
        const uint32_t k = tid + i * KT;
        if (i * KT < image_vec && k < image_vec) lds4[k] = piece[i];
      }
      for (uint32_t k = tid + RT_STAGE_PIECES * KT; k < image_vec; k += KT) lds4[k] = image4[k];     // more than 73 spheres (one-wave workgroups: 17)
    } else {
      if (tid < image_words) lds_raw[tid] = stage0;
      for (uint32_t k = tid + RT_WG_THREADS; k < image_words; k += RT_WG_THREADS) lds_raw[k] = image[k];
    }
  };
  // the uniform-material path: materials and texture descriptors where they lie in HBM, read with scalar loads.  A wave it turns
  // away (a horizon, a mirror, stars) has touched nothing yet: it stages now and takes the general path
  [[maybe_unused]] bool uni_done = false;
  if constexpr (UNI_OK) {
    if (RT_UNI_TRY()) {
      uni_done = trace_pixel<REFRACT, COUNT, GRID, SS2, false, W1, true>(L, (const rt_mtl *)L.lds_image, (const rt_texture_desc *)((const double *)L.lds_image + mtl_words), acc,
                                                                         cull_lds, cull0, lane, 0.0, 0.0, 0.0, 0.0, o, ray, rgb, cnt, is_probe, P0.cand | (cell << 24));
      if (!uni_done) {
        uint32_t tid4 = threadIdx.x;
        if constexpr (MTL_ONLY) tid4 = rt_lane_again(); else
        asm volatile("" : "+v"(tid4));                 // opaque: no address is kept in registers across the attempt
        stage_issue(tid4);
        stage_finish(tid4);
      }
#ifdef RT_TESTING
      else if (lane == 0u && L.uniform_waves != nullptr) {                                      // test build: waves that took the path ...
        atomicAdd(L.uniform_waves, 1ull);
        if (cell & 1u) atomicAdd(L.uniform_waves + 1, 1ull);                                     // ... and of those, the ones that took their checker cell from the table
      }
#endif
    }
  }
  if (!uni_done) {                                    // the general path: every wave that did not shade above
    if (!UNI_OK || !RT_UNI_TRY()) stage_finish(tid);
    if constexpr (IMAGE_IN_LDS) __syncthreads();

    // this wave's pixel block in the units of d0/d1 (every lane holds the same four numbers)
    const double bw = SS2 ? 15.0 : 7.0, bh = SS2 ? 3.0 : 7.0;
    const double lx = SS2 ? (double)(2u * ((lane >> 2) & 7u) + (sub & 1u)) : (double)(lane & 7u);
    const double ly = SS2 ? (double)(2u * (lane >> 5) + (sub >> 1)) : (double)(lane >> 3);
    // (a wave the uniform-material path turned away has an entry that names its candidate: it skips the cull, the only reader of the
    // block's rectangle - which is then not computed, so that d0 / d1 are not held in registers across that attempt)
    double blk_x0 = 0.0, blk_x1 = 0.0, blk_y0 = 0.0, blk_y1 = 0.0;
    if (!UNI_OK || !RT_UNI_TRY()) { blk_x0 = d0 - lx; blk_x1 = blk_x0 + bw; blk_y1 = d1 + ly; blk_y0 = blk_y1 - bh; }
    trace_pixel<REFRACT, COUNT, GRID, SS2, false, W1>(L, mtl, tex, acc, cull_lds, cull0, lane, blk_x0, blk_x1, blk_y0, blk_y1, o, ray, rgb, cnt, is_probe, P0.cand);
  }                                                    // if (!uni_done)
  }                                                    // else of if (P0.sky)
#undef RT_UNI_TRY

  // ---- A10 RGBA8 store ----
  uint32_t tid2 = threadIdx.x;
  if constexpr (W1 && !GRID) tid2 = rt_lane_again(); else
  asm volatile("" : "+v"(tid2));                       // opaque: recompute the pixel instead of keeping it live (see rt_pixel_of)
  const rt_pixel P1 = rt_pixel_of<SS2, W1>(L, tid2);
#if !RT_STRICT
  const uint32_t wide = rt_cold_args()->wide_stores;   // RT_WIDE_* (the 16-byte stores below) ...
  // ... used here with the launch-record fields every arm of the epilogue asks for first - scatter, rgb24, the width, `out` and the frame
  // stride - so that all their loads go out beside the entry's and its one wait covers them (rt_head_batch says why): the parent's
  // epilogue stood through four dependent scalar waits on its way to its stores.  (Loaded behind the trace: none is held across it.)
  asm volatile("" :: "s"(wide), "s"(L.scatter), "s"(L.rgb24), "s"(L.w), "s"(L.out), "s"(L.frame_stride));
#endif
  const uint32_t frame_i = blockIdx.z;
  const bool valid = P1.valid;
  // (WAVE_FLAGS: a sky run's colour is taken HERE - see the trace's head.  Until this line `rgb` is uninitialised in a sky run's wave, and set by
  // one of the two paths in every other wave: that rests on P1.sky == P0.sky, which holds because P1 is P0's entry read again - same slot of the
  // launch table, which no kernel writes while a launch that reads it runs - so the wave that skipped the trace is exactly the wave that stores
  // the constant)
  if constexpr (WAVE_FLAGS) { if (P1.sky) { rgb[0] = L.sky_rgb[0]; rgb[1] = L.sky_rgb[1]; rgb[2] = L.sky_rgb[2]; } }
  const uint32_t r8 = to_byte(rgb[0]), g8 = to_byte(rgb[1]), b8 = to_byte(rgb[2]);
  // scatter: every frame of the batch has its own destination (the frame buffer of the rank that owns it, peer-mapped
  // over xGMI) and rows go to their place in the FRAME, so nothing is left to exchange or to de-interleave; a tile row
  // is whole 128-byte lines written by one workgroup, which is what a remote store wants
#if RT_STRICT
  uint32_t *__restrict__ out = L.scatter ? L.out_frames[frame_i] : L.out + (size_t)frame_i * L.frame_stride;
  const uint32_t orow = L.scatter ? P1.frow : P1.lrow;
#endif
  uint32_t rgbw;                                       // this lane's pixel as 0x00BBGGRR
  if (!SS2) rgbw = r8 | (g8 << 8) | (b8 << 16);
  else {
    // 2x2 box filter across the 4 lanes of a quad: (a+b+c+d+2)>>2 per channel (10-bit fields); all four lanes end
    // up with the pixel
    uint32_t packed = r8 | (g8 << 10) | (b8 << 20);
    packed += __shfl_xor(packed, 1);
    packed += __shfl_xor(packed, 2);
    rgbw = (((packed & 1023u) + 2u) >> 2) | ((((packed >> 10) & 1023u) + 2u) >> 2 << 8) | ((((packed >> 20) & 1023u) + 2u) >> 2 << 16);
  }
  // A sky entry of the launch table stands for a RUN of consecutive 32-pixel blocks of one row block (rt_tables_gpu.hip): the
  // workgroup stores the same constant into each of them; every other workgroup stores its one block.
#if RT_STRICT
  const uint32_t n_run = 1u;
#else
  const uint32_t n_run = P1.sky ? P1.run : 1u;
#endif
#if defined(RT_ABLATE_STORE) && !RT_STRICT
  // timing experiment only (profiles/ab_build.sh <name> "-DRT_ABLATE_STORE" product, or "-DRT_ABLATE_STORE=2"): what a launch costs
  // WITHOUT its RGBA8 frame stores (2: without the sky runs' stores only).  The pixel is computed to its last instruction (the empty asm
  // uses it), and the stores stand behind a scalar test of a launch-record value that no launch has (grid z is below 65536) and the
  // compiler cannot know: none executes, none is removed.  No Makefile target defines it.  (Not tied to RT_TESTING, like
  // RT_ABLATE_QAMP: the test build's trace kernels run 23x the product's time, and a ceiling is priced on the product's kernels.)
  asm volatile("" :: "v"(rgbw));
  const bool store_off = ((RT_ABLATE_STORE + 0) == 2 ? P1.sky : true) && rt_cold_args()->n_frames != ~0u;
#endif
#if !RT_STRICT
  // 16 bytes per storing lane (rt_wide.h), where the host found every group of four pixels whole and aligned (rt_device.h:
  // rt_wide_stores_of) - such a launch is RGBA8 into the call's band, so this arm asks for neither rgb24 nor scatter.  The flags come
  // from the kernarg segment (rt_cold_args: no scalar register is held across the trace), read above beside the entry's load, whose
  // wait covers them and the arm's three launch-record fields.  Every other launch: the arms below, as they were.
  if (wide != 0u) {
    const uint32_t lane2 = tid2 & 63u, wave2 = rt_wave_of<W1>(tid2), pix = rgbw | 0xff000000u;
    const uint32_t px0 = P1.px & ~(RT_TILE_W - 1u);                                // the entry's first pixel: a block starts at a multiple of 32
    uint32_t *const band = L.out + (size_t)frame_i * L.frame_stride + (size_t)(P1.lrow - P1.trow) * L.w;     // ... and its first row in the call's output band
#if defined(RT_ABLATE_STORE)
    if (store_off) {} else
#endif
    if (P1.sky) {
      // a sky run: block t of the run is ONE instruction of wave t % 4 - eight whole 128-byte lines
      const rt_wide_piece wp = rt_wide_sky(lane2);
      const rt_px4 v = {pix, pix, pix, pix};
      for (uint32_t t = wave2; t < n_run; t += 4u) {
        const uint32_t px = px0 + t * RT_TILE_W + wp.col;
        if (wp.row < P1.rows_valid && px < L.w) rt_store16(band + (size_t)wp.row * L.w + px, v, (wide & RT_WIDE_THROUGH_SKY) != 0u);
      }
    } else {
      // a traced block: the wave's piece of a row is 8 pixels = two stores; a group's first lane collects the other three
      // pixels from its own 16-lane row
      const rt_wide_piece wp = rt_wide_traced(SS2, wave2, lane2);
      const rt_px4 v = {pix, rt_row_down<SS2 ? 4 : 1>(pix), rt_row_down<SS2 ? 8 : 2>(pix), rt_row_down<SS2 ? 12 : 3>(pix)};
      const uint32_t px = px0 + wp.col;
      if (wp.stores && wp.row < P1.rows_valid && px < L.w) rt_store16(band + (size_t)wp.row * L.w + px, v, (wide & RT_WIDE_THROUGH_TRACED) != 0u);
    }
  } else
#endif
  {
#if !RT_STRICT
  // (the product build asks for the destination here, behind the arm above, which has its own and never reads `scatter`)
  uint32_t *__restrict__ out = L.scatter ? L.out_frames[frame_i] : L.out + (size_t)frame_i * L.frame_stride;
  const uint32_t orow = L.scatter ? P1.frow : P1.lrow;
#endif
  if (!W1 && !L.rgb24 && L.scatter && !SS2) {          // workgroup-uniform (the host launches the four-wave variant for scatter stores)
    // Peer stores want whole lines: a wave's 8x8 block is eight 32-byte pieces, one per row, and memory on the far side
    // of an xGMI link has no L2 of ours in front of it to merge them.  So the workgroup transposes its 32x8 tile through
    // LDS - every lane parks its pixel in its own fold-state slot 0, dead by now - and each wave then stores two whole
    // 128-byte rows of the tile.
    uint32_t *tile = (uint32_t *)(lds_raw + lds_words);
    tile[2u * tid2] = rgbw;
    __syncthreads();
    const uint32_t xr = tid2 & 31u, rr = tid2 >> 5;     // this work-item's pixel of the tile in row-major order
    const uint32_t v = tile[2u * (((xr >> 3) << 6) + (rr << 3) + (xr & 7u))];
    const uint32_t lane2 = tid2 & 63u;
    const uint32_t dr = rr - (lane2 >> 3);              // row of the tile: difference in wrap-around arithmetic
    const uint32_t trow2 = P1.trow + dr, frow2 = P1.frow + dr;
    uint32_t px2 = P1.px - ((tid2 >> 6) * 8u + (lane2 & 7u)) + xr;
    for (uint32_t t = 0; t < n_run; t++, px2 += RT_TILE_W) {
#if RT_STRICT
      const bool row_ok2 = trow2 < L.tile_rows && frow2 < L.h;
#else
      const bool row_ok2 = trow2 < P1.rows_valid;      // rows of the block inside its tile and the frame (from the table entry)
#endif
      if (row_ok2 && px2 < L.w) out[(size_t)frow2 * L.w + px2] = v | 0xff000000u;
    }
  } else if (!L.rgb24) {                               // wave-uniform
    uint32_t pxq = P1.px;
#if defined(RT_ABLATE_STORE) && !RT_STRICT
    if (store_off) {} else
#endif
    for (uint32_t t = 0; t < n_run; t++, pxq += RT_TILE_W) {
#if RT_STRICT
      const bool validq = valid;
#else
      const bool validq = (pxq < L.w) && (P1.trow < P1.rows_valid);
#endif
      if (validq && P1.sub == 0u) out[(size_t)orow * L.w + pxq] = rgbw | 0xff000000u;
    }
  } else {
    // RT_FLAG_RGB24: the 8 pixels a wave holds of one row are 24 bytes = 6 words.  Word j of the group takes its bytes
    // from pixels p = j + j/3 and p + 1, shifted by (j mod 3) bytes; lanes j < 6 of the group store.  w % 4 == 0 (host
    // check), so a group at the right edge holds 8 or 4 pixels = 6 or 3 whole words and rows start word-aligned.
    const uint32_t lane2 = tid2 & 63u;
    const uint32_t slot = SS2 ? lane2 >> 2 : lane2;    // pixel slot in the wave; a row's 8 slots are consecutive
    const uint32_t j = slot & 7u, j3 = (j * 11u) >> 5; // j3 = j / 3 for j < 8
    const uint32_t p = (slot & ~7u) + j + j3, sh = (j - 3u * j3) * 8u;
    const uint32_t pn = (j < 6u) ? p + 1u : p;         // lanes 6,7 store nothing; keep their source lane inside the group
    const uint32_t lo = __shfl(rgbw, SS2 ? (p << 2) : p), hi = __shfl(rgbw, SS2 ? (pn << 2) : pn);
    const uint32_t word = (lo >> sh) | (hi << (24u - sh));
    uint32_t x0 = P1.px - j;                           // first pixel of the group (a multiple of 8)
    for (uint32_t t = 0; t < n_run; t++, x0 += RT_TILE_W) {
      const uint32_t in_row = (x0 + 8u <= L.w) ? 6u : ((x0 + 4u <= L.w) ? 3u : 0u);
#if RT_STRICT
      const bool row_ok = (P1.trow < L.tile_rows) && (P1.frow < L.h);
#else
      const bool row_ok = P1.trow < P1.rows_valid;
#endif
      if (!(row_ok && j < in_row && P1.sub == 0u)) continue;
      // RT_FLAG_COMPACT: the block whole, at its place in the LAUNCH (a compact band: rows of 32 pixels = 24 words, 8 - or 2 - of them)
      if (L.compact) out[(size_t)rt_entry_index<W1>() * (RT_TILE_W * 3u / 4u * (SS2 ? 2u : RT_TILE_H)) + P1.trow * (RT_TILE_W * 3u / 4u) + ((rt_wave_of<W1>(tid2) * 8u) >> 2) * 3u + j] = word;
      else out[((P1.lrow * L.w + x0) >> 2) * 3u + j] = word;
    }
  }
  }

#if defined(RT_WAVE_LOG) && !RT_STRICT
  if (unsigned long long *const wl = rt_cold_args()->wave_log; wl != nullptr && (tid2 & 63u) == 0u)
    wl[((size_t)(blockIdx.z * gridDim.x + blockIdx.x) * WG_WAVES + (tid2 >> 6)) * 4u + 1u] = __builtin_amdgcn_s_memrealtime();
#endif
  if (COUNT) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      unsigned long long v = valid ? cnt[c] : 0u;
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
      if ((tid2 & 63u) == 0) atomicAdd(&L.counters[c], v);
    }
  }
}

#if RT_STRICT
// rt_retrace - the second, list-driven launch of a product frame (strict build only).  Its items are
//   * the samples the product launch marked (L.marks: a sampler coordinate within rounding of a texel / checker boundary),
//   * the centre row and the centre column of an odd sample grid that fall into this call's tiles: x - w/2 + 0.5 == 0 there
//     (main.js:186), so the primary ray - and every ray it spawns that stays in that plane - lies in a coordinate plane through the
//     camera, a sphere centred on that plane is met with a normal component of exactly 0, and u or v lands exactly ON a boundary,
//   * every sample of the call when the list overflowed (or the test build asks for it);
// each is traced with the reference's own operation sequence - trace_pixel in ITEM mode: every sphere in the scene's own order,
// materials read from HBM, no wave-wide step (a wave's lanes hold unrelated samples) - and stored where the product launch
// stored it (band, RGB24 band, or its row of the frame in scatter mode).  With supersample 2 the pixel's four samples are all
// traced (the product launch kept only their average).  A grid-stride loop: the number of items is only known on the device.
// Work-item 0 clears the NEXT launch's counter and publishes this launch's count to the host (rt_launch.hip skips this launch from
// then on if a frame of this scene, camera, size and tile set has no item at all).
template <bool REFRACT, bool SS2>
__global__ void __launch_bounds__(RT_WG_THREADS) rt_retrace(const rt_launch L) {
  const uint32_t count = L.marks[L.marks_slot];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    L.marks[L.marks_slot ^ 1u] = 0u;
    if (L.marks_known) __hip_atomic_store(L.marks_known, ((unsigned long long)L.known_tag << 32) | (count + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const uint32_t band_rows = L.n_tiles * L.tile_rows;
  const bool everything = count > L.marks_cap || L.retrace_all != 0u;
  const unsigned long long n_list = everything ? 0ull : count;
  const unsigned long long n_row = (!everything && L.centre_row != ~0u) ? (unsigned long long)L.w * L.n_frames : 0ull;
  const unsigned long long n_col = (!everything && L.centre_col != ~0u) ? (unsigned long long)band_rows * L.n_frames : 0ull;
  const unsigned long long n_all = everything ? (unsigned long long)band_rows * L.w * L.n_frames : 0ull;
  const unsigned long long total = n_list + n_row + n_col + n_all;
  const unsigned long long *list = (const unsigned long long *)(L.marks + 4);
  const rt_mtl *mtl = (const rt_mtl *)L.lds_image;                         // (HBM: nothing is staged here)
  const rt_texture_desc *tex = (const rt_texture_desc *)((const char *)L.lds_image + (size_t)L.n_objects * sizeof(rt_mtl));
  // supersample 2: the four samples of an item's pixel in four adjacent lanes (a quad: the same item, the same control flow), their
  // bytes summed across the quad - a marked sample of a many-sphere scene is a deep tree, and four of them one after the other were
  // 0.35 ms of a 0.34 ms frame (profiles/r04_ab_log.md)
  constexpr unsigned long long SUBS = SS2 ? 4ull : 1ull;
  for (unsigned long long ii = (unsigned long long)blockIdx.x * RT_WG_THREADS + threadIdx.x; ii < total * SUBS; ii += (unsigned long long)gridDim.x * RT_WG_THREADS) {
    const unsigned long long i = ii / SUBS;
    uint32_t px, frow, lrow, f;
    bool have_lrow = false;
    lrow = 0u;
    if (i < n_list) {
      const unsigned long long e = list[i];
      const uint32_t sx = (uint32_t)(e & 0xfffffu), sy = (uint32_t)((e >> 20) & 0xfffffu);
      f = (uint32_t)(e >> 40);
      px = SS2 ? sx >> 1 : sx; frow = SS2 ? sy >> 1 : sy;
    } else if (i < n_list + n_row) {
      const unsigned long long k = i - n_list;
      f = (uint32_t)(k / L.w); px = (uint32_t)(k - (unsigned long long)f * L.w); frow = L.centre_row;
    } else {
      unsigned long long k = i - n_list - n_row;
      if (!everything) { f = (uint32_t)(k / band_rows); lrow = (uint32_t)(k - (unsigned long long)f * band_rows); px = L.centre_col; }
      else { f = (uint32_t)(k / ((unsigned long long)band_rows * L.w)); k -= (unsigned long long)f * band_rows * L.w; lrow = (uint32_t)(k / L.w); px = (uint32_t)(k - (unsigned long long)lrow * L.w); }
      const uint32_t tile_i = lrow / L.tile_rows, trow = lrow - tile_i * L.tile_rows;
      frow = (L.tile_first + tile_i * L.tile_stride) * L.tile_rows + trow;
      have_lrow = true;
    }
    if (!have_lrow) {                                    // the row's place in this call's band, if the call renders it at all
      const uint32_t t = frow / L.tile_rows;
      if (t < L.tile_first || (t - L.tile_first) % L.tile_stride != 0u || (t - L.tile_first) / L.tile_stride >= L.n_tiles) continue;
      lrow = ((t - L.tile_first) / L.tile_stride) * L.tile_rows + (frow - t * L.tile_rows);
    }
    if (px >= L.w || frow >= L.h || f >= L.n_frames) continue;
    uint32_t sum[3] = {0u, 0u, 0u};
    const uint32_t sub = (uint32_t)(ii % SUBS);
    {
      const uint32_t sx = SS2 ? 2u * px + (sub & 1u) : px, sy = SS2 ? 2u * frow + (sub >> 1) : frow;
      // A1 primary ray (main.js:186-193), literally
      const double d0 = ((double)sx - L.proj_w) + 0.5, d1 = (L.proj_h - (double)sy) - 0.5, d2 = L.proj_d;
      const v3 o = mk(L.cam_origin[0], L.cam_origin[1], L.cam_origin[2]);
      const v3 target = mk(o.x + L.cam_axis_x[0] * d0 + L.cam_axis_y[0] * d0 + L.cam_axis_z[0] * d0,
                           o.y + L.cam_axis_x[1] * d1 + L.cam_axis_y[1] * d1 + L.cam_axis_z[1] * d1,
                           o.z + L.cam_axis_x[2] * d2 + L.cam_axis_y[2] * d2 + L.cam_axis_z[2] * d2);
      double rl;
      const v3 ray = unit(mk(target.x - o.x, target.y - o.y, target.z - o.z), &rl);
      double rgb[3];
      uint32_t cnt[3] = {0u, 0u, 0u};
      trace_pixel<REFRACT, false, false, SS2, true>(L, mtl, tex, nullptr, nullptr, rt_geom{0.0, 0.0, 0.0, 0.0}, 0u, 0.0, 0.0, 0.0, 0.0, o, ray, rgb, cnt, false, 0u, sx, sy, f);
      sum[0] += to_byte(rgb[0]); sum[1] += to_byte(rgb[1]); sum[2] += to_byte(rgb[2]);
    }
    if (SS2) {
      uint32_t packed = sum[0] | (sum[1] << 10) | (sum[2] << 20);
      packed += __shfl_xor(packed, 1);
      packed += __shfl_xor(packed, 2);
      sum[0] = ((packed & 1023u) + 2u) >> 2; sum[1] = (((packed >> 10) & 1023u) + 2u) >> 2; sum[2] = (((packed >> 20) & 1023u) + 2u) >> 2;
      if (sub != 0u) continue;
    }
    if (L.scatter) L.out_frames[f][(size_t)frow * L.w + px] = sum[0] | (sum[1] << 8) | (sum[2] << 16) | 0xff000000u;
    else if (!L.rgb24) L.out[(size_t)f * L.frame_stride + (size_t)lrow * L.w + px] = sum[0] | (sum[1] << 8) | (sum[2] << 16) | 0xff000000u;
    else if (!L.compact) {
      uint8_t *o8 = (uint8_t *)(L.out + (size_t)f * L.frame_stride) + ((size_t)lrow * L.w + px) * 3u;
      o8[0] = (uint8_t)sum[0]; o8[1] = (uint8_t)sum[1]; o8[2] = (uint8_t)sum[2];
    } else {
      // a compact band: the sample's block is workgroup b of the product launch - class start + entries of its class in the rows
      // above + its rank in the row (rt_tables_gpu.hip: rt_table_emit) -, its pixel row r, column i of the block's 32 x RH pixels
      const uint32_t RH = SS2 ? 2u : RT_TILE_H, y = lrow / RH, x = px / RT_TILE_W, at = y * L.tiles_x + x;
      const uint32_t it = L.tb_item[at];
      if (!it || (it >> 16)) continue;                     // (inside a run of sky blocks: a compact band holds none)
      const uint32_t bin = (it & 0xffffu) - 1u, b = L.tb_bin_start[bin] + L.tb_row_hist[(size_t)y * L.tb_bins + bin] + L.tb_rank_in_row[at];
      uint8_t *o8 = (uint8_t *)(L.out + (size_t)f * L.frame_stride) + (size_t)b * (RT_TILE_W * 3u * RH) + ((size_t)(lrow - y * RH) * RT_TILE_W + (px - x * RT_TILE_W)) * 3u;
      o8[0] = (uint8_t)sum[0]; o8[1] = (uint8_t)sum[1]; o8[2] = (uint8_t)sum[2];
    }
  }
}

// rt_trace_rays - caller-supplied rays (include/rt_hip.h: rt_scene_trace_rays_device; strict build only).  One work-item per record
// {org[3], dir[3]} of the list, a grid-stride loop; ray j is intersectWorld(L.segs, objects, org, dir) (main.js:216-336) with the
// direction as given - trace_pixel in ITEM mode, as rt_retrace runs it: every sphere in the scene's own order with the generic
// discriminant, materials read from HBM, no launch table, no cull, nothing anchored at a camera, and no wave-wide step (a wave's
// lanes hold unrelated rays).  The stars sampler's pix is the ray's index in the caller's list, ray_base + j (below 2^31: it is handed
// over as sample x of row 0).
// `order` (rt_scene_trace_rays_ordered_device; NULL: the list's own order): work-item j takes ray i = order[j] instead of ray j - it
// reads record i, hands over pix = ray_base + i and stores at i, so every output is what the plain launch puts there, and only which
// rays share a wave changes.  An entry >= n_rays is skipped.  The pointer is a kernel argument of its own, not a field of rt_launch:
// the frame kernels' argument segment stays as it is.  With an order the loads and stores below are gathers and scatters of whole
// records.
// Memory: a record is 48 bytes and the list 16-byte aligned - three 16-byte loads per lane; rgba is one dword per lane (a wave stores
// 256 contiguous bytes), rgb three 8-byte stores.  A ray with a non-finite component is not traced (NaN x 3; the store rule makes
// 0, 0, 0, 255 of it): what the caller supplies decides no address here - sphere, texel and checker indices come out of comparisons
// that NaN fails (no hit), a truncation that is clamped (texel) and to_int32_bit0 (0 or 1) for every finite ray, whatever overflows
// on the way down the tree - and the guard keeps that argument to finite inputs.
template <bool REFRACT>
__global__ void __launch_bounds__(RT_WG_THREADS) rt_trace_rays(const rt_launch L, const uint32_t *order) {
  const rt_mtl *mtl = (const rt_mtl *)L.lds_image;                         // (HBM: nothing is staged here)
  const rt_texture_desc *tex = (const rt_texture_desc *)((const char *)L.lds_image + (size_t)L.n_objects * sizeof(rt_mtl));
  for (uint32_t item = blockIdx.x * RT_WG_THREADS + threadIdx.x; item < L.n_rays; item += gridDim.x * RT_WG_THREADS) {
    uint32_t j;
    if (!lit_ordered(order, item, L.n_rays, &j)) continue;                 // (an order's entry that names no ray)
    const lit_ray R = lit_load_ray(L.rays, j);
    double rgb[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
    if (R.finite) {
      uint32_t cnt[3] = {0u, 0u, 0u};
      trace_pixel<REFRACT, false, false, false, true>(L, mtl, tex, nullptr, nullptr, rt_geom{0.0, 0.0, 0.0, 0.0}, 0u, 0.0, 0.0, 0.0, 0.0, mk(R.ox, R.oy, R.oz),
                                                      mk(R.rx, R.ry, R.rz), rgb, cnt, false, 0u, L.ray_base + j, 0u, 0u);
    }
    if (L.ray_rgb) { double *o = L.ray_rgb + 3u * (size_t)j; o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2]; }
    if (L.ray_rgba) L.ray_rgba[j] = to_byte(rgb[0]) | (to_byte(rgb[1]) << 8) | (to_byte(rgb[2]) << 16) | 0xff000000u;
  }
}
#endif

}  // namespace

// ---- host side: this translation unit's kernels by variant (rt_device.h: rt_trace_variant), and their launch ----
#if RT_STRICT
#define RT_KERNEL_NAME rt_kernel_trace_strict
#else
#define RT_KERNEL_NAME rt_kernel_trace_fast
#endif
// The ONE place that names this build's instantiations: one line each.  NULL: the variant is not this build's (or no launch has it).
// The host's scratch query (rt_api.hip: variant_scratch) and the launcher below both go by this address.
extern "C" const void *RT_KERNEL_NAME(rt_trace_variant v) {
  struct row { rt_trace_variant v; const void *kernel; };
#define RT_TRACE(R, C, S, G, W1) {{RT_STRICT != 0, false, false, R, C, S, G, W1}, (const void *)&rt_trace<R, C, S, G, W1>}
  static const row table[] = {                      // (the code object lists its kernels in the order of these rows)
#if !RT_STRICT
    // GRID: the shadow-grid variant, a separate instantiation so that scenes with few spheres do not carry its registers (the host
    // leaves the cull rectangles out of the LDS image exactly for the scenes that have a shadow grid or a bounce table).
    // GRID, one-wave workgroups (reflection only): SS2
    RT_TRACE(false, false, false, true, true),   RT_TRACE(false, false, true, true, true),
    // GRID, four-wave workgroups: REFRACT x SS2
    RT_TRACE(false, false, false, true, false),  RT_TRACE(false, false, true, true, false),
    RT_TRACE(true, false, false, true, false),   RT_TRACE(true, false, true, true, false),
    // few spheres, one-wave workgroups (reflection only): SS2
    RT_TRACE(false, false, false, false, true),  RT_TRACE(false, false, true, false, true),
    // few spheres, four-wave workgroups: REFRACT x SS2
    RT_TRACE(false, false, false, false, false), RT_TRACE(false, false, true, false, false),
    RT_TRACE(true, false, false, false, false),  RT_TRACE(true, false, true, false, false),
    // counting: REFRACT x SS2
    RT_TRACE(false, true, false, false, false),  RT_TRACE(false, true, true, false, false),
    RT_TRACE(true, true, false, false, false),   RT_TRACE(true, true, true, false, false),
#else
    // rt_retrace: REFRACT x SS2
    {{true, true, false, false, false, false, false, false}, (const void *)&rt_retrace<false, false>},
    {{true, true, false, false, false, true, false, false}, (const void *)&rt_retrace<false, true>},
    {{true, true, false, true, false, false, false, false}, (const void *)&rt_retrace<true, false>},
    {{true, true, false, true, false, true, false, false}, (const void *)&rt_retrace<true, true>},
    // rt_trace_rays: REFRACT
    {{true, false, true, false, false, false, false, false}, (const void *)&rt_trace_rays<false>},
    {{true, false, true, true, false, false, false, false}, (const void *)&rt_trace_rays<true>},
    // rt_trace: REFRACT x COUNT x SS2
    RT_TRACE(false, false, false, false, false), RT_TRACE(false, false, true, false, false),
    RT_TRACE(true, false, false, false, false),  RT_TRACE(true, false, true, false, false),
    RT_TRACE(false, true, false, false, false),  RT_TRACE(false, true, true, false, false),
    RT_TRACE(true, true, false, false, false),   RT_TRACE(true, true, true, false, false),
#endif
  };
#undef RT_TRACE
  for (const row &r : table) if (rt_variant_bits(r.v) == rt_variant_bits(v)) return r.kernel;
  return nullptr;
}

// Launch of the variant's kernel.  A frame launch (rt_trace): the grid comes from the record - flat (L->grid_x workgroups, one per
// launch-table entry: the product launch) or the plain grid (x: 32-pixel tiles across the frame; y: tiles x row blocks of 8 rows, or 2
// when supersampling; z: frames) - with lds_bytes of dynamic LDS.  A list-driven launch (rt_retrace, rt_trace_rays): n_wg workgroups;
// `order` is rt_trace_rays' second argument (NULL or n_rays entries).  Returns a hipError_t as int.
extern "C" int RT_LAUNCH_NAME(const rt_launch *L, rt_trace_variant v, unsigned n_wg, const uint32_t *order, unsigned lds_bytes, hipStream_t stream) {
  const void *f = RT_KERNEL_NAME(v);
  if (!f) return (int)hipErrorInvalidDeviceFunction;
  dim3 grid(L->grid_x ? L->grid_x : (L->order ? L->tiles_x * L->n_tiles * L->rb_per_tile : L->tiles_x),
            L->grid_y ? L->grid_y : (L->order ? 1u : L->n_tiles * L->rb_per_tile), L->n_frames), block(RT_WG_THREADS);
  if (v.retrace || v.rays) { grid = dim3(n_wg ? n_wg : 1u); lds_bytes = 0u; }
  // one-wave workgroups (rt_pixel_of, W1): four per table entry, whole groups of eight entries (the slots behind the last entry are
  // zero: their workgroups leave at once)
  else if (v.one_wave) { grid = dim3(((grid.x + 7u) / 8u) * 32u, 1u, L->n_frames); block = dim3(64u); }
  void *args[] = {(void *)L}, *args_rays[] = {(void *)L, (void *)&order};          // (`order` is rt_trace_rays' alone)
  (void)hipLaunchKernel(f, grid, block, v.rays ? args_rays : args, lds_bytes, stream);
  return (int)hipGetLastError();
}
