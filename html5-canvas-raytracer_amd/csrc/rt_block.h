// rt_block.h — what the product kernel's launch table states about ONE block of samples, written once for the host
// (rt_tables.cpp: build_launch_table, the CPU tests' oracle and the no-GPU probe) and for the device (rt_tables_gpu.hip: the
// table as the library builds it, one work-item per block).  Plain binary64, IEEE sqrt and division, no contraction (both
// translation units are compiled without it): the two builds give the same words.
//
// A block is the 32 x 8 pixels (x supersample) of one workgroup of the trace kernel.  The rays of its samples lie inside the
// circular cone around the box's centre direction that contains its four corner directions (half-angle alpha); a sphere with
// centre C (seen from the camera) and radius R is met by SOME ray of that cone only if the angle between the cone's axis and C
// is at most alpha + asin(R / |C|).  From that, with margins far above the kernel's rounding:
//   * touched    - can any sphere but the enclosing one show in the block?  If not, and the scene's background is a constant,
//                  the block is SKY: its workgroup stores the constant and traces nothing;
//   * candidates - the (at most two) loop-order spheres the block's primary rays can meet at all (count << 16 | second << 8 |
//                  first), or 0 = no statement: the kernel then tests those and skips its cull;
//   * shadow masks (at most two lights) - where can the block's primary hits lie?  On candidate sphere i at distances
//                  t(c) = c - sqrt(c^2 - k), c = d.C, which over the cone is the interval between t at the largest and at the
//                  smallest c, so inside the ball around the cone's axis point at the mid distance with radius^2 = (dt/2)^2 +
//                  2 t2 m (1 - cos alpha); sphere j can stand between such a point and light k only if the angle between
//                  (Q - L) and (C_j - L) is at most asin(rho / |Q - L|) + asin(R_j / |C_j - L|) and its nearest point is not
//                  beyond the patch.  The union over the block's candidates, per light, is a 16-bit set of loop-order sphere
//                  indices (0xffffffff = no statement: scan everything); with more than 16 loop spheres a light's set is stored
//                  as empty (0) or not (0xffff);
//   * checker cells (RT_TABLE_CELLS) - for a block with ONE candidate whose sampler is the sphere checker: which of its four 8-pixel
//                  columns lie, with every sample, inside one checker cell, and that cell's parity (rt_column_cell); bits 18..25 of
//                  the candidates' word; with RT_TABLE_AXES also which of the other columns lie inside one cell of ONE of the checker's
//                  two axes (rt_cells_word); bits 26..30;
//   * first-bounce set (RT_TABLE_FIRST_BOUNCE) - for a block of one or two candidates of which at least one is a mirror: the loop-order
//                  spheres a ray REFLECTED at a primary hit of the block can meet at all (rt_first_bounce_set); bit 31 and bits 18..30
//                  of the candidates' word, never beside checker cells;
//   * second node (RT_TABLE_SECOND_NODE) - for a block that states a first-bounce set: which of its candidates the walk of that set may leave
//                  out (a ray reflected at a mirror cannot be accepted at that mirror again: rt_self_clear), and whether nothing is left then - every
//                  reflected ray of the block ends on the background (rt_second_node_bits); bits 24..26 of word 1, which a block that is
//                  no sky run leaves free;
//   * cost       - 1 + the weights of the spheres whose screen rectangle (the primary-ray cull's) touches the block, + what its
//                  mirrors show of the scene's dearest spheres (rt_bounce_cost): what ranks the blocks dearest first.
#ifndef RT_BLOCK_H
#define RT_BLOCK_H

#include <math.h>
#include <stdint.h>

#include "rt_fdlibm.h"

#if defined(__HIPCC__)
#define RT_HD __host__ __device__
#else
#define RT_HD
#endif

#define RT_TABLE_SKY 1u          /* mark sky blocks */
#define RT_TABLE_MASKS 2u        /* shadow masks */
#define RT_TABLE_CANDS 4u        /* primary candidates */
#define RT_TABLE_WIDE 8u         /* more than 16 loop spheres: a light's set is empty (0) or not (0xffff) */
#define RT_TABLE_RANK 16u        /* list the blocks dearest first */
#define RT_TABLE_GEOMETRY 32u    /* the camera is usable for the cone test (finite, non-zero axis sums, positive projection distance) */
#define RT_TABLE_NO_SKY 64u      /* RT_FLAG_NO_SKY: the table holds no entry for sky blocks (their slots stay zero: no workgroup renders them) */
#define RT_TABLE_SKY_ONLY 128u   /* RT_FLAG_SKY_ONLY: the table holds ONLY the sky runs */
#define RT_TABLE_BOUNCE 256u     /* ranked launch of a scene with a sphere that both reflects and refracts: a block's cost also counts such spheres seen in its mirrors */
#define RT_TABLE_CELLS 512u      /* checker cells: word 3 also says which 8-pixel columns of a one-candidate block lie inside ONE checker cell (rt_column_cell) */
#define RT_TABLE_AXES 1024u      /* checker cells, per axis (with RT_TABLE_CELLS): a column that is NOT inside one cell may still lie inside one cell of ONE axis (rt_cells_word) */
#define RT_TABLE_FIRST_BOUNCE 2048u /* first-bounce sets: word 3 of a block whose candidates include a mirror also names the spheres its reflected rays can meet (rt_first_bounce_set) */
#define RT_TABLE_SECOND_NODE 4096u /* second node (with RT_TABLE_FIRST_BOUNCE): word 1 of an entry that states a first-bounce set also says what the node after the primary may skip (rt_second_node_bits) */
#define RT_TABLE_SECOND_DARK 8192u /* ... and (with shadow masks) whether anything can shadow that node's hits (rt_cand_second_dark).  HOST BUILD ONLY, set by the host probe alone: counted below what pays, the device build does not know it, no kernel reads it (docs/EVIDENCE.md) */
#define RT_SKY_RUN_MAX 32u       /* consecutive sky blocks of a row block that share ONE entry */
#define RT_CAND_MASK 0x3ffffu     /* word 3, bits 0..17: the candidates; what every reader of them keeps */
#define RT_CELL_SHIFT 18u        /* ... bits 18..21: column c (bit 18 + c) lies inside one checker cell; bits 22..25: that cell's parity; RT_TABLE_AXES: and bits 26..30, rt_cells_word */
// Word 3's bits 18..31 hold EITHER checker cells (bit 31 clear) OR a first-bounce set (bit 31 set; bit 18 + j: loop sphere j, at most 13 of them),
// never both: a set is only stated for an entry without a cell bit, and every candidate of a stating entry is a sphere of a scene without
// refraction - and without an enclosing sphere that reflects: that sphere is outside the loops, the candidates and this statement, and a lane
// of a stating block that misses every candidate meets it - at least one of them a mirror at a depth of 2 or more.  So an entry with bit 31 set is either not tried by the trace kernels' uniform-material path
// (two candidates) or - one candidate, which is then the mirror - turned away by that path's material test before it reads a cell bit.
#define RT_FB_STATED 0x80000000u  /* word 3, bit 31: bits 18..30 are the block's first-bounce set */
#define RT_FB_MAX_LOOP 13u        /* ... which names loop spheres 0..12: scenes of more state nothing */
// Word 1's bits 24..30 hold `run - 1` in a sky run's entry (bit 31 set) and are free in every other entry: an entry that states a first-bounce
// set says there what the node AFTER the primary may skip (RT_TABLE_SECOND_NODE; rt_second_node_bits).  Bits 27 and 28 say the same
// about that node's shadow scans (RT_TABLE_SECOND_DARK: the host probe's flag; the host build alone states them).
// WHO READS WHAT: the trace kernels read SELF0 and SELF1 and NOTHING ELSE.  SKY, DARK0 and DARK1 are held to the reference's rules by
// tests/test_second_node.py, but no GPU test covers a kernel that acts on them, because none does: a kernel that starts to read one owes its
// own byte-for-byte test first.
#define RT_SN_SHIFT 24u           /* word 1, bit 24 + ... */
#define RT_SN_SELF0 1u            /* ... 0: the walk of the set may leave out candidate 0 (word 3's bits 0..7) */
#define RT_SN_SELF1 2u            /* ... 1: and candidate 1 (bits 8..15; only beside a count of 2) */
#define RT_SN_SKY 4u              /* ... 2: the set without the candidates left out is empty - every reflected ray of the block meets no loop sphere (NO KERNEL READS IT: ending such rays at the primary node measured no gain, docs/EVIDENCE.md) */
#define RT_SN_DARK0 8u            /* ... 3: no loop sphere can stand between light 0 and any second-node hit of the block (rt_cand_second_dark; NO KERNEL READS IT, no launch's table states it) */
#define RT_SN_DARK1 16u           /* ... 4: the same for light 1 */
#define RT_SN_MASK 0x1fu          /* (bits 24..28: what a reader keeps) */
#define RT_COST_MAX 1023u        /* costs are clamped here (the ranking only has to order the blocks roughly) */

// a sphere as the cone test sees it (one per sphere but the enclosing one, scene order)
struct rt_ball {
  double c[3];                   // unit vector from the camera to the centre (the raw difference when `everywhere`)
  double o[3];                   // the centre
  double len, R, k;              // |centre - camera|, radius x (1 + 1e-7), len^2 - r^2 (with the TRUE radius: the tangent length bounds the hit distances)
  double sin_b, cos_b;           // of asin(R / len)
  double tangent;                // sqrt(max(k, 0)): the distance at which a ray from the camera grazes the sphere
  // as an OCCLUDER seen from light k (at most two lights matter for the masks): centre - light, its length wl, wl - R, and sin / cos of
  // asin(R / wl); `always`: the light is inside the sphere (or nothing finite can be said): it is in every set
  double lw[2][3], wl[2], wl_minus_R[2], s2[2], c2[2];
  uint32_t always[2];
  uint32_t loop;                 // index in the product kernel's loop order (enclosing sphere last)
  uint32_t everywhere;           // the camera is inside / on / too near: no statement about any block
  uint32_t bounce;               // cost ranking (RT_TABLE_BOUNCE, depth >= 3) and first-bounce sets (RT_TABLE_FIRST_BOUNCE, depth >= 2): bit 0 the sphere reflects, bit 1 it refracts
  uint32_t heavy;                // ... and its weight if it does BOTH (every hit a two-child node of the ray tree, main.js:268-278), else 0
  // checker cells (RT_TABLE_CELLS): the sphere's sampler is the checker with both frequencies in (0, 2^17] (the product kernel's range,
  // zero - stripes - left out); its frequencies and its TRUE radius (the kernel's normal is (h - o) / r)
  uint32_t checker, pad;
  double fu, fv, r;
};

// a sphere's screen rectangle on the workgroup grid and what a block that shows it is expected to cost
struct rt_cost_rect { double ys0, ys1; uint32_t tx0, tx1, weight, pad; };

struct rt_table_params {
  double as0, as1, as2;          // camera axis sums (main.js:187-191, quirk q1)
  double cam[3];
  double proj_w, proj_h, proj_d; // of the sample grid
  double epsilon;
  double lights[2][3];
  uint32_t tiles_x, ny, rb_per_tile;
  uint32_t tile_rows, tile_first, tile_stride, n_tiles;
  uint32_t ss, rows_per_wg, wg_w, wg_h;     // output rows / samples a workgroup covers
  uint32_t w, h;
  uint32_t n_balls, n_lights, n_rects, flags;
  uint32_t cost_bins;            // a block's cost lies in 1 .. cost_bins (1 when the launch is not ranked)
  uint32_t pad;
};

// first SAMPLE row of row block y of the launch
RT_HD inline double rt_block_row0(const rt_table_params &P, uint32_t y) {
  const uint32_t tile_i = y / P.rb_per_tile, rb = y - tile_i * P.rb_per_tile;
  return ((double)(P.tile_first + (uint64_t)tile_i * P.tile_stride) * P.tile_rows + (double)rb * P.rows_per_wg) * P.ss;
}

RT_HD inline uint32_t rt_block_cost(const rt_table_params &P, const rt_cost_rect *rects, uint32_t x, uint32_t y) {
  const double row0 = rt_block_row0(P, y);
  uint32_t cost = 2u;                                  // (sky runs are 1: the last class of a ranked table is theirs alone - a compact band's blocks are then 0 .. n - 1)
  for (uint32_t j = 0; j < P.n_rects; j++) {
    const rt_cost_rect &r = rects[j];
    if (x < r.tx0 || x > r.tx1) continue;
    if (row0 + P.wg_h <= r.ys0 || row0 > r.ys1) continue;
    cost += r.weight;
  }
  return cost < RT_COST_MAX ? cost : RT_COST_MAX;
}

// The statement of block (x, y) in pieces, so that the host (one block after the other, rt_block_statement below) and the device
// (rt_tables_gpu.hip: eight work-items per block, one sphere each) run the SAME operations on the same values and state the same words.

// the cone of the block's primary rays: unit axis, cos / sin of the half-angle; hit: the block counts as touched whatever the spheres
// say; doubt: nothing can be said about it (no geometry, or a box wider than a half space: never at these fields of view)
struct rt_cone { double ax[3], cos_a, sin_a; uint32_t hit, doubt; };

// ... of the samples X0 .. X1 x Y0 .. Y1 (sample centres, in the units of the reference's ray)
RT_HD inline rt_cone rt_box_cone(const rt_table_params &P, double X0, double X1, double Y0, double Y1) {
  rt_cone K;
  const double cx[4] = {X0, X1, X0, X1}, cy[4] = {Y0, Y0, Y1, Y1};
  double u[4][3], ax[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < 4; k++) {                      // the reference's ray: (s0 * X, s1 * Y, s2 * D), main.js:186-193 (q1)
    const double dx = P.as0 * cx[k], dy = P.as1 * cy[k], dz = P.as2 * P.proj_d, il = 1.0 / sqrt(dx * dx + dy * dy + dz * dz);
    u[k][0] = dx * il; u[k][1] = dy * il; u[k][2] = dz * il;
    for (int c = 0; c < 3; c++) ax[c] += u[k][c];
  }
  const double al = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  bool hit = !(al > 1e-3);                           // (a box wider than a half space)
  double cos_a = 1.0;
  if (!hit) {
    const double ial = 1.0 / al;
    for (int c = 0; c < 3; c++) ax[c] *= ial;
    for (int k = 0; k < 4; k++) cos_a = fmin(cos_a, ax[0] * u[k][0] + ax[1] * u[k][1] + ax[2] * u[k][2]);
    cos_a = fmax(cos_a - 1e-9, 0.0);                 // a slightly wider cone
    hit = !(cos_a > 1e-3);
  }
  K.ax[0] = ax[0]; K.ax[1] = ax[1]; K.ax[2] = ax[2];
  K.cos_a = cos_a; K.sin_a = sqrt(fmax(0.0, 1.0 - cos_a * cos_a));
  K.hit = K.doubt = hit ? 1u : 0u;
  return K;
}

RT_HD inline rt_cone rt_block_cone(const rt_table_params &P, uint32_t x, uint32_t y) {
  rt_cone K;
  K.ax[0] = K.ax[1] = K.ax[2] = 0.0; K.cos_a = 1.0; K.sin_a = 0.0; K.hit = 1u; K.doubt = 1u;
  if (!(P.flags & RT_TABLE_GEOMETRY)) return K;
  const double row0 = rt_block_row0(P, y);
  const double Y1 = (P.proj_h - 0.5) - row0, Y0 = Y1 - (double)(P.wg_h - 1u);
  const double X0 = (double)((uint64_t)x * P.wg_w) + (0.5 - P.proj_w), X1 = X0 + (double)(P.wg_w - 1u);
  return rt_box_cone(P, X0, X1, Y0, Y1);
}

// Cost ranking only: what a block's MIRRORS add to its cost.  The scene's dearest pixels are the hits on a sphere that both reflects and
// refracts (a binary ray tree: up to 31 nodes at depth 8) - and, after them, the pixels of OTHER spheres in which such a sphere is
// mirrored (measured, profiles/r04_ab_log.md: in the reference's own scene those blocks' waves ran 100-150 us, were ranked with the
// ordinary mirrors, started 100-140 us into a 200 us launch and WERE its last 70 us).  For candidate sphere ci of the block that
// reflects (or refracts): where the cone's axis meets it, the mirrored (or straight-through) direction there, a spread - the cone's
// half-angle magnified by the curvature, everything when the axis only grazes the sphere - and for every heavy sphere j the same
// angle test as everywhere else in this file.  A hit adds half of j's weight.  An estimate that only RANKS: no margin is owed,
// but host and device must compute the same number (plain binary64, no contraction, IEEE sqrt and division).
RT_HD inline uint32_t rt_bounce_cost(const rt_table_params &P, const rt_cone &K, const rt_ball *balls, uint32_t ci) {
  const rt_ball &B = balls[ci];
  if (!B.bounce || B.everywhere) return 0u;
  const double *ax = K.ax;
  const double cs = ax[0] * B.c[0] + ax[1] * B.c[1] + ax[2] * B.c[2], c = B.len * cs, disc = c * c - B.k;
  const bool graze = !(B.k > 0.0) || !(disc > 0.0);
  const double t = graze ? B.tangent : c - sqrt(disc);
  const double Q[3] = {P.cam[0] + t * ax[0], P.cam[1] + t * ax[1], P.cam[2] + t * ax[2]};
  double n[3] = {Q[0] - B.o[0], Q[1] - B.o[1], Q[2] - B.o[2]};
  const double nl = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  if (!(nl > 0.0)) return 0u;
  n[0] /= nl; n[1] /= nl; n[2] /= nl;
  const double cosi = -(ax[0] * n[0] + ax[1] * n[1] + ax[2] * n[2]);
  const bool wide = graze || !(cosi > 0.1);
  const double s_sig = wide ? 1.0 : fmin(1.0, K.sin_a * (1.0 + 2.0 * t / (B.R * cosi)) * 1.5 + 0.02), c_sig = sqrt(1.0 - s_sig * s_sig);
  const double s_thr = fmin(1.0, s_sig + 0.5), c_thr = sqrt(1.0 - s_thr * s_thr);          // straight through a refracting sphere: bent by up to ~30 degrees
  const double dr[3] = {ax[0] + 2.0 * cosi * n[0], ax[1] + 2.0 * cosi * n[1], ax[2] + 2.0 * cosi * n[2]};
  uint32_t extra = 0u;
  for (uint32_t j = 0; j < P.n_balls; j++) {
    const rt_ball &H = balls[j];
    if (!H.heavy || j == ci) continue;
    const double W[3] = {H.o[0] - Q[0], H.o[1] - Q[1], H.o[2] - Q[2]};
    const double wl = sqrt(W[0] * W[0] + W[1] * W[1] + W[2] * W[2]);
    if (!(wl > 0.0)) continue;
    const double sb = fmin(1.0, H.R / wl), cb = sqrt(1.0 - sb * sb);
    bool sees = false;
    if (B.bounce & 1u) sees = (dr[0] * W[0] + dr[1] * W[1] + dr[2] * W[2]) >= (c_sig * cb - s_sig * sb) * wl;
    if (!sees && (B.bounce & 2u)) sees = (ax[0] * W[0] + ax[1] * W[1] + ax[2] * W[2]) >= (c_thr * cb - s_thr * sb) * wl;
    if (sees) extra += H.heavy / 2u;
  }
  return extra;
}

// can some ray of the cone meet sphere B?  0: no; 1: yes (or NaN: touched); 2: the camera is inside / on / too near B - no statement
// about any block
RT_HD inline uint32_t rt_ball_touch(const rt_cone &K, const rt_ball &B) {
  if (B.everywhere) return 2u;
  const double cos_ab = K.cos_a * B.cos_b - K.sin_a * B.sin_b;          // cos(alpha + beta); alpha + beta < pi here
  const double cs = K.ax[0] * B.c[0] + K.ax[1] * B.c[1] + K.ax[2] * B.c[2];
  return (cs < cos_ab - 1e-7) ? 0u : 1u;             // untouched iff angle(axis, C) > alpha + beta, with a margin
}

// word 3 from the set of candidates (a bit per ball, at most 256; n_cand of them): count << 16 | loop index of the second << 8 |
// loop index of the first (in index order: the tie-break of the search), or 0
RT_HD inline uint32_t rt_cand_word(const rt_table_params &P, const rt_ball *balls, const uint64_t cand[4], uint32_t n_cand) {
  if (!(P.flags & RT_TABLE_CANDS) || n_cand == 0u || n_cand > 2u) return 0u;
  uint32_t idx[2] = {0u, 0u}, got = 0;
  for (uint32_t j = 0; j < P.n_balls && got < n_cand; j++) if (cand[j >> 6] >> (j & 63u) & 1ull) idx[got++] = balls[j].loop;
  uint32_t i0 = idx[0], i1 = n_cand > 1u ? idx[1] : 0u;
  if (n_cand > 1u && i1 < i0) { const uint32_t t = i0; i0 = i1; i1 = t; }
  return (n_cand << 16) | (i1 << 8) | i0;
}

// where the block's primary hits on candidate sphere B lie: inside the ball (Q, rho).  false: no statement can be made
struct rt_patch { double Q[3], rho; };
RT_HD inline bool rt_cand_patch(const rt_table_params &P, const rt_cone &K, const rt_ball &B, rt_patch *pt) {
  const double *ax = K.ax;
  const double cos_a = K.cos_a, sin_a = K.sin_a;
  // the primary hits on sphere ci: distances [t1, t2] along rays within alpha of the axis
  const double cs = fmin(1.0, fmax(-1.0, ax[0] * B.c[0] + ax[1] * B.c[1] + ax[2] * B.c[2])), sn = sqrt(1.0 - cs * cs);
  const double c_hi = B.len * ((cs * cos_a + sn * sin_a >= 1.0 || sn <= sin_a) ? 1.0 : cs * cos_a + sn * sin_a);
  const double c_lo = fmax(B.len * (cs * cos_a - sn * sin_a), B.tangent);
  // (the kernel takes the FAR root when the near one lies within epsilon of the origin, main.js:431-436: a camera that close
  // to a sphere gets no statement)
  if (!(B.k > 0.0) || !(c_hi * c_hi >= B.k) || !(c_hi >= c_lo) || !(B.len - B.R >= 2.0 * fabs(P.epsilon))) return false;
  const double t1 = (c_hi - sqrt(fmax(c_hi * c_hi - B.k, 0.0))) * (1.0 - 1e-6), t2 = (c_lo - sqrt(fmax(c_lo * c_lo - B.k, 0.0))) * (1.0 + 1e-6);
  if (!(t2 >= t1) || !(t1 >= 0.0) || !(t2 <= 1.7976931348623157e308)) return false;
  const double m = 0.5 * (t1 + t2);
  pt->rho = sqrt(0.25 * (t2 - t1) * (t2 - t1) + 2.0 * t2 * m * (1.0 - cos_a)) * (1.0 + 1e-6) + 1e-9 * t2;
  pt->Q[0] = P.cam[0] + m * ax[0]; pt->Q[1] = P.cam[1] + m * ax[1]; pt->Q[2] = P.cam[2] + m * ax[2];
  return true;
}

// candidate sphere ci, its primary hits inside the patch `pt`: which spheres can stand between them and light k - OR-ed into mk[k]
RT_HD inline void rt_cand_masks(const rt_table_params &P, const rt_patch &pt, const rt_ball *balls, uint32_t ci, uint32_t mk[2]) {
  const double *Q = pt.Q;
  const double rho = pt.rho;
  const bool wide = (P.flags & RT_TABLE_WIDE) != 0u;
  for (uint32_t k = 0; k < P.n_lights; k++) {
    if (wide && mk[k] == 0xffffu) continue;        // many spheres: a light's set is "empty or not", and it already is not
    const double V[3] = {Q[0] - P.lights[k][0], Q[1] - P.lights[k][1], Q[2] - P.lights[k][2]};
    const double dist = sqrt(V[0] * V[0] + V[1] * V[1] + V[2] * V[2]);
    // the patch seen from the light: a cone of half-angle asin(rho / dist) around V (the light inside the patch: every sphere)
    const bool patch_ok = (dist > rho * (1.0 + 1e-7)) && (dist <= 1.7976931348623157e308);
    const double s1 = patch_ok ? rho / dist : 0.0, c1 = sqrt(1.0 - s1 * s1), reach = (dist + rho) * (1.0 + 1e-7);
    for (uint32_t j = 0; j < P.n_balls; j++) {
      if (j == ci) continue;                       // a hit on sphere ci skips ci itself (main.js:294)
      const rt_ball &O = balls[j];
      bool inc = true;                             // light inside the occluder or the patch
      if (patch_ok && !O.always[k]) {
        // angle(V, W) <= asin(rho / dist) + asin(R / wl), as cosines scaled by |V| |W| (no division per sphere), and the occluder's
        // nearest point not beyond the patch
        const double cos12 = c1 * O.c2[k] - s1 * O.s2[k], vw = V[0] * O.lw[k][0] + V[1] * O.lw[k][1] + V[2] * O.lw[k][2];
        inc = !(vw < (cos12 - 1e-7) * (dist * O.wl[k])) && (O.wl_minus_R[k] <= reach);
      }
      if (inc) { if (wide) { mk[k] = 0xffffu; break; } mk[k] |= 1u << O.loop; }
    }
  }
}

// ... patch and masks in one step, for a caller that wants nothing else of the patch.  false: no statement can be made (the block's word is
// then 0xffffffff whatever the other candidates say)
RT_HD inline bool rt_cand_patch_masks(const rt_table_params &P, const rt_cone &K, const rt_ball *balls, uint32_t ci, uint32_t mk[2]) {
  rt_patch pt;
  if (!rt_cand_patch(P, K, balls[ci], &pt)) return false;
  rt_cand_masks(P, pt, balls, ci, mk);
  return true;
}

// First-bounce set (RT_TABLE_FIRST_BOUNCE).  Candidate sphere ci is a mirror, its primary hits lie inside the patch `pt` = (Q, rho): which
// loop spheres can a ray REFLECTED at such a hit meet at any t >= 0?  Returns their set (bit j: loop sphere j; ci itself is always in), or
// 0: no statement.  No estimate anywhere: every step is a bound, with the margins of this file's other tests.
//   normal     a hit h has h - o = qo + e, qo = Q - o, |e| <= rho: the normal lies within dn of n0 = qo / |qo|, sin dn = rho / |qo|
//              (rho < 0.7 |qo| is required: dn < 45 degrees);
//   direction  the primary direction lies within alpha of the cone's axis ax.  Reflection at a FIXED normal keeps the angle between two
//              directions; reflecting a FIXED direction at two normals dn apart gives results 2 dn apart (the two reflections differ by
//              a rotation of twice the normals' angle).  So every reflected direction lies within sigma = alpha + 2 dn of
//              r0 = ax - 2 (ax . n0) n0; sines and cosines by the addition formulas; sigma >= pi / 2: no statement;
//   sphere j   a reflected ray starts within rho of Q, so it meets sphere j at t >= 0 only if the ray from Q with the same direction meets
//              the ball (C_j, R_j (1 + 1e-7) + rho) at t >= 0: Q inside that ball, or angle(r0, C_j - Q) <= sigma + asin((R_j + rho) /
//              |C_j - Q|) - a sum below pi, tested as a cosine scaled by |C_j - Q|.
// (the cone of the reflected rays: axis r0, cos / sin of sigma; their origins lie within pt.rho of pt.Q.  false: no bound)
struct rt_fb_cone { double r0[3], c_sig, s_sig; };
RT_HD inline bool rt_first_bounce_cone(const rt_cone &K, const rt_patch &pt, const rt_ball &B, rt_fb_cone *F) {
  const double qo[3] = {pt.Q[0] - B.o[0], pt.Q[1] - B.o[1], pt.Q[2] - B.o[2]};
  const double lq = sqrt(qo[0] * qo[0] + qo[1] * qo[1] + qo[2] * qo[2]);
  if (!(pt.rho < 0.7 * lq) || !(lq <= 1.7976931348623157e308)) return false;
  const double s_dn = pt.rho / lq * (1.0 + 1e-7), c_dn = sqrt(1.0 - s_dn * s_dn);
  const double s_2dn = 2.0 * s_dn * c_dn, c_2dn = 1.0 - 2.0 * s_dn * s_dn;
  const double c_sig = (K.cos_a * c_2dn - K.sin_a * s_2dn) - 1e-7;                 // cos(alpha + 2 dn), a slightly wider cone
  if (!(c_sig > 0.0)) return false;
  F->c_sig = c_sig; F->s_sig = sqrt(1.0 - c_sig * c_sig);
  const double il = 1.0 / lq, n0[3] = {qo[0] * il, qo[1] * il, qo[2] * il};
  const double an = K.ax[0] * n0[0] + K.ax[1] * n0[1] + K.ax[2] * n0[2];
  F->r0[0] = K.ax[0] - 2.0 * an * n0[0]; F->r0[1] = K.ax[1] - 2.0 * an * n0[1]; F->r0[2] = K.ax[2] - 2.0 * an * n0[2];
  return true;
}
RT_HD inline uint32_t rt_first_bounce_set(const rt_table_params &P, const rt_patch &pt, const rt_fb_cone &F, const rt_ball *balls, uint32_t ci) {
  const rt_ball &B = balls[ci];
  const double *r0 = F.r0;
  const double c_sig = F.c_sig, s_sig = F.s_sig;
  uint32_t set = 1u << B.loop;
  for (uint32_t j = 0; j < P.n_balls; j++) {
    if (j == ci) continue;
    const rt_ball &O = balls[j];
    const double W[3] = {O.o[0] - pt.Q[0], O.o[1] - pt.Q[1], O.o[2] - pt.Q[2]};
    const double wl2 = W[0] * W[0] + W[1] * W[1] + W[2] * W[2], Rb = O.R + pt.rho;
    bool in = true;                                // Q inside the widened ball, or nothing finite can be said
    if (wl2 > Rb * Rb * (1.0 + 1e-6) && wl2 <= 1.7976931348623157e308) {
      // cos(sigma + beta) |W| with sin beta = Rb / |W|: cos beta |W| = sqrt(|W|^2 - Rb^2), sin beta |W| = Rb - one square root per sphere, no
      // division; the margin 1e-7 |W| taken from the 1-norm, which is no smaller
      const double w1 = fabs(W[0]) + fabs(W[1]) + fabs(W[2]);
      in = !(r0[0] * W[0] + r0[1] * W[1] + r0[2] * W[2] < (c_sig * sqrt(wl2 - Rb * Rb) - s_sig * Rb) - 1e-7 * w1);
    }
    if (in) set |= 1u << O.loop;
  }
  return set;
}
// Second node (RT_TABLE_SECOND_NODE).  A mirror B of a stating block is in the block's set because its own reflected rays start ON it: the walk
// at the node after the primary tests B with the reference's generic form (main.js:420-439) from the hit point h along the reflected direction
// d, and in exact arithmetic finds the roots t0 = 2 tca <= 0 and t1 = 0, neither of them >= epsilon.  rt_self_clear bounds what rounding can
// make of t1 - the kernels' rounding and the reference's alike (u = 1.2e-16 above the unit roundoff 2^-53; the product kernel's rsqrt, good to
// 4.1e-15 = 36 u, scales a direction and is counted where a scale reaches the result) - in terms of
//     S = |C| + R + |camera|_1 + |centre|_1,
// which is no smaller than any coordinate of h, than the hit distance t, than the sphere's radius r and than |C| = |centre - camera|.
//   primary discriminant  disc = tca^2 - (C.C - r^2) with tca = d0.C: the dot products, the square and the host's C.C - r^2 are each good to a few
//              u S^2; together dp = 16 u S^2.  Its square root thc is then off by min(sqrt(dp), dp / thc) - at grazing incidence, thc -> 0, the
//              error of the root is the SQUARE ROOT of the rounding - and the hit distance t = tca - thc by Dt <= that + 5 u S;
//   hit point  h = camera + d0 t is rounded per coordinate (<= 4 u S) and d0's scale moves it by 36 u t; sliding h along the ray by Dt moves
//              its distance from the centre by Dt thc / r + Dt^2 / (2 r) (thc = r cos(incidence)), which with the line above is at most
//              2 dp / r: the hit lies eta = 2 dp / r + 64 u S off the sphere at most.  eta <= r / 1000 is required (the normal (h - o) / r is
//              then a unit vector to 1e-3 and the reflection keeps the sign of d0.n);
//   direction  the reflected ray leaves the sphere: d.(o - h) = d0.(h - o) (1 + O(eta / r)), and d0.(h - o) = Dt - thc up to 64 u S, which is
//              positive only where thc < Dt <= dp / thc, i.e. by less than sqrt(dp).  So tca2 = d.(o - h) <= tau = sqrt(dp) + 64 u S;
//   second discriminant  disc2 = r^2 - (|o - h|^2 - tca2^2) = tca2^2 - (|o - h|^2 - r^2) + rounding, |o - h|^2 - r^2 >= -(2 r eta + eta^2), the
//              rounding of the three dot products, of the differences and of d's scale (72 u tca2^2) at most 128 u S^2:
//              disc2 <= tca2^2 + k, k = 2 r eta + eta^2 + 128 u S^2 - "the square root of rounding times r^2" once more;
//   far root   t1 = tca2 + sqrt(disc2) grows with tca2, so t1 <= tau + sqrt(tau^2 + k) <= 2 tau + sqrt(k); t0 <= tca2 <= tau.
// The statement is made when SIXTEEN times that bound (256 times the unit roundoff under the square roots) is still no more than epsilon:
// neither root can then reach epsilon and the test cannot accept.  For the reference's scene (S ~ 30, epsilon 1e-3) the bound is 7e-6; a
// mirror hundreds of units across or away, or an epsilon of 1e-6, states nothing.  The primary hit is the NEAR root of a camera outside the
// sphere: rt_cand_patch (a stating block has one) requires |C| - R >= 2 |epsilon|.
// The forms of the primary hit the bound was written against: the product kernels' anchored test (rt_kernel_trace.h: RT_ANCHORED, disc =
// fma(tca, tca, -Ca) with the host's Ca = C.C - r^2, h = p + d t) and the reference's generic one (disc = r^2 - (C.C - tca^2): the same terms,
// rounded in another order, inside the same dp), which the strict kernels and the C restatement run; the product kernels' square root and
// rsqrt as rt_kernel_math.h measures them (1.1e-16 and 4.1e-15).  A kernel that finds its primary hit another way - through a transformed
// ray, in lower precision - is outside the derivation and must not read the bits.
RT_HD inline bool rt_self_clear(const rt_table_params &P, const rt_ball &B) {
  const double u = 1.2e-16, r = B.R;
  const double S = B.len + r + (fabs(P.cam[0]) + fabs(P.cam[1]) + fabs(P.cam[2])) + (fabs(B.o[0]) + fabs(B.o[1]) + fabs(B.o[2]));
  if (!(r > 0.0) || !(S <= 1.7976931348623157e308)) return false;
  const double dp = 16.0 * u * S * S, eta = 2.0 * dp / r + 64.0 * u * S;
  if (!(eta <= 1e-3 * r)) return false;
  const double tau = sqrt(dp) + 64.0 * u * S, k = 2.0 * r * eta + eta * eta + 128.0 * u * S * S;
  return 16.0 * (2.0 * tau + sqrt(k)) <= P.epsilon;                // (a negative or NaN epsilon states nothing)
}
// ... of a block: what candidate ci keeps IN the walk - the other spheres its reflected rays can meet (s: its rt_first_bounce_set, 0 if it is no
// mirror or states none), and itself unless rt_self_clear holds.  OR-ed over the block's candidates: a candidate of the block's set that is
// in no candidate's keep may be left out.
RT_HD inline uint32_t rt_cand_second_keep(const rt_table_params &P, const rt_ball *balls, uint32_t ci, uint32_t s) {
  const rt_ball &B = balls[ci];
  if (!(P.flags & RT_TABLE_SECOND_NODE) || !s) return 0u;
  return (s & ~(1u << B.loop)) | (rt_self_clear(P, B) ? 0u : 1u << B.loop);
}
// ... of a block: OR `*set` over its candidates, one call each.  false: the block states no set (a candidate refracts, or a mirror among
// them has no patch or no bound); a candidate that does not reflect adds nothing (its hits spawn no ray); *keep: OR of rt_cand_second_keep
RT_HD inline bool rt_cand_first_bounce(const rt_table_params &P, const rt_cone &K, const rt_ball *balls, uint32_t ci, bool patch_ok, const rt_patch &pt, uint32_t *set, uint32_t *keep) {
  const rt_ball &B = balls[ci];
  if (B.bounce & 2u) return false;
  if (!(B.bounce & 1u)) return true;
  rt_fb_cone F;
  const uint32_t s = (patch_ok && rt_first_bounce_cone(K, pt, B, &F)) ? rt_first_bounce_set(P, pt, F, balls, ci) : 0u;
  *set |= s;
  *keep |= rt_cand_second_keep(P, balls, ci, s);
  return s != 0u;
}
// word 3's upper bits from the block's set (0: none of its candidates is a mirror), whether every candidate could be stated, and the
// word so far (candidates and checker cells)
RT_HD inline uint32_t rt_first_bounce_word(const rt_table_params &P, uint32_t cands, bool ok, uint32_t set) {
  if (!(P.flags & RT_TABLE_FIRST_BOUNCE) || !ok || !set || !(cands & RT_CAND_MASK) || (cands >> RT_CELL_SHIFT)) return 0u;
  return RT_FB_STATED | (set << RT_CELL_SHIFT);
}

// word 1's upper bits from word 3 (candidates and, if stated, the set) and the block's keep
RT_HD inline uint32_t rt_second_node_bits(const rt_table_params &P, uint32_t cands, uint32_t keep) {
  if (!(P.flags & RT_TABLE_SECOND_NODE) || !(cands & RT_FB_STATED)) return 0u;
  const uint32_t set = (cands >> RT_CELL_SHIFT) & ((1u << RT_FB_MAX_LOOP) - 1u), drop = set & ~keep;
  const uint32_t c0 = cands & 255u, c1 = (cands >> 8) & 255u, n = (cands >> 16) & 3u;
  uint32_t bits = 0u;
  if (c0 < RT_FB_MAX_LOOP && ((drop >> c0) & 1u)) bits |= RT_SN_SELF0;
  if (n == 2u && c1 < RT_FB_MAX_LOOP && ((drop >> c1) & 1u)) bits |= RT_SN_SELF1;
  if (!(set & ~drop)) bits |= RT_SN_SKY;
  return bits << RT_SN_SHIFT;
}

// DARK (RT_TABLE_SECOND_DARK, with RT_TABLE_SECOND_NODE and shadow masks) - HOST ONLY: rt_block_statement, the host's build, states it for the
// host probe (profiles/count_second_node.py counts with it; tests/test_second_node.py holds it); the device build neither calls nor compiles
// any of it, no launch's table carries the bits and no kernel reads them - counted below what pays (docs/EVIDENCE.md).  Where can the SECOND-node hits of mirror candidate ci lie on receiver sphere B, and which
// spheres can stand between them and light k?  rt_cand_patch, generalised from the camera's cone to the reflected rays' (origins within
// rho of Q, directions within sigma of r0): a hit is h = (Q + e) + t d, |e| <= rho, and t is the near root from Q of the sphere shifted by
// -e: c = d.(C - e) lies in |C| cos(angle +- sigma) +- rho, k = |C - e|^2 - r^2 in [(|C| - rho)^2 - R^2, (|C| + rho)^2 - r_lo^2] (R the widened
// radius, r_lo = R (1 - 2e-7) below the true one); t = k / (c + sqrt(c^2 - k)) grows with k and falls with c, so it lies between its values
// at (c_hi, k_lo) and (c_lo, k_hi).  EVERY ray must meet the sphere from outside (c_lo >= sqrt(k_hi), with room; origins 2 epsilon off it):
// a cone that grazes the receiver has no finite patch and nothing is stated.  The ball is rt_cand_patch's, around Q + m r0, plus rho.
inline bool rt_bounce_patch(const rt_table_params &P, const rt_patch &pt, const rt_fb_cone &F, const rt_ball &B, rt_patch *out) {
  const double W[3] = {B.o[0] - pt.Q[0], B.o[1] - pt.Q[1], B.o[2] - pt.Q[2]};
  const double len = sqrt(W[0] * W[0] + W[1] * W[1] + W[2] * W[2]), rho = pt.rho;
  if (!(len - B.R - rho >= 2.0 * fabs(P.epsilon)) || !(len <= 1.7976931348623157e308)) return false;
  const double cs = fmin(1.0, fmax(-1.0, (F.r0[0] * W[0] + F.r0[1] * W[1] + F.r0[2] * W[2]) / len)), sn = sqrt(1.0 - cs * cs);
  const double up = cs * F.c_sig + sn * F.s_sig;
  const double c_hi = len * ((up >= 1.0 || sn <= F.s_sig) ? 1.0 : up) + rho, c_lo = len * (cs * F.c_sig - sn * F.s_sig) - rho;
  const double r_lo = B.R * (1.0 - 2e-7), k_lo = (len - rho) * (len - rho) - B.R * B.R, k_hi = (len + rho) * (len + rho) - r_lo * r_lo;
  if (!(k_lo > 0.0) || !(c_lo >= sqrt(k_hi) * (1.0 + 1e-7)) || !(c_hi >= c_lo)) return false;
  const double t1 = (c_hi - sqrt(fmax(c_hi * c_hi - k_lo, 0.0))) * (1.0 - 1e-6), t2 = (c_lo - sqrt(fmax(c_lo * c_lo - k_hi, 0.0))) * (1.0 + 1e-6);
  if (!(t2 >= t1) || !(t1 >= 0.0) || !(t2 <= 1.7976931348623157e308)) return false;
  const double m = 0.5 * (t1 + t2);
  out->rho = sqrt(0.25 * (t2 - t1) * (t2 - t1) + 2.0 * t2 * m * (1.0 - F.c_sig)) * (1.0 + 1e-6) + 1e-9 * t2 + rho * (1.0 + 1e-6);
  out->Q[0] = pt.Q[0] + m * F.r0[0]; out->Q[1] = pt.Q[1] + m * F.r0[1]; out->Q[2] = pt.Q[2] + m * F.r0[2];
  return true;
}
// ... of mirror candidate ci with first-bounce set s: per light the spheres that can shadow a second-node hit on any receiver of s (its own
// sphere is no receiver when rt_self_clear holds), as mk[0] | mk[1] << 16; 0xffffffff: a receiver without a patch - no statement
inline uint32_t rt_cand_second_dark(const rt_table_params &P, const rt_patch &pt, const rt_fb_cone &F, const rt_ball *balls, uint32_t ci, uint32_t s) {
  uint32_t mk[2] = {0u, 0u};
  for (uint32_t j = 0; j < P.n_balls; j++) {
    const rt_ball &R = balls[j];
    if (!((s >> R.loop) & 1u)) continue;
    if (j == ci) { if (rt_self_clear(P, R)) continue; return 0xffffffffu; }
    rt_patch q;
    if (!rt_bounce_patch(P, pt, F, R, &q)) return 0xffffffffu;
    rt_cand_masks(P, q, balls, j, mk);
  }
  return mk[0] | (mk[1] << 16);
}
// ... of a block with a stated set: bits 27 / 28 of word 1 (each mirror candidate's patch, cone and set worked out once more: the host has the time)
inline uint32_t rt_block_second_dark(const rt_table_params &P, const rt_cone &K, const rt_ball *balls, const uint64_t cand[4]) {
  if (!(P.flags & RT_TABLE_SECOND_DARK) || !(P.flags & RT_TABLE_MASKS) || !P.n_lights) return 0u;
  uint32_t dark = 0u;
  for (uint32_t ci = 0; ci < P.n_balls; ci++) {
    if (!(cand[ci >> 6] >> (ci & 63u) & 1ull) || !(balls[ci].bounce & 1u)) continue;
    rt_patch pt;
    rt_fb_cone F;
    if (!rt_cand_patch(P, K, balls[ci], &pt) || !rt_first_bounce_cone(K, pt, balls[ci], &F)) return 0u;
    dark |= rt_cand_second_dark(P, pt, F, balls, ci, rt_first_bounce_set(P, pt, F, balls, ci));
  }
  return ((!(dark & 0xffffu) ? RT_SN_DARK0 : 0u) | ((P.n_lights >= 2u && !(dark >> 16)) ? RT_SN_DARK1 : 0u)) << RT_SN_SHIFT;
}

// Checker cells (RT_TABLE_CELLS).  A block with ONE candidate whose sampler is the sphere checker (main.js:126-133): do all the primary
// rays of column `col` of the block - the 8 x 8 pixels (supersample 2: the 16 x 4 samples) of one wave of the one-wave trace kernels -
// meet the candidate, and all inside the SAME checker cell?  Returns a set of RT_COL_* bits: RT_COL_U / RT_COL_V - every sample's u f_u
// (v f_v) lies inside ONE unit cell, RT_COL_U_ODD / RT_COL_V_ODD - that cell's index is odd; RT_COL_CELL (| RT_COL_ODD) - both hold, so
// all samples lie in one checker cell (of that parity).  0: no statement.
//   The hit point is bounded PER OBJECT AXIS, not by a ball: a floor column seen at a grazing angle is a strip, long in depth and a few
// centimetres across, and a ball around it hands the strip's length to every coordinate.
//   direction   the column's raw rays are (s0 X, s1 Y, s2 D), X in [X0, X1], Y in [Y0, Y1] (quirk q1: a box with the frame's axes as edges);
//               the length's range [L0, L1] follows from the ranges of (s0 X)^2 and (s1 Y)^2, and a component of the unit direction is
//               the raw component's interval over [L0, L1], each end times the reciprocal of the length that pushes it outwards;
//   distance    t = c - sqrt(c^2 - k), c = d.C (C: camera -> centre), decreasing in c; c = N / L with N = raw ray . C linear in X, Y - its
//               range is that of its four corner values - so c lies in [N_lo / L1, min(N_hi / L0, |C|)], N_lo > 0.  EVERY ray meets the
//               sphere: the column's cone (rt_box_cone) lies inside the silhouette, clear of the horizon, as before;
//   hit point   (h - o).a lies in (cam - o).a + [t1, t2] x [d_lo, d_hi].a (an interval product), t widened by 1e-6 relative and each end by
//               1e-9 t2 and the rounding of cam - o; v first: without RT_TABLE_AXES a column whose v cannot be stated is done;
//   v = asin(-(h - o).z / r) / pi + 1/2:   asin is monotonic; an end at or beyond a pole: no statement about v;
//   u = atan2(-(h - o).y, -(h - o).x) / 2 pi + 1/2:   the point (-(h - o).x, -(h - o).y) lies in a rectangle; one that contains or touches the
//               z axis, or the branch cut at +-pi: no statement about u.  Else the angle has no extremum inside the rectangle and is monotonic
//               along each edge: its range is attained at two corners, chosen by the rectangle's signs (d angle / dx = -y / rho^2,
//               d angle / dy = x / rho^2).
// An axis is stated when [lo f, hi f] lies inside one unit cell and at least `margin` off its ends: 2^-18, twice the kernel's prefilter
// band (RT_XY_INDEX in rt_kernel.hip: a fraction within 2^-20 below or 2^-19 above an integer; the scaled mark tolerance only acts INSIDE
// that band), plus 1e-10 f for the rounding of this bound and of the kernel's own u, v (a few ulp of 1/2, times f) - so no sample of a
// stated column can reach the precise test or the mark list on that axis.
// Plain binary64 and fdlibm's asin / atan2 restated (rt_fdlibm.h): the same bits on the host and on the device.
#define RT_COL_CELL 1u
#define RT_COL_ODD 2u
#define RT_COL_U 4u
#define RT_COL_U_ODD 8u
#define RT_COL_V 16u
#define RT_COL_V_ODD 32u
RT_HD inline void rt_block_place(const rt_table_params &P, uint32_t x, uint32_t y, uint32_t *w0, uint32_t *w1);
// lo f .. hi f inside one unit cell, `margin` off its ends: 1 | (the cell's index & 1) << 1, else 0
RT_HD inline uint32_t rt_axis_cell(double lo, double hi, double f) {
  const double x0 = lo * f, x1 = hi * f, mg = 3.814697265625e-06 + 1e-10 * f, k = floor(x0);
  if (!(x1 >= x0) || !(k >= 0.0) || !(k <= 4294967295.0) || !(x0 - k >= mg) || !((k + 1.0) - x1 >= mg)) return 0u;
  return 1u | (((uint32_t)k & 1u) << 1);
}
// (h - o).a for hit distances in [t1, t2] and the raw ray's component in [r0, r1]; i0 >= i1 > 0: the reciprocals of the length's ends
RT_HD inline void rt_axis_range(double r0, double r1, double i0, double i1, double t1, double t2, double cam, double o, double *lo, double *hi) {
  const double d_lo = r0 * (r0 >= 0.0 ? i1 : i0), d_hi = r1 * (r1 >= 0.0 ? i0 : i1);
  const double pad = 1e-9 * t2 + 4e-16 * (fabs(cam) + fabs(o)), e = cam - o;
  *lo = e + fmin(t1 * d_lo, t2 * d_lo) - pad; *hi = e + fmax(t1 * d_hi, t2 * d_hi) + pad;
}
// (not forced inline: inlined into the device build's row kernel it spills well over a hundred scalar registers there and the table build
// is slower than with the call: docs/EVIDENCE.md)
RT_HD inline uint32_t rt_column_cell(const rt_table_params &P, const rt_ball &B, uint32_t x, uint32_t y, uint32_t col) {
  if (!B.checker || B.everywhere) return 0u;
  uint32_t w0, w1;
  rt_block_place(P, x, y, &w0, &w1);
  if (((w0 >> 11) & 15u) != P.rows_per_wg) return 0u;            // a block only partly inside its tile or the frame
  const double row0 = rt_block_row0(P, y);
  const double Y1 = (P.proj_h - 0.5) - row0, Y0 = Y1 - (double)(P.wg_h - 1u);
  const uint32_t cw = P.wg_w / 4u;
  const double X0 = (double)((uint64_t)x * P.wg_w + (uint64_t)col * cw) + (0.5 - P.proj_w), X1 = X0 + (double)(cw - 1u);
  const rt_cone K = rt_box_cone(P, X0, X1, Y0, Y1);
  if (K.doubt) return 0u;
  // EVERY ray of the column's cone meets the sphere from outside: the cone lies inside the silhouette, clear of the horizon (d.C >= the
  // tangent length, with room).  (The kernel takes the FAR root when the near one lies within epsilon of the origin, main.js:431-436: a
  // camera that close to a sphere gets no statement.)
  const double cs = fmin(1.0, fmax(-1.0, K.ax[0] * B.c[0] + K.ax[1] * B.c[1] + K.ax[2] * B.c[2])), sn = sqrt(1.0 - cs * cs);
  if (!(B.k > 0.0) || !(B.len - B.R >= 2.0 * fabs(P.epsilon)) || !(B.r > 0.0)) return 0u;
  if (!(B.len * (cs * K.cos_a - sn * K.sin_a) >= B.tangent * (1.0 + 1e-7))) return 0u;
  // the raw rays' box, the length's range and the unit direction's components
  const double ax = P.as0 * X0, bx = P.as0 * X1, ay = P.as1 * Y0, by = P.as1 * Y1, rz = P.as2 * P.proj_d;
  const double rx0 = fmin(ax, bx), rx1 = fmax(ax, bx), ry0 = fmin(ay, by), ry1 = fmax(ay, by);
  const double qx0 = (rx0 <= 0.0 && rx1 >= 0.0) ? 0.0 : fmin(ax * ax, bx * bx), qx1 = fmax(ax * ax, bx * bx);
  const double qy0 = (ry0 <= 0.0 && ry1 >= 0.0) ? 0.0 : fmin(ay * ay, by * by), qy1 = fmax(ay * ay, by * by);
  const double L0 = sqrt(qx0 + qy0 + rz * rz) * (1.0 - 1e-15), L1 = sqrt(qx1 + qy1 + rz * rz) * (1.0 + 1e-15);
  if (!(L0 > 0.0) || !(L1 <= 1.7976931348623157e308)) return 0u;
  // the hit distances [t1, t2]: c = N / L, N linear over the box
  const double Cx = B.c[0] * B.len, Cy = B.c[1] * B.len, Cz = B.c[2] * B.len;
  const double n00 = ax * Cx + ay * Cy + rz * Cz, n10 = bx * Cx + ay * Cy + rz * Cz, n01 = ax * Cx + by * Cy + rz * Cz, n11 = bx * Cx + by * Cy + rz * Cz;
  const double N_lo = fmin(fmin(n00, n10), fmin(n01, n11)), N_hi = fmax(fmax(n00, n10), fmax(n01, n11));
  if (!(N_lo > 0.0)) return 0u;
  const double c_hi = fmin(N_hi / L0, B.len), c_lo = fmax(N_lo / L1, B.tangent);
  if (!(c_hi * c_hi >= B.k) || !(c_hi >= c_lo)) return 0u;
  const double t1 = (c_hi - sqrt(fmax(c_hi * c_hi - B.k, 0.0))) * (1.0 - 1e-6), t2 = (c_lo - sqrt(fmax(c_lo * c_lo - B.k, 0.0))) * (1.0 + 1e-6);
  if (!(t2 >= t1) || !(t1 >= 0.0) || !(t2 <= 1.7976931348623157e308)) return 0u;
  // h - o per axis (the reciprocal lengths' two roundings - 2e-16 of a component - vanish in the 1e-9 t2 added to each end)
  const double i0 = 1.0 / L0, i1 = 1.0 / L1;
  double wz0, wz1;
  rt_axis_range(rz, rz, i0, i1, t1, t2, P.cam[2], B.o[2], &wz0, &wz1);
  // v
  uint32_t sv = 0u;
  const double s_lo = -wz1 / B.r, s_hi = -wz0 / B.r;
  if (s_lo > -1.0 && s_hi < 1.0) sv = rt_axis_cell(fd_asin(s_lo) / (M_PI / 2.0) / 2.0 + 0.5, fd_asin(s_hi) / (M_PI / 2.0) / 2.0 + 0.5, B.fv);
  if (!(sv & 1u) && !(P.flags & RT_TABLE_AXES)) return 0u;         // no whole cell without v, and nobody asks for u alone
  // u: the rectangle [px0, px1] x [py0, py1] of (-(h - o).x, -(h - o).y)
  uint32_t su = 0u;
  double wx0, wx1, wy0, wy1;
  rt_axis_range(rx0, rx1, i0, i1, t1, t2, P.cam[0], B.o[0], &wx0, &wx1);
  rt_axis_range(ry0, ry1, i0, i1, t1, t2, P.cam[1], B.o[1], &wy0, &wy1);
  const double px0 = -wx1, px1 = -wx0, py0 = -wy1, py1 = -wy0;
  if ((py0 > 0.0 || py1 < 0.0 || px0 > 0.0) && px1 >= px0 && py1 >= py0) {        // neither the axis nor the branch cut
    const double xa = py1 < 0.0 ? px1 : px0, ya = xa > 0.0 ? py1 : py0;          // the corner of the largest angle
    const double xb = py0 > 0.0 ? px1 : px0, yb = xb > 0.0 ? py0 : py1;          // ... of the smallest
    const double phi_hi = fd_atan2(ya, xa) + 1e-12, phi_lo = fd_atan2(yb, xb) - 1e-12;
    if (phi_lo > -3.14159 && phi_hi < 3.14159) su = rt_axis_cell(phi_lo / M_PI / 2.0 + 0.5, phi_hi / M_PI / 2.0 + 0.5, B.fu);
  }
  uint32_t st = ((su & 1u) ? RT_COL_U | ((su & 2u) ? RT_COL_U_ODD : 0u) : 0u) | ((sv & 1u) ? RT_COL_V | ((sv & 2u) ? RT_COL_V_ODD : 0u) : 0u);
  if ((su & 1u) && (sv & 1u)) st |= RT_COL_CELL | (((su ^ sv) & 2u) ? RT_COL_ODD : 0u);
  return st;
}

// word 3's upper bits for a block whose word 3 names ONE candidate, ball ci: the four columns' statements
RT_HD inline uint32_t rt_cell_bits(uint32_t col, uint32_t st) { return ((st & 1u) << (RT_CELL_SHIFT + col)) | (((st >> 1) & 1u) << (RT_CELL_SHIFT + 4u + col)); }
// ... from the four columns' RT_COL_* sets, six bits per column (st4 = OR of rt_column_cell(col) << 6 col).  Bits 18..25 are the whole-cell
// statements, and what bits 18..21 say never depends on the option: bit 18 + c set means "column c lies inside ONE checker cell", and a
// reader that knows nothing of the per-axis statements (every trace kernel today) reads bit 22 + c only beside it.  RT_TABLE_AXES
// adds, for the columns WITHOUT a whole-cell statement, ONE axis' statement (a column that can state both axes has its whole cell
// stated); the entry names one axis for all its columns - the one more of them can state (a tie: u) -
//   bit 26 + c   column c lies inside one unit cell of that axis: a wave would have to work out the OTHER coordinate only;
//   bit 22 + c   (the parity slot, unused by a column without bit 18 + c) that cell's index & 1;
//   bit 30       the axis: 0 - u is stated (main.js:127), 1 - v (main.js:128).
// Without RT_TABLE_AXES bits 26..31 are zero, and bits 22..25 are only set beside their column's bit 18 + c.
RT_HD inline uint32_t rt_cells_word(const rt_table_params &P, uint32_t st4) {
  uint32_t bits = 0u, nu = 0u, nv = 0u;
  for (uint32_t col = 0; col < 4u; col++) {
    const uint32_t st = (st4 >> (6u * col)) & 63u;
    bits |= rt_cell_bits(col, st);
    if (!(st & RT_COL_CELL)) { nu += (st & RT_COL_U) ? 1u : 0u; nv += (st & RT_COL_V) ? 1u : 0u; }
  }
  if (!(P.flags & RT_TABLE_AXES) || nu + nv == 0u) return bits;
  const bool v = nv > nu;
  for (uint32_t col = 0; col < 4u; col++) {
    const uint32_t st = (st4 >> (6u * col)) & 63u;
    if ((st & RT_COL_CELL) || !(st & (v ? RT_COL_V : RT_COL_U))) continue;
    bits |= (1u << (RT_CELL_SHIFT + 8u + col)) | (((st & (v ? RT_COL_V_ODD : RT_COL_U_ODD)) ? 1u : 0u) << (RT_CELL_SHIFT + 4u + col));
  }
  return bits | (v ? 1u << (RT_CELL_SHIFT + 12u) : 0u);
}

// touched / candidates / shadow masks of block (x, y), one block after the other (the host); *touched = 1 also when nothing can be said
RT_HD inline void rt_block_statement(const rt_table_params &P, const rt_ball *balls, uint32_t x, uint32_t y, uint32_t *touched, uint32_t *cands_out, uint32_t *smask_out,
                                     uint32_t *bounce_extra, uint32_t *second_out) {
  *touched = 1u; *cands_out = 0u; *smask_out = 0xffffffffu; *bounce_extra = 0u; *second_out = 0u;
  const rt_cone K = rt_block_cone(P, x, y);
  bool hit = K.hit != 0u, doubt = K.doubt != 0u;
  if (!(P.flags & RT_TABLE_GEOMETRY)) return;
  // which spheres the cone can meet: a bit per ball (at most 256)
  uint64_t cand[4] = {0ull, 0ull, 0ull, 0ull};
  uint32_t n_cand = 0;
  for (uint32_t j = 0; j < P.n_balls && !doubt; j++) {
    const uint32_t t = rt_ball_touch(K, balls[j]);
    if (t == 2u) { hit = doubt = true; break; }
    if (t) { hit = true; cand[j >> 6] |= 1ull << (j & 63u); n_cand++; }
  }
  *touched = hit ? 1u : 0u;
  if (doubt || n_cand == 0u) return;
  *cands_out = rt_cand_word(P, balls, cand, n_cand);
  if ((P.flags & RT_TABLE_CELLS) && (*cands_out >> 16) == 1u)
    for (uint32_t ci = 0; ci < P.n_balls; ci++)
      if (cand[ci >> 6] >> (ci & 63u) & 1ull) {
        uint32_t st4 = 0u;
        for (uint32_t col = 0; col < 4u; col++) st4 |= rt_column_cell(P, balls[ci], x, y, col) << (6u * col);
        *cands_out |= rt_cells_word(P, st4);
      }
  if (P.flags & RT_TABLE_BOUNCE)
    for (uint32_t ci = 0; ci < P.n_balls; ci++) if (cand[ci >> 6] >> (ci & 63u) & 1ull) *bounce_extra += rt_bounce_cost(P, K, balls, ci);
  // shadow masks and first-bounce set: each candidate's patch worked out once for both (as the device build does)
  const bool want_masks = (P.flags & RT_TABLE_MASKS) != 0u;
  const bool want_fb = (P.flags & RT_TABLE_FIRST_BOUNCE) && (*cands_out & RT_CAND_MASK) && !(*cands_out >> RT_CELL_SHIFT);
  if (!want_masks && !want_fb) return;
  uint32_t mk[2] = {0u, 0u}, fb_set = 0u, fb_keep = 0u;
  bool masks_ok = want_masks, fb_ok = true;
  for (uint32_t ci = 0; ci < P.n_balls; ci++) {
    if (!(cand[ci >> 6] >> (ci & 63u) & 1ull)) continue;
    rt_patch pt;
    const bool patch_ok = rt_cand_patch(P, K, balls[ci], &pt);
    if (want_fb) fb_ok = rt_cand_first_bounce(P, K, balls, ci, patch_ok, pt, &fb_set, &fb_keep) && fb_ok;
    if (masks_ok) {
      if (!patch_ok) masks_ok = false; else rt_cand_masks(P, pt, balls, ci, mk);
      if (mk[0] == 0xffffu && mk[1] == 0xffffu) masks_ok = false;       // many spheres, both sets not empty: the word is 0xffffffff whatever follows
    }
  }
  if (want_fb) { *cands_out |= rt_first_bounce_word(P, *cands_out, fb_ok, fb_set); *second_out = rt_second_node_bits(P, *cands_out, fb_keep); }
#if !defined(__HIP_DEVICE_COMPILE__)
  if (want_fb && (*cands_out & RT_FB_STATED)) *second_out |= rt_block_second_dark(P, K, balls, cand);      // (the host probe's flag: rt_block_second_dark)
#endif
  if (masks_ok) *smask_out = mk[0] | (mk[1] << 16);
}

// the two words of an entry that describe WHERE its block is: word 0 = tile_x | rows_valid << 11 | first frame row << 15,
// word 1 = first row in this call's output band (| (run - 1) << 24 | sky << 31, or | rt_second_node_bits, added by the caller)
RT_HD inline void rt_block_place(const rt_table_params &P, uint32_t x, uint32_t y, uint32_t *w0, uint32_t *w1) {
  const uint32_t tile_i = y / P.rb_per_tile, rb = y - tile_i * P.rb_per_tile;
  const uint32_t trow0 = rb * P.rows_per_wg;                                             // first row of the block inside its tile
  const uint64_t frow0 = (uint64_t)(P.tile_first + (uint64_t)tile_i * P.tile_stride) * P.tile_rows + trow0;
  uint32_t rows_valid = 0;
  if (trow0 < P.tile_rows && frow0 < P.h) {
    rows_valid = P.rows_per_wg;
    if (P.tile_rows - trow0 < rows_valid) rows_valid = P.tile_rows - trow0;
    if (P.h - frow0 < rows_valid) rows_valid = (uint32_t)(P.h - frow0);
  }
  *w0 = (rows_valid << 11) | ((uint32_t)(frow0 < P.h ? frow0 : 0u) << 15) | x;              // frow0 < 65536 + 8: 17 bits
  *w1 = tile_i * P.tile_rows + trow0;                                                      // < 2^24 (checked by the caller): bits 24..31 are free
}

#endif
