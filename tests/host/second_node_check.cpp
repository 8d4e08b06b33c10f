// second_node_check - the second-node statement of csrc/rt_block.h (rt_self_clear, rt_cand_second_keep, rt_bounce_patch, rt_cand_second_dark,
// rt_second_node_bits) on a CPU, stand-alone: tests/test_second_node.py builds this with the host compiler, -ffp-contract=off and
// -fsanitize=address,undefined and runs it.  It states every block of a few small frames of hand-made scenes - two mirrors and a matte
// sphere over a floor, two lights - through rt_block_statement with every flag set, for ordinary cameras and for inputs chosen to reach the
// edges of the arithmetic (an epsilon of 0, below 0, NaN and tiny; coordinates of 1e150 and 1e300, whose squares leave the range; a camera
// on a sphere; a mirror that touches its neighbour; zero radius), and holds each word to the bits' own rules:
//   no bit without a stated set; SELF1 only beside two candidates; a dropped candidate is a candidate of the set; SKY exactly when
//   nothing is left of the set; DARK k only for a light that exists; nothing at all when epsilon cannot carry the bound.
// Prints the number of blocks stated and of each bit; exit status 1 on a broken rule.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "rt_block.h"

struct sphere { double o[3], r; uint32_t bounce; };

static rt_ball ball_of(const double cam[3], const double lights[2][3], uint32_t n_lights, const sphere &s, uint32_t loop) {
  rt_ball B;
  memset(&B, 0, sizeof B);
  for (int c = 0; c < 3; c++) { B.o[c] = s.o[c]; B.c[c] = s.o[c] - cam[c]; }
  B.len = sqrt(B.c[0] * B.c[0] + B.c[1] * B.c[1] + B.c[2] * B.c[2]);
  B.R = s.r * (1.0 + 1e-7);
  B.k = B.len * B.len - s.r * s.r;
  B.loop = loop;
  B.everywhere = (!(s.r > 0.0) || !(B.len <= 1.7976931348623157e308) || !(B.R <= 1.7976931348623157e308) || !(B.len > B.R * (1.0 + 1e-7))) ? 1u : 0u;
  if (!B.everywhere) { for (int c = 0; c < 3; c++) B.c[c] /= B.len; B.sin_b = B.R / B.len; B.cos_b = sqrt(1.0 - B.sin_b * B.sin_b); }
  B.tangent = sqrt(fmax(B.k, 0.0));
  B.bounce = s.bounce;
  for (uint32_t k = 0; k < n_lights; k++) {
    for (int c = 0; c < 3; c++) B.lw[k][c] = B.o[c] - lights[k][c];
    B.wl[k] = sqrt(B.lw[k][0] * B.lw[k][0] + B.lw[k][1] * B.lw[k][1] + B.lw[k][2] * B.lw[k][2]);
    B.always[k] = (!(B.wl[k] > B.R * (1.0 + 1e-7)) || !(B.wl[k] <= 1.7976931348623157e308)) ? 1u : 0u;
    B.wl_minus_R[k] = B.wl[k] - B.R;
    B.s2[k] = B.always[k] ? 0.0 : B.R / B.wl[k];
    B.c2[k] = sqrt(1.0 - B.s2[k] * B.s2[k]);
  }
  return B;
}

static unsigned long long g_blocks, g_stating, g_bit[5];

// one frame of w x h pixels: every block through rt_block_statement; false: a rule is broken
static bool frame(const char *name, const double cam[3], double scale, double eps, uint32_t n_lights, const std::vector<sphere> &sp, uint32_t w, uint32_t h, bool expect_nothing) {
  rt_table_params P;
  memset(&P, 0, sizeof P);
  P.as0 = -1.0; P.as1 = 1.0; P.as2 = -1.0;
  for (int c = 0; c < 3; c++) P.cam[c] = cam[c] * scale;
  P.proj_w = 0.5 * w; P.proj_h = 0.5 * h; P.proj_d = 0.5 * h / tan(0.5 * 0.7853981633974483);
  P.epsilon = eps;
  const double lights[2][3] = {{5.0 * scale, 10.0 * scale, 5.0 * scale}, {5.0 * scale, 10.0 * scale, 0.0}};
  for (uint32_t k = 0; k < n_lights; k++) for (int c = 0; c < 3; c++) P.lights[k][c] = lights[k][c];
  P.tiles_x = (w + 31u) / 32u; P.ny = (h + 7u) / 8u; P.rb_per_tile = P.ny;
  P.tile_rows = h; P.tile_first = 0u; P.tile_stride = 1u; P.n_tiles = 1u;
  P.ss = 1u; P.rows_per_wg = 8u; P.wg_w = 32u; P.wg_h = 8u; P.w = w; P.h = h;
  P.n_lights = n_lights; P.cost_bins = 1u;
  P.flags = RT_TABLE_SKY | RT_TABLE_MASKS | RT_TABLE_CANDS | RT_TABLE_GEOMETRY | RT_TABLE_FIRST_BOUNCE | RT_TABLE_SECOND_NODE | RT_TABLE_SECOND_DARK;
  std::vector<rt_ball> balls;
  for (size_t j = 0; j < sp.size(); j++) {
    sphere s = sp[j];
    for (int c = 0; c < 3; c++) s.o[c] *= scale;
    s.r *= scale;
    balls.push_back(ball_of(P.cam, lights, n_lights, s, (uint32_t)j));
  }
  P.n_balls = (uint32_t)balls.size();
  for (uint32_t y = 0; y < P.ny; y++)
    for (uint32_t x = 0; x < P.tiles_x; x++) {
      uint32_t touched, cands, smask, extra, second;
      rt_block_statement(P, balls.data(), x, y, &touched, &cands, &smask, &extra, &second);
      g_blocks++;
      const uint32_t sn = second >> RT_SN_SHIFT;
      bool ok = (second & ~(RT_SN_MASK << RT_SN_SHIFT)) == 0u;
      if (!(cands & RT_FB_STATED)) ok = ok && sn == 0u;
      else {
        g_stating++;
        const uint32_t set = (cands >> RT_CELL_SHIFT) & ((1u << RT_FB_MAX_LOOP) - 1u), n = (cands >> 16) & 3u, c0 = cands & 255u, c1 = (cands >> 8) & 255u;
        uint32_t drop = 0u;
        if (sn & RT_SN_SELF0) drop |= 1u << c0;
        if (sn & RT_SN_SELF1) { ok = ok && n == 2u; drop |= 1u << c1; }
        ok = ok && (drop & ~set) == 0u && (((sn & RT_SN_SKY) != 0u) == ((set & ~drop) == 0u));
        for (uint32_t j = 0; j < P.n_balls; j++) if ((drop >> j) & 1u) ok = ok && (balls[j].bounce & 1u);
        if (n_lights < 2u) ok = ok && !(sn & RT_SN_DARK1);
        if (n_lights < 1u) ok = ok && !(sn & RT_SN_DARK0);
        if (expect_nothing) ok = ok && sn == 0u;
        for (int b = 0; b < 5; b++) g_bit[b] += (sn >> b) & 1u;
      }
      if (!ok) { fprintf(stderr, "%s: block (%u, %u): candidates %08x, second-node word %08x break a rule\n", name, x, y, cands, second); return false; }
    }
  return true;
}

int main() {
  const double nan = NAN;
  const std::vector<sphere> scene = {{{-1.5, 1.0, 0.0}, 1.0, 1u}, {{1.5, 1.0, 0.0}, 1.0, 1u}, {{0.0, 2.5, -2.0}, 0.5, 0u}, {{0.0, -500.0, 0.0}, 500.0, 0u}};
  std::vector<sphere> touching = scene;
  touching[1].o[0] = 0.5;                                 // the second mirror touches the first
  std::vector<sphere> flat = scene;
  flat[0].r = 0.0;                                        // a sphere of radius zero
  const double cam[3] = {0.0, 1.5, 10.0}, near_cam[3] = {-1.5, 1.0, 1.0 + 1e-9}, inside[3] = {-1.5, 1.0, 0.0};
  bool ok = true;
  ok = ok && frame("h8-like", cam, 1.0, 1e-3, 2u, scene, 3840u, 2160u, false);
  ok = ok && frame("one light", cam, 1.0, 1e-3, 1u, scene, 320u, 180u, false);
  ok = ok && frame("no light", cam, 1.0, 1e-3, 0u, scene, 320u, 180u, false);
  ok = ok && frame("ragged", cam, 1.0, 1e-3, 2u, scene, 333u, 187u, false);
  ok = ok && frame("touching mirrors", cam, 1.0, 1e-3, 2u, touching, 320u, 180u, false);
  ok = ok && frame("zero radius", cam, 1.0, 1e-3, 2u, flat, 320u, 180u, false);
  ok = ok && frame("camera on a mirror", near_cam, 1.0, 1e-3, 2u, scene, 160u, 90u, false);
  ok = ok && frame("camera inside a mirror", inside, 1.0, 1e-3, 2u, scene, 160u, 90u, false);
  ok = ok && frame("epsilon 0", cam, 1.0, 0.0, 2u, scene, 320u, 180u, true);
  ok = ok && frame("epsilon < 0", cam, 1.0, -1e-3, 2u, scene, 320u, 180u, true);
  ok = ok && frame("epsilon NaN", cam, 1.0, nan, 2u, scene, 320u, 180u, true);
  ok = ok && frame("epsilon 1e-12", cam, 1.0, 1e-12, 2u, scene, 320u, 180u, true);
  ok = ok && frame("epsilon huge", cam, 1.0, 1e300, 2u, scene, 320u, 180u, false);
  ok = ok && frame("scale 1e4", cam, 1e4, 1e-3, 2u, scene, 320u, 180u, true);
  ok = ok && frame("scale 1e150", cam, 1e150, 1e-3, 2u, scene, 160u, 90u, true);
  ok = ok && frame("scale 1e300", cam, 1e300, 1e-3, 2u, scene, 160u, 90u, true);
  ok = ok && frame("scale 1e-150", cam, 1e-150, 1e-3, 2u, scene, 160u, 90u, false);
  if (!ok) return 1;
  printf("%llu blocks, %llu state a set; SELF0 %llu SELF1 %llu SKY %llu DARK0 %llu DARK1 %llu\n", g_blocks, g_stating, g_bit[0], g_bit[1], g_bit[2], g_bit[3], g_bit[4]);
  return (g_bit[0] && g_bit[2] && g_bit[3] && g_bit[4]) ? 0 : 1;      // (not vacuous: the ordinary frames state every kind of bit but, perhaps, SELF1)
}
