// ambient_check - csrc/rt_ambient.h on a CPU: tests/test_ambient.py builds this with the plain host compiler and -ffp-contract=off (the
// header needs nothing of HIP) and runs it.  Three checks, exit status 1 and a line on stderr where one fails:
//   1. the frame: t, bt, l orthonormal for the axis normals, l2 = +-1 exactly, l2 = +-0 and 4096 seeded unit normals - the three lengths
//      and the three dot products within 4 * 2^-52 (each component is a handful of correctly rounded operations on values <= 1),
//      measured in long double; the largest error seen is printed
//   2. the entry index: it wraps at n_dirs with a large base, at 2^64 before the reduction, and the per-receiver walk (amb_walk) gives
//      the expression's value for every sample
//   3. a receiver that is not scanned (a miss; a non-finite word in point or normal) yields six NaNs and skip -1
#include "rt_ambient.h"

#include <math.h>
#include <stdio.h>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "ambient_check: " __VA_ARGS__); fprintf(stderr, "\n"); failures++; } } while (0)

static uint64_t lcg_state = 0x9e3779b97f4a7c15ull;
static double lcg_unit() {       // in (-1, 1)
  lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(int64_t)(lcg_state >> 11) / 4503599627370496.0 - 1.0;
}

static long double dotl(const double a[3], const double b[3]) {
  return (long double)a[0] * b[0] + (long double)a[1] * b[1] + (long double)a[2] * b[2];
}

static long double frame_error(const double l[3]) {
  double t[3], bt[3];
  amb_frame(l, t, bt);
  long double worst = 0.0L;
  const long double e[6] = {sqrtl(dotl(t, t)) - 1.0L, sqrtl(dotl(bt, bt)) - 1.0L, sqrtl(dotl(l, l)) - 1.0L, dotl(t, bt), dotl(t, l), dotl(bt, l)};
  for (int k = 0; k < 6; k++) { const long double a = fabsl(e[k]); if (!(a <= worst)) worst = a; }
  return worst;
}

int main() {
  // 1. the frame
  const long double bound = 4.0L * ldexpl(1.0L, -52);
  long double worst = 0.0L;
  const double fixed[][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}, {1, 0, 0.0}, {1, 0, -0.0}, {0, 1, -0.0}, {-1, 0, -0.0},
                             {0.6, 0.8, 0.0}, {0.6, -0.8, -0.0}};
  for (const auto &l : fixed) {
    const long double e = frame_error(l);
    CHECK(e <= bound, "frame of (%g, %g, %g): error %Lg above %Lg", l[0], l[1], l[2], e, bound);
    if (e > worst) worst = e;
  }
  int seeded = 0;
  while (seeded < 4096) {
    double l[3] = {lcg_unit(), lcg_unit(), lcg_unit()};
    if (seeded % 8 == 0) l[2] = l[2] < 0.0 ? -1.0 + 1e-9 * (l[2] + 1.0) : l[2] * 1e-12;      // close to the pole of the construction; close to the seam l2 = 0
    if (lit_unit(&l[0], &l[1], &l[2]) == 0.0) continue;
    const long double e = frame_error(l);
    CHECK(e <= bound, "frame of (%.17g, %.17g, %.17g): error %Lg above %Lg", l[0], l[1], l[2], e, bound);
    if (!(e <= worst)) worst = e;
    seeded++;
  }
  printf("AMBIENT frame: largest orthonormality error %.3Le = %.3Lf x 2^-52 over %d normals (bound 4 x 2^-52)\n", worst, worst / ldexpl(1.0L, -52),
         seeded + (int)(sizeof fixed / sizeof fixed[0]));

  // 2. the entry index
  CHECK(amb_entry(0, 0, 0, 5, 16) == 5 && amb_entry(123, 7, 0, 5, 16) == 5, "stride 0 gives entry s");
  CHECK(amb_entry(0, 9, 7, 3, 64) == (9 * 7 + 3) % 64, "a small index");
  CHECK(amb_entry(1ull << 40, 5, 7, 3, 64) == (uint32_t)((((1ull << 40) + 5) * 7 + 3) % 64), "a large base");
  {
    // base + i = 2^63 + 1, stride 2: the product wraps to 2; (2 + 3) % 7 = 5, while the unwrapped value would give (2^64 + 5) % 7 = 0
    CHECK(amb_entry((1ull << 63), 1, 2, 3, 7) == 5, "the index wraps at 2^64 before the reduction: got %u", amb_entry((1ull << 63), 1, 2, 3, 7));
    const uint64_t bases[] = {0, 1, 262144, (1ull << 40) + 12345, (1ull << 63), ~0ull - 3, ~0ull};
    const uint64_t items[] = {0, 1, 63, 262143, 2147483646};
    const uint32_t strides[] = {0, 1, 7, 65537, 0xffffffffu}, tables[] = {1, 5, 16, 64, 1000, 65536};
    for (uint64_t base : bases) for (uint32_t stride : strides) for (uint32_t n_dirs : tables) for (uint64_t i : items) {
      const amb_walk W = amb_walk_of(base, i, stride, n_dirs);
      const uint32_t n_samples = n_dirs < 1024u ? n_dirs : 1024u;
      for (uint32_t s = 0; s < n_samples; s++) {
        const uint32_t want = amb_entry(base, i, stride, s, n_dirs), got = amb_walk_entry(W, s, n_dirs);
        if (want != got || want >= n_dirs) { CHECK(false, "walk: base %llu i %llu stride %u s %u n_dirs %u: %u, expression %u", (unsigned long long)base, (unsigned long long)i, stride, s, n_dirs, got, want); break; }
      }
    }
    // P + s wraps: P = 2^64 - 2 (base + i = 2^63 - 1, stride 2)
    const amb_walk W = amb_walk_of((1ull << 63) - 1, 0, 2, 1000);
    for (uint32_t s = 0; s < 8; s++) CHECK(amb_walk_entry(W, s, 1000) == amb_entry((1ull << 63) - 1, 0, 2, s, 1000), "walk where P + s wraps, s %u", s);
  }

  // 3. receivers that are not scanned
  {
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    struct { int32_t object; double p[3], n[3]; } bad[] = {{-1, {0, 0, 0}, {0, 0, 0}}, {-1, {1, 2, 3}, {0, 1, 0}}, {3, {nan, 0, 0}, {0, 1, 0}}, {3, {0, 0, inf}, {0, 1, 0}},
                                                            {3, {0, 0, 0}, {0, nan, 0}}, {0, {0, 0, 0}, {-inf, 0, 0}}};
    for (const auto &b : bad) for (int inside = 0; inside < 2; inside++) {
      const amb_receiver R = amb_receiver_of(b.object, inside, b.p[0], b.p[1], b.p[2], b.n[0], b.n[1], b.n[2]);
      double seg[6];
      amb_segment(R, 0.6, 0.0, 0.8, seg);
      CHECK(!R.scanned && R.skip == -1, "a record that is not scanned has skip -1 (object %d)", b.object);
      for (int c = 0; c < 6; c++) CHECK(seg[c] != seg[c], "a record that is not scanned gives six NaNs (object %d, word %d)", b.object, c);
    }
    // ... and one that is: origin = point, skip = object, the facing normal turned for a receiver seen from inside
    const amb_receiver R = amb_receiver_of(4, 1, 1.0, 2.0, 3.0, 0.0, 0.0, 1.0);
    double seg[6];
    amb_segment(R, 0.0, 0.0, 1.0, seg);
    CHECK(R.scanned && R.skip == 4 && seg[0] == 1.0 && seg[1] == 2.0 && seg[2] == 3.0 && seg[3] == 0.0 && seg[4] == 0.0 && seg[5] == -1.0,
          "an inside receiver scans along -normal: (%g, %g, %g)", seg[3], seg[4], seg[5]);
  }
  return failures ? 1 : 0;
}
