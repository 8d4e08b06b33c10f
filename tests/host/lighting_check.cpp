// lighting_check - csrc/rt_lighting.h on a CPU: tests/test_lighting.py builds this with the plain host compiler and -ffp-contract=off (the
// header needs nothing of HIP) and runs it.  Four checks, exit status 1 and a line on stderr where one fails:
//   1. the segment: 4096 seeded points, normals and lights - shadow_vec is a unit vector within 4 * 2^-52 (three correctly rounded
//      products with 1 / len on components <= len), len * len is mag within 2 ulp, shadow_dot is the dot product it says, and
//      a light at the point itself leaves the zero vector, len 0 and a dot that does not face; the largest length error is printed
//   2. the light's place: at radius 0 the light itself, bit for bit, with no table (NULL); otherwise light + radius * o per component
//   3. the facing rule and the step behind the scan: a NaN dot goes on, 0 and -0 do not; an intensity of 0 or -0 adds nothing and
//      is not counted, a NaN is added and counted
//   4. a receiver that is not scanned (a miss; a non-finite word in point or normal) has skip -1; one seen from inside faces along -normal
#include "rt_lighting.h"

#include <math.h>
#include <stdio.h>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "lighting_check: " __VA_ARGS__); fprintf(stderr, "\n"); failures++; } } while (0)

static uint64_t lcg_state = 0x9e3779b97f4a7c15ull;
static double lcg_unit() {       // in (-1, 1)
  lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(int64_t)(lcg_state >> 11) / 4503599627370496.0 - 1.0;
}

int main() {
  // 1. the segment
  const long double bound = 4.0L * ldexpl(1.0L, -52);
  long double worst = 0.0L;
  for (int it = 0; it < 4096; it++) {
    const double p[3] = {9.0 * lcg_unit(), 9.0 * lcg_unit(), 9.0 * lcg_unit()};
    double l[3] = {lcg_unit(), lcg_unit(), lcg_unit()};
    if (lit_unit(&l[0], &l[1], &l[2]) == 0.0) continue;
    const double scale = it % 8 == 0 ? 1e-7 : 12.0;                  // lights close to the point among them
    const double pos[3] = {p[0] + scale * lcg_unit(), p[1] + scale * lcg_unit(), p[2] + scale * lcg_unit()};
    const lgt_segment S = lgt_segment_of(p, l, pos);
    if (S.len == 0.0) continue;
    const long double n2 = (long double)S.sv[0] * S.sv[0] + (long double)S.sv[1] * S.sv[1] + (long double)S.sv[2] * S.sv[2];
    const long double e = fabsl(sqrtl(n2) - 1.0L);
    CHECK(e <= bound, "shadow_vec of iteration %d: length error %Lg above %Lg", it, e, bound);
    if (!(e <= worst)) worst = e;
    CHECK(fabsl((long double)S.len * S.len - S.mag) <= 2.0L * ldexpl((long double)S.mag, -52), "len * len is not mag within 2 ulp (iteration %d)", it);
    CHECK(S.sd == (S.sv[0] * l[0] + S.sv[1] * l[1]) + S.sv[2] * l[2], "shadow_dot is the stated expression (iteration %d)", it);
    CHECK(lgt_traced(S), "a finite segment is traced (iteration %d)", it);
  }
  printf("LIGHTING segment: largest length error of shadow_vec %.3Le = %.3Lf x 2^-52 (bound 4 x 2^-52)\n", worst, worst / ldexpl(1.0L, -52));
  {
    const double p[3] = {1.0, 2.0, 3.0}, l[3] = {0.0, 1.0, 0.0};
    const lgt_segment S = lgt_segment_of(p, l, p);
    CHECK(S.len == 0.0 && S.mag == 0.0 && S.sv[0] == 0.0 && S.sv[1] == 0.0 && S.sv[2] == 0.0 && S.sd == 0.0 && !lgt_faces(S), "a light at the point itself");
    const double far[3] = {1e200, 2.0, 3.0};
    const lgt_segment T = lgt_segment_of(p, l, far);                 // mag overflows: len +Infinity, shadow_vec 0 * ... and the dot a NaN or 0
    CHECK(T.mag == __builtin_inf() && T.len == __builtin_inf(), "a light so far that mag overflows: mag %g", T.mag);
  }

  // 2. the light's place
  {
    const double light[3] = {5.0, 10.0, -0.0}, o[3] = {0.25, -0.5, 0.125};
    double pos[3];
    lgt_light_pos(light, 0.0, nullptr, pos);
    CHECK(pos[0] == 5.0 && pos[1] == 10.0 && pos[2] == 0.0 && __builtin_signbit(pos[2]), "radius 0 is the light itself, bit for bit");
    lgt_light_pos(light, 1.5, o, pos);
    CHECK(pos[0] == 5.0 + 1.5 * 0.25 && pos[1] == 10.0 + 1.5 * -0.5 && pos[2] == -0.0 + 1.5 * 0.125, "light + radius * o");
  }

  // 3. facing, and the step behind the scan
  {
    lgt_segment S;
    S.sv[0] = S.sv[1] = S.sv[2] = 0.0; S.mag = 4.0; S.len = 2.0;
    S.sd = __builtin_nan(""); CHECK(lgt_faces(S), "a NaN shadow_dot goes on");
    S.sd = 0.0; CHECK(!lgt_faces(S), "shadow_dot 0 does not face");
    S.sd = -0.0; CHECK(!lgt_faces(S), "shadow_dot -0 does not face");
    S.sd = -0.5; CHECK(!lgt_faces(S), "a negative shadow_dot does not face");
    S.sd = 0.5; CHECK(lgt_faces(S), "a positive shadow_dot faces");
    double diffuse = 0.25; uint32_t count = 0;
    lgt_contribute(S, 0.0, &diffuse, &count); lgt_contribute(S, -0.0, &diffuse, &count);
    CHECK(diffuse == 0.25 && count == 0, "an intensity of 0 adds nothing");
    lgt_contribute(S, 50.0, &diffuse, &count);
    CHECK(diffuse == 0.25 + (50.0 * 0.5) / 4.0 && count == 1, "(li * sd) / mag is added: %g", diffuse);
    lgt_contribute(S, __builtin_nan(""), &diffuse, &count);
    CHECK(diffuse != diffuse && count == 2, "a NaN intensity is added and counted");
  }

  // 4. receivers
  {
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    struct { int32_t object; double p[3], n[3]; } bad[] = {{-1, {0, 0, 0}, {0, 0, 0}}, {-1, {1, 2, 3}, {0, 1, 0}}, {3, {nan, 0, 0}, {0, 1, 0}}, {3, {0, 0, inf}, {0, 1, 0}},
                                                            {3, {0, 0, 0}, {0, nan, 0}}, {0, {0, 0, 0}, {-inf, 0, 0}}};
    for (const auto &b : bad) for (int inside = 0; inside < 2; inside++) {
      const lgt_receiver R = lgt_receiver_of(b.object, inside, b.p[0], b.p[1], b.p[2], b.n[0], b.n[1], b.n[2]);
      CHECK(!R.scanned && R.skip == -1, "a record that is not scanned has skip -1 (object %d)", b.object);
    }
    const lgt_receiver R = lgt_receiver_of(4, 1, 1.0, 2.0, 3.0, 0.0, 0.0, 1.0);
    CHECK(R.scanned && R.skip == 4 && R.p[0] == 1.0 && R.p[1] == 2.0 && R.p[2] == 3.0 && R.l[0] == 0.0 && R.l[1] == 0.0 && R.l[2] == -1.0,
          "an inside receiver faces along -normal: (%g, %g, %g)", R.l[0], R.l[1], R.l[2]);
  }
  return failures ? 1 : 0;
}
