// spec_walk_check.cpp — the specular power's multiply sequence (csrc/rt_spec_walk.h), checked on a CPU against the documented loop
//     r = 1.0; do { if (k & 1) r *= b; b *= b; k >>= 1; } while (k);
// bit for bit, for every exponent n in 0..4096 and 2 000 bases x in (0, 1] - random ones over 300 binades, the ends of the range, bases next
// to 1 and bases whose powers come out denormal or zero - in every form of the header: the gap form (count-trailing-zeros), the ladder at
// the kernels' length and at lengths 0, 1 and 3 (so that exponents of this range run its loop and its hand-over), and the per-lane form, alone
// and with a longer-lived neighbour in its wave.  It also counts the multiplies of the gap and ladder forms: floor(log2 n) squarings and
// popcount(n) - 1 products, i.e. no 1.0 * b and no squaring behind the top bit.
// It also holds the integer form of a predicate on a scalar double (csrc/rt_uniform_pred.h: rt_nonzero_bits, the kernels' `x != 0.0` of an
// occluder's transparency) to its floating-point statement over the edge patterns: +-0, the smallest and largest denormals, 1, the largest
// finite value, infinities, quiet and signalling NaNs of either sign, negative values, and 100 000 random patterns.
// A stand-alone program with its own main:
//   g++ -std=c++17 -O2 -I<csrc> spec_walk_check.cpp          (also with -fsanitize=address,undefined)
// The kernels compile the same header for the GPU (rt_kernel_math.h: rt_pow_spec); here `mul` is the host's binary64 product.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_spec_walk.h"
#include "rt_uniform_pred.h"

static unsigned long long n_mul;
static double mul_counted(double a, double b) { n_mul++; return a * b; }

static double documented(uint32_t k, double b) {
  double r = 1.0;
  do { if (k & 1u) r *= b; b *= b; k >>= 1; } while (k);
  return r;
}
static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

template <int LADDER> static double ladder(uint32_t n, double x) { return n == 0u ? 1.0 : rt_spec_walk_ladder<LADDER>(n, x, mul_counted); }
static double gaps(uint32_t n, double x) { return n == 0u ? 1.0 : rt_spec_walk_gaps(n, x, mul_counted); }

static unsigned long long predicates() {
  std::vector<uint64_t> ps = {0x0000000000000000ull, 0x8000000000000000ull, 0x0000000000000001ull, 0x8000000000000001ull, 0x000fffffffffffffull,
                              0x800fffffffffffffull, 0x0010000000000000ull, 0x3ff0000000000000ull, 0xbff0000000000000ull, 0x7fefffffffffffffull,
                              0xffefffffffffffffull, 0x7ff0000000000000ull, 0xfff0000000000000ull, 0x7ff8000000000000ull, 0xfff8000000000000ull,
                              0x7ff0000000000001ull, 0xfff0000000000001ull, 0x7fffffffffffffffull, 0xffffffffffffffffull, 0x0000000100000000ull,
                              0x8000000100000000ull, 0x00000000ffffffffull, 0xc059000000000000ull};
  uint64_t s = 0x2545f4914f6cdd1dull;
  for (int i = 0; i < 100000; i++) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; ps.push_back(s); }
  unsigned long long bad = 0;
  for (const uint64_t b : ps) {
    double x; std::memcpy(&x, &b, sizeof x);
    volatile double vx = x;                                                        // (the compare as the kernel's statement makes it: of the value, at run time)
    if (rt_nonzero_bits(b) != (vx != 0.0)) { if (bad++ < 10) std::printf("pattern %016llx: rt_nonzero_bits says %d, x != 0.0 says %d\n", (unsigned long long)b, (int)rt_nonzero_bits(b), (int)(vx != 0.0)); }
  }
  return bad;
}

int main() {
  if (predicates()) { std::printf("spec_walk_check: an integer predicate differs from its floating-point form\n"); return 1; }
  std::vector<double> xs = {1.0, 0.5, 0x1p-1022, 0x1p-1074, 1.0 - 0x1p-53, 1.0 - 0x1p-52, 0.99, 0x1.fffffffffffffp-2, 0x1p-100, 0x1.8p-512, 0x1.23456789abcdep-270};
  uint64_t s = 0x9e3779b97f4a7c15ull;
  while (xs.size() < 2000u) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t mant = (s >> 12) | 1u;                                      // 52 random bits
    const int e = (int)((s >> 3) % 300u);                                      // 2^-300 < x < 1: n <= 4096 reaches the denormals and zero
    uint64_t bits = ((uint64_t)(1023 - 1 - (xs.size() % 3u == 0u ? e : e % 4)) << 52) | (mant & 0xfffffffffffffull);
    double x; std::memcpy(&x, &bits, sizeof x);
    xs.push_back(x);
  }
  unsigned long long bad = 0, denormal = 0, checked = 0;
  for (uint32_t n = 0; n <= 4096u; n++) {
    const unsigned long long want_mul = n == 0u ? 0ull : (unsigned long long)(31 - __builtin_clz(n)) + (unsigned long long)(__builtin_popcount(n) - 1);
    for (const double x : xs) {
      const double want = documented(n, x);
      uint64_t wb; std::memcpy(&wb, &want, sizeof wb);
      if (want != 0.0 && (wb >> 52) == 0u) denormal++;
      const double got[6] = {gaps(n, x), 0, 0, 0, 0, 0};
      const unsigned long long m0 = n_mul; n_mul = 0;
      const double l9 = ladder<9>(n, x);
      const unsigned long long m9 = n_mul; n_mul = 0;
      const double l0 = ladder<0>(n, x), l1 = ladder<1>(n, x), l3 = ladder<3>(n, x);
      n_mul = 0;
      const auto mul = [](double a, double b) { return a * b; };
      const double alone = rt_spec_walk_lanes(n, x, mul, [](bool more) { return more; });
      int turns = 0;
      const double beside = rt_spec_walk_lanes(n, x, mul, [&turns](bool more) { return more || ++turns < 14; });      // a neighbour with a 13-bit exponent keeps the wave squaring
      const double all[7] = {got[0], l9, l0, l1, l3, alone, beside};
      static const char *const names[7] = {"gaps", "ladder<9>", "ladder<0>", "ladder<1>", "ladder<3>", "lanes", "lanes beside a longer lane"};
      for (int f = 0; f < 7; f++)
        if (!same(all[f], want)) { if (bad++ < 10) std::printf("n = %u, x = %a: %s gives %a, the documented loop %a\n", n, x, names[f], all[f], want); }
      if (m0 != want_mul || m9 != want_mul) { if (bad++ < 10) std::printf("n = %u: %llu (gaps) and %llu (ladder) multiplies, expected %llu\n", n, m0, m9, want_mul); }
      checked++;
    }
  }
  if (denormal == 0) { std::printf("no denormal result among the cases\n"); return 1; }
  if (bad) { std::printf("spec_walk_check: %llu mismatches\n", bad); return 1; }
  std::printf("spec_walk_check: %llu (n, x) pairs, %llu with a denormal result: every form agrees with the documented loop bit for bit\n", checked, denormal);
  return 0;
}
