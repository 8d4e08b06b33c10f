// rt_kernel_math.h - the trace kernels' arithmetic: vectors, the strict (IEEE, fdlibm, OCML) and product (rsq / rcp + Newton) forms of
// sqrt, division, pow, atan2 / asin, and the conversions and hashes of the samplers and the store.
// A fragment: included once by rt_kernel.hip, inside its anonymous namespace (RT_STRICT is decided there).

struct v3 { double x, y, z; };
__device__ __forceinline__ v3 mk(double x, double y, double z) { v3 r; r.x = x; r.y = y; r.z = z; return r; }
// main.js:49-51 — (a0*b0 + a1*b1) + a2*b2
__device__ __forceinline__ double dot(const v3 a, const v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// ---- math layer ----------------------------------------------------------------------------
// RT_STRICT: IEEE-754 correctly rounded sqrt and division, fdlibm's atan2 / asin and OCML pow, operation for operation
// with the JS expression trees.  Otherwise (product kernel): the hardware estimates v_rsq_f64 /
// v_rcp_f64 refined by Newton steps in FMA arithmetic (<= ~1 ulp, no denormal pre-scaling, no
// div_scale/div_fixup), reciprocal-multiplies for divisions by constants, and integer powers by
// square-and-multiply.  All of it stays binary64; the differences are last-ulp effects, which
// the +-1 LSB tolerance exists for (tests/test_gpu_parity.py holds both kernels to it).
#if RT_STRICT
__device__ __forceinline__ double rt_sqrt(double x) { return sqrt(x); }
template <bool FMIN = false> __device__ __forceinline__ double rt_sqrt_nn(double x) { return sqrt(x); }
__device__ __forceinline__ double rt_rcp(double x) { return 1.0 / x; }
__device__ __forceinline__ double rt_div(double a, double b) { return a / b; }
__device__ __forceinline__ double rt_pow(double x, double e) { return pow(x, e); }
#define RT_DIV_CONST(x, c) ((x) / (c))
// main.js:62-66 — multiply by 1/len; the zero vector is returned unchanged
__device__ __forceinline__ v3 unit(const v3 v, double *len_out) {
  const double l = sqrt(dot(v, v));
  *len_out = l;
  if (l != 0.0) { const double s = 1.0 / l; return mk(v.x * s, v.y * s, v.z * s); }
  return v;
}
#else
// Measured on MI355X (build/probe/prec.hip, 1M random inputs over 1e-6..1e8): v_rsq_f64 / v_rcp_f64 are good to
// 2^-24; one Newton step gives 4.1e-15 / 2.1e-15, two give 1.4e-16 / 1.1e-16; x*rsqrt(x) after ONE step plus
// the residual correction g += (x - g*g) * y/2 is a square root good to 1.1e-16.
// rt_rsqrt_pos is only ever used to NORMALISE a vector.  An error in the scale of a direction moves no hit
// point (p + d*t is invariant under rescaling d) and no reflection direction; it reaches only continuous
// quantities (a cosine, a distance) at the 4e-15 level, so one Newton step is enough there.
__device__ __forceinline__ double rt_rsqrt_pos(double m) {           // m > 0, finite
  const double y = __builtin_amdgcn_rsq(m);
  const double e = __builtin_fma(-(m * y), y, 1.0);
  return __builtin_fma(0.5 * y, e, y);
}
__device__ __forceinline__ double rt_sqrt(double x) {
  const double y = rt_rsqrt_pos(x);
  double g = x * y;
  g = __builtin_fma(__builtin_fma(-g, g, x), 0.5 * y, g);
  return (x > 0.0) ? g : x;                                           // +0 -> 0, NaN -> NaN, x < 0 -> x (callers never pass it)
}
// x >= 0 (or NaN): the +0 case is kept exact by clamping the estimate (rsq(0) = inf) instead of
// selecting afterwards: 0 * (a finite y) = 0 through every step below.
// The clamp is an INTEGER minimum of the estimate's high word against 0x7fe00000 (the high word of 2^1023): one VALU instruction
// with a 32-bit literal.  It used to be fmin(estimate, 1e100), whose 64-bit constant is two s_mov_b32 at each of the 22 inlined
// sites, rebuilt at every shadow test that enters (the build has no MachineLICM).  Why every result a caller can see is the old one's:
//   * For positive doubles the order of the values is the order of their high words as signed integers (then of the low words), so
//     the minimum leaves every estimate below 2^1023 - every finite one but the last binade's - as it is, and so did the old clamp
//     for an estimate <= 1e100.  The estimate is good to 2^-24 (measured, above): x >= 2^-664 = 1.31e-200 gives at most
//     2^332 (1 + 2^-24) = 8.75e99 < 1e100, and x >= 1e-200 (1 + 2^-22) still gives less than 1e100.  For all those x neither
//     clamp acts: bit for bit.  (In the band 1e-200 <= x < 1e-200 (1 + 2^-22), 2.4e-207 wide, the old clamp may have cut an estimate
//     that overshot 1e100 by its own error and this one does not: both forms then return sqrt(x) to the bound above, not
//     necessarily the same last bit.  Below 1e-200 the old clamp cut a correct estimate and returned a wrong root; this one does not.)
//   * x = +0: rsq = +inf, high word 0x7ff00000 -> 0x7fe00000, y = 2^1023.  x y = 0, e = 1, y' = 1.5 * 2^1023 (finite),
//     g = 0 y' = 0, fma(fma(-0, 0, 0), y' / 2, 0) = +0: as with 1e100.
//   * x = -0 (no caller forms it: the discriminants are differences and fma results, +0 when exact): rsq = -inf, a negative high
//     word, kept by the SIGNED minimum as fmin kept -inf: NaN both ways.
//   * x = NaN: every step below has x as an operand: NaN, whatever y is.
// FMIN (the general kernels, REFRACT): the old clamp.  There the integer form measured 0.5 % SLOWER (the reference's own scene, three runs of
// three below the parent's: docs/EVIDENCE.md, first section) - those kernels are bound by their vector side, and the two s_mov_b32 stood in
// the wait state between the v_rsq_f64 and its first use, where an s_nop stands now.
template <bool FMIN = false>
__device__ __forceinline__ double rt_sqrt_nn(double x) {
  double y;
  if constexpr (FMIN) y = __builtin_fmin(__builtin_amdgcn_rsq(x), 1e100);
  else {
    const unsigned long long yb = __builtin_bit_cast(unsigned long long, __builtin_amdgcn_rsq(x));
    const int32_t yh = (int32_t)(yb >> 32);
    y = __builtin_bit_cast(double, ((unsigned long long)(uint32_t)(yh < 0x7fe00000 ? yh : 0x7fe00000) << 32) | (uint32_t)yb);
  }
  const double e = __builtin_fma(-(x * y), y, 1.0);
  y = __builtin_fma(0.5 * y, e, y);
  const double g = x * y;
  return __builtin_fma(__builtin_fma(-g, g, x), 0.5 * y, g);
}
__device__ __forceinline__ double rt_rcp(double x) {
  double y = __builtin_amdgcn_rcp(x);
  y = __builtin_fma(y, __builtin_fma(-x, y, 1.0), y);
  return __builtin_fma(y, __builtin_fma(-x, y, 1.0), y);
}
__device__ __forceinline__ double rt_div(double a, double b) {
  const double r = rt_rcp(b);
  const double q = a * r;
  return __builtin_fma(__builtin_fma(-q, b, a), r, q);               // one correction step on the quotient
}
#define RT_DIV_CONST(x, c) rt_div_const((x), (c), 1.0 / (c))
__device__ __forceinline__ double rt_div_const(double a, double c, double rc) {
  const double q = a * rc;
  return __builtin_fma(__builtin_fma(-q, c, a), rc, q);
}
// Non-integer exponents (none in the reference scene) take OCML's pow out of line, so that its ~40
// temporaries are not part of the register budget of the loop every pixel runs.
__device__ __attribute__((noinline)) double rt_pow_generic(double x, double e) { return pow(x, e); }
// x^e, x > 0, of a material whose exponent e (read through `e` only when it is needed) the host classified as n = rt_spec_n(e).
// Integer exponents (every specular_exponent of the reference scene, main.js:108-123) by square-and-multiply: <= 2*log2(n)
// multiplies instead of OCML's ~150-instruction pow.  The multiply sequence is stated once, in rt_spec_walk.h - for bit i = 0, 1, ...:
// r *= b where bit i is set, b *= b between bits, with r = b standing for the first r = 1.0 * b (exact) - and every path below walks it
// in that order, so the result does not depend on the path.
// UNI (the uniform-material path): n comes from a scalar load - one exponent for the wave, known when the kernel is compiled - so the
// walk below is entered without the ballot that finds that out and without the second form behind it.
// LADDER (the six-wave kernels: the uniform-material path, and the uniform-exponent arm of their general path): the walk as a ladder of RT_SPEC_LADDER steps on the condition code
// (rt_spec_walk.h: two tests and at most two multiplies per bit above the lowest set one, no inner loop: an exponent of 10 is 25 scalar
// instructions where the gap form below is 31 - measured, 6 x 51 947 per headline launch: docs/EVIDENCE.md, "Scalar forms"); exponents of more
// bits than the ladder has steps go on in its loop.
#include "rt_spec_walk.h"
#define RT_SPEC_LADDER 9                                             // steps above the lowest set bit: exponents below 1024 never reach the loop
template <bool UNI = false, bool LADDER = false, class EP>           // (EP: where the material lies - const double * in any address space)
__device__ __forceinline__ double rt_pow_spec(double x, int32_t n, EP e) {
  const auto mul = [](double a, double b) __attribute__((always_inline)) { return a * b; };
  const int32_t n0 = UNI ? n : __builtin_amdgcn_readfirstlane(n);
  if (UNI || __ballot(n != n0) == 0ull) {
    // every lane here has the same exponent (a wave on one sphere: nearly all of them): walk its bits with scalar control
    if (n0 < 0) return rt_pow_generic(x, *e);
    const uint32_t k = (uint32_t)n0;
    if (k == 0u) return 1.0;
    if constexpr (LADDER) return rt_spec_walk_ladder<RT_SPEC_LADDER>(k, x, mul);
    // from set bit to set bit (the multiplies are unconditional: no select per bit)
    else return rt_spec_walk_gaps(k, x, mul);
  }
  // several exponents (silhouettes, bounce nodes on different spheres): per lane, for as many bits as the longest exponent among
  // the lanes has - the loop's exit is wave-uniform, so no lane leaves it on its own
  if (n < 0) return rt_pow_generic(x, *e);
  return rt_spec_walk_lanes((uint32_t)n, x, mul, [](bool more) __attribute__((always_inline)) { return __ballot(more) != 0ull; });
}
// main.js:62-66 — v * (1/len), len = sqrt(v.v); the zero vector is returned unchanged
__device__ __forceinline__ v3 unit(const v3 v, double *len_out) {
  const double m = dot(v, v);
  const double s = rt_rsqrt_pos(m);
  const bool ok = (m > 0.0);
  *len_out = ok ? m * s : m;
  return ok ? mk(v.x * s, v.y * s, v.z * s) : v;
}
#endif

// ---- atan2 / asin for the samplers (main.js:127-128, 446-447) --------------------------------------------------------
// RT_STRICT: fdlibm's, as the JS engines' (below).  Product kernel: OCML's argument reductions and minimax polynomials (atan: odd polynomial of degree 39
// on [0,1] after q = min/max; asin: x + x*r*P(r), r = x^2 below 1/2 and (1-|x|)/2 above with pi/2 - 2*asin(sqrt(r))), but
//   * every Horner step is ONE v_fma_f64 whose constant comes from an SGPR pair (hipcc otherwise writes the 64-bit literal
//     into the v_fmac accumulator with two v_mov_b32 per step: 64 of OCML's ~230 instructions for the pair of calls),
//   * the quotient is the kernel's rcp + Newton division, the square root its rsq + Newton one,
//   * the branch above 1/2 finishes in working precision instead of OCML's double-double tail.
// Accuracy: <= 2 ulp (OCML: <= 1); what the samplers make of it is a texel index / a checker parity, i.e. the same last-ulp
// sensitivity at boundaries that OCML, glibc and V8 already have among themselves (the one listed
// exception); the parity suite and the soaks hold the result to 1 LSB.
#if RT_STRICT
// The strict kernel computes atan2 / asin AS THE JAVASCRIPT ENGINES DO: V8 and SpiderMonkey implement Math.atan2 / Math.asin with
// a port of Sun's fdlibm (fixed argument reductions and coefficients, plain binary64 operations - deterministic everywhere), so
// restating those published algorithms operation for operation (this build has no FMA contraction; `/` and sqrt are correctly
// rounded) gives u and v the reference's own bits, where OCML's functions differ in the last ulp on a few per cent of the
// inputs - and an ulp at a texel or checker boundary is a different pixel.  Same code as
// oracle/fdlibm_trig.h, which the CPU tests compare with Node's Math.atan2 / Math.asin bit for bit on 0.9 M vectors.
#include "rt_fdlibm.h"
// atan2(y, x) and asin(w) of one surface normal (the two halves of main.js:446-447 / :127-128)
template <bool FMIN = false> __device__ __forceinline__ void rt_atan2_asin(double y, double x, double w, double *at, double *as) { *at = fd_atan2(y, x); *as = fd_asin(w); }
#else
__device__ __forceinline__ double rt_fma_k(double a, double b, double k) {     // a*b + k, k wave-uniform: v_fma_f64 v, v, v, s[..]
  double r;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(k));
  return r;
}
typedef const double __attribute__((address_space(4))) *rt_trig_kptr;
typedef double __attribute__((ext_vector_type(4))) rt_d4;
// The polynomial coefficients (OCML's, as 64-bit patterns) sit in a constant-memory table read with scalar loads: an
// s_load_dwordx8 brings four of them into SGPRs with ONE scalar instruction, where immediates would take two s_mov_b32 each
// (the scalar unit is shared by the CU's four SIMDs and is ~60 % busy in this kernel: measured, immediates made the kernel slower).
// The two Horner chains are independent, so their steps ALTERNATE (a dependent v_fma_f64 waits for its predecessor; the other
// chain's step fills the gap), and the coefficients come in eight 32-byte groups laid out for that order - atan c0..3 | atan c4..7 |
// then two steps of each chain per group: atan c8, asin c0, atan c9, asin c1 | ... - each fetched two groups ahead of its use
// (one ahead: -0.4 %, profiles/r03_ab_log.md), the first two before the quotient's dependent chain.  (Round 2 fetched 64-byte
// groups: 32 scalar registers of coefficients at the kernel's scalar-pressure peak, where the kernel had none to spare; this way
// it is 24.)
#define RT_TRIG_AHEAD 2u
__constant__ unsigned long long RT_TRIG_BITS[32] = {
    0x3eeba404b5e68a13ull, 0xbf23e260bd3237f4ull, 0x3f4b2bb069efb384ull, 0xbf67952daf56de9bull,
    0x3f7d6d43a595c56full, 0xbf8c6ea4a57d9582ull, 0x3f967e295f08b19full, 0xbf9e9ae6fc27006aull,
    0x3fa2c15b5711927aull, 0x3fa059859fea6a70ull, 0xbfa59976e82d3ff0ull, 0xbf90a5a378a05eafull,
    0x3fa82d5d6ef28734ull, 0x3f94052137024d6aull, 0xbfaae5ce6a214619ull, 0x3f7ab3a098a70509ull,
    0x3fae1bb48427b883ull, 0x3f88ed60a300c8d2ull, 0xbfb110e48b207f05ull, 0x3f8c6fa84b77012bull,
    0x3fb3b13657b87036ull, 0x3f91c6c111dccb70ull, 0xbfb745d119378e4full, 0x3f96e89f0a0adacfull,
    0x3fbc71c717e1913cull, 0x3f9f1c72c668963full, 0xbfc2492492376b7dull, 0x3fa6db6db41ce4bdull,
    0x3fc99999999952ccull, 0x3fb333333336fd5bull, 0xbfd5555555555523ull, 0x3fc5555555555380ull};
template <bool FMIN = false>                                         // (FMIN: rt_sqrt_nn's clamp, above)
__device__ __forceinline__ void rt_atan2_asin(double y, double x, double w, double *at, double *as) {
  rt_trig_kptr K = (rt_trig_kptr)(const void *)RT_TRIG_BITS;
  asm volatile("" : "+s"(K));                        // opaque: the reads below stay scalar LOADS instead of being folded back into immediates
#define RT_TRIG_GROUP(I) (*(const rt_d4 __attribute__((address_space(4))) *)(K + 4 * (I)))
  rt_d4 g[8];
  g[0] = RT_TRIG_GROUP(0); g[1] = RT_TRIG_GROUP(1);
  const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
  const double hi = __builtin_fmax(ax, ay), lo = __builtin_fmin(ax, ay);
  const double q = rt_div(lo, hi);                                   // in [0,1]; 0/0 (both zero) handled below
  const double z = q * q;
  const double yw = __builtin_fabs(w);
  const double t = __builtin_fma(yw, -0.5, 0.5);                     // (1 - |w|) / 2
  const bool big = (yw >= 0.5);
  const double r = big ? t : w * w;
  g[2] = RT_TRIG_GROUP(2);
  double p = g[0][0];
  p = rt_fma_k(p, z, g[0][1]); p = rt_fma_k(p, z, g[0][2]); p = rt_fma_k(p, z, g[0][3]);
  g[3] = RT_TRIG_GROUP(3);
  p = rt_fma_k(p, z, g[1][0]); p = rt_fma_k(p, z, g[1][1]); p = rt_fma_k(p, z, g[1][2]); p = rt_fma_k(p, z, g[1][3]);
  double pa = 0.0;
#pragma unroll
  for (uint32_t i = 2; i < 8; i++) {                                 // group i: atan step, asin step, atan step, asin step
    if (i + RT_TRIG_AHEAD < 8u) g[i + RT_TRIG_AHEAD] = RT_TRIG_GROUP(i + RT_TRIG_AHEAD);
    p = rt_fma_k(p, z, g[i][0]);
    pa = (i == 2u) ? g[i][1] : rt_fma_k(pa, r, g[i][1]);
    p = rt_fma_k(p, z, g[i][2]);
    pa = rt_fma_k(pa, r, g[i][3]);
  }
#undef RT_TRIG_GROUP
  // atan2: quadrant and special cases
  double a = __builtin_fma(q, z * p, q);                             // atan(q), q in [0,1]
  a = (ay > ax) ? (M_PI / 2.0 - a) : a;
  const bool xneg = (__builtin_bit_cast(unsigned long long, x) >> 63) != 0;      // the sign BIT: atan2(+-0, -0) = +-pi
  a = xneg ? (M_PI - a) : a;
  a = (hi == 0.0) ? (xneg ? M_PI : 0.0) : a;                         // atan2(+-0, +-0)
  *at = __builtin_copysign(a, y);                                    // NaN in, NaN out (every step above propagates it)
  // asin: x + x*r*P(r) below 1/2, pi/2 - 2*asin(sqrt((1-|x|)/2)) above
  pa = pa * r;
  const double sq = big ? rt_sqrt_nn<FMIN>(t) : yw;
  const double ww = __builtin_fma(sq, pa, sq);                       // asin(sq)
  double b = big ? __builtin_fma(-2.0, ww, M_PI / 2.0) : ww;
  b = (yw > 1.0) ? __builtin_nan("") : b;                            // |w| > 1 by an ulp (a ray through the exact pole): NaN, as Math.asin gives
  *as = __builtin_copysign(b, w);
}
#endif

// main.js:40-43 — v + n * (-(2 * v.n))
__device__ __forceinline__ v3 reflect(const v3 v, const v3 n) {
  const double t = -(2.0 * dot(v, n));
  return mk(v.x + n.x * t, v.y + n.y * t, v.z + n.z * t);
}
// Math.min(1, x) / Math.max(a, x) as used at main.js:316-317, :333-335 (NaN in x propagates)
__device__ __forceinline__ double min1(double x) { return (x > 1.0) ? 1.0 : x; }
__device__ __forceinline__ double maxa(double a, double x) { return (x < a) ? a : x; }
// The same clamps as ONE instruction each, for the product build's frame kernels where the caller has established what the select
// forms exist for.  min1 / maxa are a compare, two v_cndmask_b32 and a wait state; v_min_f64 / v_max_f64 are one issue - but they are
// IEEE minNum / maxNum: of a NaN and a number they return the NUMBER, where Math.min(1, NaN) is NaN (and NaN is byte 0).  They are
// written as inline asm because __builtin_fmin / __builtin_fmax put a canonicalising v_max_f64 x, x in front of every operand the compiler
// cannot prove canonical (a value read from LDS, an asm result).  None is needed: every operand here is the result of this kernel's own
// FP64 arithmetic or a finite constant, hence canonical, and with the IEEE mode bit of a compute kernel the instruction quiets a
// signalling NaN itself.  Equal bytes, operand by operand:
//   * rt_min1_nn(x): x is NOT NaN (the caller's test).  Then (x > 1) ? 1 : x and minNum(x, 1) are the same value, x's own zero included.
//   * rt_max_nn(a, x): x is NOT NaN; a MAY be (colour inf x albedo 0).  (x < a) ? a : x takes x when a is NaN, and so does maxNum.
//     For a == x of different signs of zero the select takes x and v_max_f64 may take +0: the value is 0 either way, and a channel's
//     only readers are to_byte - 255 * (+-0) clamped against 0, byte 0 - and the parent's fold, fma(S, x, O), whose sum with O != 0 does not
//     see the sign and with O == +-0 is a zero that goes the same two ways.  No reader divides by it or takes its sign.
//   * rt_min_nn / rt_max_nn in the fold (F = max(LO, min(HI, O + S x))): operands are sums, products and fma results of this kernel (canonical); a NaN
//     among them is swallowed as __builtin_fmin / __builtin_fmax swallowed it - the same minNum / maxNum, less the canonicalisation.
// Not for ITEM, COUNT or RT_STRICT instantiations: rt_trace_rays hands rgb to its caller as DOUBLES (the sign of a zero is visible there),
// rt_retrace and the strict kernels are the reference's own operation sequence, and the counting kernel is held to the strict one.
__device__ __forceinline__ double rt_min_nn(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double rt_max_nn(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double rt_min1_nn(double x) { double r; asm("v_min_f64 %0, %1, 1.0" : "=v"(r) : "v"(x)); return r; }
__device__ __forceinline__ double rt_max1_nn(double x) { double r; asm("v_max_f64 %0, %1, 1.0" : "=v"(r) : "v"(x)); return r; }
#if !RT_STRICT
// unit() for a caller that reads the vector only where the length it returns is non-zero (the reflection ray: `go_r = rlen != 0`): the
// length as unit() gives it, the vector WITHOUT unit()'s four selects by m > 0 (eight v_cndmask_b32 and a compare).
//   * m > 0: the selected arm, bit for bit.
//   * m == 0 (the zero vector): the length is 0 - the caller does not descend, and nobody reads the vector (NaN here: 0 x rsq(0)).
//   * m NaN (a NaN component): the length is NaN, which IS "non-zero" - the lane descends, here with a direction of three NaNs where unit()
//     returned v with its NaN among finite components.  Either ray has tca = d.L NaN at every sphere (a sum with a NaN term), hence a NaN
//     root that is never `closer_`: it meets nothing in either form, and a miss - the miss colour, or the flat enclosing sphere, whose colour
//     is a constant or a hash of the pixel's index (rt_scene.hip: enclosing_flat) - does not read d.
__device__ __forceinline__ v3 unit_go(const v3 v, double *len_out) {
  const double m = dot(v, v);
  const double s = rt_rsqrt_pos(m);
  *len_out = (m > 0.0) ? m * s : m;
  return mk(v.x * s, v.y * s, v.z * s);
}
#endif

// Counter-based stand-in for Math.random() in the stars sampler (main.js:135-139): lowbias32 twice over the sample's
// index in the frame and the node's position in the ray tree (root 1, reflect child 2p, refract child 2p+1), with the
// index's high word XORed by mix = lowbias32(seed) (include/rt_hip.h: RT_SAMPLER_STARS).  lowbias32(0) == 0: at seed 0
// identical to oracle/restate.js and oracle/rt_oracle.c, which know no seed.
__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ double star_uniform(uint32_t pix_lo, uint32_t pix_hi, uint32_t path, uint32_t mix) {
  return (double)lowbias32(pix_lo ^ lowbias32(path + 0x9e3779b9u * ((pix_hi ^ mix) + 1u))) * (1.0 / 4294967296.0);
}

// ECMAScript ToInt32(x) & 1   (main.js:129-130)
__device__ __forceinline__ int to_int32_bit0(double x) {
  if (fabs(x) < 2147483648.0) return (int)x & 1;     // the common case: one truncating conversion
  if (!(fabs(x) < RT_INF)) return 0;                 // NaN, +-Infinity -> 0
  double t = trunc(x);
  if (fabs(t) >= 4294967296.0) t = t - floor(t / 4294967296.0) * 4294967296.0;
  return (int)((long long)t & 1);
}

// Uint8ClampedArray store of 255*c (main.js:195-197): NaN -> 0, clamp, round half to even
__device__ __forceinline__ uint32_t to_byte(double c) {
#if RT_STRICT
  // fmax(NaN, 0) = 0 and the clamp precede the conversion, so v_cvt_u32_f64 never sees an out-of-range
  // value; v_rndne_f64 rounds half to even.
  return (uint32_t)__builtin_rint(__builtin_fmin(__builtin_fmax(255.0 * c, 0.0), 255.0));
#else
  // Four operations instead of five: the product is rounded to binary64 FIRST, exactly as the reference's `255 * rgb[c]` is
  // (main.js:195) - values of the form k + 1/2 are common there (0.04 % of all channels: 255 * (j/255) / 2 ...) and the store's
  // round-half-to-even must see them as the ties they are - then clamped, and ONE addition onto 1.5*2^52 (whose ulp is 1) does
  // the rounding to nearest-even and leaves the byte in the sum's low mantissa word (v_rndne + v_cvt in one operation).
  // (Folding the multiplication into that addition as an fma would round the EXACT product instead: measured 1.7e-4 of all
  // channels off by one against 4e-7, profiles/r02_ab_log.md.)
  const double s = __builtin_fmin(__builtin_fmax(255.0 * c, 0.0), 255.0) + 6755399441055744.0;
  return (uint32_t)__builtin_bit_cast(unsigned long long, s);
#endif
}
