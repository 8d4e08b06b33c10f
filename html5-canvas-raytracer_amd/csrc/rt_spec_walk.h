// rt_spec_walk.h - x^k for an integer k >= 1 by square-and-multiply: the ONE statement of the multiply sequence of the product
// kernels' specular power (rt_kernel_math.h: rt_pow_spec).  Plain C++ over a multiply functor - no device builtin, no address space -
// so that a host compiler reads the same text (tests/host/spec_walk_check.cpp holds every form below to the documented loop, bit for bit).
//
// The sequence, for bit i = 0, 1, ... of k:
//     r *= b   where bit i is set; the first such is r = b (it stands for r = 1.0 * b, which is exact: no multiply is issued for it),
//     b *= b   between bits, while a higher bit remains (no squaring behind the top bit: nobody would read it).
// Every form walks it in that order, so the result does not depend on the form:
//     documented loop     r = 1.0; do { if (k & 1) r *= b; b *= b; k >>= 1; } while (k);      (its last squaring is dead, its first product exact)
//     rt_spec_walk_gaps   from set bit to set bit (count-trailing-zeros), the multiplies unconditional - the form of the general path's
//                         uniform-exponent arm and of every kernel outside the few-sphere one-wave pair
//     rt_spec_walk_ladder a ladder of LADDER steps, one per bit above the lowest set one, each two tests on the condition code: "anything
//                         above?" in front of the squaring (the shift's own result) and the bit in front of the product; bits beyond the
//                         ladder (k >= 2^(LADDER + 1) at the least) continue in a loop of the same step
//     rt_spec_walk_lanes  k per lane: the documented loop itself, every lane squaring for as long as ANY lane has bits left (`any` is the
//                         wave-wide test; the squarings behind a lane's own top bit are read by no product of that lane)
// `mul(a, b)` is the product in the caller's arithmetic (binary64 a * b); k == 0 is the caller's (x^0 = 1, no multiply at all).
#ifndef RT_SPEC_WALK_H
#define RT_SPEC_WALK_H

#include <stdint.h>

#ifndef RT_SPEC_WALK_FN
#if defined(__HIPCC__)
#define RT_SPEC_WALK_FN __device__ __forceinline__
#else
#define RT_SPEC_WALK_FN static inline
#endif
#endif

template <class MUL>
RT_SPEC_WALK_FN double rt_spec_walk_gaps(uint32_t k, double x, MUL mul) {          // k != 0
  double b = x;
  uint32_t g = (uint32_t)__builtin_ctz(k);
  for (uint32_t i = 0; i < g; i++) b = mul(b, b);
  double r = b;
  for (k >>= g + 1u; k != 0u; k >>= g + 1u) {
    g = (uint32_t)__builtin_ctz(k);
    for (uint32_t i = 0; i <= g; i++) b = mul(b, b);
    r = mul(r, b);
  }
  return r;
}

// One step of the ladder and the steps above it.  Every step's way out is the fall through its own closing brace: all exits meet behind the
// outermost one, so no exit is carried as a flag.  RT_SPEC_WALK_PIN keeps a multiply inside the branch that decides it - a compiler may
// otherwise issue it unconditionally and select (one multiply more per clear bit).
#define RT_SPEC_WALK_PIN() asm volatile("")
template <int LEFT, class MUL>
RT_SPEC_WALK_FN void rt_spec_walk_step(uint32_t k, double &b, double &r, MUL mul) {
  if constexpr (LEFT > 0) {
    k >>= 1;
    if (k != 0u) {
      RT_SPEC_WALK_PIN();
      b = mul(b, b);
      if (k & 1u) { RT_SPEC_WALK_PIN(); r = mul(r, b); }
      rt_spec_walk_step<LEFT - 1>(k, b, r, mul);
    }
  } else {
    for (k >>= 1; k != 0u; k >>= 1) {                                              // bits beyond the ladder: the same step, as a loop
      b = mul(b, b);
      if (k & 1u) { RT_SPEC_WALK_PIN(); r = mul(r, b); }
    }
  }
}
template <int LADDER, class MUL>
RT_SPEC_WALK_FN double rt_spec_walk_ladder(uint32_t k, double x, MUL mul) {        // k != 0
  double b = x;
  const uint32_t g = (uint32_t)__builtin_ctz(k);                                    // up to the lowest set bit: r = b there
  for (uint32_t i = 0; i < g; i++) b = mul(b, b);
  k >>= g;
  double r = b;
  rt_spec_walk_step<LADDER>(k, b, r, mul);
  return r;
}

template <class MUL, class ANY>
RT_SPEC_WALK_FN double rt_spec_walk_lanes(uint32_t k, double x, MUL mul, ANY any) {
  double r = 1.0, b = x;
  do { if (k & 1u) r = mul(r, b); b = mul(b, b); k >>= 1; } while (any(k != 0u));
  return r;
}

#endif
