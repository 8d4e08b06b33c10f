// rt_uniform_pred.h - integer forms of floating-point predicates on a wave-uniform binary64 value, i.e. one that lies in a scalar register
// pair.  A floating-point compare of scalar operands is a VECTOR instruction whose result is a lane mask - v_cmp_*_f64 into a register pair,
// s_and_b64 vcc, exec and a branch through vcc; the integer form is scalar arithmetic that ends on the condition code.
// Plain C++ on the value's bit pattern, so that a host compiler reads the same text: tests/host/spec_walk_check.cpp holds each form to its
// floating-point statement over the edge patterns (+-0, denormals, 1, infinities, quiet and signalling NaNs, negative values).
#ifndef RT_UNIFORM_PRED_H
#define RT_UNIFORM_PRED_H

#include <stdint.h>

#ifndef RT_UNIFORM_PRED_FN
#if defined(__HIPCC__)
#define RT_UNIFORM_PRED_FN __device__ __forceinline__
#else
#define RT_UNIFORM_PRED_FN static inline
#endif
#endif

// x != 0.0, for EVERY pattern.  x == 0.0 holds for exactly two patterns, +0 (all bits clear) and -0 (the sign bit alone): the patterns whose
// 63 bits below the sign are all clear.  Every other pattern compares unequal to zero - denormals, normals and infinities of either sign because
// they are other numbers, NaNs of either kind because a NaN is unequal to everything - and has a bit set below the sign.  So x != 0.0 is
// "the pattern shifted left by one is not zero": one 64-bit scalar shift, whose condition code is that test.
RT_UNIFORM_PRED_FN bool rt_nonzero_bits(uint64_t bits) { return (bits << 1) != 0u; }

#endif
