// Launch record of the probe kernel (rt_probe.hip), shared with its host side (rt_probe_api.hip).  Not part of the ABI.
#ifndef RT_PROBE_H
#define RT_PROBE_H

#include "rt_gather.h"        // rt_gather_launch: the record the receivers mapping reads, taken as it is

#define RT_PROBE_CAP 1024u               // lanes per workgroup at most (rt_probe.hip's header comment says why)
// (RT_PROBE_MAX_WEIGHTS, include/rt_hip.h: 3 * 16 = 48 chains, one wave folds them all)
#define RT_PROBE_PLAIN_LANE 48u         // the three plain chains' lanes of the first wave: behind the weighted ones

static_assert(3u * RT_PROBE_MAX_WEIGHTS <= RT_PROBE_PLAIN_LANE && RT_PROBE_PLAIN_LANE + 3u <= 64u, "every chain has a lane of the first wave");

// Passed by value in the kernel arguments: everything here is wave-uniform.
struct rt_probe_launch {
  rt_gather_launch G;              // as rt_gather_kernel reads it; G.S.n receivers = workgroups
  const double *weights;           // n_dirs rows of n_weights doubles, or NULL (8-byte aligned)
  double *coef;                    // n x n_weights x 3, or NULL
  uint32_t n_weights;              // 0..RT_PROBE_MAX_WEIGHTS; 0: weights and coef are NULL
  uint32_t block;                  // B = min(RT_PROBE_CAP, 64 * ceil(n_samples / 64)): lanes per workgroup
};

// B for n_samples (1..1024)
inline uint32_t rt_probe_block(uint32_t n_samples) {
  const uint32_t b = 64u * ((n_samples + 63u) / 64u);
  return b < RT_PROBE_CAP ? b : RT_PROBE_CAP;
}

// Asynchronous on `hip_stream` (a hipStream_t); returns a hipError_t as int.
extern "C" int rt_launch_probe(const rt_probe_launch *L, void *hip_stream);
// the kernel's private segment, bytes per lane, from the code object (for the scratch guard); returns a hipError_t as int
extern "C" int rt_probe_scratch(size_t *bytes_per_lane);

#endif
