// rt_probe.hip — gathered light for SHORT receiver lists, and its weighted sums (include/rt_hip.h: rt_probe_outputs,
// rt_scene_gather_probes_device).  rt_gather_kernel gives a receiver one lane, so 64 probes of 1024 samples are one wave that walks 1024
// trees one after another.  Here a receiver has a WORKGROUP and its samples have the lanes.  Nothing is new arithmetic: the table entry,
// the receiver, the segment and the walk of a sample are the calls rt_gather_kernel makes, with the same arguments, and the fold is its
// fold in its order - so the plain outputs are rt_gather_kernel's, byte for byte (tests/test_gpu_probes.py).  Built as rt_gather.hip is:
// KFLAGS, without FMA contraction, with the strict side of rt_kernel_math.h; no test switches: one object for both libraries.  One kernel:
//   rt_probe_kernel    workgroup j of the grid takes receiver order[j] (or j); an entry >= n ends the whole workgroup before anything
//                      else - the only early exit, workgroup-uniform, ahead of the barrier.  B = min(CAP, 64 ceil(n_samples / 64))
//                      lanes; lane t traces samples t, t + B, t + 2 B, ... and puts colour c_s into LDS slot s (24 bytes; dynamic LDS,
//                      24 n_samples bytes <= 24 576: a static array of that size would cap a CU at six one-wave workgroups where
//                      n_samples is small).  A lane with no sample left skips the walk and waits at the barrier.  Behind that ONE
//                      barrier the first wave folds: a lane per chain, every chain in list order - acc = c_0; acc = acc + c_s - with
//                      no FMA, no tree and no cross-lane addition, then the one division by (double)n_samples.  The plain chains are
//                      three (lanes 48..50); the weighted ones 3 n_weights (lane 3 k + ch: acc = w[e_0][k] * c_0[ch];
//                      acc = acc + (w[e_s][k] * c_s[ch])), e_s being the table entry sample s took its direction from.  rgba is
//                      packed by lane 48 from the three means (handed over by a lane read, not by arithmetic).
// Why the fold is serial: a tree or a cross-lane sum adds in another order, and binary64 addition is not associative - the result would
// no longer be rt_gather_kernel's bytes, nor the numpy fold's.  The chains' loads do not depend on each other, only the additions do:
// n_samples dependent adds of one wave, measured in docs/EVIDENCE.md, "Probes".
// An unscanned receiver is no special case here either: its segments are six NaNs, the walk returns its NaNs, and they are folded.
// CAP is 1024: __launch_bounds__(1024) leaves a lane 128 VGPRs, which is what the walk's two other users (rt_soft_trace,
// rt_gather_kernel) are built at, and the kernel fits them with no spilled register (tests/test_probe_resources.py reads the code
// object: 112 VGPRs).  The record is read inside the sample loop through a volatile pointer, as rt_gather_kernel reads it and for a like
// reason: every lane of the workgroup reads the same 80 bytes (one cache line, broadcast), and nothing of the receiver is live across
// the walk; read once outside the loop, the workgroup-uniform record and frame are kept in scalar registers across the walk, which then
// spills 20 SGPRs (and takes 123 VGPRs).  With n_samples <= 1024 every lane traces at most ONE sample.  The stack is the walk's own
// scratch array: rt_soft_trace's bytes per lane.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rt_probe.h"

namespace {
#define RT_STRICT 1
#define RT_INF __builtin_inf()
#include "rt_kernel_math.h"      // the strict side: what rt_soft_walk.h needs, and to_byte (the store rule of main.js:195-198)
#include "rt_soft_walk.h"        // soft_walk
}  // namespace

extern __shared__ double probe_colours[];                            // slot s: c_s, three doubles

__global__ void __launch_bounds__(RT_PROBE_CAP) rt_probe_kernel(const rt_probe_launch P) {
  const rt_gather_launch &L = P.G;
  const uint32_t i = L.S.order ? L.S.order[blockIdx.x] : blockIdx.x;   // (blockIdx.x < n: the grid is n workgroups)
  if (i >= L.S.n) return;                                            // an order's entry that names no receiver: the whole workgroup
  const volatile rt_hit *H = L.hits + i;                             // (read inside the loop: see the header comment; the address is workgroup-uniform)
  const amb_walk W = amb_walk_of(L.base, i, L.stride, L.n_dirs);
  const amb_walk none = {0u, 0u};                                    // (the walk's table: read by its relit branch only)
  const uint32_t ns = L.n_samples, t = threadIdx.x;
  for (uint32_t s = t; s < ns; s += P.block) {
    const double *d = L.dirs + 3u * (size_t)(L.stride == 0u ? s : amb_walk_entry(W, s, L.n_dirs));   // (stride 0: e = s < n_samples <= n_dirs)
    const double d0 = d[0], d1 = d[1], d2 = d[2];
    // the segment of (i, s): rt_ambient.h's, six NaNs for a receiver that is not scanned
    const amb_receiver R = amb_receiver_of(H->object, H->inside, H->point[0], H->point[1], H->point[2], H->normal[0], H->normal[1], H->normal[2]);
    double seg[6];
    amb_segment(R, d0, d1, d2, seg);
    lit_ray ray;
    ray.ox = seg[0]; ray.oy = seg[1]; ray.oz = seg[2]; ray.rx = seg[3]; ray.ry = seg[4]; ray.rz = seg[5];
    ray.finite = lit_finite6(seg[0], seg[1], seg[2], seg[3], seg[4], seg[5]);   // (rt_soft_trace's rule: a ray that is not finite gives NaN x 3)
    double c[3];
    soft_walk<false>(L.S, ray, L.pix_base + s * L.pix_stride + i, none, c);
    double *slot = probe_colours + 3u * s;
    slot[0] = c[0]; slot[1] = c[1]; slot[2] = c[2];
  }
  __syncthreads();
  if (t >= 64u) return;                                              // the first wave folds
  const double nsd = (double)ns;
  const uint32_t nw = P.n_weights;
  if (t < 3u * nw) {                                                 // chain (k, ch) of the weighted sums
    const uint32_t k = t / 3u, ch = t - 3u * k;
    const double *wk = P.weights + k;
    double acc = wk[(size_t)(L.stride == 0u ? 0u : amb_walk_entry(W, 0u, L.n_dirs)) * nw] * probe_colours[ch];
#pragma unroll 8
    for (uint32_t s = 1; s < ns; s++) {                              // (unrolled: the loads of eight terms are in flight, the additions keep their order)
      const uint32_t e = L.stride == 0u ? s : amb_walk_entry(W, s, L.n_dirs);
      acc = acc + (wk[(size_t)e * nw] * probe_colours[3u * s + ch]);
    }
    P.coef[(size_t)i * (3u * nw) + t] = acc / nsd;
  }
  const bool plain = t >= RT_PROBE_PLAIN_LANE && t < RT_PROBE_PLAIN_LANE + 3u && (L.S.rgb || L.S.rgba);
  double mean = 0.0;
  if (plain) {                                                       // chain ch of the mean
    const uint32_t ch = t - RT_PROBE_PLAIN_LANE;
    double acc = probe_colours[ch];
    for (uint32_t s = 1; s < ns; s++) acc = acc + probe_colours[3u * s + ch];
    mean = acc / nsd;
    if (L.S.rgb) L.S.rgb[3u * (size_t)i + ch] = mean;
  }
  if (L.S.rgba) {                                                    // (wave-uniform: every lane of the first wave takes part in the reads)
    const double r = __shfl(mean, (int)RT_PROBE_PLAIN_LANE), g = __shfl(mean, (int)RT_PROBE_PLAIN_LANE + 1), b = __shfl(mean, (int)RT_PROBE_PLAIN_LANE + 2);
    if (t == RT_PROBE_PLAIN_LANE) L.S.rgba[i] = to_byte(r) | (to_byte(g) << 8) | (to_byte(b) << 16) | 0xff000000u;
  }
}

extern "C" int rt_launch_probe(const rt_probe_launch *L, void *hip_stream) {
  hipLaunchKernelGGL(rt_probe_kernel, dim3(L->G.S.n), dim3(L->block), 24u * L->G.n_samples, (hipStream_t)hip_stream, *L);   // (n < 2^31)
  return (int)hipGetLastError();
}

extern "C" int rt_probe_scratch(size_t *bytes_per_lane) {
  hipFuncAttributes fa;
  const hipError_t e = hipFuncGetAttributes(&fa, (const void *)rt_probe_kernel);
  if (e == hipSuccess) *bytes_per_lane = (size_t)fa.localSizeBytes;
  return (int)e;
}
