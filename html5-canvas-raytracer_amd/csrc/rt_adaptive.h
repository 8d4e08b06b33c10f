// rt_adaptive.h — adaptive supersampling (include/rt_hip.h: rt_render_adaptive_device): the criterion that picks the pixels to refine
// and the box rule that makes a pixel of its k x k samples, written once for the host (the test build's rt_test_adaptive_mask, a plain
// loop) and for the device (rt_adaptive.hip: rt_adaptive_mark, rt_adaptive_refine); and the launch records of those kernels, shared
// with their host side (rt_launch.hip).  Integer arithmetic on stored bytes: the two builds give the same answers.  Not part of the ABI.
#ifndef RT_ADAPTIVE_H
#define RT_ADAPTIVE_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef RT_HD
#define RT_HD __host__ __device__
#endif
#else
#ifndef RT_HD
#define RT_HD
#endif
#endif

// The largest of |R - R'|, |G - G'|, |B - B'| of two stored pixels (0xAABBGGRR: R in the low byte; alpha plays no part): 0..255.
RT_HD inline uint32_t rt_adaptive_diff(uint32_t a, uint32_t b) {
  uint32_t m = 0u;
  for (uint32_t sh = 0u; sh < 24u; sh += 8u) {
    const uint32_t x = (a >> sh) & 255u, y = (b >> sh) & 255u, d = x > y ? x - y : y - x;
    m = d > m ? d : m;
  }
  return m;
}

// Is pixel `c` refined?  It is iff one of its 4-neighbours inside the frame differs from it by at least `threshold` (0..256) in some
// colour channel.  A neighbour outside the frame is handed over as `c` itself (difference 0): so threshold 0 refines every pixel, a
// 1 x 1 frame's included, and threshold 256 none.
RT_HD inline bool rt_adaptive_refines(uint32_t c, uint32_t left, uint32_t right, uint32_t up, uint32_t down, uint32_t threshold) {
  uint32_t m = rt_adaptive_diff(c, left);
  const uint32_t r = rt_adaptive_diff(c, right), u = rt_adaptive_diff(c, up), d = rt_adaptive_diff(c, down);
  m = r > m ? r : m; m = u > m ? u : m; m = d > m ? d : m;
  return m >= threshold;
}

// One channel of a refined pixel from the sum of its k x k sample bytes: the box rule of the two-pass supersampling (rt_launch.hip:
// rt_box_filter_kernel) and, for k = 2, of the trace kernels' quad.
RT_HD inline uint32_t rt_adaptive_box(uint32_t sum, uint32_t k) { return (sum + k * k / 2u) / (k * k); }

// The workspace: word 0 the number of refined pixels, words 1..3 unused, then one word x | y << 16 per refined pixel (at most w * h).
#define RT_ADAPTIVE_HEADER_BYTES 16u
static inline uint64_t rt_adaptive_bytes(uint64_t w, uint64_t h) { return RT_ADAPTIVE_HEADER_BYTES + 4u * w * h; }

// The refine launch's grid for a w x h frame at k x k samples: a workgroup is RT_ADAPTIVE_REFINE_WAVES waves and a wave holds 64 / (k k)
// listed pixels per turn of its grid-stride loop (rt_adaptive.hip: rt_adaptive_refine).  The count is only known on the device, so the
// grid is sized for the whole frame and capped; a list longer than one turn of the capped grid takes further turns.
#define RT_ADAPTIVE_REFINE_WAVES 4u                                   // (RT_WG_THREADS / 64: rt_launch.hip holds the two to each other)
#define RT_ADAPTIVE_REFINE_MAX_WGS 8192u                              // (measured at 3840x2160: 2048, 1024, 512, 256 workgroups are each slower: docs/EVIDENCE.md)
static inline uint32_t rt_adaptive_refine_grid(uint32_t w, uint32_t h, uint32_t k) {
  const uint64_t per_wg = (uint64_t)RT_ADAPTIVE_REFINE_WAVES * (64u / (k * k)), wgs = ((uint64_t)w * h + per_wg - 1u) / per_wg;
  return (uint32_t)(wgs < RT_ADAPTIVE_REFINE_MAX_WGS ? wgs : RT_ADAPTIVE_REFINE_MAX_WGS);
}

#if defined(__HIPCC__)
// rt_adaptive_mark's arguments (by value in the kernarg segment)
struct rt_adaptive_mark_launch {
  const uint32_t *frame;             // the base frame, w x h RGBA8
  uint8_t *mask;                     // w x h bytes, 1 = refined; or NULL
  uint32_t *work;                    // the workspace (above); word 0 is zero when the kernel starts
  uint32_t w, h, threshold;
};
// rt_adaptive_refine's second argument; its first is the rt_launch of the k w x k h SAMPLE grid (rt_device.h), bound as rt_retrace's
struct rt_adaptive_refine_launch {
  const uint32_t *work;              // the workspace rt_adaptive_mark filled
  uint32_t *out;                     // the frame, w x h RGBA8
  uint32_t w;                        // its width in PIXELS (the record's w is the sample grid's)
};
struct rt_launch;
extern "C" int rt_launch_adaptive_mark(const rt_adaptive_mark_launch *M, hipStream_t stream);
// (refract: the scene's kernel variant; k: 2, 3 or 4; n_wg workgroups of a grid-stride loop.)  Both return a hipError_t as int.
extern "C" int rt_launch_adaptive_refine(const rt_launch *L, const rt_adaptive_refine_launch *A, int refract, uint32_t k, unsigned n_wg, hipStream_t stream);
// the scratch (private segment) bytes per lane of rt_adaptive_refine<refract, k>, from the code object
extern "C" int rt_scratch_adaptive_refine(int refract, uint32_t k, size_t *bytes_per_lane);
#endif

#endif
