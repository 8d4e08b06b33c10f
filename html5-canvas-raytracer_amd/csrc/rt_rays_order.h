// Ordering a caller's ray list on the GPU (rt_rays_order.hip), shared with its host side (rt_launch.hip, rt_frame.hip).  Not part of
// the ABI.
#ifndef RT_RAYS_ORDER_H
#define RT_RAYS_ORDER_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// A sort tile: what one workgroup of RT_ORDER_WG work-items ranks per pass (RT_ORDER_ITEMS keys per work-item, one wave owning
// 64 x RT_ORDER_ITEMS consecutive keys of it).
#define RT_ORDER_WG 256u
#define RT_ORDER_ITEMS 16u
#define RT_ORDER_TILE (RT_ORDER_WG * RT_ORDER_ITEMS)
#define RT_ORDER_DIGITS 256u     // 8-bit digits: four passes over a 32-bit key

// The workspace of an ordering of n rays (1 <= n < 2^31), in bytes from its start: the list's bounds (10 words in 256 bytes), the
// digit totals of the current pass, the per-tile digit counts (digit-major), two key arrays and one index array (the caller's
// order buffer is the other).  Every part starts on a 256-byte boundary of the workspace.
struct rt_order_layout { size_t bounds, totals, hist, keys_a, keys_b, idx, bytes; uint32_t tiles; };
static inline rt_order_layout rt_order_layout_of(uint64_t n) {
  rt_order_layout l;
  l.tiles = (uint32_t)((n + RT_ORDER_TILE - 1u) / RT_ORDER_TILE);
  const size_t list = (((size_t)n * 4u) + 255u) & ~(size_t)255u;
  l.bounds = 0;
  l.totals = 256u;
  l.hist = l.totals + RT_ORDER_DIGITS * 4u;
  l.keys_a = l.hist + ((((size_t)l.tiles * RT_ORDER_DIGITS * 4u) + 255u) & ~(size_t)255u);
  l.keys_b = l.keys_a + list;
  l.idx = l.keys_b + list;
  l.bytes = l.idx + list;
  return l;
}

// The workgroups (of RT_ORDER_WG work-items, one ray each per turn) of rt_order_bounds and rt_order_keys for a list of n rays: capped, a
// grid-stride loop takes the rays beyond RT_ORDER_MAX_WGS x RT_ORDER_WG.
#define RT_ORDER_MAX_WGS 4096u
static inline uint32_t rt_order_grid(uint32_t n) {
  const uint32_t wgs = (uint32_t)(((uint64_t)n + RT_ORDER_WG - 1u) / RT_ORDER_WG);
  return wgs < RT_ORDER_MAX_WGS ? wgs : RT_ORDER_MAX_WGS;
}

// Enqueues the ordering of rays [0, n) on `stream`: bounds, keys, four radix passes; d_order receives the permutation.  Returns a
// hipError_t as int.
extern "C" int rt_launch_order_rays(uint32_t n, const double *d_rays, uint32_t *d_order, void *d_work, hipStream_t stream);

#endif
