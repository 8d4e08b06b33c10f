// rt_wide.h - the 16-byte frame stores of the product trace kernels (rt_kernel.hip, A10): which lane of a wave stores which four
// pixels of its launch-table entry's blocks.  Stated once: the kernel includes it, and so does a plain host compiler (the test build's
// probe rt_test_wide_stores in rt_api.hip and the stand-alone check rt_wide_check.cpp), which enumerate a launch's stores from its table.
//
// A launch takes these stores when every group of four pixels lies wholly inside or outside the frame and every such group is
// 16-byte aligned in memory (rt_device.h: rt_wide_stores_of).  Then
//   * a TRACED block (32 x 8 pixels, or 32 x 2 with supersample 2) is four waves, wave k rendering the 8-pixel column k: a wave's piece
//     of a row is 8 pixels = two stores.  Supersample 1: lane = 8 * row + x; the lanes with lane % 4 == 0 store the pixels of lanes
//     lane .. lane + 3.  Supersample 2: lane = 4 * (8 * row + x) + sample; the lanes with lane % 16 == 0 store the pixels of lanes lane,
//     lane + 4, lane + 8, lane + 12.  Either way a group lies inside one 16-lane row of the wave (a DPP row shift reaches it).
//   * a SKY RUN of n blocks is stored block by block, block t of the run by wave t % 4 of the entry: ONE store instruction per block,
//     lane l storing pixels 4 * (l % 8) .. + 3 of row l / 8 - eight whole 128-byte lines.
// A store is made when its row is below the entry's rows_valid and its first pixel is below the frame's width.
#ifndef RT_WIDE_H
#define RT_WIDE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define RT_WIDE_HD __host__ __device__
#else
#define RT_WIDE_HD
#endif

#define RT_WIDE_PIXELS 4u            /* pixels of one store */
#define RT_WIDE_BLOCK_W 32u          /* pixels across a block (RT_TILE_W) */

/* one lane's store: the row of the block, the first pixel's column in the block (a multiple of 4), and whether the lane stores at all */
struct rt_wide_piece { uint32_t row, col; bool stores; };

/* lanes between the pixels of a group: the group of lane l is l, l + step, l + 2 step, l + 3 step */
static inline RT_WIDE_HD uint32_t rt_wide_lane_step(bool ss2) { return ss2 ? 4u : 1u; }

/* a traced block: lane `lane` of the wave that renders column `wave` of the block */
static inline RT_WIDE_HD rt_wide_piece rt_wide_traced(bool ss2, uint32_t wave, uint32_t lane) {
  const uint32_t slot = ss2 ? lane >> 2 : lane;        /* the lane's pixel of the wave's 8 x 8 (8 x 2) block */
  rt_wide_piece p;
  p.row = slot >> 3;
  p.col = wave * 8u + (slot & 7u);
  p.stores = (lane & (4u * rt_wide_lane_step(ss2) - 1u)) == 0u;
  return p;
}

/* a sky run: lane `lane` of the wave that stores a block of the run (block t: wave t % 4, at column 32 t of the run) */
static inline RT_WIDE_HD rt_wide_piece rt_wide_sky(uint32_t lane) {
  rt_wide_piece p;
  p.row = lane >> 3;
  p.col = RT_WIDE_PIXELS * (lane & 7u);
  p.stores = true;
  return p;
}

/* Host side: every store of ONE launch-table entry (words 0 and 1: rt_kernel_entry.h) of a frame `w` pixels wide, as the kernel's
 * epilogue makes them: emit(wave of the entry, row in the call's output band, first pixel).  The kernel states the same two loops. */
template <class F>
static inline void rt_wide_entry_stores(uint32_t e0, uint32_t e1, bool ss2, uint32_t w, F emit) {
  const uint32_t px0 = (e0 & 2047u) * RT_WIDE_BLOCK_W, rows_valid = (e0 >> 11) & 15u, lrow0 = e1 & 0xffffffu;
  if (e1 >> 31) {                                      /* a sky run */
    const uint32_t run = ((e1 >> 24) & 127u) + 1u;
    for (uint32_t t = 0; t < run; t++)
      for (uint32_t lane = 0; lane < 64u; lane++) {
        const rt_wide_piece p = rt_wide_sky(lane);
        const uint32_t px = px0 + t * RT_WIDE_BLOCK_W + p.col;
        if (p.stores && p.row < rows_valid && px < w) emit(t & 3u, lrow0 + p.row, px);
      }
  } else {
    for (uint32_t wave = 0; wave < 4u; wave++)
      for (uint32_t lane = 0; lane < 64u; lane++) {
        const rt_wide_piece p = rt_wide_traced(ss2, wave, lane);
        if (p.stores && p.row < rows_valid && px0 + p.col < w) emit(wave, lrow0 + p.row, px0 + p.col);
      }
  }
}

#endif
