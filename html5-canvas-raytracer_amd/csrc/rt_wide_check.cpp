// rt_wide_check.cpp - stand-alone check of rt_wide.h (no GPU, no library): for frames cut into launch-table entries the way a launch
// table cuts them - traced blocks and sky runs of every length, partial right-edge blocks, partial last row blocks - the 16-byte stores
// the header enumerates are aligned, lie inside the frame and cover every pixel of the frame exactly once.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined rt_wide_check.cpp -o rt_wide_check && ./rt_wide_check
// (tests/test_wide_stores.py builds and runs it that way.)  Exit status 0 and "ok <stores>" on stdout, or the first violation.
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "rt_wide.h"

static int check_frame(uint32_t w, uint32_t h, bool ss2, uint32_t seed, unsigned long long *n_stores) {
  const uint32_t block_h = ss2 ? 2u : 8u, tiles_x = (w + RT_WIDE_BLOCK_W - 1u) / RT_WIDE_BLOCK_W;
  std::vector<uint8_t> hits((size_t)w * h, 0);          // allocated to the byte: a store outside it is the sanitizer's to report
  int bad = 0;
  for (uint32_t row0 = 0; row0 < h; row0 += block_h) {
    const uint32_t rows_valid = (h - row0 < block_h) ? h - row0 : block_h;
    for (uint32_t x = 0; x < tiles_x;) {
      seed = seed * 1664525u + 1013904223u;
      const bool sky = (seed >> 16) & 1u;
      uint32_t run = sky ? 1u + ((seed >> 20) % 11u) : 1u;
      if (run > tiles_x - x) run = tiles_x - x;
      const uint32_t e0 = x | (rows_valid << 11) | (row0 << 15), e1 = row0 | (sky ? ((run - 1u) << 24) | 0x80000000u : 0u);
      rt_wide_entry_stores(e0, e1, ss2, w, [&](uint32_t, uint32_t lrow, uint32_t px) {
        ++*n_stores;
        if ((px & 3u) != 0u || lrow >= h || px + RT_WIDE_PIXELS > w) { printf("w %u h %u ss2 %d: store at row %u pixel %u\n", w, h, (int)ss2, lrow, px); bad = 1; return; }
        for (uint32_t k = 0; k < RT_WIDE_PIXELS; k++) hits[(size_t)lrow * w + px + k]++;
      });
      x += run;
    }
  }
  for (size_t i = 0; i < hits.size() && !bad; i++)
    if (hits[i] != 1u) { printf("w %u h %u ss2 %d: pixel %zu stored %u times\n", w, h, (int)ss2, i, (unsigned)hits[i]); bad = 1; }
  return bad;
}

int main() {
  static const uint32_t widths[] = {4, 8, 28, 32, 36, 60, 64, 68, 132, 640, 3840}, heights[] = {1, 2, 3, 7, 8, 9, 17};
  unsigned long long n_stores = 0;
  for (uint32_t w : widths) for (uint32_t h : heights) for (int ss2 = 0; ss2 < 2; ss2++) for (uint32_t seed = 1; seed <= 3; seed++)
    if (check_frame(w, h, ss2 != 0, seed * 2654435761u, &n_stores)) return 1;
  printf("ok %llu\n", n_stores);
  return 0;
}
