// rt_kernel_entry.h - which pixel (or sample) a work-item owns: the launch-table entry of its workgroup (product build) or the plain
// grid (strict build), the entry's shadow masks, the launch record as the cold paths read it, and the mark list's append.
// A fragment: included once by rt_kernel.hip, inside its anonymous namespace.

// Which pixel (or sample) a work-item owns.  Evaluated twice from the work-item id — before the ray is generated and
// again after the trace, behind an opaque copy of the id — so that px / lrow / valid are not kept live in VGPRs across
// the whole trace (they would be the 97th register: the kernel fits the 96 of 5 waves per SIMD without them).
struct rt_pixel { uint32_t px, trow, frow, lrow, sub, rows_valid, run, cand, cell; bool valid, sky; };
// W1 - ONE-WAVE workgroups (the reflection-only many-sphere variants, rt_trace): the entry's 32 x 8 block is rendered by FOUR
// workgroups of one wave each, workgroup b = xcd + 8 * (wave + 4 * e') for entry e = 8 e' + xcd: the four waves of a block are
// consecutive workgroups of ONE XCD, and an XCD still reads one contiguous eighth of the table.
template <bool W1>
__device__ __forceinline__ uint32_t rt_entry_slot(const rt_launch &L) {
  // entry of workgroup b at (b % 8) * ceil(n / 8) + b / 8: workgroups are dealt round-robin over the 8 XCDs (speed only, never
  // correctness), so each XCD's L2 reads one contiguous eighth of the table instead of every line of it
  return (blockIdx.x & 7u) * L.order_n8 + (blockIdx.x >> (W1 ? 5 : 3));
}
// (the entry's index in the table's order: a compact band's block number)
template <bool W1>
__device__ __forceinline__ uint32_t rt_entry_index() { return W1 ? (((blockIdx.x >> 5) << 3) | (blockIdx.x & 7u)) : blockIdx.x; }
// (which of the block's four 8-pixel columns this wave renders)
template <bool W1>
__device__ __forceinline__ uint32_t rt_wave_of(uint32_t tid) { return W1 ? ((blockIdx.x >> 3) & 3u) : tid >> 6; }

// The few-sphere one-wave kernels ask for the work-item id AGAIN where it is needed behind the primary test (a marked sample, the stars'
// pixel index, the epilogue) WITHOUT keeping even the id's own register live across the trace: a one-wave workgroup's work-item id IS its
// lane id, and v_mbcnt rebuilds that exactly under any exec mask (one of the 80 VGPRs that six waves per SIMD allow).  volatile: not merged
// with an earlier one.  Every other kernel keeps its opaque copy of threadIdx.x at those places.
__device__ __forceinline__ uint32_t rt_lane_again() {
  uint32_t x;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(x));
  return x;
}

#if RT_STRICT
template <bool SS2, bool W1 = false>
__device__ __forceinline__ rt_pixel rt_pixel_of(const rt_launch &L, uint32_t tid) {
  const uint32_t wave = tid >> 6, lane = tid & 63u;
  // grid = (tiles across the frame, tiles x row blocks per tile, frames of the batch).  y splits into
  // (tile, row block) with a shift when row blocks per tile is a power of two (the 16-row tiles of the
  // multi-GPU plan), trivially for a single tile (a whole frame), else with one wave-uniform division.
  const uint32_t tile_x = blockIdx.x, by = blockIdx.y;
  uint32_t tile_i, row_block;
  if (L.n_tiles == 1u) { tile_i = 0u; row_block = by; }
  else if (L.rb_shift != ~0u) { tile_i = by >> L.rb_shift; row_block = by & ((1u << L.rb_shift) - 1u); }
  else { tile_i = by / L.rb_per_tile; row_block = by - tile_i * L.rb_per_tile; }
  rt_pixel P;
  P.sub = 0u;                                          // trow = row inside tile `tile_i`
  if (!SS2) { P.px = tile_x * RT_TILE_W + wave * 8u + (lane & 7u); P.trow = row_block * RT_TILE_H + (lane >> 3); }
  else { const uint32_t q = lane >> 2; P.sub = lane & 3u; P.px = tile_x * RT_TILE_W + wave * 8u + (q & 7u); P.trow = row_block * 2u + (q >> 3); }
  P.frow = (L.tile_first + tile_i * L.tile_stride) * L.tile_rows + P.trow;   // frame row
  P.lrow = tile_i * L.tile_rows + P.trow;                                    // row in this call's output band
  P.valid = (P.px < L.w) && (P.trow < L.tile_rows) && (P.frow < L.h);
  P.rows_valid = 0u;                                   // (product kernel only)
  P.sky = false; P.run = 1u; P.cand = 0u; P.cell = 0u;
  return P;
}
#else
// Product kernel: a FLAT grid (workgroups, 1, frames of the batch) and a launch table with one 16-byte entry per workgroup:
//   word 0 = tile_x | rows_valid << 11 | first frame row << 15      word 1 = first row in this call's output band | (run - 1) << 24 | sky << 31, or (bit 31 clear) | second-node bits << 24
//   word 2 = shadow masks                                            word 3 = primary candidates | checker cells << 18, or (bit 31) | first-bounce set << 18
// (built on the GPU per camera, frame size and tile set: rt_tables_gpu.hip, rt_block.h).  One scalar load replaces the tile /
// row-block arithmetic of the plain grid - no division, no tile parameters in registers - and decides the ORDER in which the
// hardware hands the tiles out: dearest first, so that a launch ends on cheap sky tiles instead of on the floor.  trow is the row
// inside the workgroup's block here.  (W1: rt_entry_slot above.)
template <bool SS2, bool W1 = false>
__device__ __forceinline__ rt_pixel rt_pixel_of(const rt_launch &L, uint32_t tid) {
  const uint32_t wave = rt_wave_of<W1>(tid), lane = tid & 63u;
  typedef uint32_t __attribute__((ext_vector_type(4))) rt_entry;                                     // 16 bytes (rt_tables.h: RT_ENTRY_WORDS)
  typedef const rt_entry __attribute__((address_space(4))) *order_kptr;
  const uint32_t slot = rt_entry_slot<W1>(L);
  const rt_entry e4 = *(order_kptr)((const char __attribute__((address_space(4))) *)L.order + ((size_t)slot << 4));   // s_load_dwordx4
  const uint32_t e0 = e4.x, e1 = e4.y;
  const uint32_t tile_x = e0 & 2047u, rows_valid = (e0 >> 11) & 15u, frow0 = e0 >> 15;
  rt_pixel P;
  P.sub = 0u;
  if (!SS2) { P.px = tile_x * RT_TILE_W + wave * 8u + (lane & 7u); P.trow = lane >> 3; }
  else { const uint32_t q = lane >> 2; P.sub = lane & 3u; P.px = tile_x * RT_TILE_W + wave * 8u + (q & 7u); P.trow = q >> 3; }
  P.frow = frow0 + P.trow;
  P.lrow = (e1 & 0xffffffu) + P.trow;
  P.sky = (e1 >> 31) != 0u;                            // workgroup-uniform: no sphere can show in these blocks (rt_block.h) ...
  P.run = ((e1 >> 24) & 127u) + 1u;                    // ... a run of this many 32-pixel blocks, starting at tile_x (read beside P.sky only: without bit 31 these bits are the entry's second-node bits, rt_entry_second_node below)
  P.cand = e4.w & RT_CAND_MASK;                        // the (at most two) loop spheres the block's primary rays can meet (count << 16 | second << 8 | first), or 0: cull
  // (an entry with bit 31 holds a first-bounce set in these bits instead: rt_entry_first_bounce below.  Its one candidate is then a mirror at a depth that
  // lets it reflect, and the uniform-material path - the only reader of the cells - turns the wave away by its material before it reads one: rt_block.h)
  P.cell = e4.w >> RT_CELL_SHIFT;                      // checker cells of a one-candidate block (rt_block.h: rt_column_cell): bit c - column c lies inside ONE cell, bit 4 + c - its parity
  P.rows_valid = rows_valid;                           // wave-uniform: rows of the block inside its tile and the frame
  P.valid = (P.px < L.w) && (P.trow < rows_valid);
  return P;
}
#endif

#if !RT_STRICT
// The HEAD BATCH of the few-sphere one-wave kernels: every launch-record field that the prologue, the ray generation and a one-candidate
// wave's anchored test read and that does not depend on the launch-table entry, used by ONE empty asm statement placed behind the
// entry's load (rt_trace, after rt_pixel_of).  The use keeps each field's scalar load in the kernel's first block - the compiler
// otherwise sinks every load to its first use, and a one-candidate wave then stands through a wait per field on its way to its
// primary root - where they go out beside the entry's load: the entry is unique to the wave (L2 or HBM), the fields hit the scalar
// cache, and the one wait for the entry covers them all.  Every later read of these fields is the same load; all of them are consumed
// by the end of the ray generation or were live across the kernel before (n_objects, epsilon, the image).  Headline +1.5 %; the same
// batch at the kernel's top, ahead of the table pointer's wait, +1.0 % (docs/EVIDENCE.md, first section).
__device__ __forceinline__ void rt_head_batch(const rt_launch &L) {
  asm volatile("" :: "s"(L.order), "s"(L.order_n8), "s"(L.n_objects), "s"(L.n_loop), "s"(L.segs), "s"(L.objects), "s"(L.geom_cam), "s"(L.lds_image),
               "s"(L.cam_origin[0]), "s"(L.cam_origin[1]), "s"(L.cam_origin[2]), "s"(L.ray_bias[0]), "s"(L.ray_bias[1]), "s"(L.ray_bias[2]),
               "s"(L.cam_axis_sum[0]), "s"(L.cam_axis_sum[1]), "s"(L.epsilon));
}
// Word 2 of this workgroup's launch-table entry: per light, the 16-bit set of loop-order spheres that can shadow a primary hit of
// its block (rt_block.h), or ~0u.  Read again where it is used - the primary node's lighting - instead of being kept in a
// scalar register across the cull and the search (the kernel has none to spare).
template <bool W1>
__device__ __forceinline__ uint32_t rt_entry_shadow_masks(const rt_launch &L) {
  const uint32_t slot = rt_entry_slot<W1>(L);
  return *(const uint32_t __attribute__((address_space(4))) *)((const char __attribute__((address_space(4))) *)L.order + ((size_t)slot << 4) + 8u);
}
// Word 3 of this workgroup's launch-table entry, for its first-bounce set (rt_block.h: rt_first_bounce_set): bit 31 - bits 18..30 name the loop
// spheres a ray reflected at a primary hit of the block can meet.  Read again where it is used - the node after the primary - like word 2.
template <bool W1>
__device__ __forceinline__ uint32_t rt_entry_first_bounce(const rt_launch &L) {
  const uint32_t slot = rt_entry_slot<W1>(L);
  return *(const uint32_t __attribute__((address_space(4))) *)((const char __attribute__((address_space(4))) *)L.order + ((size_t)slot << 4) + 12u);
}
// Word 1 of this workgroup's launch-table entry, for its second-node bits (rt_block.h: rt_second_node_bits; bits 24..28 of an entry that
// states a first-bounce set, zero in every other entry that is no sky run): bit 24 / 25 - the first-bounce walk may leave out candidate 0 / 1,
// bit 26 - nothing is left of the set then: every reflected ray of the block meets no loop sphere; bits 27 / 28 - nothing can shadow that
// node's hits from light 0 / 1 (in no launch's table).  The kernels read bits 24 and 25 ALONE (rt_block.h says why).  Read again where it is used - the node after the primary - like words 2 and 3.
template <bool W1>
__device__ __forceinline__ uint32_t rt_entry_second_node(const rt_launch &L) {
  const uint32_t slot = rt_entry_slot<W1>(L);
  return *(const uint32_t __attribute__((address_space(4))) *)((const char __attribute__((address_space(4))) *)L.order + ((size_t)slot << 4) + 4u) >> RT_SN_SHIFT;
}
#endif

// The launch record as the COLD paths read it: straight from the kernarg segment at the point of use (the kernel's only argument lies
// at its start), behind an opaque copy of the pointer, so that a field only the rare paths need is not loaded at kernel entry and
// held in scalar registers across the whole trace (the kernel has none to spare).  (Every kernel of this file that traces - rt_trace,
// rt_retrace - takes the launch record as its only argument.)
__device__ __forceinline__ const rt_launch __attribute__((address_space(4))) *rt_cold_args() {
  const rt_launch __attribute__((address_space(4))) *K = (const rt_launch __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(K));
  return K;
}
// A launch field that the product build reads this way and the strict build from its by-value record (it has registers to spare).
#if RT_STRICT
#define RT_COLD(FIELD) (L.FIELD)
#else
#define RT_COLD(FIELD) (rt_cold_args()->FIELD)
#endif
#if !RT_STRICT
// Append this work-item's sample to the launch's mark list (the cold end of the samplers' boundary test, a handful of samples per frame): entry = sample x |
// sample y << 20 | frame of the batch << 40; the counter of THIS launch is marks[marks_slot] (rt_launch.hip alternates two, so that
// rt_retrace can clear the next launch's while it reads its own); beyond the list's capacity only the count grows and rt_retrace
// traces every sample of the launch.
template <bool SS2>
__device__ __forceinline__ void rt_mark_append(const rt_pixel &P) {
  const rt_launch __attribute__((address_space(4))) *K = rt_cold_args();
  if (!P.valid || (K->mark_flags & RT_MARK_NEVER)) return;
  const uint32_t sx = SS2 ? 2u * P.px + (P.sub & 1u) : P.px, sy = SS2 ? 2u * P.frow + (P.sub >> 1) : P.frow;
  uint32_t *const marks = K->marks;
  const uint32_t i = atomicAdd(marks + K->marks_slot, 1u);
  if (i < K->marks_cap) ((unsigned long long *)(marks + 4))[i] = (unsigned long long)sx | ((unsigned long long)sy << 20) | ((unsigned long long)blockIdx.z << 40);
}
#endif
