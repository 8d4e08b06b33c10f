// rt_rays_order.hip — binning a caller's ray list on the GPU (include/rt_hip.h: rt_scene_order_rays_device).  The ray-list kernels run
// one ray per lane and a wave's 64 rays in lock step, so a list of unrelated rays pays for 64 ray trees per wave.  This unit computes
// a permutation of the list in which 64 consecutive entries are rays that start close to each other and point the same way; the
// ordered trace (rt_kernel.hip: rt_trace_rays with an order, rt_hits.hip: rt_ray_hit_kernel with one) then goes through the list in
// that order and still writes ray i's results at index i, so nothing a caller sees depends on the order but the time.
//
// The key (32 bits, FP32: it decides the order and never a result).  Per ray five coordinates - the origin's x, y, z and the
// direction's place (s, t) on its cube-map face (the two minor components over the major one, each in [-1, 1]; a face is continuous,
// which a frame's primary rays need: they stay on one face up to a field of view of 90 degrees) - plus the face index 0..5.  A first
// pass reduces the list's own bounds of all six (rt_order_bounds); the key pass (rt_order_keys) quantises every coordinate with a
// non-zero extent to 16 bits against them and interleaves the bits of those coordinates alone, most significant first (a Morton
// code), under three face bits when the list uses more than one face.  A list that shares one origin is therefore resolved by
// direction alone, 16 bits per axis, and a list that shares one direction by origin alone.  Rays with a non-finite component get
// the largest key 0xffffffff, finite rays at most 0xfffffffe: the non-finite ones end the order.  The key reads nothing of the scene.
//
// The sort: a least-significant-digit radix sort of (key, index) in four passes of 8 bits, stable, so equal keys keep list order and
// the result is the same on every call.  Per pass three kernels: rt_order_histogram counts each tile's digits in LDS (a tile is
// RT_ORDER_TILE keys, one workgroup) into a digit-major table; rt_order_scan turns each digit's row into exclusive prefixes and leaves
// the digit totals; rt_order_scatter ranks its tile - within a wave by eight ballots per key (the lanes that hold the same digit)
// and mbcnt, no atomics, which keeps it stable -, puts the tile into LDS in digit order and stores it from there, so that a wave's
// stores are runs of consecutive addresses, one run per digit.  Keys and indices are separate arrays: the histogram reads 4 bytes
// per key, the first pass reads no indices (they are 0..n-1) and the last writes no keys.
// Traffic per ray: 48 (bounds) + 48 + 4 (keys) + 4 x 4 (histograms) + 12 + 16 + 16 + 12 (scatters) = 176 bytes.
#include <math.h>

#include "rt_rays_order.h"

namespace {

#include "rt_literal.h"       // the ray record and its finite test, workgroup_exclusive

// word w of the bounds block: min of coordinate w (w < 6), max of coordinate w - 6 (6 <= w < 12), as ordered integers
#define RT_ORDER_COORDS 6u

// float -> an unsigned integer with the same order (and back)
__device__ __forceinline__ uint32_t ordered_of(float f) {
  const uint32_t b = __float_as_uint(f);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t u) { return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xffffffffu)); }

// the six coordinates of ray i, every one a finite float whatever the record holds; false: the ray has a non-finite component
__device__ __forceinline__ bool ray_coords(const double *rays, uint32_t i, float c[RT_ORDER_COORDS]) {
  const lit_ray R = lit_load_ray(rays, i);
  const double big = 3.0e38;                                    // (binary64 origins beyond binary32's range share the outermost cell)
  c[0] = (float)fmin(fmax(R.ox, -big), big);
  c[1] = (float)fmin(fmax(R.oy, -big), big);
  c[2] = (float)fmin(fmax(R.oz, -big), big);
  const double dx = R.rx, dy = R.ry, dz = R.rz;
  const double ax = fabs(dx), ay = fabs(dy), az = fabs(dz);
  // the major axis (the first of equals), then the two others over it
  const int axis = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
  const double major = axis == 0 ? dx : (axis == 1 ? dy : dz), m = fabs(major);
  const double u = axis == 0 ? dy : dx, v = axis == 2 ? dy : dz;
  const double r = __builtin_amdgcn_rcp(m);                     // (approximate: the key decides no result)
  c[3] = fminf(fmaxf((float)(u * r), -1.f), 1.f);               // (a zero direction: 0 x inf = NaN, which fmaxf drops)
  c[4] = fminf(fmaxf((float)(v * r), -1.f), 1.f);
  c[5] = (float)(2 * axis + (major < 0.0 ? 1 : 0));
  return R.finite;
}

// ---- the list's bounds: per coordinate min and max over the finite rays, as ordered integers (atomic min / max: any order of
// arrival gives the same words)
__global__ void __launch_bounds__(RT_ORDER_WG) rt_order_bounds(const double *rays, uint32_t n, uint32_t *bounds) {
  __shared__ uint32_t s_b[2u * RT_ORDER_COORDS];
  if (threadIdx.x < 2u * RT_ORDER_COORDS) s_b[threadIdx.x] = threadIdx.x < RT_ORDER_COORDS ? 0xffffffffu : 0u;
  __syncthreads();
  float lo[RT_ORDER_COORDS], hi[RT_ORDER_COORDS];
  for (uint32_t d = 0; d < RT_ORDER_COORDS; d++) { lo[d] = __builtin_inff(); hi[d] = -__builtin_inff(); }
  for (uint32_t i = blockIdx.x * RT_ORDER_WG + threadIdx.x; i < n; i += gridDim.x * RT_ORDER_WG) {
    float c[RT_ORDER_COORDS];
    if (ray_coords(rays, i, c))
      for (uint32_t d = 0; d < RT_ORDER_COORDS; d++) { lo[d] = fminf(lo[d], c[d]); hi[d] = fmaxf(hi[d], c[d]); }
  }
  for (uint32_t d = 0; d < RT_ORDER_COORDS; d++) {
    atomicMin(&s_b[d], ordered_of(lo[d]));
    atomicMax(&s_b[RT_ORDER_COORDS + d], ordered_of(hi[d]));
  }
  __syncthreads();
  if (threadIdx.x < RT_ORDER_COORDS) atomicMin(&bounds[threadIdx.x], s_b[threadIdx.x]);
  else if (threadIdx.x < 2u * RT_ORDER_COORDS) atomicMax(&bounds[threadIdx.x], s_b[threadIdx.x]);
}

// ---- the keys
__global__ void __launch_bounds__(RT_ORDER_WG) rt_order_keys(const double *rays, uint32_t n, const uint32_t *bounds, uint32_t *keys) {
  // wave-uniform: which coordinates the list resolves at all, and their scales
  float lo[RT_ORDER_COORDS], scale[RT_ORDER_COORDS];
  bool active[RT_ORDER_COORDS];
  for (uint32_t d = 0; d < RT_ORDER_COORDS; d++) {
    lo[d] = float_of(bounds[d]);
    const float ext = float_of(bounds[RT_ORDER_COORDS + d]) - lo[d];          // (no finite ray at all: -inf, nothing is active)
    active[d] = ext > 0.f;
    scale[d] = active[d] ? 65535.f / ext : 0.f;                              // (an extent beyond binary32's range: 0, one cell)
  }
  const uint32_t budget = active[5] ? 29u : 32u;                               // three face bits on top when more than one face is in use
  for (uint32_t i = blockIdx.x * RT_ORDER_WG + threadIdx.x; i < n; i += gridDim.x * RT_ORDER_WG) {
    float c[RT_ORDER_COORDS];
    const bool finite = ray_coords(rays, i, c);
    uint32_t q[5];
    for (uint32_t d = 0; d < 5u; d++) q[d] = (uint32_t)fminf(fmaxf((c[d] - lo[d]) * scale[d], 0.f), 65535.f);   // (fmaxf(NaN, 0) = 0)
    uint32_t key = 0u, left = budget;
    for (int b = 15; b >= 0; b--)
      for (uint32_t d = 0; d < 5u; d++)
        if (active[d] && left) { key = (key << 1) | ((q[d] >> b) & 1u); left--; }
    if (active[5]) key |= (uint32_t)c[5] << 29;
    key = key < 0xfffffffeu ? key : 0xfffffffeu;
    keys[i] = finite ? key : 0xffffffffu;
  }
}

// ---- the radix passes
// tile b's digit counts -> hist[digit * tiles + b]
__global__ void __launch_bounds__(RT_ORDER_WG) rt_order_histogram(const uint32_t *keys, uint32_t n, uint32_t shift, uint32_t tiles, uint32_t *hist) {
  __shared__ uint32_t s_h[RT_ORDER_DIGITS];
  s_h[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t base = blockIdx.x * RT_ORDER_TILE;
  for (uint32_t k = 0; k < RT_ORDER_ITEMS; k++) {
    const uint32_t i = base + k * RT_ORDER_WG + threadIdx.x;
    if (i < n) atomicAdd(&s_h[(keys[i] >> shift) & (RT_ORDER_DIGITS - 1u)], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * tiles + blockIdx.x] = s_h[threadIdx.x];
}

// workgroup d: row d of the table -> exclusive prefixes over the tiles; totals[d] = the digit's count in the list
__global__ void __launch_bounds__(RT_ORDER_WG) rt_order_scan(uint32_t *hist, uint32_t tiles, uint32_t *totals) {
  __shared__ uint32_t s_tmp[RT_ORDER_WG];
  uint32_t *row = hist + (size_t)blockIdx.x * tiles;
  uint32_t carry = 0u;
  for (uint32_t base = 0; base < tiles; base += RT_ORDER_WG) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < tiles ? row[i] : 0u;
    uint32_t total;
    const uint32_t ex = workgroup_exclusive<RT_ORDER_WG>(v, s_tmp, &total);
    if (i < tiles) row[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0u) totals[blockIdx.x] = carry;
}

// One tile of one pass: rank, reorder in LDS, store.  Wave w of the workgroup owns keys [w * 64 * ITEMS, (w + 1) * 64 * ITEMS) of the
// tile and goes through them 64 at a time, so the order inside a tile is (wave, round, lane) = list order.  idx_in NULL: the indices
// are the positions themselves (the first pass); keys_out NULL: the keys are not needed any more (the last).
__global__ void __launch_bounds__(RT_ORDER_WG) rt_order_scatter(const uint32_t *keys_in, const uint32_t *idx_in, uint32_t *keys_out, uint32_t *idx_out,
                                                                uint32_t n, uint32_t shift, uint32_t tiles, const uint32_t *hist, const uint32_t *totals) {
  constexpr uint32_t WAVES = RT_ORDER_WG / 64u;
  __shared__ uint32_t s_wave[WAVES][RT_ORDER_DIGITS];   // per wave: the digit's count so far, then the count in the waves before it
  __shared__ uint32_t s_tile[RT_ORDER_DIGITS];          // where the digit's run starts in the tile
  __shared__ uint32_t s_dest[RT_ORDER_DIGITS];          // where it starts in the output
  __shared__ uint32_t s_tmp[RT_ORDER_WG];
  __shared__ uint32_t s_key[RT_ORDER_TILE], s_idx[RT_ORDER_TILE];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t w = 0; w < WAVES; w++) s_wave[w][tid] = 0u;
  __syncthreads();
  const uint32_t tile_base = blockIdx.x * RT_ORDER_TILE, wave_base = tile_base + wave * (64u * RT_ORDER_ITEMS);
  volatile uint32_t *mine = s_wave[wave];
  uint32_t key[RT_ORDER_ITEMS], at[RT_ORDER_ITEMS];
#pragma unroll
  for (uint32_t k = 0; k < RT_ORDER_ITEMS; k++) {
    const uint32_t i = wave_base + k * 64u + lane;
    const bool valid = i < n;
    key[k] = valid ? keys_in[i] : 0xffffffffu;
    const uint32_t d = (key[k] >> shift) & (RT_ORDER_DIGITS - 1u);
    // the lanes of the wave that hold the same digit
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < 8u; b++) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long set = __ballot(bit);
      peers &= bit ? set : ~set;
    }
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(peers >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)peers, 0u));
    const uint32_t before = mine[d];                            // (every peer reads it before their first lane adds to it)
    at[k] = before + rank;
    if (valid && rank == 0u) mine[d] = before + (uint32_t)__popcll(peers);
  }
  __syncthreads();
  {
    // digit tid: its count per wave -> the waves' exclusive prefixes; the tile's and the list's runs
    uint32_t count = 0u;
    for (uint32_t w = 0; w < WAVES; w++) { const uint32_t c = s_wave[w][tid]; s_wave[w][tid] = count; count += c; }
    uint32_t total;
    s_tile[tid] = workgroup_exclusive<RT_ORDER_WG>(count, s_tmp, &total);
    s_dest[tid] = workgroup_exclusive<RT_ORDER_WG>(totals[tid], s_tmp, &total) + hist[(size_t)tid * tiles + blockIdx.x];
  }
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < RT_ORDER_ITEMS; k++) {
    const uint32_t i = wave_base + k * 64u + lane;
    if (i < n) {
      const uint32_t d = (key[k] >> shift) & (RT_ORDER_DIGITS - 1u);
      const uint32_t p = s_tile[d] + s_wave[wave][d] + at[k];    // (< the tile's valid keys <= RT_ORDER_TILE: the counts are of these keys)
      if (p < RT_ORDER_TILE) { s_key[p] = key[k]; s_idx[p] = idx_in ? idx_in[i] : i; }
    }
  }
  __syncthreads();
  const uint32_t left = n - tile_base, m = left < RT_ORDER_TILE ? left : RT_ORDER_TILE;
  for (uint32_t k = 0; k < RT_ORDER_ITEMS; k++) {
    const uint32_t e = k * RT_ORDER_WG + tid;
    if (e < m) {
      const uint32_t kk = s_key[e], d = (kk >> shift) & (RT_ORDER_DIGITS - 1u);
      const uint32_t g = s_dest[d] + (e - s_tile[d]);
      if (g < n) {                                              // (always: the totals are the counts of these keys)
        if (keys_out) keys_out[g] = kk;
        idx_out[g] = s_idx[e];
      }
    }
  }
}

}  // namespace

extern "C" int rt_launch_order_rays(uint32_t n, const double *d_rays, uint32_t *d_order, void *d_work, hipStream_t stream) {
  const rt_order_layout l = rt_order_layout_of(n);
  uint8_t *w = (uint8_t *)d_work;
  uint32_t *bounds = (uint32_t *)(w + l.bounds), *totals = (uint32_t *)(w + l.totals), *hist = (uint32_t *)(w + l.hist);
  uint32_t *keys_a = (uint32_t *)(w + l.keys_a), *keys_b = (uint32_t *)(w + l.keys_b), *idx = (uint32_t *)(w + l.idx);
  hipError_t e = hipMemsetAsync(bounds, 0xff, RT_ORDER_COORDS * 4u, stream);
  if (e == hipSuccess) e = hipMemsetAsync(bounds + RT_ORDER_COORDS, 0, RT_ORDER_COORDS * 4u, stream);
  if (e != hipSuccess) return (int)e;
  const uint32_t grid = rt_order_grid(n);                                                           // grid-stride beyond
  hipLaunchKernelGGL(rt_order_bounds, dim3(grid), dim3(RT_ORDER_WG), 0, stream, d_rays, n, bounds);
  hipLaunchKernelGGL(rt_order_keys, dim3(grid), dim3(RT_ORDER_WG), 0, stream, d_rays, n, (const uint32_t *)bounds, keys_a);
  const uint32_t *keys_in[4] = {keys_a, keys_b, keys_a, keys_b};
  const uint32_t *idx_in[4] = {nullptr, idx, d_order, idx};
  uint32_t *keys_out[4] = {keys_b, keys_a, keys_b, nullptr};
  uint32_t *idx_out[4] = {idx, d_order, idx, d_order};
  for (uint32_t p = 0; p < 4u; p++) {
    hipLaunchKernelGGL(rt_order_histogram, dim3(l.tiles), dim3(RT_ORDER_WG), 0, stream, keys_in[p], n, 8u * p, l.tiles, hist);
    hipLaunchKernelGGL(rt_order_scan, dim3(RT_ORDER_DIGITS), dim3(RT_ORDER_WG), 0, stream, hist, l.tiles, totals);
    hipLaunchKernelGGL(rt_order_scatter, dim3(l.tiles), dim3(RT_ORDER_WG), 0, stream, keys_in[p], idx_in[p], keys_out[p], idx_out[p], n, 8u * p,
                       l.tiles, (const uint32_t *)hist, (const uint32_t *)totals);
  }
  return (int)hipGetLastError();
}
