// rt_kernel_tables.h - where the kernels' data lies and how it is fetched: the scalar-loaded sphere and bit-set tables, the material
// record and texture descriptor of a hit (per lane, or one for the wave), and the records of the recursion stack.
// A fragment: included once by rt_kernel.hip, inside its anonymous namespace.

// The scene tables walked by the wave-uniform loops live in global memory that nothing writes
// during the launch.  Typing them as CONSTANT address space (4) makes every uniform-index read an
// s_load into SGPRs by construction, whatever else is in the loop.
typedef const rt_geom __attribute__((address_space(4))) *geom_kptr;
typedef const rt_sphere __attribute__((address_space(4))) *sphere_kptr;

// A frame of the explicit recursion stack: everything intersectWorld still needs after its
// recursive calls return (main.js:320-336) — the lighting and sampler terms do not depend on the
// children, so they are evaluated before descending.
template <bool REFRACT> struct frame;
template <> struct frame<false> { double amb[3], ds[3], a3; };
template <> struct frame<true>  { double amb[3], ds[3], a3, a4, h[3], f[3], re[3]; int has_f, phase; };
// A parked two-child node of the product general kernel: its own terms, its refraction ray, and the map F that
// was accumulated above it (S, O, LO, HI), to be restored when its reflection subtree has been evaluated.
struct park { double amb[3], ds[3], a3, a4, h[3], f[3], S, O[3], LO[3], HI[3]; uint32_t path, segs_left; int level, map_valid, hcode; };

// 64-bit table word `i` of a scalar-loaded bit-set table (shadow grids, bounce table: a few MB at most)
__device__ __forceinline__ unsigned long long rt_load_word32(const void *base, uint32_t i) {
  const char __attribute__((address_space(4))) *b = (const char __attribute__((address_space(4))) *)base;
  return *(const unsigned long long __attribute__((address_space(4))) *)(b + (i << 3));
}

// 32-bit byte offset (at most 256 spheres x 32 bytes, times at most 16 lights in the light-anchored table): base +
// zext(offset) lets the scalar load take its offset from an SGPR (s_load_dwordx8 s[..], s[base], s_off) instead of
// a 64-bit address computation per load (+0.8 % on the headline)
__device__ __forceinline__ rt_geom rt_load_geom32(geom_kptr tab, uint32_t i) {
  const rt_geom __attribute__((address_space(4))) *g =
      (const rt_geom __attribute__((address_space(4))) *)((const char __attribute__((address_space(4))) *)tab + (i << 5));
  return rt_geom{g->ox, g->oy, g->oz, g->r2};
}

// two consecutive table records with ONE scalar load (s_load_dwordx16): one memory latency per two sphere tests
struct rt_geom_pair { rt_geom a, b; };
__device__ __forceinline__ rt_geom_pair rt_load_geom_pair32(geom_kptr tab, uint32_t i) {
  typedef double __attribute__((ext_vector_type(8))) d8;
  const d8 v = *(const d8 __attribute__((address_space(4))) *)((const char __attribute__((address_space(4))) *)tab + (i << 5));
  return rt_geom_pair{rt_geom{v[0], v[1], v[2], v[3]}, rt_geom{v[4], v[5], v[6], v[7]}};
}

// Where a node's material record comes from.  In general it is per-lane data: the sphere THAT LANE hit, fetched through a per-lane
// offset (LDS; the many-sphere variants: HBM / L2).  A wave of a block whose launch-table entry names ONE primary candidate has one
// record for all 64 lanes (trace_pixel, UNI): it is read where it lies in HBM through the constant address space, i.e. with scalar
// loads into SGPRs at the point of use, like the geometry tables.  The node's code is the same source for both: it is written
// against rt_mtl_src<UNI>::type and the accessors below.
#define RT_AS4 __attribute__((address_space(4)))
template <bool UNI> struct rt_mtl_src { typedef const rt_mtl type; };
template <> struct rt_mtl_src<true> { typedef const rt_mtl RT_AS4 type; };
template <bool UNI>
__device__ __forceinline__ typename rt_mtl_src<UNI>::type *rt_mtl_at(const rt_mtl *mtl, uint32_t i) {     // a 32-bit byte offset from the table's base
  if constexpr (UNI) return (const rt_mtl RT_AS4 *)((const char RT_AS4 *)(const void *)mtl + i * (uint32_t)sizeof(rt_mtl));
  else return (const rt_mtl *)((const char *)mtl + i * (uint32_t)sizeof(rt_mtl));
}
__device__ __forceinline__ int rt_mtl_kind(const rt_mtl &m) { return m.sampler_kind; }
__device__ __forceinline__ int rt_mtl_texture(const rt_mtl &m) { return m.texture; }
// (uniform: the two 16-bit fields as ONE aligned 32-bit scalar load - gfx950 has no 16-bit scalar load, and a 16-bit field that is
// not 4-byte aligned would come through the vector memory path)
static_assert(offsetof(rt_mtl, sampler_kind) % 4 == 0 && offsetof(rt_mtl, texture) == offsetof(rt_mtl, sampler_kind) + 2, "rt_mtl: sampler_kind | texture share a word");
__device__ __forceinline__ uint32_t rt_mtl_kind_word(const rt_mtl RT_AS4 &m) {
  return *(const uint32_t RT_AS4 *)((const char RT_AS4 *)&m + offsetof(rt_mtl, sampler_kind));
}
__device__ __forceinline__ int rt_mtl_kind(const rt_mtl RT_AS4 &m) { return (int)(int16_t)(rt_mtl_kind_word(m) & 0xffffu); }
__device__ __forceinline__ int rt_mtl_texture(const rt_mtl RT_AS4 &m) { return (int)(int16_t)(rt_mtl_kind_word(m) >> 16); }
template <bool UNI>
__device__ __forceinline__ rt_texture_desc rt_tex_desc(const rt_texture_desc *tex, int i) {
  if constexpr (UNI) { const rt_texture_desc RT_AS4 *t = (const rt_texture_desc RT_AS4 *)(const void *)tex + i; return rt_texture_desc{t->width, t->height, t->texels_offset}; }
  else return tex[i];
}
