// rt_kernel_trace.h - trace_pixel: one intersectWorld call tree for one sample (A2 - A9 of rt_kernel.hip's head comment), and the
// statement macros of its stages, each with the locals of trace_pixel it reads and writes.
// A fragment: included once by rt_kernel.hip, inside its anonymous namespace, after the three other fragments.

#include "rt_uniform_pred.h"     // rt_nonzero_bits: the integer form of `x != 0.0` on a scalar double (RT_OA4_NONZERO)

// ---- closest hit (A2 / A3) -------------------------------------------------------------------------------------------------
// main.js:420-439, as a "candidate root" test.  With thc >= 0 (or NaN) the reference's two-armed
// root selection reduces to: cand = (t0 < eps) ? t1 : t0, and the sphere is hit at cand unless
// cand < eps (both roots behind the epsilon).  NaN fails every comparison, exactly as it loses
// `check.t < hit.t` / `t < light_len` in the reference.  inside = (t0 < eps), which for an
// accepted root equals the reference's (t0 < 0.001) || (t1 < 0.001) (main.js:445).
//
// Two forms of the line-sphere discriminant:
//   generic  (any origin p):     L = o - p, tca = d.L, d2 = L.L - tca^2, miss if d2 > r2   — the reference's own
//   anchored (uniform origin a): the host precomputes La = o - a and Ca = La.La - r2 per sphere; then
//            tca = d.La and r2 - d2 = tca^2 - Ca: 4 operations instead of 10.  Used (product kernel only)
//            for primary rays (a = camera) and for shadow rays walked FROM the light (a = light k), whose
//            line is the same line, so the same discriminant decides hit or miss.
// Both helpers must be called inside `if (hit)`; RT_PIN keeps the bookkeeping in that branch so that a
// wave whose 64 rays all miss pays one s_cbranch_execz and nothing else.
#define RT_PIN() asm volatile("")
// One candidate: the sqrt and the bookkeeping stay inside the hit branch (RT_PIN).
// (the candidate root t_ of a ray that meets the sphere's line - DISC >= 0 -, and whether the ray starts inside: in_)
// RT_ROOT(TCA, DISC): reads eps; declares thc_, t0_, t1_, in_ and t_ in the scope it stands in.
#define RT_ROOT(TCA, DISC)                                                                    \
        const double thc_ = rt_sqrt_nn<REFRACT>(DISC);                                                 \
        const double t0_ = (TCA) - thc_, t1_ = (TCA) + thc_;                                  \
        const bool in_ = (t0_ < eps);                                                         \
        const double t_ = in_ ? t1_ : t0_;
// RT_CAND(IDX, TCA, DISC): reads eps; reads and writes ht, hcode (the closest hit so far).
#define RT_CAND(IDX, TCA, DISC)                                                               \
      if (!((DISC) < 0.0)) {                                                                  \
        RT_PIN();                                                                             \
        RT_ROOT(TCA, DISC)                                                                    \
        const bool closer_ = (t_ < ht) && !(t_ < eps);   /* strict <: first wins */           \
        ht = closer_ ? t_ : ht;                                                               \
        hcode = closer_ ? ((int)(2u * (IDX)) + (in_ ? 1 : 0)) : hcode;                        \
      }
// generic form, the reference's own (main.js:422-425): disc = r2 - d2
// RT_GENERIC(IDX, G): reads p, d, eps; reads and writes ht, hcode.
#define RT_GENERIC(IDX, G)                                                                    \
      {                                                                                       \
        const v3 Lv_ = mk((G).ox - p.x, (G).oy - p.y, (G).oz - p.z);                          \
        const double tca_ = dot(d, Lv_);                                                      \
        const double disc_ = (G).r2 - (dot(Lv_, Lv_) - tca_ * tca_);                          \
        RT_CAND(IDX, tca_, disc_)                                                             \
      }
// anchored form (origin = camera): disc = tca^2 - Ca
// RT_ANCHORED_DISC(G): reads d; declares tca_, disc_.  RT_ANCHORED(IDX, G): reads d, eps; reads and writes ht, hcode.
#define RT_ANCHORED_DISC(G)                                                                   \
        const double tca_ = d.x * (G).ox + d.y * (G).oy + d.z * (G).oz;                       \
        const double disc_ = __builtin_fma(tca_, tca_, -(G).r2);
#define RT_ANCHORED(IDX, G)                                                                   \
      {                                                                                       \
        RT_ANCHORED_DISC(G)                                                                   \
        RT_CAND(IDX, tca_, disc_)                                                             \
      }

// ---- error magnification Q ------------------------------------------------------------------------------------------------
#if !RT_STRICT
// How far this kernel's own rounding has been MAGNIFIED on the way to the current hit: Q bounds the error of the hit's NORMAL in units
// of 1.1e-16 (a float, rounded up: an estimate that only widens a tolerance).  A ray with origin error P and direction error D meets
// a sphere of radius r after t at incidence cosine c (sine s): a sideways shift of the ray moves the hit along the surface by 1/c of
// it, so the normal inherits (P + t D) / (r c); the distance itself, t = tca - thc, is rounded to ~eps t (1 + t / (2 r c)) - the
// near root cancels when the ray grazes - and moves the hit along the ray, the normal by s / r of it; the mirrored (or refracted)
// ray leaves with D' <= 3 D + 4 Q and P' = r Q.  With D dominated by the previous normal's error:
//     Q_hit = Q_parent (6 t + r_parent) / (r c)  +  (t / r) (1 / c + s (1 + t / (2 r c))),        Q = 0 at the camera
// (r_parent Q_parent is the origin's position error: from a small sphere onto a large one it all but vanishes; the parent's radius
// rides along as one exponent byte, rounded up).
// A primary hit on the floor has Q ~ 1e-2, on the reference's small spheres 1e1 - 1e3; every bounce off a sphere of radius r at
// distance t multiplies it by ~6 t / (r c), a grazing one by far more (profiles/r04_ab_log.md section 4: the adversarial soak's
// flipped pixel had ONE bounce).  The samplers' boundary test scales its tolerance by max(1, Q / RT_Q_FLAT): RT_XY_INDEX below;
// RT_Q_FLAT is a third of the Q at which the flat tolerance (2e-13 in u, v = Q 1.1e-16 / 2 pi) is exactly the bound.  The scaled tolerance is honoured
// up to the hot path's prefilter band (a fraction within 2^-20 of an integer): 36 x the flat tolerance at the largest admitted frequency
// (2^17 per unit; beyond, the scene is a strict scene), 950 x at the reference's 5000 - a bound that routes every high-Q sample to the
// cold block marks the reference's own scene's deep internal reflections by the dozen per frame (the recurrence is a worst case: inside a
// sphere errors do not compound the way it assumes), profiles/r04_ab_log.md section 4.  Updated per
// BOUNCE, not per node: it is the Q of the current hit at every node below the primary, and is filled in for the primary when it
// spawns a ray (at the node's top, where the hit's distance is at hand).
// (it lives in the upper half of `level` as a bfloat16, rounded up: a 97th vector register would cost the kernel a wave per SIMD)
// Q of a hit from its parent's (see trace_pixel: "How far this kernel's own rounding has been magnified"): x = t / r, c = |d.n|
__device__ __forceinline__ float rt_q_of(float qp, float x, float c, float rp_over_r) {
  const float ic = __builtin_amdgcn_rcpf(fmaxf(c, 1e-30f));                    // (s taken as 1: no square root on the way)
  return fminf(ic * (qp * (6.f * x + rp_over_r) + x + 0.5f * x * x) + x, 1e30f);
}
// (rt_lvl, RT_Q_GET, rt_r_get read `level`; level = rt_q_put(level, q) / rt_r_put(level, r) write Q and the radius byte into it)
__device__ __forceinline__ int rt_lvl(int lv) { return lv & 255; }
#define RT_Q_GET(L_) __builtin_bit_cast(float, (uint32_t)(L_) & 0xffff0000u)
__device__ __forceinline__ int rt_q_put(int lv, float q) { return (int)(((uint32_t)lv & 0xffffu) | ((__builtin_bit_cast(uint32_t, q) + 0xffffu) & 0xffff0000u)); }
// bits 8..15: the exponent byte of a power of two >= the radius of the sphere this hit lies on (the next hit's r_parent)
__device__ __forceinline__ float rt_r_get(int lv) { return __builtin_bit_cast(float, ((uint32_t)lv & 0xff00u) << 15); }
__device__ __forceinline__ int rt_r_put(int lv, float r) { return (int)(((uint32_t)lv & 0xffff00ffu) | ((((__builtin_bit_cast(uint32_t, r) >> 23) + 1u) & 255u) << 8)); }
constexpr float RT_Q_FLAT = 4096.f;
#define RT_Q_OF(QP, T, INVR, C, RP) rt_q_of((QP), (T) * (INVR), (C), (RP) * (INVR))
#else
__device__ __forceinline__ int rt_lvl(int lv) { return lv; }
#endif

// ---- sampler index and boundary mark (A8, product build) ------------------------------------------------------------------------
#if !RT_STRICT
// A sampler coordinate x = u * frequency decides a texel (main.js:344-347) or a checker parity (main.js:129-130) by its integer
// part, and this kernel's u, v differ from the reference's in their last bits (its hit point and normal do).  A sample with a
// coordinate within L.flag_tol (RT_FLAG_T1 x the scene's largest sampler frequency: 1e-9 for the reference's checker) of an
// integer is decided in the reference by the last bits of ITS arithmetic: it is appended to the launch's mark list and
// traced again, operation for operation, by the strict build's rt_retrace (rt_launch.hip).  The test on the hot path is integer work on the bits of x + 1.5 * 2^32, a sum whose ulp
// is 2^-20: its mantissa holds floor(x) (from bit 20 up) - the texel index, the checker parity - and 20 fraction bits;
// "fraction within 2^-20 of 0 or 1" (6e-6 of the hits) sends the sample to the precise test, which also takes floor(x)
// again (the sum rounds a fraction above 1 - 2^-21 up).  (Checker frequencies outside [0, 2^31), where the sum does not hold
// ToInt32's parity, make the scene a strict-kernel scene: rt_scene.hip.)
// RT_XY_INDEX: iu, iv = floor(xu), floor(xv) and the boundary mark
// RT_XY_INDEX(XU, XV, FU, FV): declares su, sv, iu, iv, near_; reads L, h, d, n, m, level, map_valid, acc, sp, parked; UNI: may `return false`
// from trace_pixel; otherwise may append the sample to the mark list (rt_mark_append).
#define RT_XY_INDEX(XU, XV, FU, FV)                                                                                \
          const unsigned long long su = __builtin_bit_cast(unsigned long long, (XU) + 6442450944.0), sv = __builtin_bit_cast(unsigned long long, (XV) + 6442450944.0);   \
          uint32_t iu = __builtin_amdgcn_alignbit((uint32_t)(su >> 32), (uint32_t)su, 20u) ^ 0x80000000u;       /* floor(x) for x in [0, 2^31) ... */ \
          uint32_t iv = __builtin_amdgcn_alignbit((uint32_t)(sv >> 32), (uint32_t)sv, 20u) ^ 0x80000000u;       \
          /* ... unless the fraction is within 2^-20 of an integer <=> the 20 fraction bits are 0xfffff, 0 or 1 (NaN, infinity: 0) */ \
          const bool near_ = (min(((uint32_t)su + 1u) & 0xfffffu, ((uint32_t)sv + 1u) & 0xfffffu) <= 2u);           \
          /* (UNI: a wave with such a sample - ~4e-4 of them by the band's width, not measured - has stored and marked nothing yet: it goes back to the general path, which decides below) */ \
          if constexpr (UNI) { if (__ballot(near_) != 0ull) return false; }                                    \
          if (!UNI && near_) {                                                                                  \
            RT_PIN();                                                                                             \
            iu = (uint32_t)(XU); iv = (uint32_t)(XV);                  /* truncation = floor (x >= 0); NaN -> 0 */  \
            const rt_launch __attribute__((address_space(4))) *K = rt_cold_args();                                \
            /* the tolerance grows with what this hit's normal error has been magnified by (qamp; a primary hit's Q from the camera) */ \
            float q_here = RT_Q_GET(level);                                                                        \
            if (rt_lvl(level) == 0 && q_here == 0.f) {                  /* (a primary hit that spawns nothing: not filled in above) */ \
              const float ex = (float)(h.x - K->cam_origin[0]), ey = (float)(h.y - K->cam_origin[1]), ez = (float)(h.z - K->cam_origin[2]);   \
              q_here = RT_Q_OF(0.f, __builtin_sqrtf(ex * ex + ey * ey + ez * ez), (float)m.inv_r, __builtin_fabsf((float)dot(d, n)), 0.f);       \
            }                                                                                                     \
            double tol = (K->mark_flags & RT_MARK_ALL) ? 2.0 : K->flag_tol * (double)fmaxf(1.f, q_here * (1.f / RT_Q_FLAT));   \
            /* ... and a sample whose colour cannot move the pixel by a byte is left alone: the pixel is F(x) = max(LO, min(HI, O + S x)) \
               of this node's colour x (and of the parked nodes' maps above it), |dF| <= S |dx|, and a flipped texel / parity moves x by \
               at most 2 when every albedo and colour of the scene lies in [0, 1] (RT_MARK_WEIGHT: the host's check) */              \
            if ((K->mark_flags & (RT_MARK_WEIGHT | RT_MARK_ALL)) == RT_MARK_WEIGHT) {                              \
              double S_ = map_valid ? acc[0] : 1.0;                                                               \
              if constexpr (FOLD_FORWARD && REFRACT) for (int i_ = 0; i_ < sp; i_++) S_ *= (parked[i_].map_valid ? parked[i_].S : 1.0) * parked[i_].a3;   \
              if (__builtin_fabs(S_) * 510.0 < 0.9) tol = -1.0;                                                    \
            }                                                                                                     \
            /* (a frequency of exactly 0 - stripes - makes the coordinate exactly 0 on every hit: it carries no error and decides nothing) */ \
            const bool zf = !(K->mark_flags & RT_MARK_ZERO);                                                       \
            const bool bu = (zf && (FU) == 0.0 && (XU) == 0.0) || (__builtin_fabs((XU) - __builtin_rint(XU)) >= tol);    \
            const bool bv = (zf && (FV) == 0.0 && (XV) == 0.0) || (__builtin_fabs((XV) - __builtin_rint(XV)) >= tol);    \
            if (!(bu & bv)) {                                                                                     /* NaN: marked */ \
              uint32_t t3 = threadIdx.x;                                                                          \
              if constexpr (W1 && !GRID) t3 = rt_lane_again(); else                                               \
              asm volatile("" : "+v"(t3));                                                                        \
              rt_mark_append<SS2>(rt_pixel_of<SS2, W1>(L, t3));                                                        \
            }                                                                                                     \
          }
#endif

// ---- shadow scan (A7) -----------------------------------------------------------------------------------------------------------
// RT_SDISC(G, TC, DISC): declares TC, DISC (strict build: and Lv_); reads sv (strict build: and h).
// RT_SROOTS(TC, THC, T0, T1): declares T0, T1; product build: reads llen (the scan walks from the light).
#if !RT_STRICT
#define RT_SDISC(G, TC, DISC)                                                                 \
            const double TC = -(sv.x * (G).ox + sv.y * (G).oy + sv.z * (G).oz);               \
            const double DISC = __builtin_fma(TC, TC, -(G).r2);
#define RT_SROOTS(TC, THC, T0, T1) const double T0 = llen - (TC + THC), T1 = llen - (TC - THC);
#else
#define RT_SDISC(G, TC, DISC)                                                                 \
            const v3 Lv_ = mk((G).ox - h.x, (G).oy - h.y, (G).oz - h.z);                      \
            const double TC = dot(sv, Lv_);                                                   \
            const double DISC = (G).r2 - (dot(Lv_, Lv_) - TC * TC);
#define RT_SROOTS(TC, THC, T0, T1) const double T0 = TC - THC, T1 = TC + THC;
#endif
// RT_SHADOW(J, G) - the counting variant's: reads hi, eps, llen, objs, sv (strict build: and h); reads and writes li, blocked, tests.
#define RT_SHADOW(J, G)                                                                       \
            {                                                                                 \
              const bool other_ = ((int)(J) != hi);                                           \
              if (COUNT && other_ && !blocked) tests++;                                       \
              RT_SDISC(G, tc_, disc_)                                                         \
              if (other_ && !(disc_ < 0.0) && !blocked) {                                     \
                RT_PIN();                                                                     \
                const double thc_ = rt_sqrt_nn<REFRACT>(disc_);                                        \
                RT_SROOTS(tc_, thc_, t0_, t1_)                                                \
                const double t_ = (t0_ < eps) ? t1_ : t0_;                                    \
                if ((t_ < llen) && !(t_ < eps)) {                                             \
                  RT_PIN();                                                                   \
                  const double oa4_ = objs[J].albedo[4];                                      \
                  if (oa4_ != 0.0) li = rt_div(li, oa4_);   /* transparent occluder brightens (q2) */ \
                  else { li = 0.0; blocked = true; }                                          \
                }                                                                             \
              }                                                                               \
            }
// The scans the product and strict kernels run (everything but the counting variant): no per-lane `break`.  A lane that
// is already blocked (li == 0) keeps testing, and whatever it hits leaves li at 0 (0 / albedo, or 0), exactly where the
// reference's `break` (main.js:301) left it.  The loop is then wave-uniform: the exec-mask bookkeeping of a divergent loop
// exit - about 10 scalar instructions per iteration, for every wave - is gone (measured: +4.6 % on the headline).
// RT_SHADOW_U(J, G): reads hi, eps, llen, objs, sv (strict build: and h), SIX_FORMS; reads and writes li.
// (RT_OA4_NONZERO: the occluder's transparency is a scalar load - `x != 0.0` of a scalar is a vector compare into a lane mask and a branch through vcc; the
// few-sphere one-wave kernels test the pattern instead, on the condition code: rt_uniform_pred.h, with the argument that it is the same for every pattern)
// (the pattern passes through an opaque scalar copy: the compiler otherwise recognises the shift-and-test as `x != 0.0` and writes the vector compare again)
__device__ __forceinline__ bool rt_nonzero_scalar(double x) {
  unsigned long long b_ = __builtin_bit_cast(unsigned long long, x);
  asm volatile("" : "+s"(b_));
  return rt_nonzero_bits(b_);
}
#define RT_OA4_NONZERO(X) (SIX_FORMS ? rt_nonzero_scalar(X) : ((X) != 0.0))
#define RT_SHADOW_U(J, G)                                                                     \
            {                                                                               \
              RT_SDISC(G, tc_, disc_)                                                       \
              if (((int)(J) != hi) && !(disc_ < 0.0)) {                                     \
                RT_PIN();                                                                   \
                const double thc_ = rt_sqrt_nn<REFRACT>(disc_);                                      \
                RT_SROOTS(tc_, thc_, t0_, t1_)                                              \
                const double t_ = (t0_ < eps) ? t1_ : t0_;                                  \
                if ((t_ < llen) && !(t_ < eps) && li != 0.0) {                              \
                  RT_PIN();                                                                 \
                  const double oa4_ = objs[J].albedo[4];                                    \
                  li = RT_OA4_NONZERO(oa4_) ? rt_div(li, oa4_) : 0.0;                       \
                }                                                                           \
              }                                                                             \
            }

// ---- the end of a lane's chain (the six-wave kernels) -------------------------------------------------------------------------------
// RT_CHAIN_END(): reads and writes ret; reads SIX_WAVES, map_valid, acc.  The chain of one-child nodes ends at this node with colour `ret`:
// the accumulated map is applied HERE, in the branch that made the colour (the other kernels apply it behind the node's body, where the
// ending and the descending lanes' paths have met), and the lane leaves the loop by a plain `break`.  `ret` is then a value of that branch
// alone: it meets no other path, nothing of it is zeroed per turn, and no test of an opaque constant stands at the exit.  A block that
// always leaves is no part of the loop: in the code object the whole chain end - the leaf's three channel sums, the application - stands
// BEHIND the node loop and runs once per wave, for all its lanes together, on what each lane held when it left.
#define RT_CHAIN_END()                                                                                                          \
        if constexpr (SIX_WAVES) {                                                                                              \
          if (map_valid) {                                                                                                      \
            const double S_ = acc[0];                                                                                           \
            _Pragma("unroll")                                                                                                   \
            for (int c = 0; c < 3; c++) ret[c] = rt_max_nn(acc[(4 + c) * 64u], rt_min_nn(acc[(7 + c) * 64u], __builtin_fma(S_, ret[c], acc[(1 + c) * 64u])));   \
          }                                                                                                                     \
        }

// One intersectWorld call tree for one sample.  UNI (product reflection-only one-wave-workgroup kernels only): the caller has found the
// wave's launch-table entry to name exactly ONE primary candidate, cand_host & 255, and hands over `mtl` / `tex` as the image in HBM.
// The call then shades the wave on the uniform-material path - the one anchored test without closest-hit selects, the candidate's
// record in scalar registers, the sampler, the light loop's material tests and the specular exponent decided on the scalar unit, no
// LDS access, no fold state, no node loop - if, wave-uniformly, the material spawns no ray at this depth, its sampler is colour,
// checker or texture, EVERY lane's primary ray meets the candidate from outside it, and no lane's sampler coordinate lies in the boundary test's
// prefilter band (derived, not measured: ~6 x 2^-20 per sample x 64 samples = ~4e-4 of the waves; the general path marks such samples); otherwise it returns false before it has stored or marked
// anything and the caller runs the general path (UNI = false), unchanged.  The per-lane arithmetic is this function's own: the same
// statements in the same order, with the general path's bookkeeping compiled out (if constexpr).  Returns true when rgb is set.
template <bool REFRACT, bool COUNT, bool GRID, bool SS2, bool ITEM = false, bool W1 = false, bool UNI = false>
__device__ __forceinline__ bool trace_pixel(const rt_launch &L, const rt_mtl *mtl, const rt_texture_desc *tex,
                                            [[maybe_unused]] double *acc, [[maybe_unused]] const rt_geom *cull_lds, [[maybe_unused]] const rt_geom cull0, [[maybe_unused]] uint32_t lane,
                                            [[maybe_unused]] double blk_x0, [[maybe_unused]] double blk_x1, [[maybe_unused]] double blk_y0,
                                            [[maybe_unused]] double blk_y1, v3 p, v3 d, double rgb[3], uint32_t cnt[3],
                                            [[maybe_unused]] bool is_probe, [[maybe_unused]] uint32_t cand_host,
                                            [[maybe_unused]] uint32_t own_sx = 0u, [[maybe_unused]] uint32_t own_sy = 0u, [[maybe_unused]] uint32_t own_f = 0u) {
  static_assert(!UNI || (W1 && !REFRACT && !COUNT && !ITEM && !RT_STRICT), "uniform-material path: the one-wave-workgroup product kernels");
#ifdef RT_TESTING
  uint32_t probe_n = 0;                                  // test build: nodes of this sample's ray tree recorded so far
  double probe_li = 0.0;
#endif
  const sphere_kptr objs = (sphere_kptr)L.objects;
  const geom_kptr geom = (geom_kptr)L.geom;
  const uint32_t N = L.n_objects, NL = L.n_lights;
  const double eps = L.epsilon;
  const uint32_t NLOOP = L.n_loop;                      // spheres the per-ray loops walk: N, or N-1 with an enclosing sphere
  const uint32_t enc = L.enclosing;                      // device index of the enclosing sphere (== NLOOP), or ~0u
  // where the primary-ray cull's rectangles are: the product kernels know at compile time (the host launches the many-sphere
  // variant exactly for the scenes whose LDS image leaves them out), the strict and counting kernels ask the launch record
  // (the few-sphere one-wave kernels stage their materials alone - rt_kernel.hip, MTL_ONLY - and read the rectangles from L.cull here)
  const bool cull_lds_on = (!RT_STRICT && !COUNT) ? (!GRID && !W1) : (L.cull_in_lds != 0u);
#if RT_STRICT
  constexpr bool FOLD_FORWARD = false;
#else
  constexpr bool FOLD_FORWARD = true;       // the recursion is folded on the way down (see the descend step)
#endif
  // The reflection-only product frame kernels issue their clamps as one instruction each, restore no sign on the reflection's normal and select
  // nothing in its normalisation (rt_kernel_math.h: rt_min_nn ..., unit_go, with the argument for equal bytes; docs/EVIDENCE.md, "Vector diet").
  // Not the REFRACT kernels (bound by their parked stack, not examined), nor ITEM / COUNT / the strict build (rt_kernel_math.h says why).
  constexpr bool LEAN = !RT_STRICT && !REFRACT && !COUNT && !ITEM;
  // The six-wave kernels, both paths (UNI and the general path's WAVE_NODE form): the scalar forms that are theirs alone - the specular walk's
  // ladder (rt_pow_spec), a light's occluder set by one 64-bit shift (occ, below), the pair test on the scalar mk in the uniform path's scan too,
  // and RT_OA4_NONZERO (above).  The four-wave forms and every other kernel keep the parent's code (docs/EVIDENCE.md, "Scalar forms").
  [[maybe_unused]] constexpr bool SIX_FORMS = LEAN && W1 && !GRID;
  [[maybe_unused]] frame<REFRACT> stack[FOLD_FORWARD ? 1 : RT_MAX_SEGS];
  // product general kernel: nodes with BOTH a reflection and a refraction child are parked here while their
  // reflection subtree is traced (everything else needs no stack)
  [[maybe_unused]] park parked[(FOLD_FORWARD && REFRACT) ? RT_MAX_SEGS : 1];
  [[maybe_unused]] int sp = 0;
  [[maybe_unused]] bool map_valid = false;             // false: the accumulated map F is the identity
  int level = 0;
  [[maybe_unused]] uint32_t tree_path = 1u;            // general kernel: position in the ray tree (root 1, reflect 2p, refract 2p+1)
#if defined(RT_TESTING) && defined(RT_ABLATE_BOUNCE)
  uint32_t segs_left = L.segs ? 1 : 0;
#else
  uint32_t segs_left = L.segs;
#endif
  double ret[3] = {0.0, 0.0, 0.0};
  // The few-sphere one-wave kernels (80 VGPRs, six waves per SIMD), general path: a lane's chain ends in the branch that made its colour
  // (RT_CHAIN_END), and the ambient and reflection coefficients are read a second time behind the lighting (below).  (The colour used to be
  // parked in the lane's fold-state slots O[0..2] and read back behind the loop, with `ret` zeroed at every turn's top and an exit through
  // an opaque test that kept the stores inside the loop; with the chain end in its branch the registers fit without: docs/EVIDENCE.md.)
  constexpr bool SIX_WAVES = FOLD_FORWARD && W1 && !GRID && !REFRACT && !COUNT && !ITEM && !UNI;
  // The few-sphere reflection-only product kernels: every node has at most one child, so every lane still in the node loop is at the same node
  // in every turn of it, and which node that is - the primary ray's, the first bounce's, a later one - is a COUNT of the loop's turns in a
  // scalar register.  (As booleans carried from turn to turn the same facts were lane masks: an exec-mask save, test and restore at every
  // use, and every value derived from them - the shadow scan's pair mask - a vector register tested per lane.)  In these kernels the
  // count is rt_lvl(level), and `map_valid` is "not the primary node".
  constexpr bool WAVE_NODE = LEAN && !GRID && !UNI;
  [[maybe_unused]] uint32_t turn = 0u;

  // ---- A2 / A3 candidates: the primary ray's here, a bounced ray's at the top of its node ----
  // A3: closest hit.  The winner is kept as (ht, hcode) with hcode = 2*index + inside, so a candidate costs one
  // 64-bit and one 32-bit select.
  double ht = RT_INF; int hcode = -1;
  // (a bounced ray's full scan and the shadow scan:) Both loops are unrolled by two by hand (the pinned branches make them convergent,
  // which rules out the compiler's runtime unrolling); a pair's two records come with ONE s_load_dwordx16 (rt_load_geom_pair32).
  if constexpr (UNI) { if (segs_left == 0) return false; }
  if (segs_left != 0) {
        // Primary rays.  First a wave-wide cull: lane j compares sphere j's conservative screen rectangle
        // (host, resolution-independent: bounds of X/D and Y/D over the pixels whose LINE meets the sphere)
        // with the rectangle of this wave's 8x8 pixel block; __ballot turns the 64 verdicts into one scalar
        // mask and only the surviving spheres are tested, in index order (the tie-break is preserved).
        // A wave of sky pixels tests nothing; a wave of floor pixels tests the floor.  The cull only prunes, so the strict
        // kernel uses it too (with the reference's own discriminant for the survivors) and stays bit-identical.
        [[maybe_unused]] const geom_kptr ga = (geom_kptr)L.geom_cam;
#if !RT_STRICT
        // A block for which the table names at most two spheres its primary rays can meet at all (word 3 of its entry;
        // a floor block names the floor) tests those and skips the cull.
        if constexpr (UNI) {
          // ONE candidate (the caller's test of the entry).  Its material decides first, on the scalar unit; then the one anchored test,
          // whose root is every lane's closest hit if every lane has one: no (ht, hcode) selects.  A lane that misses - the horizon -
          // sends the wave back to the general path.
          const uint32_t i = cand_host & 255u;
          const rt_geom g0 = rt_load_geom32(ga, i);
          typename rt_mtl_src<true>::type &mu = *rt_mtl_at<true>(mtl, i);
          if ((mu.albedo[3] > 0.0 && segs_left > 1) || rt_mtl_kind(mu) == RT_SAMPLER_STARS) return false;
          RT_ANCHORED_DISC(g0)
          const double t0_ = tca_ - rt_sqrt_nn<REFRACT>(disc_);          // (RT_ROOT's near root)
          // ... and so does a lane that starts INSIDE the candidate (RT_ROOT's in_ = t0_ < eps, whose root would be the far one): the test is
          // on the near root alone - no far root, no select - and the path takes l = n below, with nothing per lane.  (Today the launch
          // table names no sphere the camera is inside of - rt_block.h, rt_ball.everywhere - so no wave leaves for this reason; the path's
          // correctness does not rest on that property of the table.)
          const bool met_ = !(disc_ < 0.0) && (t0_ < ht) && !(t0_ < eps);
          if (__ballot(!met_) != 0ull) return false;
#if defined(RT_TESTING) && defined(RT_ABLATE_UNIFORM)   /* counting experiment only (profiles/ab_build.sh): what the launch issues WITHOUT the shading of these waves */
          rgb[0] = rgb[1] = rgb[2] = 0.0;
          return true;
#endif
          ht = t0_; hcode = (int)(2u * i);
        } else
        if (cand_host != 0u) {                        // count << 16 | second << 8 | first (loop indices, ascending)
          { const uint32_t i = cand_host & 255u; const rt_geom g0 = rt_load_geom32(ga, i); RT_ANCHORED(i, g0) }
          if (cand_host >= (2u << 16)) { const uint32_t i = (cand_host >> 8) & 255u; const rt_geom g0 = rt_load_geom32(ga, i); RT_ANCHORED(i, g0) }
        } else
#endif
        for (uint32_t base = 0; base < NLOOP; base += 64u) {
          const uint32_t j = base + lane;
          // {x_lo, x_hi, y_lo, y_hi} in units of 1/D.  Few spheres: from the LDS image.  Many: one record per lane from HBM (L2) -
          // the first 64 were fetched before the ray was generated (cull0), scenes of more spheres fetch the rest here
          const uint32_t jj = j < NLOOP ? j : 0u;
          double c0 = cull0.ox, c1 = cull0.oy, c2 = cull0.oz, c3 = cull0.r2;
          // (explicit address spaces: the compiler otherwise selects the POINTER and issues one flat load for both cases)
          if constexpr (ITEM) {
          } else if (cull_lds_on) {
            const rt_geom __attribute__((address_space(3))) *g = (const rt_geom __attribute__((address_space(3))) *)cull_lds + jj;
            c0 = g->ox; c1 = g->oy; c2 = g->oz; c3 = g->r2;
          } else if (base != 0u || (W1 && !GRID)) {
            const rt_geom __attribute__((address_space(1))) *g = (const rt_geom __attribute__((address_space(1))) *)L.cull + jj;
            c0 = g->ox; c1 = g->oy; c2 = g->oz; c3 = g->r2;
          }
          const rt_geom cr = rt_geom{c0, c1, c2, c3};
          // five compares, their 64-bit masks combined on the scalar unit (as one boolean expression the compiler may build
          // the conjunction in vector registers instead: ~15 more vector instructions per wave in the many-sphere variant)
          unsigned long long m = __ballot(j < NLOOP) & __ballot(cr.ox * L.proj_d <= blk_x1) & __ballot(cr.oy * L.proj_d >= blk_x0) &
                                 __ballot(cr.oz * L.proj_d <= blk_y1) & __ballot(cr.r2 * L.proj_d >= blk_y0);
          // (rt_retrace: a wave's lanes hold unrelated samples and only some of them run - no wave-wide cull, every sphere in scene order)
          if constexpr (ITEM) m = (NLOOP - base >= 64u) ? ~0ull : ((1ull << (NLOOP - base)) - 1ull);
          while (m) {
            const uint32_t i = base + (uint32_t)__builtin_ctzll(m);
            m &= m - 1ull;
#if RT_STRICT
            const rt_geom g0 = rt_load_geom32(geom, i);
            RT_GENERIC(i, g0)
#else
            const rt_geom g0 = rt_load_geom32(ga, i);
            RT_ANCHORED(i, g0)
#endif
          }
        }
  }
  bool searched = true;                // the primary ray's candidates were found above (culled; camera-anchored in the product kernel)
  // (few-sphere reflection-only product kernels) wave-uniform like `searched`: the node being evaluated is the one AFTER the primary - in these kernels
  // every node has at most one child, so every lane still in the loop is at the same level in every turn of it
  // (WAVE_NODE: both, and map_valid, are set from the turn's number at the loop's head; carried from turn to turn they are lane masks)
  [[maybe_unused]] bool first_bounce = false;
#if !RT_STRICT
  // A wave none of whose primary rays met a sphere of the loops, in a scene whose enclosing sphere is flat AND constant in colour
  // (the reference's skybox with a plain colour): every pixel of the wave is that sphere's ambient term, max(color*albedo[0],
  // min(1, color*0 + color*0)) (main.js:326-336 with no light and no child), which the host evaluated once.  Nothing else runs.
  if (!UNI && L.sky_fast && segs_left != 0 && __ballot(hcode >= 0) == 0ull) {
    if (COUNT) { cnt[0]++; cnt[2] += N; }
    rgb[0] = L.sky_rgb[0]; rgb[1] = L.sky_rgb[1]; rgb[2] = L.sky_rgb[2];
    return true;
  }
#endif

  if (segs_left != 0) {
    for (;;) {
      // (WAVE_NODE) which node this turn evaluates: 0 the primary ray's, 1 the first bounce's, ...; counted at the turn's top, where every
      // lane in the loop passes, so that it stays a scalar
      [[maybe_unused]] const uint32_t node_no = turn;
      if constexpr (WAVE_NODE) {
        turn++;
        searched = (node_no == 0u); first_bounce = (node_no == 1u); map_valid = (node_no != 0u);
      }
      // ---------------- evaluate one intersectWorld node (segs_left > 0 here) ----------------
      if (COUNT) cnt[0]++;
      if (!UNI && !searched) {                           // reflection / refraction rays: any origin, generic form
        bool scanned = false;
#if !RT_STRICT
        if constexpr (GRID) {
          if (rt_cold_args()->bounce_table != nullptr) {
            // Many spheres: a bounced ray starts ON the sphere it just hit (`hcode` still names it) and its direction
            // falls in one cell of a cube map.  The host stored, per (sphere, cell), the bit set of the spheres that
            // ANY ray leaving that sphere's ball in ANY direction of that cell can meet (conservative: angle between
            // the cell and the line of centres against asin((r_i + r_j) / distance), rt_tables.cpp build_bounce_table).
            // The wave tests the UNION over its active lanes, walked like the shadow grid's cells (readlane + ballot,
            // correct under divergence), in index order, so the strict-< tie-break of the full scan is kept.
            const uint32_t from = (uint32_t)(hcode >> 1);
            const double ax = __builtin_fabs(d.x), ay = __builtin_fabs(d.y), az = __builtin_fabs(d.z);
            const bool bx = (ax >= ay) && (ax >= az), by = !bx && (ay >= az);
            const double dm = bx ? d.x : (by ? d.y : d.z);
            const double du = bx ? d.y : d.x, dv = (bx || by) ? d.z : d.y;
            const double sc = (0.5 * RT_BGRID) * __builtin_amdgcn_rcp(__builtin_fabs(dm));   // 2^-24 is plenty: the host's cells overlap by 1e-6
            const double fu = __builtin_fmin(__builtin_fmax(__builtin_fma(du, sc, 0.5 * RT_BGRID), 0.0), (double)(RT_BGRID - 1u));
            const double fv = __builtin_fmin(__builtin_fmax(__builtin_fma(dv, sc, 0.5 * RT_BGRID), 0.0), (double)(RT_BGRID - 1u));
            const uint32_t face = (bx ? 0u : (by ? 2u : 4u)) + ((dm < 0.0) ? 1u : 0u);
            const uint32_t key = from * RT_BCELLS + face * (RT_BGRID * RT_BGRID) + (uint32_t)fv * RT_BGRID + (uint32_t)fu;
            const uint32_t words = (NLOOP + 63u) >> 6;
            ht = RT_INF; hcode = -1;
            for (uint32_t wd = 0; wd < words; wd++) {
              unsigned long long cand = 0ull, todo = __ballot(true);
              uint32_t distinct = 0;
              while (todo) {
                const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)__builtin_ctzll(todo));
                cand |= rt_load_word32(rt_cold_args()->bounce_table, k0 * words + wd);
                todo &= ~__ballot(key == k0);
                if (++distinct == 16u && todo) {           // a wave whose rays fan out over many cells: scan everything
                  cand = (wd + 1u == words && (NLOOP & 63u)) ? ((1ull << (NLOOP & 63u)) - 1ull) : ~0ull;
                  break;
                }
              }
              while (cand) {
                const uint32_t j = (wd << 6) + (uint32_t)__builtin_ctzll(cand);
                cand &= cand - 1ull;
                const rt_geom g0 = rt_load_geom32(geom, j);
                RT_GENERIC(j, g0)
              }
            }
            scanned = true;
          }
        }
#endif
#if !RT_STRICT
        // Few spheres, no refraction: at the node after the primary the launch table may name the spheres a ray reflected at a primary hit of this
        // block can meet at all (word 3 of the entry: rt_block.h, rt_first_bounce_set).  The wave walks that set on the scalar unit, like the primary
        // cull's survivors, in index order - the strict-< tie-break of the full scan is kept - and tests nothing else.
        if constexpr (!GRID && !REFRACT && !COUNT && !ITEM) {
          if (first_bounce) {
            uint32_t fb = rt_entry_first_bounce<W1>(L);
#ifdef RT_TESTING
            if (L.no_first_bounce) fb = 0u;               // test build (RT_NO_FIRST_BOUNCE): every wave on the full scan
#endif
            if (fb >> 31) {
              ht = RT_INF; hcode = -1;
              uint32_t m = (fb >> RT_CELL_SHIFT) & ((1u << RT_FB_MAX_LOOP) - 1u);
              // ... less the candidates that word 1 of the entry says no reflected ray of the block can be accepted at: the mirror the ray
              // starts on, whose test finds a far root of 0 up to rounding (rt_block.h: rt_self_clear).  Scalar work only.  (The word's own
              // load, not one 16-byte load for both words: measured the same, docs/EVIDENCE.md.)
              uint32_t sn = rt_entry_second_node<W1>(L);
#ifdef RT_TESTING
              if (L.no_second_node) sn = 0u;                // test build (RT_NO_SECOND_NODE): the whole set is walked
              if ((sn & (RT_SN_SELF0 | RT_SN_SELF1)) && L.uniform_waves != nullptr && __builtin_ctzll(__ballot(true)) == (int)lane) atomicAdd(L.uniform_waves + 3, 1ull);
#endif
              if (sn & RT_SN_SELF0) m &= ~(1u << (fb & 255u));
              if (sn & RT_SN_SELF1) m &= ~(1u << ((fb >> 8) & 255u));
              while (m) {
                const uint32_t i = (uint32_t)__builtin_ctz(m);
                m &= m - 1u;
                const rt_geom g0 = rt_load_geom32(geom, i);
                RT_GENERIC(i, g0)
              }
              scanned = true;
#ifdef RT_TESTING
              if (L.uniform_waves != nullptr && __builtin_ctzll(__ballot(true)) == (int)lane) atomicAdd(L.uniform_waves + 2, 1ull);
#endif
            }
          }
        }
#endif
        if (!scanned) {
          ht = RT_INF; hcode = -1;
          uint32_t i = 0;
          for (; i + 2 <= NLOOP; i += 2) {
            const rt_geom_pair gp = rt_load_geom_pair32(geom, i);
            const rt_geom g0 = gp.a, g1 = gp.b;
            RT_GENERIC(i, g0) RT_GENERIC(i + 1, g1)
          }
          if (i < NLOOP) { const rt_geom g0 = rt_load_geom32(geom, i); RT_GENERIC(i, g0) }
        }
      }
      [[maybe_unused]] const bool primary_node = UNI || searched;       // wave-uniform: this node is the primary ray's
      if constexpr (!WAVE_NODE) {                                       // (WAVE_NODE: the three are set from the turn's number, above)
      first_bounce = searched;                                          // ... and the next one, if any, the first bounce's
      searched = false;
      }
      // ---- the enclosing sphere ----
      // The enclosing sphere (every other sphere, light and the camera strictly inside it: a skybox) is
      // kept LAST in the device tables and outside the loops above: it can only be the closest hit of a
      // ray that hits nothing else.  Only the lanes still without a hit evaluate it.
      if (!UNI && enc != ~0u && hcode < 0) {
        if (L.enclosing_flat) {
          // ... and when that sphere is flat - no lighting, no children, a colour that does not depend on the hit point (the
          // reference's skybox: albedo [1,0,0,0,0], main.js:124) - WHERE the ray meets it does not matter: a ray that starts
          // strictly inside it always does (main.js:429-439 returns t1 > 0.001), so the test is not evaluated at all
          ht = 1.0; hcode = (int)(2u * enc + 1u);
        } else {
          const rt_geom g0 = rt_load_geom32(geom, enc);
          RT_GENERIC(enc, g0)
        }
      }
      if (COUNT) cnt[2] += N;
      const int hi = UNI ? (int)(cand_host & 255u) : (hcode >> 1);      // (UNI: the one candidate - a scalar)
      const bool inside = (hcode & 1) != 0;
      bool descend = false;
#if defined(RT_TESTING) && defined(RT_ABLATE_SHADE)
      if (true) { ret[0] = ht; ret[1] = (double)hcode; ret[2] = 0.0; RT_CHAIN_END() } else
#endif
      if (!UNI && hcode < 0) {                        // main.js:231 (with a flat sky of constant colour: that sky's pixel term, see rt_launch.hip bind_kernel)
        // (product build: read where it is used, from the kernarg segment: six scalar registers less across the whole loop)
        { const auto &mc = RT_COLD(miss_color); ret[0] = mc[0]; ret[1] = mc[1]; ret[2] = mc[2]; }
#ifdef RT_TESTING
        if (is_probe && probe_n < RT_PROBE_NODES) {
          double *q = L.probe + (size_t)(probe_n++) * RT_PROBE_WORDS;
          for (uint32_t z = 0; z < RT_PROBE_WORDS; z++) q[z] = 0.0;
          q[0] = (double)(REFRACT ? tree_path : (1u << rt_lvl(level))); q[1] = -1.0; q[2] = ht; q[9] = d.x; q[10] = d.y; q[11] = d.z;
          q[17] = (double)segs_left; q[19] = p.x; q[20] = p.y; q[21] = p.z; q[23] = 1.0;
        }
#endif
        RT_CHAIN_END()
      } else {
        typename rt_mtl_src<UNI>::type &m = *rt_mtl_at<UNI>(mtl, (uint32_t)hi);      // per-lane index, a 32-bit offset (LDS; the many-sphere variant: HBM / L2); UNI: the wave's one record, scalar loads
        // A2 ext part for the closest hit only (main.js:440-447; pure, so deferring it is exact)
        const v3 h = mk(p.x + d.x * ht, p.y + d.y * ht, p.z + d.z * ht);
#if RT_STRICT
        double nlen;
        const v3 n = unit(mk(h.x - m.origin[0], h.y - m.origin[1], h.z - m.origin[2]), &nlen);
#else
        // the hit point lies on the sphere, so |h - o| is r up to the rounding of h: scale by the stored 1/r
        const double inv_r = m.inv_r;
        const v3 n = mk((h.x - m.origin[0]) * inv_r, (h.y - m.origin[1]) * inv_r, (h.z - m.origin[2]) * inv_r);
#endif
        v3 l;                                                           // hit.l, quirk q5
        // (UNI: no lane is inside the candidate - a wave with one left before its hit test's ballot, above - so l is n)
        if constexpr (UNI) l = n;
        else l = inside ? mk(-n.x, -n.y, -n.z) : n;
        double a0 = m.albedo[0];                                        // (a0, a3: SIX_WAVES reads them again behind the lighting, below)
        const double a1 = m.albedo[1], a2 = m.albedo[2];
        double a3 = m.albedo[3];
        const double a4 = REFRACT ? m.albedo[4] : 0.0;
#if !RT_STRICT && !defined(RT_ABLATE_QAMP)     /* (RT_ABLATE_QAMP: timing experiment, profiles/ab_build.sh) */
        // Q of this hit (see above): for a bounced ray's hit, and for a primary hit that will spawn a ray (ht is at hand here)
        // (WAVE_NODE: rt_lvl(level) is the turn's number - a scalar test, and no test at all below the primary)
        if (!UNI && ((WAVE_NODE ? node_no != 0u : rt_lvl(level) != 0) || ((a3 > 0.0 || a4 > 0.0) && segs_left > 1))) {      // (UNI: a primary hit that spawns nothing)
          const float ir_ = (float)inv_r;
          const float q_ = RT_Q_OF(RT_Q_GET(level), (float)ht, ir_, __builtin_fabsf((float)dot(d, n)), rt_r_get(level));
          level = rt_q_put(level, q_);
          level = rt_r_put(level, __builtin_amdgcn_rcpf(ir_));
        }
#endif

        // ---- A8 sampler ----
        // A8 sampler (main.js:320).  Pure, so it is evaluated here, before the lighting, where few values
        // are live: the OCML atan2/asin bodies are the register-pressure peak of the kernel.
        double col[3];
#if defined(RT_TESTING) && defined(RT_ABLATE_SAMPLER)   /* timing experiments only (profiles/ab_build.sh); never defined in the product build */
        const int kind = RT_SAMPLER_COLOR;
#else
        const int kind = rt_mtl_kind(m);
#endif
#if RT_STRICT
        if (kind == RT_SAMPLER_TEXTURE) {
          double t_at, t_as;
          rt_atan2_asin<REFRACT>(-n.z, -n.x, -n.y, &t_at, &t_as);
          const double u = RT_DIV_CONST(t_at, M_PI) / 2.0 + 0.5;   // main.js:446 (q6: two divisions)
          const double v = RT_DIV_CONST(t_as, M_PI / 2.0) / 2.0 + 0.5;  // main.js:447
          const rt_texture_desc td = rt_tex_desc<UNI>(tex, rt_mtl_texture(m));
          const double xd = ceil(u * (double)td.width) - 1.0, yd = ceil(v * (double)td.height) - 1.0;
          uint32_t xi = (xd > 0.0) ? (uint32_t)xd : 0u, yi = (yd > 0.0) ? (uint32_t)yd : 0u;
          xi = min(xi, td.width - 1u); yi = min(yi, td.height - 1u);   // memory safety only; u,v <= 1
          const uint32_t texel = *(const uint32_t *)(L.texel_base + td.texels_offset + ((size_t)yi * td.width + xi) * 4u);
          col[0] = RT_DIV_CONST((double)(texel & 255u), 255.0); col[1] = RT_DIV_CONST((double)((texel >> 8) & 255u), 255.0);
          col[2] = RT_DIV_CONST((double)((texel >> 16) & 255u), 255.0);
          if (xd != xd || yd != yd) col[0] = col[1] = col[2] = __builtin_nan("");   // texels[NaN] is undefined in JS
        } else if (kind == RT_SAMPLER_CHECKER) {
          double t_at, t_as;
          rt_atan2_asin<REFRACT>(-n.y, -n.x, -n.z, &t_at, &t_as);
          const double u = RT_DIV_CONST(t_at, M_PI) / 2.0 + 0.5;   // main.js:127 (its own axes)
          const double v = RT_DIV_CONST(t_as, M_PI / 2.0) / 2.0 + 0.5;  // main.js:128
          const int c = to_int32_bit0(u * m.c[6]) ^ to_int32_bit0(v * m.c[7]);
          col[0] = m.c[3 * c]; col[1] = m.c[3 * c + 1]; col[2] = m.c[3 * c + 2];
#else
        // ---- Texture (main.js:143-145, 343-351, u, v of :446-447) and sphere-checker (main.js:126-133, its own u, v), and the
        // boundary marks.
        // (UNI: the sampler is the wave's - ONE inlined copy of the atan2 / asin pair serves both, its arguments chosen by the scalar kind)
        [[maybe_unused]] double t_at, t_as;
        // (UNI, bit 24 of cand_host: the launch table states that every sample of this wave meets the candidate inside ONE checker cell,
        // clear of the boundary test's band - parity in bit 28, rt_block.h: rt_column_cell.  The wave then agrees on nothing: no u, v)
        // (few-sphere kernels only: the many-sphere one-wave form has no scalar register left for it - tests/test_kernel_resources.py)
        [[maybe_unused]] const bool one_cell = UNI && !GRID && kind == RT_SAMPLER_CHECKER && (cand_host & (1u << 24)) != 0u;
        // UNI: ONE decision tree on the scalar sampler kind, the commonest wave first - a floor block with its cell stated falls through to
        // its colours; then plain colour; then the two samplers that need u, v, behind their one atan2 / asin pair.  Every arm is entered
        // by a scalar compare and leaves for the lighting.  (As one chain of conditions shared with the general path every arm's outcome
        // was a lane-mask flag set in one block and tested in the next: ~39 scalar instructions and six taken branches between the
        // cell-stated wave's primary root and its light loop, ~22 now - the arms' exits still meet in one test; docs/EVIDENCE.md, first section.)
        if (UNI && one_cell) {
          // the cell's colour: three scalar operands, fetched through a scalar offset (nothing per lane)
          const uint32_t c3 = (cand_host >> 28) & 1u ? 3u : 0u;
          col[0] = m.c[c3]; col[1] = m.c[c3 + 1u]; col[2] = m.c[c3 + 2u];
        } else if (UNI && kind != RT_SAMPLER_TEXTURE && kind != RT_SAMPLER_CHECKER) {      // (stars were turned away before the hit test)
          col[0] = m.c[0]; col[1] = m.c[1]; col[2] = m.c[2];
        } else {
        if constexpr (UNI) {
          const bool tx_ = (kind == RT_SAMPLER_TEXTURE);
          rt_atan2_asin<REFRACT>(tx_ ? -n.z : -n.y, -n.x, tx_ ? -n.y : -n.z, &t_at, &t_as);
        }
        if (kind == RT_SAMPLER_TEXTURE) {
          if constexpr (!UNI) rt_atan2_asin<REFRACT>(-n.z, -n.x, -n.y, &t_at, &t_as);
          const double u = RT_DIV_CONST(t_at, M_PI) / 2.0 + 0.5;   // main.js:446 (q6: two divisions)
          const double v = RT_DIV_CONST(t_as, M_PI / 2.0) / 2.0 + 0.5;  // main.js:447
          const rt_texture_desc td = rt_tex_desc<UNI>(tex, rt_mtl_texture(m));
          const double xu = u * (double)td.width, xv = v * (double)td.height;
          // max(0, ceil(x) - 1) (main.js:344-345) is floor(x) for every x >= 0 that is not an integer, and the integers are marked:
          // the index comes out of the fixed-point sum (u, v in [0, 1]; widths and heights <= 16384)
          RT_XY_INDEX(xu, xv, 1.0, 1.0)                              // (UNI: `return false` from HERE when a lane is inside the prefilter band)
          const uint32_t xi = min(iu, td.width - 1u), yi = min(iv, td.height - 1u);   // memory safety only; u,v <= 1
          const uint32_t texel = *(const uint32_t *)(rt_cold_args()->texel_base + td.texels_offset + ((size_t)yi * td.width + xi) * 4u);
          col[0] = RT_DIV_CONST((double)(texel & 255u), 255.0); col[1] = RT_DIV_CONST((double)((texel >> 8) & 255u), 255.0);
          col[2] = RT_DIV_CONST((double)((texel >> 16) & 255u), 255.0);
        } else if (kind == RT_SAMPLER_CHECKER) {
          if constexpr (!UNI) rt_atan2_asin<REFRACT>(-n.y, -n.x, -n.z, &t_at, &t_as);
          const double u = RT_DIV_CONST(t_at, M_PI) / 2.0 + 0.5;   // main.js:127 (its own axes)
          const double v = RT_DIV_CONST(t_as, M_PI / 2.0) / 2.0 + 0.5;  // main.js:128
          const double xu = u * m.c[6], xv = v * m.c[7];
          RT_XY_INDEX(xu, xv, m.c[6], m.c[7])                        // (UNI: `return false` from HERE when a lane is inside the prefilter band)
          const int c = (int)((iu ^ iv) & 1u);                       // the parity of floor(x) = ToInt32(x) & 1 for x in [0, 2^31)
          if constexpr (UNI) {                                        // both colours are in scalar registers: the lane picks
            // (opaque copies: the compiler otherwise selects the ADDRESS per lane and fetches through the vector memory path)
            double k0 = m.c[0], k1 = m.c[1], k2 = m.c[2], k3 = m.c[3], k4 = m.c[4], k5 = m.c[5];
            asm volatile("" : "+s"(k0), "+s"(k1), "+s"(k2), "+s"(k3), "+s"(k4), "+s"(k5));
            col[0] = c ? k3 : k0; col[1] = c ? k4 : k1; col[2] = c ? k5 : k2;
          } else { col[0] = m.c[3 * c]; col[1] = m.c[3 * c + 1]; col[2] = m.c[3 * c + 2]; }
#endif
        } else if (!UNI && kind == RT_SAMPLER_STARS) {      // (UNI: stars stay on the general path)
          // the sample's index in the FRAME (not in this call's tiles), recomputed from the work-item id so that it
          // costs no register outside this branch; `path` is the node's position in the ray tree
          uint32_t sx = own_sx, sy = own_sy, f = own_f;   // rt_retrace hands the sample and its frame over
          if constexpr (!ITEM) {
            f = blockIdx.z;                          // the frame of the batch
            uint32_t t3 = threadIdx.x;
            if constexpr (W1 && !GRID) t3 = rt_lane_again(); else
            asm volatile("" : "+v"(t3));
            const rt_pixel P = rt_pixel_of<SS2, W1>(L, t3);
            sx = SS2 ? 2u * P.px + (P.sub & 1u) : P.px; sy = SS2 ? 2u * P.frow + (P.sub >> 1) : P.frow;
          }
          const unsigned long long pix = (unsigned long long)sy * (SS2 ? 2u * L.w : L.w) + sx;
          const uint32_t path = REFRACT ? tree_path : (1u << rt_lvl(level));
          // the seed of this frame, read here from the kernarg segment: no other path holds it in a register
          const rt_launch __attribute__((address_space(4))) *K = rt_cold_args();
          const uint32_t mix = lowbias32(K->stars_seed + K->stars_step * f);
          double c = star_uniform((uint32_t)pix, (uint32_t)(pix >> 32), path, mix);
          c = (c >= m.c[6]) ? 0.0 : c * m.c[7];     // main.js:137-138
          col[0] = col[1] = col[2] = c;
        } else { col[0] = m.c[0]; col[1] = m.c[1]; col[2] = m.c[2]; }
#if !RT_STRICT
        }                                                               // (the third arm of the product build's tree above)
#endif

        // general product kernel: the sampled colour waits in LDS (slots 10-12 of the lane's fold state) while the
        // lights are scanned: six registers fewer across the hottest loop, which is what lets this kernel fit
        // 96 VGPRs = 5 waves per SIMD
        if constexpr (FOLD_FORWARD && REFRACT) {
#pragma unroll
          for (int c = 0; c < 3; c++) acc[(10 + c) * RT_WG_THREADS] = col[c];
        }

        // ---- A7 lights and shadow scan ----
        // A7 lighting and shadows
        double diffuse = 0.0, specular = 0.0;
        [[maybe_unused]] double draw = 0.0, sraw = 0.0;                // (UNI: the light loop's sums before their clamps, for the leaf's NaN test)
#if defined(RT_TESTING) && defined(RT_ABLATE_LIGHT)
        if (false) {
#else
        if (a1 > 0.0 || a2 > 0.0) {
#endif
          double li = RT_COLD(light_intensity);                        // shared across lights (q2); product build: read where it is used (two scalar registers less across the loop)
#if !RT_STRICT
          [[maybe_unused]] uint32_t smask = ~0u;
          if constexpr (!COUNT) { if (primary_node) smask = rt_entry_shadow_masks<W1>(L); }
          // (SIX_FORMS) the entry's word - all ones at a node below the primary - under 32 set bits: light k's set is then ONE 64-bit shift by 16 min(k, 2) - the
          // set of light 0 or 1, or all ones from the third light on - in place of a test of k and a test of the set, combined as lane masks
          [[maybe_unused]] const unsigned long long smask64 = 0xffffffff00000000ull | smask;
#endif
          for (uint32_t k = 0; k < NL; k++) {
            double llen;
            // light k from the kernarg segment through a 32-bit byte offset (scalar load with an SGPR offset)
            const double *lk = (const double *)((const char *)&L.lights[0][0] + (uint32_t)(k * 24u));
#if !RT_STRICT
            // few spheres (no shadow grid): the scan's first two records are READ here, with the light's position, so that their latency
            // could hide behind the light vector's normalisation (measured -0.3 % on the headline when it was written, and +0.4 % where
            // the grid path made it a wasted load).  In today's code object the compiler sinks the load to its use: the s_load_dwordx16
            // stands behind the normalisation, in front of the scan's first pair, in both copies of the loop - and a block whose entry
            // says that nothing can shadow it (no_occluder) does not load at all.  Pinning the load here (an opaque copy of the pair
            // in front of the facing test) makes every light of every wave pay for it: headline -1.7 % (docs/EVIDENCE.md, first section)
            [[maybe_unused]] rt_geom_pair gp_first;
            if constexpr (!GRID && !COUNT) {
              [[maybe_unused]] const geom_kptr gl = (geom_kptr)L.geom_light;
              gp_first = rt_load_geom_pair32(gl, k * L.n_objects);
            }
#endif
            const v3 sraw = mk(lk[0] - h.x, lk[1] - h.y, lk[2] - h.z);
            const double lmag = dot(sraw, sraw);
#if RT_STRICT
            const v3 sv = unit(sraw, &llen);
#else
            const double inv_llen = rt_rsqrt_pos(lmag);               // lights never coincide with a surface point
            llen = lmag * inv_llen;
            const v3 sv = mk(sraw.x * inv_llen, sraw.y * inv_llen, sraw.z * inv_llen);
#endif
            const double sdot = dot(sv, l);
#if RT_STRICT
            if (sdot <= 0.0) continue;                                 // surface faces away (main.js:292)
#else
            if (!(sdot > 0.0)) continue;                               // the same; and a light AT the hit point: lmag == 0 makes sdot 0 there, NaN here
#endif
            if (COUNT) cnt[1]++;
            // Shadow scan (main.js:293-304) over every sphere but the one just hit (q3).  A fully blocked lane
            // keeps li == 0 whatever follows, so leaving the loop is a pure shortcut, taken per pair.
            uint32_t tests = 0;
            bool blocked = false;
#if !RT_STRICT
            // walked from the light: origin = light k (uniform), direction = -sv, the hit point is at llen
            const geom_kptr gl = (geom_kptr)L.geom_light;
            const uint32_t glo = k * L.n_objects;                      // light k's table: a 32-bit index offset (rt_load_geom32)
#else
            const geom_kptr gl = geom;
            const uint32_t glo = 0u;
#endif
#if defined(RT_TESTING) && defined(RT_ABLATE_SHADOW)
            const uint32_t NS = 0;
#elif defined(RT_TESTING) && defined(RT_ABLATE_SHADOW4)
            const uint32_t NS = NLOOP > 4u ? NLOOP - 4u : NLOOP;      // timing only: what skipping four tests per light would be worth
#else
            const uint32_t NS = NLOOP;
#endif
#if !RT_STRICT
            // Primary hits of a block whose table entry says that NO sphere can stand between the block's hit points and light k
            // (rt_block.h, shadow masks; most floor blocks): neither grid nor scan.
            bool no_occluder = false;
            [[maybe_unused]] uint32_t occ = ~0u;                        // (SIX_FORMS) bits 0..15: the spheres that can shadow this block from light k (a bounced node, a third light: all ones)
            if constexpr (SIX_FORMS) {
              occ = (uint32_t)(smask64 >> (16u * (k < 2u ? k : 2u)));
              if constexpr (UNI) asm volatile("" : "+s"(occ));          // (opaque on the uniform path alone: a word, not two conditions.  The general path's node count is a value of a loop that lanes leave one by one, which a build may regard as per-lane: no scalar constraint there)
              no_occluder = (occ & 0xffffu) == 0u;
            } else
            if constexpr (!COUNT) no_occluder = primary_node && k < 2u && ((smask >> (16u * k)) & 0xffffu) == 0u;
            if (no_occluder) {
            } else
            if (GRID && rt_cold_args()->shadow_grid != nullptr && li != 0.0) {
              // Many spheres: cull the scan with the light's grid.  The host cut light k's view of the scene
              // (projective coordinates x'/z', y'/z' in a frame looking from the light at the scene) into
              // RT_SGRID x RT_SGRID cells and stored, per cell, the bit set of spheres whose conservative rectangle
              // (same construction as the primary-ray cull, with the light as the eye) touches it.  A lane's shadow
              // ray lies on the line from the light through its hit point, so only the spheres of that point's cell
              // can block it.  The wave tests the UNION over its active lanes: the distinct cells are walked with
              // readlane/ballot (correct under divergence: it never relies on inactive lanes), typically 1-4 of them.
              const void *const sgrid = rt_cold_args()->shadow_grid;     // (read where it is used: the many-sphere kernels have no scalar register to spare)
              const double __attribute__((address_space(4))) *gh = (const double __attribute__((address_space(4))) *)sgrid + 16u * k;
              const v3 vv = mk(-sraw.x, -sraw.y, -sraw.z);                                   // light -> hit point
              const double vx = gh[0] * vv.x + gh[1] * vv.y + gh[2] * vv.z, vy = gh[3] * vv.x + gh[4] * vv.y + gh[5] * vv.z;
              const double vz = gh[6] * vv.x + gh[7] * vv.y + gh[8] * vv.z;
              const double iz = rt_rcp(vz);
              const double fx = __builtin_fmin(__builtin_fmax((vx * iz - gh[9]) * gh[11], 0.0), (double)(RT_SGRID - 1));
              const double fy = __builtin_fmin(__builtin_fmax((vy * iz - gh[10]) * gh[12], 0.0), (double)(RT_SGRID - 1));
              const bool proj = (vz > 0.0) && (fx == fx) && (fy == fy);
              const uint32_t cell = proj ? (uint32_t)fy * RT_SGRID + (uint32_t)fx : (uint32_t)(RT_SGRID * RT_SGRID);   // last cell: every sphere
              const uint32_t words = (NLOOP + 63u) >> 6;
              const uint32_t cells_at = 16u * NL + k * (RT_SGRID * RT_SGRID + 1u) * words;      // in 64-bit words from the grid's start
              for (uint32_t wd = 0; wd < words; wd++) {
                unsigned long long cand = 0ull, todo = __ballot(true);
                while (todo) {
                  const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)cell, (int)__builtin_ctzll(todo));
                  cand |= rt_load_word32(sgrid, cells_at + c0 * words + wd);
                  todo &= ~__ballot(cell == c0);
                }
                while (cand) {
                  const uint32_t j = (wd << 6) + (uint32_t)__builtin_ctzll(cand);
                  cand &= cand - 1ull;
                  const rt_geom g0 = rt_load_geom32(gl, glo + j);
                  RT_SHADOW_U(j, g0)                                                          // the grid variant never counts
                }
              }
            } else
#endif
            if (!COUNT) {
              // (UNI: pinned, so that the wave's scalar no_occluder test above stays a compare and a branch of its own instead of being folded,
              // as a lane mask, into this per-lane test's exec mask)
              if constexpr (UNI) RT_PIN();
              if (li != 0.0) {
                uint32_t j = 0;
#if !RT_STRICT
                // a non-empty set still skips the PAIRS of the scan neither sphere of which is in it (a loop over just the named
                // spheres would cost the kernel its 96th register)
                // (WAVE_NODE: primary_node is a scalar compare, so mk - the entry's word, a shift and an OR - lives in a scalar register and a pair
                // is decided by a scalar bit test and a branch of its own; elsewhere primary_node is a lane mask, mk a vector register selected
                // under it, and every pair tests it per lane.  At a bounced node mk is ~0 and the scalar test still runs: a second copy of the
                // scan without it spilled ten scalar registers in the six-wave kernels and measured slower - docs/EVIDENCE.md)
                [[maybe_unused]] uint32_t mk = ~0u;
                if constexpr (SIX_FORMS) mk = occ | 0xffff0000u;      // (the same word: k >= 2 and every node below the primary have all ones)
                else
                if constexpr (!GRID) { if (primary_node && k < 2u) mk = (smask >> (16u * k)) | 0xffff0000u; }
                if constexpr (!GRID) {
                  if (NS >= 2u) { if (mk & 3u) { const rt_geom g0 = gp_first.a, g1 = gp_first.b; RT_SHADOW_U(0u, g0) RT_SHADOW_U(1u, g1) } j = 2u; }
                }
#endif
                for (; j + 2 <= NS; j += 2) {
#if !RT_STRICT
                  // (WAVE_NODE: mk is a scalar, and the same test is a shift, an AND and a branch on the scalar unit - bits 30 and 31 of mk are set)
                  // (the few-sphere uniform path: its mk is a scalar word as well - occ, above - and takes the same form)
                  if constexpr (WAVE_NODE || (UNI && !GRID)) { if (((mk >> (j < 30u ? j : 30u)) & 3u) == 0u) continue; } else
                  if (!GRID && j < 31u && ((mk >> j) & 3u) == 0u) continue;       // (sets name 16 spheres; the upper half of mk is all ones: beyond bit 30 every pair is scanned)
#endif
                  const rt_geom_pair gp = rt_load_geom_pair32(gl, glo + j);
                  const rt_geom g0 = gp.a, g1 = gp.b;
                  RT_SHADOW_U(j, g0) RT_SHADOW_U(j + 1, g1)
                }
#if !RT_STRICT
                if (j < NS && (GRID || j >= 32u || ((mk >> j) & 1u))) { const rt_geom g0 = rt_load_geom32(gl, glo + j); RT_SHADOW_U(j, g0) }
#else
                if (j < NS) { const rt_geom g0 = rt_load_geom32(gl, glo + j); RT_SHADOW_U(j, g0) }
#endif
              }
            } else
            if (COUNT || li != 0.0) {                  // li == 0 on entry (an earlier light was blocked) cannot change
              uint32_t j = 0;
              for (; j + 2 <= NS; j += 2) {
                const rt_geom g0 = rt_load_geom32(gl, glo + j), g1 = rt_load_geom32(gl, glo + j + 1);
                RT_SHADOW(j, g0) RT_SHADOW(j + 1, g1)
                if (blocked) break;
              }
              if (j < NS && !blocked) { const rt_geom g0 = rt_load_geom32(gl, glo + j); RT_SHADOW(j, g0) }
            }
            if (COUNT) cnt[2] += tests;
            if (li == 0.0) continue;
#if RT_STRICT
            diffuse += li * sdot / lmag;                               // main.js:306
#else
            diffuse += (li * sdot) * (inv_llen * inv_llen);            // 1/lmag = (1/llen)^2, already at hand
#endif
#if defined(RT_TESTING) && defined(RT_ABLATE_SPEC)
            if (false) {
#else
            if (a2 > 0.0) {                                            // main.js:307-314
#endif
#if RT_STRICT
              double ql;
              const v3 q = unit(reflect(mk(-sv.x, -sv.y, -sv.z), l), &ql);
              const double spd = d.x * -q.x + d.y * -q.y + d.z * -q.z;
#else
              // reflect(-sv, l) = -sv + l*(2 sv.l): sv.l is sdot, and the mirror image of a unit vector in
              // a unit normal is a unit vector, so the reference's re-normalisation moves it by an ulp at most
              const double t2 = 2.0 * sdot;
              const v3 q = mk(__builtin_fma(l.x, t2, -sv.x), __builtin_fma(l.y, t2, -sv.y), __builtin_fma(l.z, t2, -sv.z));
              const double spd = -(d.x * q.x + d.y * q.y + d.z * q.z);
#endif
#if !RT_STRICT
              // (materials in HBM - the reflection-only many-sphere variants -: the record's address is derived again here, from the hit
              // code, so that no 64-bit pointer lives across the shadow scans)
              typename rt_mtl_src<UNI>::type *spec_m = &m;
              if constexpr (GRID && !REFRACT && !COUNT && !UNI) {
                uint32_t off_ = (uint32_t)hi * (uint32_t)sizeof(rt_mtl);
                asm volatile("" : "+v"(off_));
                spec_m = (const rt_mtl *)((const char *)mtl + off_);
              }
              const int32_t spec_n = spec_m->spec_n;
              if (spd > 0.0) specular += rt_pow_spec<UNI, SIX_FORMS>(spd, spec_n, &spec_m->specular_exponent);
#else
              if (spd > 0.0) specular += rt_pow(spd, m.specular_exponent);
#endif
            }
          }
          if constexpr (UNI) {
            // one-instruction clamps (a NaN sum comes out as 1 here: the wave's leaf below tests the raw sums and takes the select forms then)
            draw = diffuse; sraw = specular;
            diffuse = rt_min1_nn(diffuse) * a1;
            specular = rt_min1_nn(specular) * a2;
          } else {
          diffuse = min1(diffuse) * a1;
          specular = min1(specular) * a2;
          }
#ifdef RT_TESTING
          probe_li = li;
#endif
        }

        // (the few-sphere one-wave kernels) The ambient and the reflection coefficient are not needed by the lighting: they are read AGAIN
        // here, the same two LDS words through an index the compiler cannot match with the first read, so that four registers less are
        // held across the shadow scans.  A reload: the same bits.
        if constexpr (SIX_WAVES) {
          uint32_t hi2 = (uint32_t)hi;
          asm volatile("" : "+v"(hi2));
          const rt_mtl &m2 = *rt_mtl_at<false>(mtl, hi2);
          a0 = m2.albedo[0]; a3 = m2.albedo[3];
        }

        // ---- A4 / A5 directions ----
        // A4 reflection direction.  (Computed AFTER the lighting: in program order the reference does it before, but it
        // is pure, and placed here neither r nor f — nor n, which is l with its sign restored — occupies registers
        // across the shadow scans, the hottest loop of the kernel.)
#if RT_STRICT
        const v3 nq = n;
#else
        const v3 nq = inside ? mk(-l.x, -l.y, -l.z) : l;
#endif
        v3 r = mk(0, 0, 0); double rlen = 0.0;
        // (with segs_left == 1 the child returns [0,0,0] at main.js:221 whatever its direction: skip it)
#if !RT_STRICT
        // LEAN: the mirror image in l instead of nq = +-l - d - 2 (d.nq) nq holds nq as a product of two, and negation is exact in every
        // product, sum and fma on the way: the same bits for nq and -nq, without the three v_xor and six v_cndmask_b32 that restore the sign
        // (the REFRACT kernels keep nq: the refraction reads its sign).  unit_go: the lanes that read r are those with rlen != 0 (go_r, below).
        if constexpr (LEAN) { if (!UNI && a3 > 0.0 && segs_left > 1) r = unit_go(reflect(d, l), &rlen); } else
#endif
        if (!UNI && a3 > 0.0 && segs_left > 1) r = unit(reflect(d, nq), &rlen);     // (UNI: decided against, for the wave, before the hit test)
        // A5 refraction direction
        v3 f = mk(0, 0, 0); double flen = 0.0;
        if (REFRACT && a4 > 0.0 && segs_left > 1) {
          const double dn = dot(d, nq);
          double cosi = -((dn < -1.0) ? -1.0 : min1(dn));              // -Math.max(-1, Math.min(1, dot))
          v3 nn = nq; double eta;
          if (cosi < 0.0) { cosi = -cosi; nn = mk(-nq.x, -nq.y, -nq.z); eta = m.refract_index; }
          else eta = rt_rcp(m.refract_index);
          const double k = 1.0 - eta * eta * (1.0 - cosi * cosi);
          if (k > 0.0) {
            const double q = eta * cosi - rt_sqrt(k);
            f = mk(d.x * eta + nn.x * q, d.y * eta + nn.y * q, d.z * eta + nn.z * q);
          } else f = reflect(d, nn);                                   // total internal reflection
          f = unit(f, &flen);
        }

        // ---- A6 fold / descend ----
        if constexpr (FOLD_FORWARD && REFRACT) {
#pragma unroll
          for (int c = 0; c < 3; c++) col[c] = acc[(10 + c) * RT_WG_THREADS];
        }
        const bool go_r = !UNI && (rlen != 0.0);
        const bool go_f = REFRACT && (flen != 0.0);
#ifdef RT_TESTING
        if (is_probe && probe_n < RT_PROBE_NODES) {
          double *q = L.probe + (size_t)(probe_n++) * RT_PROBE_WORDS;
          q[0] = (double)(REFRACT ? tree_path : (1u << rt_lvl(level))); q[1] = (double)hcode; q[2] = ht;
          q[3] = h.x; q[4] = h.y; q[5] = h.z; q[6] = n.x; q[7] = n.y; q[8] = n.z; q[9] = d.x; q[10] = d.y; q[11] = d.z;
          q[12] = col[0]; q[13] = col[1]; q[14] = col[2]; q[15] = diffuse; q[16] = specular; q[17] = (double)segs_left;
          q[18] = probe_li; q[19] = p.x; q[20] = p.y; q[21] = p.z; q[22] = (double)(go_r ? 1 : 0) + 2.0 * (go_f ? 1 : 0); q[23] = 1.0;
        }
#endif
        if (!go_r && !go_f) {
          // children are absent or return [0,0,0] (segs == 0, main.js:221): x + 0*a == x
          if constexpr (UNI) {
            // The wave's eight clamps as one instruction each (rt_kernel_math.h: rt_min1_nn, rt_max_nn) if NO lane holds a NaN in a
            // clamped quantity: the light loop's two sums and the three channel sums, all five added into one number that is NaN if
            // any of them is (an inf - inf false alarm only takes the exact arm).  The ambient term col * a0 may be NaN in either arm.
            double x[3];
#pragma unroll
            for (int c = 0; c < 3; c++) x[c] = col[c] * diffuse + col[c] * specular;
            const double poison = (((draw + sraw) + x[0]) + x[1]) + x[2];
            if (__ballot(poison != poison) == 0ull) {
#pragma unroll
              for (int c = 0; c < 3; c++) ret[c] = rt_max_nn(col[c] * a0, rt_min1_nn(x[c]));
            } else {
              // a NaN in the wave: the statements of the general path, from the raw sums (zero, and no product with a1 or a2, where the light loop did not run)
#if defined(RT_TESTING) && defined(RT_ABLATE_LIGHT)
              const bool lit = false;
#else
              const bool lit = (a1 > 0.0 || a2 > 0.0);
#endif
              const double d2 = lit ? min1(draw) * a1 : 0.0, s2 = lit ? min1(sraw) * a2 : 0.0;
#pragma unroll
              for (int c = 0; c < 3; c++) ret[c] = maxa(col[c] * a0, min1(col[c] * d2 + col[c] * s2));
            }
          } else {
#pragma unroll
          for (int c = 0; c < 3; c++) ret[c] = maxa(col[c] * a0, min1(col[c] * diffuse + col[c] * specular));
          RT_CHAIN_END()
          }
        } else if constexpr (FOLD_FORWARD) {
          // Each level maps its child's colour x through  f(x) = max(amb, min(1, (ds [+ other child]) + a*x))
          // (main.js:326-336), a non-decreasing clamped-affine map, and compositions of such maps are again
          // clamped-affine.  So the pixel, as a function of the colour of the ray currently being traced, is kept in
          // closed form  F(x) = max(LO, min(HI, O + S*x))  (S one scalar; O, LO, HI per channel) and updated on the
          // way DOWN: a node with ONE child (reflection-only or refraction-only: mirrors, metals, glass) needs no
          // stack and no unwinding at any depth.  The ten doubles live in LDS (lane-major, conflict-free), touched
          // once per bounce.   F o f:  S' = S*a,  O' = O + S*ds,  LO' = clampF(O + S*amb),  HI' = clampF(O + S*max(amb,1))
          // A node with BOTH children (a bubble) is parked with the map accumulated so far, its reflection subtree is
          // traced under a fresh (identity) map, and when that subtree's colour is known the node continues as a
          // one-child node through its refraction ray (main.js:268-278: reflection is evaluated before refraction).
          const uint32_t T = W1 ? 64u : RT_WG_THREADS;
          double A[3], D[3];
#pragma unroll
          for (int c = 0; c < 3; c++) { A[c] = col[c] * a0; D[c] = col[c] * diffuse + col[c] * specular; }
          const bool via_f = REFRACT && !go_r;                          // the only child is the refraction ray
          if (REFRACT && go_r && go_f) {
            park &pk = parked[sp++];
#pragma unroll
            for (int c = 0; c < 3; c++) { pk.amb[c] = A[c]; pk.ds[c] = D[c]; }
            pk.a3 = a3; pk.a4 = a4; pk.h[0] = h.x; pk.h[1] = h.y; pk.h[2] = h.z; pk.f[0] = f.x; pk.f[1] = f.y; pk.f[2] = f.z;
            pk.path = tree_path; pk.segs_left = segs_left; pk.level = level; pk.map_valid = map_valid; pk.hcode = hcode;
            if (map_valid) {
              pk.S = acc[0];
#pragma unroll
              for (int c = 0; c < 3; c++) { pk.O[c] = acc[(1 + c) * T]; pk.LO[c] = acc[(4 + c) * T]; pk.HI[c] = acc[(7 + c) * T]; }
            }
            map_valid = false;
            p = h; d = r; tree_path = 2u * tree_path;
          } else {
            const double coef = via_f ? a4 : a3;
            if (!map_valid) {
              acc[0] = coef;
#pragma unroll
              for (int c = 0; c < 3; c++) { acc[(1 + c) * T] = D[c]; acc[(4 + c) * T] = A[c]; acc[(7 + c) * T] = LEAN ? rt_max1_nn(A[c]) : __builtin_fmax(A[c], 1.0); }
            } else {
              const double S = acc[0];
#pragma unroll
              for (int c = 0; c < 3; c++) {
                const double O = acc[(1 + c) * T], LO = acc[(4 + c) * T], HI = acc[(7 + c) * T];
                if constexpr (LEAN) {
                  // (the same minNum / maxNum without a canonicalising v_max_f64 x, x in front of each value read from LDS: they are this
                  // kernel's own results - rt_kernel_math.h)
                  const double l2 = __builtin_fma(S, A[c], O), h2 = __builtin_fma(S, rt_max1_nn(A[c]), O);
                  acc[(1 + c) * T] = __builtin_fma(S, D[c], O);
                  acc[(4 + c) * T] = rt_max_nn(LO, rt_min_nn(HI, l2));
                  acc[(7 + c) * T] = rt_max_nn(LO, rt_min_nn(HI, h2));
                } else {
                const double l2 = __builtin_fma(S, A[c], O), h2 = __builtin_fma(S, __builtin_fmax(A[c], 1.0), O);
                acc[(1 + c) * T] = __builtin_fma(S, D[c], O);
                acc[(4 + c) * T] = __builtin_fmax(LO, __builtin_fmin(HI, l2));
                acc[(7 + c) * T] = __builtin_fmax(LO, __builtin_fmin(HI, h2));
                }
              }
              acc[0] = S * coef;
            }
            if constexpr (!WAVE_NODE) map_valid = true;                 // (WAVE_NODE: "not the primary node", set at the turn's top)
            p = h; d = via_f ? f : r; tree_path = 2u * tree_path + (via_f ? 1u : 0u);
          }
          level++; segs_left--;
          descend = true;
        } else {
          frame<REFRACT> &fr = stack[level];
#pragma unroll
          for (int c = 0; c < 3; c++) { fr.amb[c] = col[c] * a0; fr.ds[c] = col[c] * diffuse + col[c] * specular; }
          fr.a3 = a3;
          if constexpr (REFRACT) {
            fr.a4 = a4; fr.h[0] = h.x; fr.h[1] = h.y; fr.h[2] = h.z; fr.f[0] = f.x; fr.f[1] = f.y; fr.f[2] = f.z;
            fr.re[0] = fr.re[1] = fr.re[2] = 0.0;
            fr.has_f = go_f; fr.phase = go_r ? 0 : 1;
          }
          p = h; d = go_r ? r : f;
          tree_path = 2u * tree_path + (go_r ? 0u : 1u);
          level++; segs_left--;
          descend = true;
        }
      }
      if (descend) continue;

      // (SIX_WAVES: the lane's colour is folded - RT_CHAIN_END, in the branch that ended its chain; it leaves)
      if constexpr (SIX_WAVES) break;
      else if constexpr (FOLD_FORWARD) {
        // a chain of one-child nodes ended with colour `ret`: apply the accumulated map once
        const uint32_t T = W1 ? 64u : RT_WG_THREADS;
        if (map_valid) {
          const double S = acc[0];
#pragma unroll
          for (int c = 0; c < 3; c++) {
            if constexpr (LEAN) ret[c] = rt_max_nn(acc[(4 + c) * T], rt_min_nn(acc[(7 + c) * T], __builtin_fma(S, ret[c], acc[(1 + c) * T])));
            else ret[c] = __builtin_fmax(acc[(4 + c) * T], __builtin_fmin(acc[(7 + c) * T], __builtin_fma(S, ret[c], acc[(1 + c) * T])));
          }
        }
        bool resumed = false;
        if constexpr (REFRACT) {
          if (sp > 0) {
            // `ret` is the colour of a parked node's reflection child: fold it into the node's constant term, put the
            // map that was accumulated above the node back, and go on through the node's refraction ray
            const park &pk = parked[--sp];
            const double coef = pk.a4;
            if (!pk.map_valid) {
              acc[0] = coef;
#pragma unroll
              for (int c = 0; c < 3; c++) {
                acc[(1 + c) * T] = pk.ds[c] + ret[c] * pk.a3; acc[(4 + c) * T] = pk.amb[c]; acc[(7 + c) * T] = __builtin_fmax(pk.amb[c], 1.0);
              }
            } else {
              const double S = pk.S;
#pragma unroll
              for (int c = 0; c < 3; c++) {
                const double Dn = pk.ds[c] + ret[c] * pk.a3;
                const double l2 = __builtin_fma(S, pk.amb[c], pk.O[c]), h2 = __builtin_fma(S, __builtin_fmax(pk.amb[c], 1.0), pk.O[c]);
                acc[(1 + c) * T] = __builtin_fma(S, Dn, pk.O[c]);
                acc[(4 + c) * T] = __builtin_fmax(pk.LO[c], __builtin_fmin(pk.HI[c], l2));
                acc[(7 + c) * T] = __builtin_fmax(pk.LO[c], __builtin_fmin(pk.HI[c], h2));
              }
              acc[0] = S * coef;
            }
            map_valid = true;
            p = mk(pk.h[0], pk.h[1], pk.h[2]); d = mk(pk.f[0], pk.f[1], pk.f[2]);
            tree_path = 2u * pk.path + 1u; segs_left = pk.segs_left - 1u; level = pk.level + 1;
            hcode = pk.hcode;                          // the refraction ray starts on the parked node's sphere (bounce table)

            resumed = true;
          }
        }
        if (!resumed) break;
      } else {
        // ---------------- return `ret` to the parents (post-order fold, main.js:268-278, :326-336) ----------------
        bool resumed = false;
        while (level > 0) {
          level--; segs_left++; tree_path >>= 1;
          frame<REFRACT> &fr = stack[level];
          if constexpr (REFRACT) {
            if (fr.phase == 0) {
              fr.re[0] = ret[0] * fr.a3; fr.re[1] = ret[1] * fr.a3; fr.re[2] = ret[2] * fr.a3;
              if (fr.has_f) {                            // now the refraction child of the same node
                fr.phase = 1;
                p = mk(fr.h[0], fr.h[1], fr.h[2]); d = mk(fr.f[0], fr.f[1], fr.f[2]);
                tree_path = 2u * tree_path + 1u;
                level++; segs_left--;
                resumed = true;
                break;
              }
#pragma unroll
              for (int c = 0; c < 3; c++) ret[c] = maxa(fr.amb[c], min1(fr.ds[c] + fr.re[c]));
            } else {
#pragma unroll
              for (int c = 0; c < 3; c++) ret[c] = maxa(fr.amb[c], min1(fr.ds[c] + fr.re[c] + ret[c] * fr.a4));
            }
          } else {
#pragma unroll
            for (int c = 0; c < 3; c++) ret[c] = maxa(fr.amb[c], min1(fr.ds[c] + ret[c] * fr.a3));
          }
        }
        if (!resumed) break;
      }
    }
  }
  rgb[0] = ret[0]; rgb[1] = ret[1]; rgb[2] = ret[2];
  return true;
}

#undef RT_Q_GET
#undef RT_Q_OF
#undef RT_ROOT
#undef RT_CAND
#undef RT_GENERIC
#undef RT_ANCHORED_DISC
#undef RT_ANCHORED
#undef RT_XY_INDEX
#undef RT_SDISC
#undef RT_SROOTS
#undef RT_SHADOW
#undef RT_SHADOW_U
#undef RT_CHAIN_END
