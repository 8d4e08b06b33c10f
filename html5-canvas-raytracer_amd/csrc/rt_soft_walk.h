// rt_soft_walk.h - intersectWorld(segs, objects, org, dir) (main.js:216-336) of ONE ray per lane, walked depth-first over an explicit
// per-lane stack: the node evaluation, the light loop, the fold and the stack of the soft trace (rt_soft.hip, whose header comment says
// what each step restates), as one device function for the kernels that trace a ray inside a loop of their own.  Callers:
//   rt_soft_trace (rt_soft.hip)       soft_walk<true>: one ray per work-item, the levels lv < L.levels relit with sampled lights
//   rt_gather_kernel (rt_gather.hip)  soft_walk<false>, once per sample of a receiver: the lights where they stand
// RELIT = false compiles the relit branch away: no table read, no sample loop beyond its first turn, no division - what the walk does
// at L.levels == 0, so its colours are rt_soft_trace's at levels 0 bit for bit.
// A .hip unit includes this inside its anonymous namespace BEHIND rt_kernel_math.h with RT_STRICT 1 (v3, dot, unit, reflect, min1,
// rt_sqrt / rt_rcp / rt_pow, star_uniform, to_int32_bit0), and is built without FMA contraction.
// The walk is wave-level code: the outer loop runs while any lane of the wave has a node to evaluate, the sphere, light and sample loops
// are wave-uniform with lanes masked, and a ballot ends a shadow scan.  Every lane of a wave that is still in the kernel must call it
// together (a wave-uniform call site); a lane whose ray is not finite, or a call at depth 0, takes part with nothing to do.
// The stack (RT_SOFT_FRAMES frames of RT_SOFT_FRAME_DOUBLES doubles, indexed by the lane's level) is the function's own array: scratch.
#ifndef RT_SOFT_WALK_H
#define RT_SOFT_WALK_H

#include "rt_soft.h"

typedef const double __attribute__((address_space(4))) *kdouble;        // scalar loads: the address is wave-uniform

static_assert(offsetof(rt_sphere, albedo) == 64 && offsetof(rt_sphere, specular_exponent) == 56, "rt_sphere: albedo[4] is byte 96");
static_assert(RT_SOFT_FRAMES <= 31u, "a frame's state is one bit of a 32-bit word");

// val = the colour of ray R.  pix: the ROOT ray's index in the caller's list (the stars sampler's, at every level); W: the table walk of
// that index (read where RELIT and L.stride != 0 only).  L.rays, L.order, L.rgb, L.rgba, L.n and L.pix_base are the caller's business.
template <bool RELIT>
__device__ __forceinline__ void soft_walk(const rt_soft_launch &L, const lit_ray &R, const uint32_t pix, const amb_walk &W, double val[3]) {
  const double eps = L.epsilon, radius = L.light_radius;
  const uint32_t N = L.n_objects, segs = L.segs;
  const char __attribute__((address_space(4))) *tab = (const char __attribute__((address_space(4))) *)L.objects;
  const kdouble soffs = (kdouble)L.offs;
  const uint32_t mix = lowbias32(L.stars_seed);

  double stk[RT_SOFT_FRAMES][RT_SOFT_FRAME_DOUBLES];                     // indexed by the lane's level: scratch
  uint32_t pend_f = 0u, in_r = 0u;                                       // bit lv: frame lv's refract child is still to come / its reflect child is out
  uint32_t lv = 0u, path = 1u;
  v3 p = mk(R.ox, R.oy, R.oz), d = mk(R.rx, R.ry, R.rz);
  // intersectWorld(0, ...) is [0,0,0] (main.js:221); a ray that is not finite is a miss whose sample is NaN x 3 (rt_nodes_shade)
  val[0] = val[1] = val[2] = R.finite ? 0.0 : __builtin_nan("");
  bool active = R.finite && segs != 0u;

  while (__builtin_amdgcn_ballot_w64(active) != 0) {
    // ---- the closest hit: main.js:220-231, 420-451, every sphere in blob order, strict <, first wins
    const bool fin = lit_finite6(p.x, p.y, p.z, d.x, d.y, d.z);        // (a child ray that is not finite is not traced either: rt_nodes_shade's guard)
    double ht = __builtin_inf();
    int32_t hi = -1, hin = 0;
    for (uint32_t j = 0; j < N; j++) {
      const kdouble g = (kdouble)(tab + (size_t)j * sizeof(rt_sphere));
      const double gx = g[0], gy = g[1], gz = g[2], r2 = g[3];
      if (!active || !fin) continue;
      lit_closest_step((int32_t)j, gx, gy, gz, r2, p.x, p.y, p.z, d.x, d.y, d.z, eps, &ht, &hi, &hin);
    }
    const bool hit = hi >= 0;
    const rt_sphere *sp = L.objects + (hit ? hi : 0);                    // (per lane; a miss reads sphere 0 and uses nothing of it)

    // ---- hit.p, hit.n (main.js:440-445)
    v3 h = mk(0.0, 0.0, 0.0), n = mk(0.0, 0.0, 0.0);
    if (hit) {
      double hp[3], hn[3];
      lit_hit_point(p.x, p.y, p.z, d.x, d.y, d.z, ht, sp->origin[0], sp->origin[1], sp->origin[2], hp, hn);
      h = mk(hp[0], hp[1], hp[2]); n = mk(hn[0], hn[1], hn[2]);
    }
    const v3 l = hin ? mk(-n.x, -n.y, -n.z) : n;                         // hit.l, quirk q5
    const double a0 = hit ? sp->albedo[0] : 0.0, a1 = hit ? sp->albedo[1] : 0.0, a2 = hit ? sp->albedo[2] : 0.0;
    const double a3 = hit ? sp->albedo[3] : 0.0, a4 = hit ? sp->albedo[4] : 0.0;

    // ---- the sampler (main.js:320), as rt_nodes_shade has it; hit.u, hit.v (main.js:446-447) where a texture reads them
    double col[3];
    if (!hit) {
      const double nan = __builtin_nan("");
      col[0] = fin ? L.miss_color[0] : nan; col[1] = fin ? L.miss_color[1] : nan; col[2] = fin ? L.miss_color[2] : nan;
    } else {
      const int kind = sp->sampler_kind;
      if (kind == RT_SAMPLER_TEXTURE) {
        double hn[3] = {n.x, n.y, n.z}, hu, hv;
        lit_hit_uv(hn, &hu, &hv);
        const uint32_t ti = (uint32_t)sp->texture < RT_MAX_TEXTURES ? (uint32_t)sp->texture : 0u;   // memory safety only: the upload checked it
        const rt_texture_desc td = L.textures[ti];
        const double xd = ceil(hu * (double)td.width) - 1.0, yd = ceil(hv * (double)td.height) - 1.0;
        uint32_t xi = (xd > 0.0) ? (uint32_t)xd : 0u, yi = (yd > 0.0) ? (uint32_t)yd : 0u;
        xi = min(xi, td.width - 1u); yi = min(yi, td.height - 1u);       // memory safety only; u,v <= 1
        const uint32_t texel = *(const uint32_t *)(L.texel_base + td.texels_offset + ((size_t)yi * td.width + xi) * 4u);
        col[0] = (double)(texel & 255u) / 255.0; col[1] = (double)((texel >> 8) & 255u) / 255.0; col[2] = (double)((texel >> 16) & 255u) / 255.0;
        if (xd != xd || yd != yd) col[0] = col[1] = col[2] = __builtin_nan("");   // texels[NaN] is undefined in JS
      } else if (kind == RT_SAMPLER_CHECKER) {
        const double u = fd_atan2(-n.y, -n.x) / M_PI / 2.0 + 0.5;         // main.js:127 (its own axes)
        const double v = fd_asin(-n.z) / (M_PI / 2.0) / 2.0 + 0.5;        // main.js:128
        const int c = to_int32_bit0(u * sp->checker_freq[0]) ^ to_int32_bit0(v * sp->checker_freq[1]);
        const double *cc = &sp->checker_color[0][0] + 3 * c;
        col[0] = cc[0]; col[1] = cc[1]; col[2] = cc[2];
      } else if (kind == RT_SAMPLER_STARS) {
        double c = star_uniform(pix, 0u, path, mix);
        c = (c >= sp->checker_freq[0]) ? 0.0 : c * sp->checker_freq[1];   // main.js:137-138
        col[0] = col[1] = col[2] = c;
      } else { col[0] = sp->color[0]; col[1] = sp->color[1]; col[2] = sp->color[2]; }
    }

    // ---- lights and shadow scans (main.js:280-318): rt_relight_kernel's sample loop where the node is relit, rt_nodes_shade's single
    // pass where it is not.  Every lane of the wave walks the loops; `shading` / `part` / `lit` / `live` mask its part
    const bool shading = active && hit && (a1 > 0.0 || a2 > 0.0);
    const bool relit = RELIT && lv < L.levels;
    const double spec_e = sp->specular_exponent;
    const uint32_t trips = RELIT && __builtin_amdgcn_ballot_w64(shading && relit) != 0 ? L.n_samples : 1u;
    double acc_d = 0.0, acc_s = 0.0;
    for (uint32_t s = 0; s < trips; s++) {
      const bool part = shading && (relit || s == 0u);                  // (a node that is not relit: sample 0 only)
      double o[3] = {0.0, 0.0, 0.0};
      if (RELIT && radius != 0.0) {
        if (L.stride == 0u) {                                            // one entry for the whole launch: scalar loads
          const kdouble q = soffs + 3u * (size_t)s;                      // (e = s: s < n_samples <= n_offs)
          o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
        } else if (part && relit) {
          const double *q = L.offs + 3u * (size_t)amb_walk_entry(W, s, L.n_offs);
          o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
        }
      }
      double diffuse = 0.0, specular = 0.0;
      double li = L.light_intensity;                                     // one intensity, carried from light to light (q2)
      for (uint32_t k = 0; k < L.n_lights; k++) {
        const double light[3] = {L.lights[k][0], L.lights[k][1], L.lights[k][2]};   // (the kernel arguments: scalar loads)
        double pos[3];
        lgt_light_pos(light, radius, o, pos);
        if (!relit) { pos[0] = light[0]; pos[1] = light[1]; pos[2] = light[2]; }     // (the shade kernel's light: where it stands)
        const v3 sraw = mk(pos[0] - h.x, pos[1] - h.y, pos[2] - h.z);
        const double lmag = dot(sraw, sraw);
        double llen;
        const v3 sv = unit(sraw, &llen);
        const double sdot = dot(sv, l);
        const bool lit = part && !(sdot <= 0.0);                         // surface faces away (main.js:292)
        bool live = lit && li != 0.0;                                    // (a lane whose intensity is 0 already can gain nothing: shade's rule)
        int32_t blocker;
        for (uint32_t j = 0; j < N; j++) {
          if (__builtin_amdgcn_ballot_w64(live) == 0) break;             // no lane of the wave has a sphere left to meet
          const kdouble g = (kdouble)(tab + (size_t)j * sizeof(rt_sphere));
          const double gx = g[0], gy = g[1], gz = g[2], r2 = g[3];
          const double o4 = g[12];                                       // albedo[4]: byte 96 of the record
          if (!live || (int32_t)j == hi) continue;
          lit_scan_step((int32_t)j, gx, gy, gz, r2, o4, h.x, h.y, h.z, sv.x, sv.y, sv.z, eps, llen, &li, &blocker, &live);
        }
        if (lit && li != 0.0) {
          diffuse += li * sdot / lmag;                                   // main.js:306
          if (a2 > 0.0) {                                                // main.js:307-314
            double ql;
            const v3 q = unit(reflect(mk(-sv.x, -sv.y, -sv.z), l), &ql);
            const double spd = d.x * -q.x + d.y * -q.y + d.z * -q.z;
            if (spd > 0.0) specular += rt_pow(spd, spec_e);
          }
        }
      }
      if (part) {
        const double diffuse_s = min1(diffuse) * a1, specular_s = min1(specular) * a2;   // main.js:316-317, per sample
        acc_d = s == 0u ? diffuse_s : acc_d + diffuse_s;
        acc_s = s == 0u ? specular_s : acc_s + specular_s;
      }
    }
    if (shading && relit) { acc_d = acc_d / (double)L.n_samples; acc_s = acc_s / (double)L.n_samples; }
    if (!shading) { acc_d = 0.0; acc_s = 0.0; }

    if (active) {
      // ---- the two directions (main.js:233-266); below the last level none is followed
      bool ret = true;                                                   // this lane has a colour to hand to its parent
      if (!hit) { val[0] = col[0]; val[1] = col[1]; val[2] = col[2]; }
      else {
        v3 r = mk(0.0, 0.0, 0.0); double rlen = 0.0;
        v3 f = mk(0.0, 0.0, 0.0); double flen = 0.0;
        const bool deeper = lv + 1u < segs;
        if (deeper && a3 > 0.0) r = unit(reflect(d, n), &rlen);
        if (deeper && a4 > 0.0) {
          const double dn = dot(d, n);
          double cosi = -((dn < -1.0) ? -1.0 : min1(dn));                // -Math.max(-1, Math.min(1, dot))
          v3 nn = n; double eta;
          if (cosi < 0.0) { cosi = -cosi; nn = mk(-n.x, -n.y, -n.z); eta = sp->refract_index; }
          else eta = rt_rcp(sp->refract_index);
          const double kk = 1.0 - eta * eta * (1.0 - cosi * cosi);
          if (kk > 0.0) {
            const double q = eta * cosi - rt_sqrt(kk);
            f = mk(d.x * eta + nn.x * q, d.y * eta + nn.y * q, d.z * eta + nn.z * q);
          } else f = reflect(d, nn);                                     // total internal reflection
          f = unit(f, &flen);
        }
        const bool go_r = rlen != 0.0, go_f = flen != 0.0;               // (rt_nodes_shade's children; none below the last level)
        double shade[3], amb[3];
#pragma unroll
        for (int c = 0; c < 3; c++) { shade[c] = col[c] * acc_d + col[c] * acc_s; amb[c] = col[c] * a0; }
        if (go_r || go_f) {
          double *F = stk[lv];                                           // (lv + 1 < segs <= 16: lv < RT_SOFT_FRAMES)
          if (!go_r) { shade[0] = shade[0] + 0.0; shade[1] = shade[1] + 0.0; shade[2] = shade[2] + 0.0; }   // re = 0.0, added all the same
          F[0] = shade[0]; F[1] = shade[1]; F[2] = shade[2]; F[3] = amb[0]; F[4] = amb[1]; F[5] = amb[2];
          F[6] = a3; F[7] = a4; F[8] = h.x; F[9] = h.y; F[10] = h.z; F[11] = f.x; F[12] = f.y; F[13] = f.z;
          const uint32_t bit = 1u << lv;
          if (go_r) { in_r |= bit; if (go_f) pend_f |= bit; d = r; path = 2u * path; }
          else { d = f; path = 2u * path + 1u; }
          p = h;
          lv++;
          ret = false;
        } else {
#pragma unroll
          for (int c = 0; c < 3; c++) val[c] = jsmax(amb[c], jsmin(1.0, shade[c] + 0.0 + 0.0));   // rt_nodes_fold, no child visited
        }
      }
      // ---- back up the tree: the frames whose children are all in are folded; one whose refract child is still to come sends it out
      while (ret && lv != 0u) {
        double *F = stk[lv - 1u];
        const uint32_t bit = 1u << (lv - 1u);
        if (in_r & bit) {
          in_r &= ~bit;
          const double w3 = F[6];
          const double s0 = F[0] + val[0] * w3, s1 = F[1] + val[1] * w3, s2 = F[2] + val[2] * w3;
          if (pend_f & bit) {
            pend_f &= ~bit;
            F[0] = s0; F[1] = s1; F[2] = s2;
            p = mk(F[8], F[9], F[10]); d = mk(F[11], F[12], F[13]);
            path = path + 1u;                                            // 2 parent -> 2 parent + 1
            ret = false;
          } else {
            val[0] = jsmax(F[3], jsmin(1.0, s0 + 0.0)); val[1] = jsmax(F[4], jsmin(1.0, s1 + 0.0)); val[2] = jsmax(F[5], jsmin(1.0, s2 + 0.0));   // rf = 0.0
            lv--; path >>= 1;
          }
        } else {
          const double w4 = F[7];
          val[0] = jsmax(F[3], jsmin(1.0, F[0] + val[0] * w4)); val[1] = jsmax(F[4], jsmin(1.0, F[1] + val[1] * w4));
          val[2] = jsmax(F[5], jsmin(1.0, F[2] + val[2] * w4));
          lv--; path >>= 1;
        }
      }
      if (ret) active = false;                                           // (lv == 0: val is the ray's colour)
    }
  }
}

#endif
