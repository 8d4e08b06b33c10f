// literal_check - csrc/rt_literal.h on a CPU: tests/test_literal.py builds this with the host compiler and -ffp-contract=off, writes the
// input file, and compares the output file bit for bit with the C restatement's probe records and the Python restatement of the scan.
//   literal_check <in> <out>
// in:  blocks until the end of the file, each { uint32 n_spheres, n_queries; double eps; n_spheres x {ox, oy, oz, r2, albedo[4]};
//      n_queries x {ray[6], length, intensity, int64 skip}; n_queries x uint32 order }
// out: per block n_queries x { rt_hit (80 bytes); double intensity; int32 blocker, 0; double jsmin(length, intensity), jsmax(...) },
//      query j's at place j.  Work-item `item` takes query order[item], as the list kernels do; a place no entry names keeps 0x5A bytes.
// Every exit of the sphere test and of the scan step is counted; the run fails if one that can be taken was not.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rt_hip.h"

// rt_literal.h numbers its exits: 0-6 the sphere test, 7-9 the scan step
enum { EXITS = 10, EXIT_EQ_SWAPPED = 5 };
static unsigned long long g_exits[EXITS];
#define RT_LIT_EXIT(k) (g_exits[k]++)
#include "rt_literal.h"

struct query { double ray[6], length, intensity; long long skip; };
struct result { rt_hit hit; double intensity; int32_t blocker, zero; double lo, hi; };
static_assert(sizeof(query) == 72 && sizeof(rt_hit) == 80 && sizeof(result) == 112, "the file's records");

static bool read_all(FILE *f, void *p, size_t n) { return n == 0 || fread(p, n, 1, f) == 1; }

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
  unsigned long long skipped_spheres = 0, skipped_entries = 0, not_finite = 0;
  uint32_t head[2];
  while (fread(head, sizeof head, 1, in) == 1) {
    const uint32_t ns = head[0], nq = head[1];
    double eps;
    std::vector<double> table(5u * (size_t)ns);
    std::vector<query> qs(nq);
    std::vector<uint32_t> order(nq);
    if (!read_all(in, &eps, sizeof eps) || !read_all(in, table.data(), table.size() * sizeof(double)) || !read_all(in, qs.data(), nq * sizeof(query)) ||
        !read_all(in, order.data(), nq * sizeof(uint32_t))) { fprintf(stderr, "a short block\n"); return 2; }
    // the ray list as the kernels see it: records of six doubles on a 16-byte boundary
    double *rays = (double *)aligned_alloc(16, ((size_t)nq * 48u + 15u) / 16u * 16u + 16u);
    for (uint32_t j = 0; j < nq; j++) memcpy(rays + 6u * (size_t)j, qs[j].ray, 48);
    std::vector<result> res(nq);
    memset(res.data(), 0x5A, nq * sizeof(result));
    for (uint32_t item = 0; item < nq; item++) {
      uint32_t j;
      if (!lit_ordered(order.data(), item, nq, &j)) { skipped_entries++; continue; }
      const lit_ray R = lit_load_ray(rays, j);
      const query &Q = qs[j];
      result r;
      memset(&r, 0, sizeof r);
      // ---- the closest hit and its record, as rt_hits.hip's rt_ray_hit_kernel
      double ht = __builtin_inf();
      int32_t hi = -1, hin = 0;
      if (R.finite)
        for (uint32_t k = 0; k < ns; k++) {
          const double *g = &table[5u * (size_t)k];
          lit_closest_step((int32_t)k, g[0], g[1], g[2], g[3], R.ox, R.oy, R.oz, R.rx, R.ry, R.rz, eps, &ht, &hi, &hin);
        }
      r.hit.object = hi; r.hit.inside = hin; r.hit.t = ht;
      if (hi >= 0) {
        const double *g = &table[5u * (size_t)hi];
        lit_hit_point(R.ox, R.oy, R.oz, R.rx, R.ry, R.rz, ht, g[0], g[1], g[2], r.hit.point, r.hit.normal);
        lit_hit_uv(r.hit.normal, &r.hit.u, &r.hit.v);
      }
      // ---- the shadow scan, as rt_occlusion.hip's kernel
      double li = Q.intensity;
      r.blocker = -1;
      bool live = R.finite;
      for (uint32_t k = 0; live && k < ns; k++) {
        if ((long long)k == Q.skip) { skipped_spheres++; continue; }
        const double *g = &table[5u * (size_t)k];
        lit_scan_step((int32_t)k, g[0], g[1], g[2], g[3], g[4], R.ox, R.oy, R.oz, R.rx, R.ry, R.rz, eps, Q.length, &li, &r.blocker, &live);
      }
      if (!R.finite) { li = __builtin_nan(""); not_finite++; }
      r.intensity = li;
      r.lo = jsmin(Q.length, Q.intensity); r.hi = jsmax(Q.length, Q.intensity);
      res[j] = r;
    }
    free(rays);
    if (nq && fwrite(res.data(), nq * sizeof(result), 1, out) != 1) { fprintf(stderr, "cannot write\n"); return 2; }
  }
  if (fclose(out) != 0) return 2;
  fclose(in);
  static const char *names[EXITS] = {"miss_wide", "behind", "far", "near", "eq_behind", "eq_swapped", "eq", "scan_beyond", "scan_glass", "scan_opaque"};
  int rc = 0;
  for (int k = 0; k < EXITS; k++) {
    printf("EXIT %s %llu\n", names[k], g_exits[k]);
    // eq_swapped (t1 < eps <= t0 with t0 >= t1) needs thc < 0, which sqrt never returns: no finite or non-finite input takes it
    if (k == EXIT_EQ_SWAPPED ? g_exits[k] != 0 : g_exits[k] == 0) { fprintf(stderr, "exit %s: taken %llu times\n", names[k], g_exits[k]); rc = 1; }
  }
  printf("EXIT scan_skip %llu\nEXIT order_skip %llu\nEXIT not_finite %llu\n", skipped_spheres, skipped_entries, not_finite);
  if (!skipped_spheres || !skipped_entries || !not_finite) { fprintf(stderr, "the skip index, an order entry that names no query or a non-finite ray is missing\n"); rc = 1; }
  return rc;
}
