// view_samples_check - csrc/rt_view_samples.h on a CPU: tests/test_view_samples.py builds this with the plain host compiler and
// -ffp-contract=off (the header needs nothing of HIP), writes the cases below, and compares what comes back with the library's
// rt_view_sample_rays bit for bit.
//   view_samples_check <in> <out>
// in:  cases back to back: uint32 model, w, h, first_row, rows, pad; double fov_deg, scale, origin[3], axis_x[3], axis_y[3], axis_z[3],
//      dx, dy, lu, lv, radius, focus; then the sample's panorama tables: 2 w and 2 h doubles
// out: per case rows * w records of six doubles
#include "rt_view_samples.h"

#include <stdio.h>
#include <vector>

struct sample_case { uint32_t model, w, h, first_row, rows, pad; double fov_deg, scale, o[3], ax[3], ay[3], az[3]; rt_view_sample_params s; };

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  sample_case c;
  while (fread(&c, sizeof c, 1, in) == 1) {
    std::vector<double> lon(2u * (size_t)c.w), lat(2u * (size_t)c.h);
    if (fread(lon.data(), sizeof(double), lon.size(), in) != lon.size() || fread(lat.data(), sizeof(double), lat.size(), in) != lat.size()) return 2;
    rt_view_params P = {};
    P.model = c.model; P.w = c.w; P.h = c.h;
    P.proj_w = (double)c.w / 2.0; P.proj_h = (double)c.h / 2.0;
    P.proj_d = rt_view_proj_d(c.fov_deg, P.proj_w);
    P.scale = c.scale;
    for (int k = 0; k < 3; k++) { P.o[k] = c.o[k]; P.ax[k] = c.ax[k]; P.ay[k] = c.ay[k]; P.az[k] = c.az[k]; }
    P.lon = lon.data(); P.lat = lat.data();
    for (uint32_t y = c.first_row; y < c.first_row + c.rows; y++)
      for (uint32_t x = 0; x < c.w; x++) {
        double r[6];
        rt_view_sample_ray(P, c.s, x, y, r);
        if (fwrite(r, sizeof r, 1, out) != 1) return 3;
      }
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 3;
}
