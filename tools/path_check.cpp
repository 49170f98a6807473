// One bounce of a ray path (query_core.h: path_bounce, behind lane_core.h's sphere_root and rehit_full -- what paths_kernel runs when a lane's
// fold has ended on one sphere) on the host, over cases read from a file: the CPU suite holds the numpy restatement (tests/path_ref.py:
// bounce_cases) equal to this arithmetic bit for bit, without a GPU.
// A case is 16 float32: ray origin xyz, direction xyz, sphere centre xyz, colour rgb, radius, light rgb.  The fold of the one sphere is
// closest_update(sphere_root(..)) from (1e9, none); the winner is re-intersected with rehit_full and the bounce taken at `depth` of
// `max_depth` (the same for every case of a run; default 0 of 50).  For each case 20 uint32 are written: the outcome (0 escaped, 1 absorbed,
// 2 truncated, 3 continue), then the bits of hit7 (7 words), the new ray's origin and direction (6), the new light (3) and the colour (3).
// usage: path_check <cases.bin> <out.bin> [depth max_depth]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "query_core.h"

using namespace rtk;

int main(int argc, char **argv) {
  if (argc != 3 && argc != 5) {
    fprintf(stderr, "usage: path_check <cases.bin> <out.bin> [depth max_depth]\n");
    return 2;
  }
  const int depth = argc == 5 ? atoi(argv[3]) : 0, max_depth = argc == 5 ? atoi(argv[4]) : 50;
  FILE *in = fopen(argv[1], "rb");
  if (!in) {
    fprintf(stderr, "path_check: cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<float> cases;
  float row[16];
  while (fread(row, sizeof(float), 16, in) == 16) cases.insert(cases.end(), row, row + 16);
  fclose(in);
  const size_t n = cases.size() / 16;
  std::vector<uint32_t> out(20 * n);
  size_t kinds[4] = {0, 0, 0, 0};
  for (size_t i = 0; i < n; ++i) {
    const float *c = &cases[16 * i];
    Ray r;
    r.ox = c[0]; r.oy = c[1]; r.oz = c[2];
    r.dx = c[3]; r.dy = c[4]; r.dz = c[5];
    ray_derive(r);
    const float rad = c[12], inv_rad = 1.0f / rad;
    float best = kTMax, t = 0.0f;
    int bestj = -1;
    closest_update(sphere_root(r, c[6], c[7], c[8], rad), 0, best, bestj);
    const bool have = bestj >= 0 && rehit_full(r, best, c[6], c[7], c[8], rad, &t);
    float h[7], nl[3], col[3];
    Ray nr;
    const int code = path_bounce(r, have, t, c[6], c[7], c[8], c[9], c[10], c[11], inv_rad, c[13], c[14], c[15], depth, max_depth, h, &nr, nl, col);
    const uint32_t kind = code == kPathContinue ? 3u : static_cast<uint32_t>(code);
    const float vals[19] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], nr.ox, nr.oy, nr.oz, nr.dx, nr.dy, nr.dz, nl[0], nl[1], nl[2],
                            col[0], col[1], col[2]};
    out[20 * i] = kind;
    memcpy(&out[20 * i + 1], vals, sizeof(vals));
    kinds[kind] += 1;
  }
  FILE *o = fopen(argv[2], "wb");
  if (!o || fwrite(out.data(), sizeof(uint32_t), out.size(), o) != out.size()) {
    fprintf(stderr, "path_check: cannot write %s\n", argv[2]);
    return 2;
  }
  fclose(o);
  printf("%zu cases at depth %d of %d: %zu escaped, %zu absorbed, %zu truncated, %zu continue\n", n, depth, max_depth, kinds[0], kinds[1], kinds[2],
         kinds[3]);
  return 0;
}
