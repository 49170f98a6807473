// cull_guard_check.cpp -- whole renders at the limits of the culling proof's guards, on the CPU (lane_core.h: cull_limit).
// Not a product path, not the oracle.  In the CPU test suite (tests/test_cull_edges_cpu.py writes the cases of tests/edge_cull.py as raw
// float32 files and reads the lines printed here).
//
// tools/cull_bound_check.cpp hammers the proof's two inequalities on single (ray, sphere) pairs with constants of its own; this program takes a
// SCENE and its CAMERAS: the host's decision (rt::cull_scene_constants on the canonical tree's height, rt::cull_origin_ok per camera) and the
// constants c2 / kappa as rt::cull_finish derives them, and then every pixel's whole ray chain (primary ray and every bounce, lane_core.h's
// own arithmetic).  Every ray walks the canonical tree (rt::build_lbvh) twice:
//   * un-culled, as the reference folds: every inner child against the fixed (0, 1e9);
//   * every inner child clamped to cull_limit(best*, cull_weight(r, c2), kappa), best* being the ray's FINAL best root -- no traversal order can
//     know a smaller `best` at any box, so this is the strongest limit any order could apply, and every box any order culls is culled here.
// A different winner (root or leaf) is a violation.  The chain goes on from the un-culled result, so the pixels are the reference's.
//
//   build/cull_guard_check <spheres.f32> <cams.f32> <h> <w> [max_depth = 50] [halve = 0]
// spheres.f32: n x 7 floats {pos.xyz, colour.rgb, radius}; cams.f32: k x 12 floats {origin, llc, horizontal, vertical}.
// halve = 1 replaces the limit by 0.5 * best* (a limit that is plainly wrong): the program must then REPORT violations -- the proof's own
// margin has so much slack on whole scenes that scaling it down is not noticed, so this is what shows that the comparison can fail.
// A launch is culled only where the scene and the camera pass; the clamped walk is played only for such cameras (culled_walk = 1), for the
// others boxes_limit repeats boxes.  Exit 0 unless the files cannot be read.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lane_core.h"
#include "rt_host.hpp"

using namespace rtk;

namespace {

std::vector<float> read_floats(const char *path) {
  std::vector<float> v;
  FILE *f = std::fopen(path, "rb");
  if (!f) return v;
  float buf[4096];
  size_t got;
  while ((got = std::fread(buf, sizeof(float), 4096, f)) > 0) v.insert(v.end(), buf, buf + got);
  std::fclose(f);
  return v;
}

struct Walk {
  float best = kTMax;
  int bestj = -1;
  unsigned long long boxes = 0;
};

// The fold's result over the canonical tree: a leaf is tested iff every ancestor's box passes (the root's against (0, 1e9), as a ray starts;
// every other inner node's against (0, clamp)).  clamp = kTMax is the reference's walk.
Walk walk(const rt::Lbvh &b, const Ray &r, float clamp, std::vector<int32_t> &stack) {
  Walk w;
  w.boxes = 1;
  if (!box_hit(r, b.bmin[0], b.bmin[1], b.bmin[2], b.bmax[0], b.bmax[1], b.bmax[2])) return w;
  stack.clear();
  stack.push_back(0);
  while (!stack.empty()) {
    const int32_t node = stack.back();
    stack.pop_back();
    const int32_t kids[2] = {b.left[static_cast<size_t>(node)], b.right[static_cast<size_t>(node)]};
    for (int k = 0; k < 2; ++k) {
      if (rt::ptr_is_leaf(kids[k])) {
        const int32_t j = rt::ptr_leaf_index(kids[k]);
        const rt::Sphere &s = b.L[static_cast<size_t>(j)];
        closest_update(sphere_root(r, s.px, s.py, s.pz, s.radius), j, w.best, w.bestj);
      } else {
        const float *lo = &b.bmin[3 * static_cast<size_t>(kids[k])], *hi = &b.bmax[3 * static_cast<size_t>(kids[k])];
        ++w.boxes;
        if (box_hit_clamped(r, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], clamp)) stack.push_back(kids[k]);
      }
    }
  }
  return w;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: cull_guard_check <spheres.f32> <cams.f32> <h> <w> [max_depth] [halve]\n");
    return 2;
  }
  const std::vector<float> sf = read_floats(argv[1]), cf = read_floats(argv[2]);
  const int h = std::atoi(argv[3]), w = std::atoi(argv[4]);
  const int max_depth = argc > 5 ? std::atoi(argv[5]) : 50;
  const bool halve = argc > 6 && std::atoi(argv[6]) != 0;
  if (sf.size() < 14 || sf.size() % 7 != 0 || cf.empty() || cf.size() % 12 != 0 || h <= 0 || w <= 0) {
    std::fprintf(stderr, "cull_guard_check: bad input\n");
    return 2;
  }
  std::vector<rt::Sphere> ts(sf.size() / 7);
  std::memcpy(ts.data(), sf.data(), sf.size() * sizeof(float));
  const rt::Lbvh bvh = rt::build_lbvh(ts);
  const rt::TravLayout tl = rt::make_trav_layout(bvh, 1);
  const rt::CullConst cc = rt::cull_scene_constants(ts, tl.height);
  float r_min = INFINITY;
  for (const rt::Sphere &s : ts) r_min = fminf(r_min, s.radius);
  std::printf("scene n=%zu height=%d sweeps=%d ok=%d c2=%a kappa=%a halve=%d\n", ts.size(), tl.height, bvh.sweeps, cc.ok ? 1 : 0,
              static_cast<double>(cc.c2), static_cast<double>(cc.kappa), halve ? 1 : 0);

  std::vector<int32_t> stack;
  const size_t ncam = cf.size() / 12;
  for (size_t ci = 0; ci < ncam; ++ci) {
    Cam cam;
    std::memcpy(&cam, &cf[12 * ci], sizeof cam);
    const bool origin_ok = rt::cull_origin_ok(cc, &cf[12 * ci]);
    const bool play = cc.ok && origin_ok;
    unsigned long long rays = 0, hits = 0, primary_hits = 0, primary_gated = 0, finite_w2 = 0, boxes = 0, boxes_limit = 0, violations = 0;
    unsigned long long rmin_hits = 0;
    int longest = 0;
    uint32_t checksum = 0;
    for (int row = 0; row < h; ++row) {
      for (int col = 0; col < w; ++col) {
        Ray r = primary_ray(cam, col, row, w, h);
        float lr = 1.0f, lg = 1.0f, lb = 1.0f;
        int depth = 0, chain = 0;
        int32_t pixel = 0;
        for (;;) {
          ++rays;
          ++chain;
          const Walk ref = walk(bvh, r, kTMax, stack);
          boxes += ref.boxes;
          const float w2 = cull_weight(r, cc.c2);
          const bool gated = !(w2 < kNoHit);
          if (!gated) ++finite_w2;
          if (chain == 1 && gated) ++primary_gated;
          if (play) {
            const float lim = halve ? 0.5f * ref.best : cull_limit(ref.best, w2, cc.kappa);
            const Walk cut = walk(bvh, r, lim, stack);
            boxes_limit += cut.boxes;
            if (cut.best != ref.best || cut.bestj != ref.bestj) ++violations;
          } else {
            boxes_limit += ref.boxes;
          }
          float sp[4] = {0.0f, 0.0f, 0.0f, 1.0f}, c[3] = {0.0f, 0.0f, 0.0f};
          if (ref.bestj >= 0) {
            const rt::Sphere &s = bvh.L[static_cast<size_t>(ref.bestj)];
            sp[0] = s.px; sp[1] = s.py; sp[2] = s.pz; sp[3] = s.radius;
            c[0] = s.cr; c[1] = s.cg; c[2] = s.cb;
            ++hits;
            if (chain == 1) ++primary_hits;
            if (s.radius == r_min) ++rmin_hits;
          }
          if (!finish_ray(r, ref.best, ref.bestj, sp[0], sp[1], sp[2], sp[3], c[0], c[1], c[2], 1.0f / sp[3], lr, lg, lb, depth, max_depth, &pixel)) break;
        }
        if (chain > longest) longest = chain;
        checksum = checksum * 31u + static_cast<uint32_t>(pixel);
      }
    }
    std::printf("cam %zu origin_ok=%d culled_walk=%d rays=%llu hits=%llu primary_hits=%llu primary_gated=%llu rmin_hits=%llu longest_chain=%d "
                "finite_w2=%llu boxes=%llu boxes_limit=%llu violations=%llu checksum=%08x\n",
                ci, origin_ok ? 1 : 0, play ? 1 : 0, rays, hits, primary_hits, primary_gated, rmin_hits, longest, finite_w2, boxes, boxes_limit,
                violations, checksum);
  }
  return 0;
}
