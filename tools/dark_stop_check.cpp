// dark_stop_check.cpp -- the render path's dark stop on the CPU (lane_core.h: light_is_dead).  Not a product path, not the oracle.
// In the CPU test suite (tests/test_dark_stop_cpu.py).
//
// Every pixel's bounce chain is walked in FULL with lane_core.h's own arithmetic (primary_ray, the fold over the canonical tree of
// rt::build_lbvh with the reference's fixed (0, 1e9) box interval, finish_ray), and the place where the pooled kernel's SHADE would stop it is
// marked: the first scatter after which light_is_dead(lr, lg, lb) holds.  The stopped chain's pixel is 0 by the rule; the full chain's pixel
// is what its last ray leaves.  Printed: rays, box tests and sphere tests of both (counted as the oracle counts them: a box test per inner node
// reached, the root included, a sphere test per leaf child of a node whose box passed), the checksums of both images (c = c * 31 + pixel), the
// pixels that were cut, the pixels that DIFFER, and the longest chain of either.
//
// The float -> int conversion of a packed pixel is the DEVICE's here (NaN -> 0, saturating), not the host compiler's: scenes with infinite or
// NaN colours are part of the argument, and C leaves their conversion undefined.
//
//   build/dark_stop_check <rgbbox | irreg | spheres.f32> <cam.f32 | -> <h> <w> [max_depth = 50] [rule = 0]
// spheres.f32: n x 7 floats {pos.xyz, colour.rgb, radius}; cam.f32: 12 floats {origin, llc, horizontal, vertical} ("-": the named scene's own
// camera for h x w).  rule = 1 states the rule WRONGLY -- any ONE channel zero -- and must be found (differ > 0 wherever a wall of a saturated
// colour is seen against the sky).  Exit 0 unless the input cannot be read.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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
  unsigned long long boxes = 0, spheres = 0;
};

// The reference's fold over the canonical tree: every inner node reached is tested against (0, 1e9), every leaf child of a passing node is tested.
Walk walk(const rt::Lbvh &b, const Ray &r, std::vector<int32_t> &stack) {
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
        ++w.spheres;
        closest_update(sphere_root(r, s.px, s.py, s.pz, s.radius), j, w.best, w.bestj);
      } else {
        const float *lo = &b.bmin[3 * static_cast<size_t>(kids[k])], *hi = &b.bmax[3 * static_cast<size_t>(kids[k])];
        ++w.boxes;
        if (box_hit(r, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2])) stack.push_back(kids[k]);
      }
    }
  }
  return w;
}

// v_cvt_i32_f32: NaN -> 0, out of range -> the nearest end
int32_t device_f2i(float v) {
  if (v != v) return 0;
  if (v >= 2147483648.0f) return INT32_MAX;
  if (v <= -2147483648.0f) return INT32_MIN;
  return static_cast<int32_t>(v);
}
int32_t device_pack(float r, float g, float b) {   // pack_pixel with the device's conversion
  const uint32_t ir = static_cast<uint32_t>(device_f2i(255.99f * r)), ig = static_cast<uint32_t>(device_f2i(255.99f * g)),
                 ib = static_cast<uint32_t>(device_f2i(255.99f * b));
  return static_cast<int32_t>((ir << 16) | (ig << 8) | ib);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: dark_stop_check <rgbbox | irreg | spheres.f32> <cam.f32 | -> <h> <w> [max_depth] [rule]\n");
    return 2;
  }
  const std::string what = argv[1];
  const int h = std::atoi(argv[3]), w = std::atoi(argv[4]);
  const int max_depth = argc > 5 ? std::atoi(argv[5]) : 50;
  const int rule = argc > 6 ? std::atoi(argv[6]) : 0;
  if (h <= 0 || w <= 0 || max_depth < 1) {
    std::fprintf(stderr, "dark_stop_check: bad size or max_depth\n");
    return 2;
  }
  rt::SceneDesc sc;
  const bool named = what == "rgbbox" || what == "irreg";
  if (what == "rgbbox") sc = rt::make_rgbbox();
  else if (what == "irreg") sc = rt::make_floor(100, 600.0f);
  else {
    const std::vector<float> sf = read_floats(argv[1]);
    if (sf.size() < 14 || sf.size() % 7 != 0) {
      std::fprintf(stderr, "dark_stop_check: cannot read %s as n x 7 floats, n >= 2\n", argv[1]);
      return 2;
    }
    sc.spheres.resize(sf.size() / 7);
    std::memcpy(sc.spheres.data(), sf.data(), sf.size() * sizeof(float));
  }
  Cam cam;
  if (std::strcmp(argv[2], "-") == 0) {
    if (!named) {
      std::fprintf(stderr, "dark_stop_check: a scene from a file needs a camera file\n");
      return 2;
    }
    const rt::Camera c = rt::scene_camera(sc, h, w);
    static_assert(sizeof(Cam) == sizeof(rt::Camera), "12 floats each");
    std::memcpy(&cam, &c, sizeof cam);
  } else {
    const std::vector<float> cf = read_floats(argv[2]);
    if (cf.size() != 12) {
      std::fprintf(stderr, "dark_stop_check: cannot read %s as 12 floats\n", argv[2]);
      return 2;
    }
    std::memcpy(&cam, cf.data(), sizeof cam);
  }
  const rt::Lbvh bvh = rt::build_lbvh(sc.spheres);

  std::vector<int32_t> stack;
  unsigned long long rays = 0, boxes = 0, spheres = 0, rays_stop = 0, boxes_stop = 0, spheres_stop = 0, cut = 0, differ = 0, cut_at2 = 0;
  int longest = 0, longest_stop = 0;
  uint32_t checksum = 0, checksum_stop = 0;
  for (int row = 0; row < h; ++row) {
    for (int col = 0; col < w; ++col) {
      Ray r = primary_ray(cam, col, row, w, h);
      float lr = 1.0f, lg = 1.0f, lb = 1.0f;
      int depth = 0, chain = 0, chain_stop = 0;
      int32_t pixel = 0;
      bool stopped = false;
      for (;;) {
        const Walk f = walk(bvh, r, stack);
        ++chain;
        rays++; boxes += f.boxes; spheres += f.spheres;
        if (!stopped) { chain_stop = chain; rays_stop++; boxes_stop += f.boxes; spheres_stop += f.spheres; }
        float sp[4] = {0.0f, 0.0f, 0.0f, 1.0f}, c[3] = {0.0f, 0.0f, 0.0f};
        if (f.bestj >= 0) {
          const rt::Sphere &s = bvh.L[static_cast<size_t>(f.bestj)];
          sp[0] = s.px; sp[1] = s.py; sp[2] = s.pz; sp[3] = s.radius;
          c[0] = s.cr; c[1] = s.cg; c[2] = s.cb;
        }
        const bool more = finish_ray_emit(r, f.best, f.bestj, sp[0], sp[1], sp[2], sp[3], c[0], c[1], c[2], 1.0f / sp[3], lr, lg, lb, depth, max_depth,
                                          [&](float cr, float cg, float cb) { pixel = device_pack(cr, cg, cb); });
        if (!more) break;
        // where SHADE asks: the fold has just scattered, lr, lg, lb hold the new light
        const bool dead = rule == 0 ? light_is_dead(lr, lg, lb) : (lr == 0.0f) | (lg == 0.0f) | (lb == 0.0f);
        if (!stopped && dead) stopped = true;
      }
      const int32_t pixel_stop = stopped ? 0 : pixel;
      if (stopped) {
        ++cut;
        if (chain_stop == 2) ++cut_at2;
      }
      if (pixel_stop != pixel) ++differ;
      if (chain > longest) longest = chain;
      if (chain_stop > longest_stop) longest_stop = chain_stop;
      checksum = checksum * 31u + static_cast<uint32_t>(pixel);
      checksum_stop = checksum_stop * 31u + static_cast<uint32_t>(pixel_stop);
    }
  }
  std::printf("scene=%s n=%zu h=%d w=%d max_depth=%d rule=%d rays=%llu boxes=%llu spheres=%llu checksum=%08x longest=%d "
              "rays_stop=%llu boxes_stop=%llu spheres_stop=%llu checksum_stop=%08x longest_stop=%d cut=%llu cut_at2=%llu differ=%llu\n",
              named ? what.c_str() : "file", sc.spheres.size(), h, w, max_depth, rule, rays, boxes, spheres, checksum, longest, rays_stop, boxes_stop,
              spheres_stop, checksum_stop, longest_stop, cut, cut_at2, differ);
  return 0;
}
