// leaf_box_check.cpp -- the leaf's own box of the pooled records on the CPU (lane_core.h: leaf_box_eps).  Not a product
// path, not the oracle.  In the CPU test suite (tests/test_leaf_box_cpu.py).
//
//   build/leaf_box_check frame <rgbbox | irreg | spheres.f32> <cam.f32 | -> <h> <w> [max_depth = 50] [scale = 1]
// Every pixel's bounce chain is walked over the product's own records (rt::make_trav_layout + rt::fill_leaf_boxes: what the kernels read)
// with lane_core.h's arithmetic, once UNFILTERED (a leaf child of a passing node is tested: the reference's set) and once FILTERED (tested
// only if box_hit passes on its slot).  Printed: the scene's constants and the host's decisions (`ok`, `camera`), sphere tests of both walks
// for full chains and for chains cut by the dark stop, the accepted roots the filter dropped along the unfiltered chains (`lost`) and the
// pixels that differ.  `scale` multiplies eps: 0 is the plain box fl(p -+ r), a negative value a SHRUNK box -- the mutants that must be found.
//
//   build/leaf_box_check hammer <cases> <seed> [scale = 1]
// The claim itself, against __float128: random and adversarial (ray, sphere) pairs inside synthetic scenes that pass leaf_box_finish -- rays
// aimed within 1e-9 .. 1e-1 radii of a silhouette, from the farthest admitted origin, axis-parallel, with zero components, with the origin ON a
// slab of the widened box.  For every accepted root: box_hit and box_hit_presorted on the widened box (`violations`: either fails), and the
// distance of P = o + g d OUTSIDE the sphere against rho / 2 in __float128 (`e1_out`: exceeded; `worst`: the largest ratio seen).
// Exit 0 unless the input cannot be read.
#include <quadmath.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
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

// v_cvt_i32_f32: NaN -> 0, out of range -> the nearest end
int32_t device_f2i(float v) {
  if (v != v) return 0;
  if (v >= 2147483648.0f) return INT32_MAX;
  if (v <= -2147483648.0f) return INT32_MIN;
  return static_cast<int32_t>(v);
}
int32_t device_pack(float r, float g, float b) {
  const uint32_t ir = static_cast<uint32_t>(device_f2i(255.99f * r)), ig = static_cast<uint32_t>(device_f2i(255.99f * g)),
                 ib = static_cast<uint32_t>(device_f2i(255.99f * b));
  return static_cast<int32_t>((ir << 16) | (ig << 8) | ib);
}

bool presorted_hit(const Ray &r, const float *lo, const float *hi) {
  const bool nx = r.ix < 0.0f, ny = r.iy < 0.0f, nz = r.iz < 0.0f;
  return box_hit_presorted(r, nx ? hi[0] : lo[0], nx ? lo[0] : hi[0], ny ? hi[1] : lo[1], ny ? lo[1] : hi[1], nz ? hi[2] : lo[2],
                           nz ? lo[2] : hi[2], 0.0f, kTMax);
}

struct Fold {
  float best = kTMax;
  int bestj = -1;
  unsigned long long spheres = 0, lost = 0;
};

// One fold over the 64-byte records: a box item is an inner node whose own box passed; `filter`: a leaf child is tested only if its slot passes.
// lost: accepted roots among the leaves the slot would drop (counted in the unfiltered walk).
Fold fold(const rt::TravLayout &t, const Ray &r, bool filter, std::vector<int32_t> &stack) {
  Fold f;
  if (!box_hit(r, t.root_lo[0], t.root_lo[1], t.root_lo[2], t.root_hi[0], t.root_hi[1], t.root_hi[2])) return f;
  stack.clear();
  stack.push_back(0);
  while (!stack.empty()) {
    const float *q = &t.nodes64[16 * static_cast<size_t>(stack.back())];
    stack.pop_back();
    for (int k = 0; k < 2; ++k) {
      int32_t ref8;
      std::memcpy(&ref8, &q[3 + 4 * k], 4);
      const bool hit = box_hit(r, q[8 * k], q[8 * k + 1], q[8 * k + 2], q[8 * k + 4], q[8 * k + 5], q[8 * k + 6]);
      if (ref8 >= 0) {
        if (hit) stack.push_back(ref8 >> 8);
        continue;
      }
      if (filter && !hit) continue;
      const int32_t j = ~(ref8 >> 8);
      const float *s = &t.sph[4 * static_cast<size_t>(j)];
      const float g = sphere_root(r, s[0], s[1], s[2], s[3]);
      ++f.spheres;
      if (!filter && !hit && g < kTMax) ++f.lost;
      closest_update(g, j, f.best, f.bestj);
    }
  }
  return f;
}

struct Chain {
  int32_t pixel = 0, pixel_stop = 0;
  unsigned long long spheres = 0, spheres_stop = 0, lost = 0;
};

Chain chain(const rt::TravLayout &t, const Cam &cam, int col, int row, int w, int h, int max_depth, bool filter, std::vector<int32_t> &stack) {
  Chain c;
  Ray r = primary_ray(cam, col, row, w, h);
  float lr = 1.0f, lg = 1.0f, lb = 1.0f;
  int depth = 0;
  bool stopped = false;
  for (;;) {
    const Fold f = fold(t, r, filter, stack);
    c.spheres += f.spheres;
    c.lost += f.lost;
    if (!stopped) c.spheres_stop += f.spheres;
    float sp[4] = {0.0f, 0.0f, 0.0f, 1.0f}, cl[3] = {0.0f, 0.0f, 0.0f};
    if (f.bestj >= 0) {
      std::memcpy(sp, &t.sph[4 * static_cast<size_t>(f.bestj)], 16);
      std::memcpy(cl, &t.col[4 * static_cast<size_t>(f.bestj)], 12);
    }
    const bool more = finish_ray_emit(r, f.best, f.bestj, sp[0], sp[1], sp[2], sp[3], cl[0], cl[1], cl[2], 1.0f / sp[3], lr, lg, lb, depth, max_depth,
                                      [&](float cr, float cg, float cb) { c.pixel = device_pack(cr, cg, cb); });
    if (!more) break;
    if (!stopped && light_is_dead(lr, lg, lb)) stopped = true;
  }
  c.pixel_stop = stopped ? 0 : c.pixel;
  return c;
}

int frame_main(int argc, char **argv) {
  if (argc < 6) return 2;
  const std::string what = argv[2];
  const int h = std::atoi(argv[4]), w = std::atoi(argv[5]);
  const int max_depth = argc > 6 ? std::atoi(argv[6]) : 50;
  const double scale = argc > 7 ? std::atof(argv[7]) : 1.0;
  if (h <= 0 || w <= 0 || max_depth < 1) return 2;
  rt::SceneDesc sc;
  const bool named = what == "rgbbox" || what == "irreg";
  if (what == "rgbbox") sc = rt::make_rgbbox();
  else if (what == "irreg") sc = rt::make_floor(100, 600.0f);
  else {
    const std::vector<float> sf = read_floats(argv[2]);
    if (sf.size() < 14 || sf.size() % 7 != 0) {
      std::fprintf(stderr, "leaf_box_check: cannot read %s as n x 7 floats, n >= 2\n", argv[2]);
      return 2;
    }
    sc.spheres.resize(sf.size() / 7);
    std::memcpy(sc.spheres.data(), sf.data(), sf.size() * sizeof(float));
  }
  Cam cam;
  if (std::strcmp(argv[3], "-") == 0) {
    if (!named) return 2;
    const rt::Camera c = rt::scene_camera(sc, h, w);
    std::memcpy(&cam, &c, sizeof cam);
  } else {
    const std::vector<float> cf = read_floats(argv[3]);
    if (cf.size() != 12) {
      std::fprintf(stderr, "leaf_box_check: cannot read %s as 12 floats\n", argv[3]);
      return 2;
    }
    std::memcpy(&cam, cf.data(), sizeof cam);
  }
  const rt::Lbvh bvh = rt::build_lbvh(sc.spheres);
  rt::TravLayout plain = rt::make_trav_layout(bvh, 1), boxed = plain;
  const rt::LeafBoxConst k = rt::leaf_box_finish(rt::cull_stats(sc.spheres.data(), sc.spheres.size()), sc.spheres.size());
  const bool cam_ok = rt::leaf_box_camera_ok(k, &cam.ox);
  rt::LeafBoxConst ks = k;   // the mutant's constants (scale 1: the product's)
  ks.q = static_cast<float>(k.q * scale); ks.lin = static_cast<float>(k.lin * scale); ks.abs = static_cast<float>(k.abs * scale);
  if (scale == 0.0) ks.ok = true;   // the plain box needs no guard to be written down
  rt::fill_leaf_boxes(boxed, ks);
  unsigned long long spheres = 0, spheres_stop = 0, filt = 0, filt_stop = 0, lost = 0, differ = 0, differ_stop = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : spheres, spheres_stop, filt, filt_stop, lost, differ, differ_stop)
  for (int row = 0; row < h; ++row) {
    std::vector<int32_t> stack;
    for (int col = 0; col < w; ++col) {
      // (a scene that fails the guards keeps zeroed slots and is never filtered: its second walk is the first)
      const Chain a = chain(boxed, cam, col, row, w, h, max_depth, false, stack), b = chain(boxed, cam, col, row, w, h, max_depth, ks.ok, stack);
      spheres += a.spheres; spheres_stop += a.spheres_stop; lost += a.lost;
      filt += b.spheres; filt_stop += b.spheres_stop;
      differ += a.pixel != b.pixel;
      differ_stop += a.pixel_stop != b.pixel_stop;
    }
  }
  if (!ks.ok) lost = 0;   // (zeroed slots say nothing about roots)
  float r_lo = INFINITY, r_hi = 0.0f;
  for (const rt::Sphere &s : sc.spheres) { r_lo = std::fmin(r_lo, s.radius); r_hi = std::fmax(r_hi, s.radius); }
  std::printf("scene=%s n=%zu h=%d w=%d max_depth=%d scale=%g ok=%d camera=%d d_eps=%.9g q=%.9g lin=%.9g abs=%.9g eps_rmin=%.9g eps_rmax=%.9g "
              "spheres=%llu spheres_stop=%llu filtered=%llu filtered_stop=%llu lost=%llu differ=%llu differ_stop=%llu\n",
              named ? what.c_str() : "file", sc.spheres.size(), h, w, max_depth, scale, k.ok ? 1 : 0, cam_ok ? 1 : 0, k.d_eps, k.q, k.lin, k.abs,
              k.ok ? leaf_box_eps(r_lo, k.q, k.lin, k.abs) : 0.0f, k.ok ? leaf_box_eps(r_hi, k.q, k.lin, k.abs) : 0.0f, spheres, spheres_stop, filt,
              filt_stop, lost, differ, differ_stop);
  return 0;
}

// ---- hammer ----
typedef __float128 f128;

int hammer_main(int argc, char **argv) {
  if (argc < 4) return 2;
  const long long cases = std::atoll(argv[2]);
  const unsigned seed = static_cast<unsigned>(std::atoll(argv[3]));
  const double scale = argc > 4 ? std::atof(argv[4]) : 1.0;
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  auto logu = [&](double lo, double hi) { return lo * std::pow(hi / lo, U(rng)); };
  auto unit = [&](double v[3]) {
    double n;
    do {
      for (int a = 0; a < 3; ++a) v[a] = 2.0 * U(rng) - 1.0;
      n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    } while (n < 1e-3 || n > 1.0);
    for (int a = 0; a < 3; ++a) v[a] /= n;
  };
  unsigned long long roots = 0, violations = 0, e1_out = 0, scenes = 0, rejected = 0;
  double worst = 0.0;
  long long done = 0;
  while (done < cases) {
    // a synthetic scene: the statistics alone (a box of centres around `mid`, radii r_min .. r_max), as large as the guards admit or smaller
    rt::CullStats st;
    const double r_min = logu(0x1p-20, 64.0), r_max = r_min * logu(1.0, 64.0);
    const double half = r_min * logu(0.5, 80.0);   // half edge of the centres' box: R = sqrt(3) half
    double mid[3];
    for (int a = 0; a < 3; ++a) {
      mid[a] = (2.0 * U(rng) - 1.0) * r_min * logu(1.0, 1000.0);
      st.lo[a] = static_cast<float>(mid[a] - half);
      st.hi[a] = static_cast<float>(mid[a] + half);
    }
    st.r_min = static_cast<float>(r_min); st.r_max = static_cast<float>(r_max);
    for (int a = 0; a < 3; ++a) st.c_max = std::max(st.c_max, std::max(std::fabs(st.lo[a]), std::fabs(st.hi[a])) + st.r_max);
    const rt::LeafBoxConst k = rt::leaf_box_finish(st, 2);
    if (!k.ok) { ++rejected; if (rejected > 100 * (scenes + 100)) break; continue; }
    ++scenes;
    const float q = static_cast<float>(k.q * scale), lin = static_cast<float>(k.lin * scale), abs = static_cast<float>(k.abs * scale);
    for (int i = 0; i < 4096 && done < cases; ++i, ++done) {
      // the sphere: a centre in the box (often a corner), a radius in the range (often an end)
      float p[3];
      for (int a = 0; a < 3; ++a) {
        const double t = U(rng) < 0.4 ? (U(rng) < 0.5 ? 0.0 : 1.0) : U(rng);
        p[a] = static_cast<float>(st.lo[a] + t * (st.hi[a] - st.lo[a]));
      }
      const double pick = U(rng);
      const float rad = static_cast<float>(pick < 0.35 ? st.r_min : pick < 0.5 ? st.r_max : logu(st.r_min, st.r_max));
      float lo[3], hi[3];
      leaf_box_bounds(p[0], p[1], p[2], rad, q, lin, abs, lo, hi);
      // the origin: as far as a camera may be (cam_max from the centre, often opposite the sphere), or on another sphere of the scene
      double o[3], dir[3];
      const int kind = static_cast<int>(U(rng) * 6.0);
      unit(dir);
      if (kind == 0 || kind == 3) {
        double away[3] = {k.centre[0] - p[0], k.centre[1] - p[1], k.centre[2] - p[2]};
        const double n = std::sqrt(away[0] * away[0] + away[1] * away[1] + away[2] * away[2]);
        if (n > 0.0 && U(rng) < 0.7) for (int a = 0; a < 3; ++a) dir[a] = away[a] / n;
        const double dist = k.cam_max * (1.0 - 0x1p-18) * (U(rng) < 0.7 ? 1.0 : U(rng));
        for (int a = 0; a < 3; ++a) o[a] = k.centre[a] + dist * dir[a];
      } else {
        for (int a = 0; a < 3; ++a) o[a] = st.lo[a] + (U(rng) < 0.5 ? (U(rng) < 0.5 ? 0.0 : 1.0) : U(rng)) * (st.hi[a] - st.lo[a]) + dir[a] * st.r_max * (1.0 + 0.2 * U(rng));
      }
      Ray r;
      r.ox = static_cast<float>(o[0]); r.oy = static_cast<float>(o[1]); r.oz = static_cast<float>(o[2]);
      // the direction: at a point of the silhouette, off by a few ulps .. a tenth of the radius either way
      double side[3];
      unit(side);
      const double to[3] = {p[0] - (double)r.ox, p[1] - (double)r.oy, p[2] - (double)r.oz};
      const double tn = std::sqrt(to[0] * to[0] + to[1] * to[1] + to[2] * to[2]);
      if (tn > 0.0) {
        const double dp = (side[0] * to[0] + side[1] * to[1] + side[2] * to[2]) / (tn * tn);
        for (int a = 0; a < 3; ++a) side[a] -= dp * to[a];
        const double sn = std::sqrt(side[0] * side[0] + side[1] * side[1] + side[2] * side[2]);
        if (sn > 1e-6) for (int a = 0; a < 3; ++a) side[a] /= sn;
      }
      const double off = U(rng) < 0.15 ? U(rng) : 1.0 + (U(rng) < 0.5 ? -1.0 : 1.0) * logu(1e-9, 1e-1);
      const double len = kind >= 3 ? logu(0x1p-11, 0x1p18) : logu(0.7, 1.3);   // sqrt of d.d in 2^-22 .. 2^36, or a bounce ray's
      double d[3];
      for (int a = 0; a < 3; ++a) d[a] = to[a] + off * rad * side[a];
      if (kind == 2 || kind == 5) {
        // axis-parallel: one or two zero components; the origin moved so that the line still grazes the sphere, sometimes ONTO a slab of the box
        const int ax = static_cast<int>(U(rng) * 3.0) % 3, bx = (ax + 1) % 3, cx = (ax + 2) % 3;
        const bool two = U(rng) < 0.5;
        d[bx] = 0.0;
        if (two) d[cx] = 0.0;
        const double ang = 6.283185307179586 * U(rng);
        const float ob = U(rng) < 0.3 ? (U(rng) < 0.5 ? lo[bx] : hi[bx]) : static_cast<float>(p[bx] + off * rad * std::cos(ang));
        (bx == 0 ? r.ox : bx == 1 ? r.oy : r.oz) = ob;
        if (two) (cx == 0 ? r.ox : cx == 1 ? r.oy : r.oz) = U(rng) < 0.3 ? (U(rng) < 0.5 ? lo[cx] : hi[cx]) : static_cast<float>(p[cx] + off * rad * std::sin(ang));
        if (d[ax] == 0.0) d[ax] = 1.0;
      }
      const double dn = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      if (!(dn > 0.0)) continue;
      r.dx = static_cast<float>(d[0] / dn * len); r.dy = static_cast<float>(d[1] / dn * len); r.dz = static_cast<float>(d[2] / dn * len);
      ray_derive(r);
      // (the guards' side: the distance to the sphere within D_eps -- moved origins of the axis-parallel cases may leave it)
      const f128 ocx = (f128)r.ox - p[0], ocy = (f128)r.oy - p[1], ocz = (f128)r.oz - p[2];
      const f128 D2 = ocx * ocx + ocy * ocy + ocz * ocz;
      if (D2 > (f128)k.d_eps * k.d_eps) continue;
      const float g = sphere_root(r, p[0], p[1], p[2], rad);
      if (!(g < kTMax)) continue;
      ++roots;
      if (!box_hit(r, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]) || !presorted_hit(r, lo, hi)) ++violations;
      const f128 Px = ocx + (f128)g * r.dx, Py = ocy + (f128)g * r.dy, Pz = ocz + (f128)g * r.dz;
      const f128 out = sqrtq(Px * Px + Py * Py + Pz * Pz) - rad;
      const f128 half_rho = 0x1p-19 * (D2 / rad + rad);
      const double ratio = static_cast<double>(out / half_rho);
      if (ratio > worst) worst = ratio;
      if (ratio > 1.0) ++e1_out;
    }
  }
  std::printf("hammer cases=%lld seed=%u scale=%g scenes=%llu roots=%llu violations=%llu e1_out=%llu worst=%.4f\n", done, seed, scale, scenes, roots,
              violations, e1_out, worst);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  int rc = 2;
  if (argc > 1 && std::strcmp(argv[1], "frame") == 0) rc = frame_main(argc, argv);
  else if (argc > 1 && std::strcmp(argv[1], "hammer") == 0) rc = hammer_main(argc, argv);
  if (rc == 2)
    std::fprintf(stderr, "usage: leaf_box_check frame <rgbbox | irreg | spheres.f32> <cam.f32 | -> <h> <w> [max_depth] [scale]\n"
                         "       leaf_box_check hammer <cases> <seed> [scale]\n");
  return rc;
}
