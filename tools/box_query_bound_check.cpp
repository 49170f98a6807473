// box_query_bound_check.cpp -- CPU check of the node test rt_spheres_in_boxes_* prunes with (query_core.h: box_may_meet, box_box_bound,
// proximity_slack with P over the box's six coordinates).  Not a product path: a hammer for a proof, in the CPU test suite
// (a short run).  Modelled on proximity_bound_check.cpp, whose points are this checker's degenerate boxes.
//
// Scenes are built by the product's host builder (rt::build_lbvh: the same boxes the device builder writes, partial top boxes of tall trees
// included).  For every sphere j of a scene and a batch of adversarial query boxes q it computes G = box_gap(q, L[j]) in binary32 and checks:
//   (S)   the safety property: with the margin T = G (the tightest one under which j is selected), no node on j's root path that the kernel
//         tests (depth >= height - sweeps) fails box_may_meet(q, box, T) -- else the walk would drop j;
//   (Q1)  the gap's own error bound against __float128: |G - g| <= 4.6 u D + u r + 2^-62 (u = 2^-24, D = the exact distance from q to c).
// Boxes: degenerate (lo == hi: on the surface, at the centre, inside, far), around the sphere, with one face tangent to it, between two
// spheres, holding the whole scene, zero-volume slabs, with a corner on a corner of an ancestor's box, random ones at small and large
// gaps; spheres: random, duplicated, radius 0, huge (|c| ~ 1e18) and tiny (~1e-30) coordinates, and "tall" scenes (geometric spacing)
// whose trees are taller than the AABB propagation's sweeps.
//   build/box_query_bound_check [scenes = 300] [seed = 1] [slack_scale = 1] [all_depths = 0]
// slack_scale 0 tests without the slack, all_depths 1 also tests the partial boxes near the root of a tall tree: the checker must then FIND
// violations of (S) (the test suite runs it both ways).
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "query_core.h"
#include "rt_host.hpp"

using namespace rtk;
typedef __float128 q128;

static q128 qabs(q128 x) { return x < 0 ? -x : x; }
static q128 qmax(q128 a, q128 b) { return a > b ? a : b; }
static q128 qsqrt_pos(q128 x) {   // Newton on a double start: enough for an error bound at 2^-24 scale
  if (x <= 0) return 0;
  q128 y = (q128)std::sqrt((double)x);
  if (y == 0) y = (q128)1e-300;
  for (int it = 0; it < 4; ++it) y = 0.5 * (y + x / y);
  return y;
}

static std::vector<rt::Sphere> make_scene(std::mt19937_64 &rng, int kind, int n) {
  std::uniform_real_distribution<double> U(0.0, 1.0);
  auto sym = [&](double s) { return (2.0 * U(rng) - 1.0) * s; };
  std::vector<rt::Sphere> s(n);
  const double scale = kind == 3 ? 1e18 : kind == 4 ? 1e-30 : std::exp2(std::floor(sym(20.0)));
  for (int i = 0; i < n; ++i) {
    double c[3] = {sym(scale), sym(scale), sym(scale)};
    double r = scale * (U(rng) < 0.5 ? 0.05 * U(rng) : 0.3 * U(rng));
    if (kind == 1) r = 0.0;                                                  // a point cloud
    if (kind == 2 && i > 0 && U(rng) < 0.5) {                                // duplicates and near-duplicates
      const rt::Sphere &o = s[(size_t)(U(rng) * i)];
      c[0] = o.px; c[1] = o.py; c[2] = o.pz; r = o.radius;
      if (U(rng) < 0.3) c[(int)(U(rng) * 3) % 3] += sym(1e-6 * scale);
    }
    if (kind == 5) {                                                         // geometric spacing: a tall tree
      const double t = std::exp2(-0.7 * i);
      c[0] = scale * t; c[1] = scale * t * 0.5; c[2] = -scale * t;
      r = scale * t * 0.1 * U(rng);
    }
    if (U(rng) < 0.05) r = 0.0;
    s[i] = rt::Sphere{(float)c[0], (float)c[1], (float)c[2], 1.0f, 1.0f, 1.0f, (float)r};
  }
  return s;
}

int main(int argc, char **argv) {
  const int scenes = argc > 1 ? atoi(argv[1]) : 300;
  const unsigned seed = argc > 2 ? (unsigned)atoi(argv[2]) : 1u;
  const float slack_scale = argc > 3 ? (float)atof(argv[3]) : 1.0f;
  const int all_depths = argc > 4 ? atoi(argv[4]) : 0;
  constexpr int kModes = 12;
  unsigned long long n_pairs = 0, n_tests = 0, n_s = 0, n_q1 = 0, n_tall = 0, n_inside = 0, n_degenerate = 0, n_flat = 0;
  double worst_q1 = 0.0;
#pragma omp parallel reduction(+ : n_pairs, n_tests, n_s, n_q1, n_tall, n_inside, n_degenerate, n_flat) reduction(max : worst_q1)
  {
    std::mt19937_64 rng(seed * 7919u + 104729u * (unsigned)omp_get_thread_num());
    std::uniform_real_distribution<double> U(0.0, 1.0);
    auto sym = [&](double s) { return (2.0 * U(rng) - 1.0) * s; };
#pragma omp for schedule(dynamic, 1)
    for (int sc = 0; sc < scenes; ++sc) {
      const int kind = sc % 6;
      const int n = kind == 5 ? 40 + (int)(U(rng) * 60) : 2 + (int)(std::exp2(11.0 * U(rng)));
      const std::vector<rt::Sphere> in = make_scene(rng, kind, n);
      const rt::Lbvh b = rt::build_lbvh(in);
      const int ni = n - 1;
      // depth of every inner node, the tree height (levels of inner nodes), and the first depth whose boxes the kernel tests
      std::vector<int> depth(ni, 0), leaf_parent(n, -1);
      int height = 1;
      std::vector<int> todo{0};
      for (size_t h = 0; h < todo.size(); ++h) {
        const int c = todo[h];
        height = std::max(height, depth[c] + 1);
        for (int kid : {b.left[c], b.right[c]}) {
          if (rt::ptr_is_leaf(kid)) leaf_parent[rt::ptr_leaf_index(kid)] = c;
          else { depth[kid] = depth[c] + 1; todo.push_back(kid); }
        }
      }
      const int exact_depth = all_depths ? 0 : std::max(0, height - b.sweeps);
      if (height > b.sweeps) n_tall++;
      // the scene's extent: the union of the spheres' own boxes, in double (the root's stored box may be partial)
      double slo[3] = {1e300, 1e300, 1e300}, shi[3] = {-1e300, -1e300, -1e300};
      for (const rt::Sphere &s : b.L)
        for (int k = 0; k < 3; ++k) {
          slo[k] = std::min(slo[k], (double)(&s.px)[k] - s.radius);
          shi[k] = std::max(shi[k], (double)(&s.px)[k] + s.radius);
        }
      for (int j = 0; j < n; ++j) {
        const rt::Sphere &s = b.L[j];
        const double c[3] = {s.px, s.py, s.pz}, r = s.radius;
        const double mag = std::fabs(c[0]) + std::fabs(c[1]) + std::fabs(c[2]) + r + 1e-30;
        std::vector<int> path;
        for (int a = leaf_parent[j]; a >= 0; a = b.parent[a]) path.push_back(a);
        for (int qi = 0; qi < 2 * kModes; ++qi) {
          const int mode = qi % kModes;
          double lo[3], hi[3];
          if (mode <= 3) {                                               // degenerate boxes: the point checker's points
            double dir[3] = {sym(1), sym(1), sym(1)};
            const double dn = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]) + 1e-300;
            const double dist = mode == 0 ? r : mode == 1 ? 0.0 : mode == 2 ? r * (1.0 + sym(1e-6)) : r + std::fabs(c[0]) * std::exp2(-20.0 * U(rng));
            for (int k = 0; k < 3; ++k) lo[k] = hi[k] = (double)(float)(c[k] + dist * dir[k] / dn);
          } else if (mode == 4) {                                        // around the sphere
            for (int k = 0; k < 3; ++k) { lo[k] = c[k] - r * (1.0 + U(rng)); hi[k] = c[k] + r * (1.0 + U(rng)); }
          } else if (mode == 5) {                                        // one face tangent to the sphere (as near as float32 allows), the others spanning the centre
            const int ax = (int)(U(rng) * 3) % 3;
            const bool above = U(rng) < 0.5;
            for (int k = 0; k < 3; ++k) { lo[k] = c[k] - mag * U(rng) * 0.1; hi[k] = c[k] + mag * U(rng) * 0.1; }
            if (above) { lo[ax] = (double)(float)(c[ax] + r); hi[ax] = lo[ax] + mag * U(rng); }
            else { hi[ax] = (double)(float)(c[ax] - r); lo[ax] = hi[ax] - mag * U(rng); }
          } else if (mode == 6) {                                        // between this sphere and another: from just off this one towards that one
            const rt::Sphere &o = b.L[(size_t)(U(rng) * n) % n];
            const double oc[3] = {o.px, o.py, o.pz};
            for (int k = 0; k < 3; ++k) {
              const double a = c[k] + (oc[k] - c[k]) * (0.2 + 0.2 * U(rng)), e = c[k] + (oc[k] - c[k]) * (0.6 + 0.2 * U(rng));
              lo[k] = std::min(a, e); hi[k] = std::max(a, e);
            }
          } else if (mode == 7) {                                        // holding the whole scene
            for (int k = 0; k < 3; ++k) { lo[k] = slo[k] - std::fabs(slo[k]) * 1e-3 * U(rng); hi[k] = shi[k] + std::fabs(shi[k]) * 1e-3 * U(rng); }
          } else if (mode == 8) {                                        // a zero-volume slab at a small gap
            const int ax = (int)(U(rng) * 3) % 3;
            for (int k = 0; k < 3; ++k) { lo[k] = c[k] - mag * U(rng); hi[k] = c[k] + mag * U(rng); }
            lo[ax] = hi[ax] = (double)(float)(c[ax] + (U(rng) < 0.5 ? 1.0 : -1.0) * (r + mag * std::exp2(-24.0 * U(rng))));
            if (U(rng) < 0.3) { const int a2 = (ax + 1) % 3; hi[a2] = lo[a2]; }   // ... or a segment
          } else if (mode == 9 && !path.empty()) {                       // outside an ancestor's box, one corner on a corner of it
            const int a = path[(size_t)(U(rng) * path.size()) % path.size()];
            for (int k = 0; k < 3; ++k) {
              const double ext = (std::fabs((double)b.bmax[3 * a + k]) + std::fabs((double)b.bmin[3 * a + k]) + 1e-30) * U(rng);
              if (U(rng) < 0.5) { lo[k] = b.bmax[3 * a + k]; hi[k] = lo[k] + ext; }
              else { hi[k] = b.bmin[3 * a + k]; lo[k] = hi[k] - ext; }
            }
          } else if (mode == 10) {                                       // far away
            const double d = mag * std::exp2(10.0 * U(rng));
            for (int k = 0; k < 3; ++k) { lo[k] = c[k] + sym(d); hi[k] = lo[k] + d * U(rng); }
          } else {                                                       // random, near
            for (int k = 0; k < 3; ++k) { lo[k] = c[k] + sym(2.0 * r + 1e-30); hi[k] = lo[k] + (2.0 * r + mag * 1e-3) * U(rng) * U(rng); }
          }
          QBox q = {(float)lo[0], (float)lo[1], (float)lo[2], (float)hi[0], (float)hi[1], (float)hi[2]};
          if (q.lox > q.hix) std::swap(q.lox, q.hix);
          if (q.loy > q.hiy) std::swap(q.loy, q.hiy);
          if (q.loz > q.hiz) std::swap(q.loz, q.hiz);
          if (!qbox_ok(q)) continue;
          const float G = box_gap(q, s.px, s.py, s.pz, s.radius);
          if (!(G <= kTMax)) continue;                                   // never selected: nothing to check
          n_pairs++;
          if (G <= 0.0f) n_inside++;
          const bool flat = q.lox == q.hix || q.loy == q.hiy || q.loz == q.hiz;
          if (q.lox == q.hix && q.loy == q.hiy && q.loz == q.hiz) n_degenerate++;
          else if (flat) n_flat++;
          // (Q1) against the exact gap
          const q128 ax = qmax(qmax((q128)q.lox - s.px, (q128)s.px - q.hix), 0), ay = qmax(qmax((q128)q.loy - s.py, (q128)s.py - q.hiy), 0),
                     az = qmax(qmax((q128)q.loz - s.pz, (q128)s.pz - q.hiz), 0);
          const q128 D = qsqrt_pos(ax * ax + ay * ay + az * az);
          const q128 g = D - (q128)s.radius;
          const q128 lim = (q128)0x1p-24 * (4.6 * D + (q128)s.radius) + (q128)0x1p-62;
          worst_q1 = std::max(worst_q1, (double)(qabs((q128)G - g) / lim));
          if (qabs((q128)G - g) > lim) n_q1++;
          // (S) every tested ancestor must admit j under T = G (box_may_meet grows with T: then under every T >= G as well)
          const float qmag = box_mag(q.lox, q.loy, q.loz, q.hix, q.hiy, q.hiz);
          for (int a : path) {
            if (depth[a] < exact_depth) continue;
            const float *nlo = &b.bmin[3 * (size_t)a], *nhi = &b.bmax[3 * (size_t)a];
            n_tests++;
            if (!box_may_meet(q, qmag, nlo[0], nlo[1], nlo[2], nhi[0], nhi[1], nhi[2], G, slack_scale)) {
              if (n_s < 3)
#pragma omp critical
                printf("  violation: scene kind %d n %d height %d sweeps %d sphere (%a %a %a r %a) box (%a %a %a)-(%a %a %a) G %a node depth %d\n",
                       kind, n, height, b.sweeps, s.px, s.py, s.pz, s.radius, q.lox, q.loy, q.loz, q.hix, q.hiy, q.hiz, G, depth[a]);
              n_s++;
            }
          }
        }
      }
    }
  }
  printf("box_query_bound_check: %llu (box, sphere) pairs (%llu at gap <= 0, %llu degenerate boxes, %llu flat), %llu box tests, %llu tall scenes: "
         "Q1 violations %llu (worst |G - g| / bound %.4f), safety violations %llu\n",
         n_pairs, n_inside, n_degenerate, n_flat, n_tests, n_tall, n_q1, worst_q1, n_s);
  return (n_q1 || n_s) ? 1 : 0;
}
