// proximity_bound_check.cpp -- CPU check of the box test rt_nearest_spheres prunes with (query_core.h: box_may_hold, proximity_slack;
// DESIGN.md 3.5e).  Not a product path: a hammer for a proof, in the CPU test suite (a short run).
//
// Scenes are built by the product's host builder (rt::build_lbvh: the same boxes the device builder writes, partial top boxes of tall trees
// included).  For every sphere j of a scene and a batch of adversarial points p it computes G = point_gap(p, L[j]) in binary32 and checks:
//   (S)   the safety property: with the threshold T = G (the tightest one under which j is selected, count mode or pruned mode), no node on
//         j's root path that the kernel tests (depth >= height - sweeps) fails box_may_hold(p, box, T) -- else the walk would drop j;
//   (P1)  the gap's own error bound against __float128: |G - g| <= 4.6 u D + u r + 2^-62 (u = 2^-24, D = |p - c|).
// Points: on the surface (a direction rounded to binary32), at the centre, inside, at random distances, far away, at the box corners of
// ancestors; spheres: random, duplicated, radius 0 (point clouds), huge (|c| ~ 1e18) and tiny (~1e-30) coordinates, and "tall" scenes
// (geometric spacing) whose trees are taller than the AABB propagation's sweeps.
//   build/proximity_bound_check [scenes = 300] [seed = 1] [slack_scale = 1] [all_depths = 0]
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
  unsigned long long n_pairs = 0, n_tests = 0, n_s = 0, n_p1 = 0, n_tall = 0, n_selected_inside = 0;
  double worst_p1 = 0.0;
#pragma omp parallel reduction(+ : n_pairs, n_tests, n_s, n_p1, n_tall, n_selected_inside) reduction(max : worst_p1)
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
      for (int j = 0; j < n; ++j) {
        const rt::Sphere &s = b.L[j];
        std::vector<int> path;
        for (int a = leaf_parent[j]; a >= 0; a = b.parent[a]) path.push_back(a);
        for (int q = 0; q < 24; ++q) {
          const int mode = q % 8;
          double dir[3] = {sym(1), sym(1), sym(1)};
          const double dn = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]) + 1e-300;
          double dist = s.radius;                                        // mode 0: on the surface
          if (mode == 1) dist = 0.0;                                     // the centre
          else if (mode == 2) dist = s.radius * U(rng);                  // inside
          else if (mode == 3) dist = s.radius * (1.0 + sym(1e-6));       // just off the surface
          else if (mode == 4) dist = s.radius + std::fabs((double)s.px) * std::exp2(-20.0 * U(rng));   // at a small gap
          else if (mode == 5) dist = (std::fabs((double)s.px) + s.radius + 1e-30) * std::exp2(10.0 * U(rng));   // far
          float p[3];
          for (int k = 0; k < 3; ++k) p[k] = (float)((&s.px)[k] + dist * dir[k] / dn);
          if (mode == 6 && !path.empty()) {                              // a corner of an ancestor's box
            const int a = path[(size_t)(U(rng) * path.size()) % path.size()];
            for (int k = 0; k < 3; ++k) p[k] = U(rng) < 0.5 ? b.bmin[3 * a + k] : b.bmax[3 * a + k];
          }
          if (mode == 7) for (int k = 0; k < 3; ++k) p[k] = (&s.px)[k] + (float)sym(std::fabs((double)s.radius) * 2.0 + 1e-30);
          if (!point_ok(p[0], p[1], p[2])) continue;
          const float G = point_gap(p[0], p[1], p[2], s.px, s.py, s.pz, s.radius);
          if (!(G <= kTMax)) continue;                                   // never selected: nothing to check
          n_pairs++;
          if (G <= 0.0f) n_selected_inside++;
          // (P1) against the exact gap
          const q128 dx = (q128)p[0] - s.px, dy = (q128)p[1] - s.py, dz = (q128)p[2] - s.pz;
          const q128 D = qsqrt_pos(dx * dx + dy * dy + dz * dz);
          const q128 g = D - (q128)s.radius;
          const q128 lim = (q128)0x1p-24 * (4.6 * D + (q128)s.radius) + (q128)0x1p-62;
          const double ratio = (double)(qabs((q128)G - g) / lim);
          worst_p1 = std::max(worst_p1, ratio);
          if (qabs((q128)G - g) > lim) n_p1++;
          // (S) every tested ancestor must admit j under T = G (box_may_hold grows with T: then under every T >= G as well)
          const float pmag = std::max(std::max(std::fabs(p[0]), std::fabs(p[1])), std::fabs(p[2]));
          for (int a : path) {
            if (depth[a] < exact_depth) continue;
            const float *lo = &b.bmin[3 * (size_t)a], *hi = &b.bmax[3 * (size_t)a];
            n_tests++;
            if (!box_may_hold(p[0], p[1], p[2], pmag, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], G, slack_scale)) {
              if (n_s < 3)
#pragma omp critical
                printf("  violation: scene kind %d n %d height %d sweeps %d sphere (%a %a %a r %a) point (%a %a %a) G %a node depth %d\n", kind, n,
                       height, b.sweeps, s.px, s.py, s.pz, s.radius, p[0], p[1], p[2], G, depth[a]);
              n_s++;
            }
          }
        }
      }
    }
  }
  printf("proximity_bound_check: %llu (point, sphere) pairs (%llu at gap <= 0), %llu box tests, %llu tall scenes: P1 violations %llu (worst "
         "|G - g| / bound %.4f), safety violations %llu\n",
         n_pairs, n_selected_inside, n_tests, n_tall, n_p1, worst_p1, n_s);
  return (n_p1 || n_s) ? 1 : 0;
}
