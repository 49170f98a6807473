// plane_query_bound_check.cpp -- CPU check of the node test rt_spheres_in_planes_* prunes with (query_core.h: planes_may_meet, plane_slack;
// DESIGN.md 3.5j) and of the gap's error bound.  Not a product path: a hammer for a proof, in the CPU test suite (a short run).  Modelled on
// box_query_bound_check.cpp.
//
// Scenes are built by the product's host builder (rt::build_lbvh: the same boxes the device builder writes, partial top boxes of tall trees
// included).  For every sphere j of a scene and a batch of adversarial plane sets (K = 1 .. 8 planes, normalised by plane_normalise as the
// kernel does) it computes G = plane_gap(planes, L[j]) in binary32 and checks:
//   (S)   the safety property: with the margin T = G (the tightest one under which j is selected), no node on j's root path that the kernel
//         tests (depth >= height - sweeps) fails planes_may_meet(planes, box, T) -- else the walk would drop j;
//   (R1)  the gap's own error bound against __float128 on the exactly normalised planes: |G - g| <= u (8.8 |c| + 5.8 W + r) + 2^-62
//         (u = 2^-24, W = max_k |d_k| / |(a_k, b_k, c_k)|).
// The deciding plane of a set: tangent to the sphere from outside or inside (as near as float32 allows), through its centre, an axis normal
// (with -0.0 components) tangent to it, at a gap of a few ulps, far away, a half-space holding the whole scene, through the most-inside
// vertex of an ancestor's box, with its normal scaled by 2^-39 or 2^39, a slab around the sphere, a frustum with the sphere at its edge;
// the other planes of a set hold the sphere, repeat the deciding one or are random.  Spheres: random, duplicated, radius 0, huge
// (|c| ~ 1e18) and tiny (~1e-30) coordinates, and "tall" scenes (geometric spacing) whose trees are taller than the AABB propagation's sweeps.
//   build/plane_query_bound_check [scenes = 300] [seed = 1] [slack_scale = 1] [all_depths = 0]
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

static std::vector<rt::Sphere> make_scene(std::mt19937_64 &rng, int kind, int n) {   // (box_query_bound_check.cpp's scenes)
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
    if (kind == 5) {                                                         // geometric spacing off the origin: a tall tree
      const double t = std::exp2(-0.7 * i);
      c[0] = scale * (3.0 + t); c[1] = scale * (2.0 + t * 0.5); c[2] = -scale * (3.0 + t);
      r = scale * t * 0.1 * U(rng);
    }
    if (U(rng) < 0.05) r = 0.0;
    s[i] = rt::Sphere{(float)c[0], (float)c[1], (float)c[2], 1.0f, 1.0f, 1.0f, (float)r};
  }
  return s;
}

template <int K>
static void eval_k(const QPlane *p, const rt::Sphere &s, float *G, float *wmag) {
  QPlane a[K];
  for (int k = 0; k < K; ++k) a[k] = p[k];
  *G = plane_gap(a, s.px, s.py, s.pz, s.radius);
  *wmag = planes_wmag(a);
}
template <int K>
static bool meet_k(const QPlane *p, float wmag, const float *lo, const float *hi, float T, float slack_scale) {
  QPlane a[K];
  for (int k = 0; k < K; ++k) a[k] = p[k];
  return planes_may_meet(a, wmag, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], T, slack_scale);
}
#define BY_K(K, call)            \
  switch (K) {                   \
    case 1: call(1); break;      \
    case 2: call(2); break;      \
    case 3: call(3); break;      \
    case 4: call(4); break;      \
    case 5: call(5); break;      \
    case 6: call(6); break;      \
    case 7: call(7); break;      \
    default: call(8); break;     \
  }

int main(int argc, char **argv) {
  const int scenes = argc > 1 ? atoi(argv[1]) : 300;
  const unsigned seed = argc > 2 ? (unsigned)atoi(argv[2]) : 1u;
  const float slack_scale = argc > 3 ? (float)atof(argv[3]) : 1.0f;
  const int all_depths = argc > 4 ? atoi(argv[4]) : 0;
  constexpr int kModes = 12;
  unsigned long long n_pairs = 0, n_tests = 0, n_s = 0, n_r1 = 0, n_tall = 0, n_inside = 0, n_scaled = 0, n_axis = 0;
  double worst_r1 = 0.0;
#pragma omp parallel reduction(+ : n_pairs, n_tests, n_s, n_r1, n_tall, n_inside, n_scaled, n_axis) reduction(max : worst_r1)
  {
    std::mt19937_64 rng(seed * 7919u + 104729u * (unsigned)omp_get_thread_num());
    std::uniform_real_distribution<double> U(0.0, 1.0);
    auto sym = [&](double s) { return (2.0 * U(rng) - 1.0) * s; };
    auto unit = [&](double *n) {
      double l;
      do {
        for (int k = 0; k < 3; ++k) n[k] = sym(1.0);
        l = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
      } while (l < 1e-3);
      for (int k = 0; k < 3; ++k) n[k] /= l;
    };
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
          const int K = 1 + (int)(U(rng) * 8) % 8;
          // raw[k] = {a, b, c, d}: plane 0 decides, built as a unit normal nn and a point x on it (inside: nn . (p - x) >= 0)
          double raw[8][4];
          double nn[3], x[3];
          unit(nn);
          double off = 0.0;   // signed distance of the centre inside the plane
          bool axis = false, scaled = false;
          if (mode == 0) off = -r;                                       // the sphere outside, tangent: gap 0 as near as float32 allows
          else if (mode == 1) off = r;                                   // inside, tangent: the far side of the sphere on the plane
          else if (mode == 2) off = 0.0;                                 // through the centre
          else if (mode == 3) {                                          // an axis normal, -0.0 components, tangent
            const int ax = (int)(U(rng) * 3) % 3;
            for (int k = 0; k < 3; ++k) nn[k] = U(rng) < 0.5 ? 0.0 : -0.0;
            nn[ax] = U(rng) < 0.5 ? 1.0 : -1.0;
            off = U(rng) < 0.7 ? -r : -r - mag * std::exp2(-24.0 * U(rng));
            axis = true;
          } else if (mode == 4) off = -r - mag * std::exp2(-18.0 - 8.0 * U(rng));   // a gap of a few ulps
          else if (mode == 5) off = sym(mag * std::exp2(10.0 * U(rng)));            // far away, either side
          else if (mode == 6) {                                          // a half-space holding the whole scene
            double far = 0.0;
            for (int k = 0; k < 3; ++k) far = std::max(far, std::max(std::fabs(slo[k]), std::fabs(shi[k])));
            off = 2.0 * far * (1.0 + U(rng));
          } else if (mode == 7 && !path.empty()) {                       // through the most-inside vertex of an ancestor's box
            const int a = path[(size_t)(U(rng) * path.size()) % path.size()];
            for (int k = 0; k < 3; ++k) x[k] = nn[k] >= 0.0 ? b.bmax[3 * a + k] : b.bmin[3 * a + k];
            off = 0.0;
            for (int k = 0; k < 3; ++k) off += nn[k] * (c[k] - x[k]);
          } else if (mode == 8 || mode == 9) {                           // the normal scaled to the ends of the valid range
            off = U(rng) < 0.5 ? -r : -r * (1.0 + sym(1e-6));
            scaled = true;
          } else if (mode == 10) off = -r * U(rng);                      // partly outside
          else off = r * (1.0 + U(rng));                                 // wholly inside
          for (int k = 0; k < 3; ++k) x[k] = c[k] - off * nn[k];
          double dd = 0.0;
          for (int k = 0; k < 3; ++k) dd -= nn[k] * x[k];
          double sc0 = axis ? 1.0 : std::exp2(std::floor(sym(6.0)));
          if (scaled) sc0 = mode == 8 ? 0x1p-39 : 0x1p39;
          for (int k = 0; k < 3; ++k) raw[0][k] = nn[k] * sc0;
          raw[0][3] = dd * sc0;
          for (int k = 1; k < K; ++k) {
            const double pick = U(rng);
            if (pick < 0.3) {                                            // a repeat of the deciding plane
              for (int e = 0; e < 4; ++e) raw[k][e] = raw[0][e];
            } else if (pick < 0.5 && mode != 6) {                        // the other face of a slab around the sphere
              const double w2 = 2.0 * std::fabs(off) + 2.0 * r + mag * U(rng);
              for (int e = 0; e < 3; ++e) raw[k][e] = -nn[e];
              raw[k][3] = -dd + w2;
            } else {                                                     // a random plane that holds the sphere, or nearly
              double n2[3];
              unit(n2);
              const double o2 = r * (U(rng) < 0.7 ? 1.0 + U(rng) : sym(1.0));
              double d2 = 0.0;
              for (int e = 0; e < 3; ++e) d2 -= n2[e] * (c[e] - o2 * n2[e]);
              const double s2 = std::exp2(std::floor(sym(6.0)));
              for (int e = 0; e < 3; ++e) raw[k][e] = n2[e] * s2;
              raw[k][3] = d2 * s2;
            }
          }
          QPlane pl[8];
          float rawf[8][4];
          bool ok = true;
          for (int k = 0; k < K; ++k) {
            for (int e = 0; e < 4; ++e) rawf[k][e] = (float)raw[k][e];
            ok = ok && plane_normalise(rawf[k][0], rawf[k][1], rawf[k][2], rawf[k][3], &pl[k]);
          }
          if (!ok) continue;
          float G, wmag;
#define EVAL(KK) eval_k<KK>(pl, s, &G, &wmag)
          BY_K(K, EVAL)
#undef EVAL
          if (!(G <= kTMax)) continue;                                   // never selected: nothing to check
          n_pairs++;
          if (G <= 0.0f) n_inside++;
          if (scaled) n_scaled++;
          if (axis) n_axis++;
          // (R1) against the exact gap of the exactly normalised planes
          q128 E = 0, Wq = 0;
          for (int k = 0; k < K; ++k) {
            const q128 A = rawf[k][0], B = rawf[k][1], C = rawf[k][2], Dq = rawf[k][3];
            const q128 len = qsqrt_pos(A * A + B * B + C * C);
            E = qmax(E, -((A * s.px + B * s.py + C * s.pz + Dq) / len));
            Wq = qmax(Wq, qabs(Dq / len));
          }
          const q128 g = E - (q128)s.radius;
          const q128 cn = qsqrt_pos((q128)s.px * s.px + (q128)s.py * s.py + (q128)s.pz * s.pz);
          const q128 lim = (q128)0x1p-24 * (8.8 * cn + 5.8 * Wq + (q128)s.radius) + (q128)0x1p-62;
          worst_r1 = std::max(worst_r1, (double)(qabs((q128)G - g) / lim));
          if (qabs((q128)G - g) > lim) n_r1++;
          // (S) every tested ancestor must admit j under T = G (planes_may_meet grows with T: then under every T >= G as well)
          for (int a : path) {
            if (depth[a] < exact_depth) continue;
            const float *nlo = &b.bmin[3 * (size_t)a], *nhi = &b.bmax[3 * (size_t)a];
            n_tests++;
            bool meets;
#define MEET(KK) meets = meet_k<KK>(pl, wmag, nlo, nhi, G, slack_scale)
            BY_K(K, MEET)
#undef MEET
            if (!meets) {
              if (n_s < 3)
#pragma omp critical
                printf("  violation: scene kind %d n %d height %d sweeps %d sphere (%a %a %a r %a) K %d mode %d plane0 (%a %a %a %a) G %a node depth %d\n",
                       kind, n, height, b.sweeps, s.px, s.py, s.pz, s.radius, K, mode, rawf[0][0], rawf[0][1], rawf[0][2], rawf[0][3], G, depth[a]);
              n_s++;
            }
          }
        }
      }
    }
  }
  printf("plane_query_bound_check: %llu (plane set, sphere) pairs (%llu at gap <= 0, %llu scaled normals, %llu axis normals), %llu node tests, "
         "%llu tall scenes: R1 violations %llu (worst |G - g| / bound %.4f), safety violations %llu\n",
         n_pairs, n_inside, n_scaled, n_axis, n_tests, n_tall, n_r1, worst_r1, n_s);
  return (n_r1 || n_s) ? 1 : 0;
}
