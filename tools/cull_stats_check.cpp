// cull_stats_check -- the culling guards computed in two stages (rt_host.hpp: cull_stats + cull_finish) against the one-pass function
// they replace, and the device's two-stage reduction of the statistics (bvh_build.hip: launch_cull_stats) modelled on the host.
//
//   1. cull_finish(cull_stats(s), n, height) == the one-pass cull_scene_constants as it was before the split (restated below, verbatim)
//   2. cull_stats over random partitions of the spheres, merged in random order (cull_stats_merge) == the sequential pass
//   3. the device's arithmetic -- fp32 fminf / fmaxf over grid-stride slices, wave and block trees, one block over the partials, c_max in
//      fp64 -- with random grids and random merge orders == the sequential pass, and the guards derived from it == the one-pass function
//
// "Equal" is: the same `bad` flag and, where it is clear, every statistic equal (== : +-0 either way) and every CullConst field bit-equal
// except the centre, which is compared with == (its sign of zero is free: rt::cull_origin_ok uses it only through squared differences).
// Scenes: random boxes, and adversarial ones -- NaN and +-inf components, radius 0 and just under 2^-20, coordinates near 2^40, +-0
// coordinates, r_min at and beside the 2^15 reach guard.
//
// usage: cull_stats_check [scenes] [seed] [mutate]     exit 0 iff no mismatch
//   mutate = 1: the device model sums |p_a| + r in fp32 instead of fp64 (the check must then fail: it sees the difference)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "rt_host.hpp"

using rt::CullConst;
using rt::CullStats;
using rt::Sphere;

namespace {

int g_mutate = 0;

// The one-pass function before the split (host_build.cpp), kept here as the yardstick.
CullConst before_split(const std::vector<Sphere> &ts, int height) {
  CullConst c;
  const size_t n = ts.size();
  if (n < 2) return c;
  const int sweeps = static_cast<int>(log2f(static_cast<float>(n))) + 2;
  if (height > sweeps) return c;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  double r_min = INFINITY, r_max = 0.0, c_max = 0.0;
  for (const Sphere &s : ts) {
    const double p[3] = {s.px, s.py, s.pz}, r = s.radius;
    if (!(r >= 0x1p-20) || !std::isfinite(r)) return c;
    r_min = std::min(r_min, r);
    r_max = std::max(r_max, r);
    for (int a = 0; a < 3; ++a) {
      if (!std::isfinite(p[a])) return c;
      lo[a] = std::min(lo[a], p[a]);
      hi[a] = std::max(hi[a], p[a]);
      c_max = std::max(c_max, std::fabs(p[a]) + r);
    }
  }
  if (c_max > 0x1p40) return c;
  double diag2 = 0.0;
  for (int a = 0; a < 3; ++a) {
    c.centre[a] = 0.5 * (lo[a] + hi[a]);
    diag2 += (hi[a] - lo[a]) * (hi[a] - lo[a]);
  }
  c.reach = 0.5 * std::sqrt(diag2) * (1.0 + 0x1p-20) + r_max;
  c.r_min = r_min;
  if (2.0 * c.reach > 0x1p15 * r_min) return c;
  const double c2 = 1.01 * (0x1p-16 / r_min + 0x1p-21);
  const double c0 = 1.01 * (0x1p-16 * r_max * r_max / r_min + 0x1p-18 * r_max + 0x1p-24 * c_max + 0x1p-21);
  c.c2 = std::nextafter(static_cast<float>(c2), INFINITY);
  c.kappa = std::nextafter(static_cast<float>(c0 / (c2 * 0.015625)), INFINITY);
  c.ok = std::isfinite(c.c2) && std::isfinite(c.kappa);
  return c;
}

// ---- the device's reduction, in its own arithmetic (bvh_build.hip: CullAcc) ----
struct Acc {
  float lo[3], hi[3], r_min, r_max;
  double c_max;
  int bad;
};
Acc acc_init() {
  Acc a;
  for (int k = 0; k < 3; ++k) {
    a.lo[k] = INFINITY;
    a.hi[k] = -INFINITY;
  }
  a.r_min = INFINITY;
  a.r_max = 0.0f;
  a.c_max = 0.0;
  a.bad = 0;
  return a;
}
void acc_merge(Acc &a, const Acc &b) {   // fminf / fmaxf / fmax: a NaN operand loses
  for (int k = 0; k < 3; ++k) {
    a.lo[k] = std::fmin(a.lo[k], b.lo[k]);
    a.hi[k] = std::fmax(a.hi[k], b.hi[k]);
  }
  a.r_min = std::fmin(a.r_min, b.r_min);
  a.r_max = std::fmax(a.r_max, b.r_max);
  a.c_max = std::fmax(a.c_max, b.c_max);
  a.bad |= b.bad;
}
void acc_add(Acc &a, const Sphere &s) {   // cull_stats_kernel's loop body
  const float p[3] = {s.px, s.py, s.pz}, r = s.radius;
  if (!(r >= 0x1p-20f) || !std::isfinite(r)) a.bad = 1;
  a.r_min = std::fmin(a.r_min, r);
  a.r_max = std::fmax(a.r_max, r);
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(p[k])) a.bad = 1;
    a.lo[k] = std::fmin(a.lo[k], p[k]);
    a.hi[k] = std::fmax(a.hi[k], p[k]);
    a.c_max = std::fmax(a.c_max, g_mutate == 1 ? static_cast<double>(std::fabs(p[k]) + r) : std::fabs(static_cast<double>(p[k])) + static_cast<double>(r));
  }
}
// merge a list of accumulators in a random order (the wave / block trees and the final pass fix one order each; any must do)
Acc merge_shuffled(std::vector<Acc> v, std::mt19937_64 &rng) {
  std::shuffle(v.begin(), v.end(), rng);
  Acc a = acc_init();
  for (const Acc &b : v) acc_merge(a, b);
  return a;
}
CullStats device_model(const std::vector<Sphere> &ts, int blocks, std::mt19937_64 &rng) {
  constexpr int kBT = 256;
  const int n = static_cast<int>(ts.size());
  std::vector<Acc> partial;
  for (int b = 0; b < blocks; ++b) {
    std::vector<Acc> threads;
    for (int t = 0; t < kBT; ++t) {
      Acc a = acc_init();
      for (int i = b * kBT + t; i < n; i += blocks * kBT) acc_add(a, ts[static_cast<size_t>(i)]);
      threads.push_back(a);
    }
    partial.push_back(merge_shuffled(threads, rng));
  }
  const Acc a = merge_shuffled(partial, rng);
  CullStats s;   // (the host's conversion: api.cpp build_from_device)
  for (int k = 0; k < 3; ++k) {
    s.lo[k] = a.lo[k];
    s.hi[k] = a.hi[k];
  }
  s.r_min = a.r_min;
  s.r_max = a.r_max;
  s.c_max = a.c_max;
  s.bad = a.bad != 0;
  return s;
}

CullStats partition_model(const std::vector<Sphere> &ts, std::mt19937_64 &rng) {
  const size_t n = ts.size();
  std::vector<size_t> idx(n);
  for (size_t i = 0; i < n; ++i) idx[i] = i;
  std::shuffle(idx.begin(), idx.end(), rng);
  std::vector<Sphere> perm(n);
  for (size_t i = 0; i < n; ++i) perm[i] = ts[idx[i]];
  std::vector<CullStats> parts;
  for (size_t at = 0; at < n;) {
    const size_t len = std::min(n - at, static_cast<size_t>(1 + rng() % (n / 3 + 1)));
    parts.push_back(rt::cull_stats(perm.data() + at, len));
    at += len;
  }
  std::shuffle(parts.begin(), parts.end(), rng);
  CullStats s;
  for (const CullStats &p : parts) s = rt::cull_stats_merge(s, p);
  return s;
}

bool same_stats(const CullStats &a, const CullStats &b) {
  if (a.bad != b.bad) return false;
  if (a.bad) return true;
  for (int k = 0; k < 3; ++k)
    if (!(a.lo[k] == b.lo[k]) || !(a.hi[k] == b.hi[k])) return false;
  return a.r_min == b.r_min && a.r_max == b.r_max && a.c_max == b.c_max;
}
bool bits_eq(double x, double y) { return std::memcmp(&x, &y, sizeof x) == 0; }
bool bits_eq(float x, float y) { return std::memcmp(&x, &y, sizeof x) == 0; }
bool same_const(const CullConst &a, const CullConst &b) {
  if (a.ok != b.ok || !bits_eq(a.c2, b.c2) || !bits_eq(a.kappa, b.kappa) || !bits_eq(a.reach, b.reach) || !bits_eq(a.r_min, b.r_min)) return false;
  for (int k = 0; k < 3; ++k)
    if (!(a.centre[k] == b.centre[k])) return false;
  return true;
}

// ---- scenes ----
float uni(std::mt19937_64 &rng, float lo, float hi) { return std::uniform_real_distribution<float>(lo, hi)(rng); }

std::vector<Sphere> random_scene(std::mt19937_64 &rng, int kind) {
  const int n = 2 + static_cast<int>(rng() % (kind == 0 ? 3000 : 700));
  const float ext = std::ldexp(1.0f, static_cast<int>(rng() % 40) - 10);
  std::vector<Sphere> ts(static_cast<size_t>(n));
  for (Sphere &s : ts) {
    s.px = uni(rng, -ext, ext); s.py = uni(rng, -ext, ext); s.pz = uni(rng, -ext, ext);
    s.cr = uni(rng, 0, 1); s.cg = uni(rng, 0, 1); s.cb = uni(rng, 0, 1);
    s.radius = ext * uni(rng, 1e-4f, 0.1f);
  }
  const size_t j = rng() % ts.size();
  Sphere &s = ts[j];
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = INFINITY;
  switch (kind) {
    case 0: break;                                            // plain
    case 1: (&s.px)[rng() % 3] = nan; break;                  // NaN coordinate
    case 2: s.radius = nan; break;                            // NaN radius
    case 3: (&s.px)[rng() % 3] = (rng() & 1) ? inf : -inf; break;
    case 4: s.radius = (rng() & 1) ? inf : -inf; break;
    case 5: s.radius = (rng() & 1) ? 0.0f : -0.0f; break;     // radius 0
    case 6: s.radius = std::nextafter(0x1p-20f, 0.0f); break; // just under 2^-20
    case 7: {                                                 // radius exactly 2^-20, the rest tight around it: the reach guard decides
      for (Sphere &t : ts) {
        t.px = uni(rng, -0.01f, 0.01f); t.py = uni(rng, -0.01f, 0.01f); t.pz = uni(rng, -0.01f, 0.01f);
        t.radius = 0x1p-20f * uni(rng, 1.0f, 2.0f);
      }
      s.radius = 0x1p-20f;
      break;
    }
    case 8: {                                                 // coordinates near 2^40 (c_max on either side of the bound)
      const float big = std::ldexp(1.0f, 40) * uni(rng, 0.999f, 1.001f);
      for (Sphere &t : ts) { t.radius = std::ldexp(1.0f, 30); }
      (&s.px)[rng() % 3] = (rng() & 1) ? big : -big;
      break;
    }
    case 9: {                                                 // +-0 coordinates everywhere the box could end
      for (Sphere &t : ts) {
        t.px = (rng() & 1) ? 0.0f : -0.0f;
        t.py = (rng() & 1) ? 0.0f : uni(rng, -1, 1);
        t.pz = (rng() & 1) ? -0.0f : uni(rng, -1, 1);
        t.radius = uni(rng, 0.01f, 0.1f);
      }
      break;
    }
    case 10: {                                                // r_min at the 2^15 reach guard: 2 (R + r_max) vs 2^15 r_min
      for (Sphere &t : ts) t.radius = 1.0f;
      // a line of centres [0, L] on x: R = L / 2 (1 + 2^-20) roughly, reach = R + 1; pick r_min so that the guard is within a few ulps
      const float L = uni(rng, 100.0f, 10000.0f);
      for (size_t i = 0; i < ts.size(); ++i) { ts[i].px = L * static_cast<float>(i) / static_cast<float>(ts.size() - 1); ts[i].py = ts[i].pz = 0.0f; }
      const double reach = 0.5 * static_cast<double>(L) * (1.0 + 0x1p-20) + 1.0;
      const float r0 = static_cast<float>(2.0 * reach / 0x1p15);
      float r = r0;
      for (int k = static_cast<int>(rng() % 7) - 3; k != 0; k += k < 0 ? 1 : -1) r = std::nextafter(r, k < 0 ? 0.0f : INFINITY);
      s.radius = r;
      break;
    }
    default: break;
  }
  return ts;
}

}  // namespace

int main(int argc, char **argv) {
  const int scenes = argc > 1 ? std::atoi(argv[1]) : 2000;
  const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
  g_mutate = argc > 3 ? std::atoi(argv[3]) : 0;
  std::mt19937_64 rng(seed);
  long checks = 0, bad_stage = 0, bad_part = 0, bad_dev = 0, ok_scenes = 0, bad_scenes = 0;
  for (int sc = 0; sc < scenes; ++sc) {
    const int kind = sc % 11;
    const std::vector<Sphere> ts = random_scene(rng, kind);
    const size_t n = ts.size();
    const CullStats seq = rt::cull_stats(ts.data(), n);
    const int sweeps = static_cast<int>(log2f(static_cast<float>(n))) + 2;
    const int height = (rng() & 1) ? 0 : static_cast<int>(rng() % static_cast<uint64_t>(sweeps + 3));
    const CullConst want = before_split(ts, height);
    (want.ok ? ok_scenes : bad_scenes)++;
    // 1. the composition
    ++checks;
    if (!same_const(rt::cull_finish(seq, n, height), want) || !same_const(rt::cull_scene_constants(ts, height), want)) {
      if (++bad_stage <= 5) std::printf("MISMATCH composition: scene %d kind %d n %zu height %d\n", sc, kind, n, height);
    }
    // 2. partitions merged in random orders
    for (int t = 0; t < 3; ++t) {
      ++checks;
      const CullStats s = partition_model(ts, rng);
      if (!same_stats(s, seq) || !same_const(rt::cull_finish(s, n, height), want)) {
        if (++bad_part <= 5) std::printf("MISMATCH partition: scene %d kind %d n %zu\n", sc, kind, n);
      }
    }
    // 3. the device's reduction: the grid launch_cull_stats uses, and a random one
    const int nb = static_cast<int>((n + 255) / 256), grids[2] = {std::min(nb, 1024), 1 + static_cast<int>(rng() % 8)};
    for (int g : grids) {
      ++checks;
      const CullStats s = device_model(ts, g, rng);
      if (!same_stats(s, seq) || !same_const(rt::cull_finish(s, n, height), want)) {
        if (++bad_dev <= 5) std::printf("MISMATCH device model: scene %d kind %d n %zu blocks %d\n", sc, kind, n, g);
      }
    }
  }
  std::printf("cull_stats_check: %d scenes (%ld with culling on, %ld off), %ld checks: %ld composition, %ld partition, %ld device-model mismatches\n",
              scenes, ok_scenes, bad_scenes, checks, bad_stage, bad_part, bad_dev);
  return (bad_stage || bad_part || bad_dev || ok_scenes == 0 || bad_scenes == 0) ? 1 : 0;
}
