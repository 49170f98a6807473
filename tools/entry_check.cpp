// entry_check.cpp -- the per-tile entry lists of the pooled kernel's ENTRY instantiations on the CPU (lane_core.h: tile_rays, tile_verdict,
// tile_frontier, tile_entry).  Not a product path, not the oracle.  In the CPU test suite (tests/test_entry_lists_cpu.py).
//
//   build/entry_check frame <rgbbox | irreg | spheres.f32> <cam.f32 | -> <h> <w> [filter = 1] [mutant = 0] [tile_step = 1]
// Every 8 x 8 tile of the frame (every tile_step-th: a sample) gets its bounds and its frontier from the product's own functions over the product's
// own records (rt::make_trav_layout + rt::fill_leaf_boxes), and every primary ray of the tile is walked twice with lane_core.h's box test: from the
// root, and from its tile's list.  Asserted per ray: 1 / d_k inside the tile's bounds (`bound_violations`) and the SAME multiset of tested leaves
// from both walks (`set_violations`) -- for the uncapped frontier and for the packed list tile_entry writes (decoded from its dwords as the kernel
// reads them).  Counted: the inner items of both walks (an item is an inner node whose box the ray passed: one lane of a BOX operation), the
// saving under the caps of 4, 6 and 8 leaves with one inner item, the lists' lengths and content, the tiles without a list, the most leaves of a packed list.
// `filter`: the walk drops a leaf child whose own widened box fails (3.4a), where the scene's slots are filled -- the launch's filter.
// `mutant`: 1 ALLMISS decided with <, 2 bounds from two corners, 3 the sign check dropped -- each must show up as a violation somewhere.
//
//   build/entry_check verdicts [mutant = 0]
// tile_verdict on hand-made and random (bounds, box) pairs against box_hit_presorted on rays sampled inside the bounds, ends included:
// ALLHIT with a missing ray, ALLMISS with a hitting one, or a hand-made case with another verdict than the stated one (`verdict_errors`).
// Exit 0 unless the input cannot be read.
#include <algorithm>
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

constexpr int kMaxI = 64, kMaxL = 256;   // the "uncapped" frontier (a list that outgrows even these counts as none)

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

// The walk BOX performs from a set of start items: box items are inner nodes whose own box passed; `filter`: a leaf child is tested only if
// its slot passes.  Returns the inner items expanded; appends the tested leaves.
unsigned long long walk(const rt::TravLayout &t, const Ray &r, bool filter, std::vector<int32_t> &stack, std::vector<int32_t> &leaves) {
  unsigned long long items = 0;
  while (!stack.empty()) {
    const float *q = &t.nodes64[16 * static_cast<size_t>(stack.back())];
    stack.pop_back();
    ++items;
    for (int k = 0; k < 2; ++k) {
      int32_t ref8;
      std::memcpy(&ref8, &q[3 + 4 * k], 4);
      const bool hit = box_hit(r, q[8 * k], q[8 * k + 1], q[8 * k + 2], q[8 * k + 4], q[8 * k + 5], q[8 * k + 6]);
      if (ref8 >= 0) {
        if (hit) stack.push_back(ref8 >> 8);
      } else if (!filter || hit) {
        leaves.push_back(~(ref8 >> 8));
      }
    }
  }
  return items;
}

template <int MUT>
int frame_run(const rt::TravLayout &t, const Cam &cam, int h, int w, bool filter, int step, const char *name) {
  const int tiles_x = (w + 7) / 8, tiles_y = (h + 7) / 8, ntiles = tiles_x * tiles_y;
  const int n_nodes = static_cast<int>(t.nodes64.size() / 16);
  const int caps[3] = {4, 6, 8};
  unsigned long long rays = 0, items_root = 0, items_list = 0, items_cap[3] = {0, 0, 0}, items_packed = 0, bound_viol = 0, set_viol = 0;
  unsigned long long counted = 0, no_list = 0, no_list_cap[3] = {0, 0, 0}, packed_lists = 0, sum_inner = 0, sum_leaf = 0;
  int packed_leaf_max = 0;   // the most leaves any packed list holds
  std::vector<int> lengths;
#pragma omp parallel
  {
    std::vector<int32_t> stack, la, lb;
    std::vector<int> my_len;
#pragma omp for schedule(dynamic, 8) reduction(+ : rays, items_root, items_list, items_cap[:3], items_packed, bound_viol, set_viol, counted, no_list, no_list_cap[:3], packed_lists, sum_inner, sum_leaf) reduction(max : packed_leaf_max)
    for (int tile = 0; tile < ntiles; tile += step) {
      const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
      const int col0 = tx * 8, col1 = std::min(col0 + 7, w - 1), row0 = ty * 8, row1 = std::min(row0 + 7, h - 1);
      TileRays tr;
      const bool rays_ok = tile_rays<MUT>(cam, pixel_u(col0, w), pixel_u(col1, w), pixel_v(row0, h), pixel_v(row1, h), &tr);
      int inner[kMaxI], leaf[kMaxL], ni = 0, nl = 0;
      const bool have = rays_ok && tile_frontier<MUT, kMaxI, kMaxL>(tr, t.root_lo, t.root_hi, t.nodes64.data(), n_nodes, filter, inner, &ni, leaf, &nl);
      uint32_t packed[kEntryDw];
      tile_entry<MUT>(tr, rays_ok, t.root_lo, t.root_hi, t.nodes64.data(), n_nodes, filter, 8, 1, packed);
      const bool have_packed = (packed[0] & kEntryValid) != 0u;
      ++counted;
      if (have) { my_len.push_back(ni + nl); sum_inner += ni; sum_leaf += nl; } else ++no_list;
      for (int c = 0; c < 3; ++c) no_list_cap[c] += !(have && ni <= 1 && nl <= caps[c]);
      packed_lists += have_packed;
      if (have_packed) packed_leaf_max = std::max(packed_leaf_max, static_cast<int>(packed[0] >> kEntryCountShift) & 15);
      // (the packed list is the frontier under the product's caps: the same decision, or the check itself is broken)
      if (have_packed != (have && ni <= 1 && nl <= kEntryLeaves)) ++set_viol;
      for (int row = row0; row <= row1; ++row)
        for (int col = col0; col <= col1; ++col) {
          const Ray r = primary_ray(cam, col, row, w, h);
          ++rays;
          if (rays_ok) {
            const float iv[3] = {r.ix, r.iy, r.iz};
            for (int k = 0; k < 3; ++k) bound_viol += !(iv[k] >= tr.imin[k] && iv[k] <= tr.imax[k]);
          }
          const bool root_hit = box_hit(r, t.root_lo[0], t.root_lo[1], t.root_lo[2], t.root_hi[0], t.root_hi[1], t.root_hi[2]);
          stack.clear(); la.clear();
          if (root_hit && n_nodes > 0) stack.push_back(0);
          const unsigned long long it_root = walk(t, r, filter, stack, la);
          std::sort(la.begin(), la.end());
          items_root += it_root;
          // from the uncapped frontier (SHADE pushes a list only behind the ray's own root test)
          unsigned long long it_list = it_root;
          if (have) {
            stack.clear(); lb.clear();
            if (root_hit) {
              for (int i = 0; i < ni; ++i) stack.push_back(inner[i]);
              lb.assign(leaf, leaf + nl);
            }
            it_list = walk(t, r, filter, stack, lb);
            std::sort(lb.begin(), lb.end());
            set_viol += la != lb;
          }
          items_list += it_list;
          for (int c = 0; c < 3; ++c) items_cap[c] += have && ni <= 1 && nl <= caps[c] ? it_list : it_root;
          // from the packed list, decoded as the kernel reads it
          unsigned long long it_packed = it_root;
          if (have_packed) {
            stack.clear(); lb.clear();
            if (root_hit) {
              if (packed[0] & kEntryInner) stack.push_back(static_cast<int32_t>(packed[1] >> 8));
              const int pn = static_cast<int>(packed[0] >> kEntryCountShift) & 15;
              for (int i = 0; i < pn; ++i) lb.push_back(~(static_cast<int32_t>(packed[2 + i]) >> 8));
            }
            it_packed = walk(t, r, filter, stack, lb);
            std::sort(lb.begin(), lb.end());
            set_viol += la != lb;
          }
          items_packed += it_packed;
        }
    }
#pragma omp critical
    lengths.insert(lengths.end(), my_len.begin(), my_len.end());
  }
  std::sort(lengths.begin(), lengths.end());
  const size_t nlist = lengths.size();
  double mean = 0.0;
  for (int v : lengths) mean += v;
  auto pct = [&](unsigned long long with) { return items_root ? 100.0 * static_cast<double>(items_root - with) / static_cast<double>(items_root) : 0.0; };
  std::printf("scene=%s h=%d w=%d filter=%d mutant=%d tile_step=%d tiles=%llu rays=%llu items_root=%llu items_list=%llu saved_pct=%.2f "
              "saved_pct_L4=%.2f saved_pct_L6=%.2f saved_pct_L8=%.2f items_packed=%llu saved_pct_packed=%.2f no_list=%llu no_list_L4=%llu no_list_L6=%llu "
              "no_list_L8=%llu packed_lists=%llu packed_leaf_max=%d len_mean=%.2f len_p95=%d len_max=%d inner_mean=%.2f leaf_mean=%.2f bound_violations=%llu set_violations=%llu\n",
              name, h, w, filter ? 1 : 0, MUT, step, counted, rays, items_root, items_list, pct(items_list), pct(items_cap[0]), pct(items_cap[1]),
              pct(items_cap[2]), items_packed, pct(items_packed), no_list, no_list_cap[0], no_list_cap[1], no_list_cap[2], packed_lists, packed_leaf_max,
              nlist ? mean / static_cast<double>(nlist) : 0.0, nlist ? lengths[std::min(nlist - 1, nlist * 95 / 100)] : 0, nlist ? lengths.back() : 0,
              nlist ? static_cast<double>(sum_inner) / static_cast<double>(nlist) : 0.0, nlist ? static_cast<double>(sum_leaf) / static_cast<double>(nlist) : 0.0,
              bound_viol, set_viol);
  return 0;
}

int frame_main(int argc, char **argv) {
  if (argc < 6) return 2;
  const std::string what = argv[2];
  const int h = std::atoi(argv[4]), w = std::atoi(argv[5]);
  const bool filter_arg = argc > 6 ? std::atoi(argv[6]) != 0 : true;
  const int mutant = argc > 7 ? std::atoi(argv[7]) : 0;
  const int step = argc > 8 ? std::max(1, std::atoi(argv[8])) : 1;
  if (h <= 0 || w <= 0 || mutant < 0 || mutant > 3) return 2;
  rt::SceneDesc sc;
  const bool named = what == "rgbbox" || what == "irreg";
  if (what == "rgbbox") sc = rt::make_rgbbox();
  else if (what == "irreg") sc = rt::make_floor(100, 600.0f);
  else {
    const std::vector<float> sf = read_floats(argv[2]);
    if (sf.size() < 14 || sf.size() % 7 != 0) {
      std::fprintf(stderr, "entry_check: cannot read %s as n x 7 floats, n >= 2\n", argv[2]);
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
      std::fprintf(stderr, "entry_check: cannot read %s as 12 floats\n", argv[3]);
      return 2;
    }
    std::memcpy(&cam, cf.data(), sizeof cam);
  }
  const rt::Lbvh bvh = rt::build_lbvh(sc.spheres);
  rt::TravLayout t = rt::make_trav_layout(bvh, 1);
  const rt::LeafBoxConst k = rt::leaf_box_finish(rt::cull_stats(sc.spheres.data(), sc.spheres.size()), sc.spheres.size());
  rt::fill_leaf_boxes(t, k);
  // (the filter as a launch decides it: the scene's slots filled and the camera inside the guard)
  const bool filter = filter_arg && k.ok && rt::leaf_box_camera_ok(k, &cam.ox);
  const char *name = named ? what.c_str() : "file";
  switch (mutant) {
  case 1: return frame_run<1>(t, cam, h, w, filter, step, name);
  case 2: return frame_run<2>(t, cam, h, w, filter, step, name);
  case 3: return frame_run<3>(t, cam, h, w, filter, step, name);
  default: return frame_run<0>(t, cam, h, w, filter, step, name);
  }
}

// ---- verdicts ----
bool ray_hit(const TileRays &t, const float i[3], const float lo[3], const float hi[3]) {
  Ray r = {};
  r.ox = t.o[0]; r.oy = t.o[1]; r.oz = t.o[2];
  r.ix = i[0]; r.iy = i[1]; r.iz = i[2];
  const bool nx = r.ix < 0.0f, ny = r.iy < 0.0f, nz = r.iz < 0.0f;
  return box_hit_presorted(r, nx ? hi[0] : lo[0], nx ? lo[0] : hi[0], ny ? hi[1] : lo[1], ny ? lo[1] : hi[1], nz ? hi[2] : lo[2],
                           nz ? lo[2] : hi[2], 0.0f, kTMax);
}

template <int MUT>
int verdicts_run() {
  unsigned long long cases = 0, errors = 0, counts[3] = {0, 0, 0};
  struct Hand { TileRays t; float lo[3], hi[3]; int want; };
  const Hand hand[] = {
      // the origin ON the far x face: every ray's tmax is 0 = tmin -- a miss, by <=
      {{{0, 0, 0}, {0.5f, 0.5f, 0.5f}, {2, 2, 2}}, {-1, -1, -1}, {0, 1, 1}, kTileAllMiss},
      // ... and on the far face of a negative direction
      {{{0, 0, 0}, {-2, -2, -2}, {-0.5f, -0.5f, -0.5f}}, {0, -1, -1}, {1, 1, 1}, kTileAllMiss},
      // a box every ray enters before it leaves
      {{{0, 0, 0}, {0.9f, 0.9f, 0.9f}, {1.1f, 1.1f, 1.1f}}, {1, 1, 1}, {2, 2, 2}, kTileAllHit},
      // a box behind the origin
      {{{0, 0, 0}, {0.9f, 0.9f, 0.9f}, {1.1f, 1.1f, 1.1f}}, {-2, -2, -2}, {-1, -1, -1}, kTileAllMiss},
      // the origin inside the box
      {{{0, 0, 0}, {-3, 0.25f, 0.5f}, {-1, 4, 0.75f}}, {-1, -1, -1}, {1, 1, 1}, kTileAllHit},
      // some rays pass, some do not
      {{{0, 0, 0}, {0.5f, 0.5f, 0.5f}, {4, 4, 4}}, {1, 1, 1}, {2, 2, 2}, kTileMixed},
      // beyond the interval's end: tmin is 1e9 or more for every ray
      {{{0, 0, 0}, {1, 1, 1}, {2, 2, 2}}, {1e9f, 1e9f, 1e9f}, {2e9f, 2e9f, 2e9f}, kTileAllMiss},
  };
  auto check = [&](const TileRays &t, const float lo[3], const float hi[3], int want, std::mt19937 &rng) {
    const int v = tile_verdict<MUT>(t, lo, hi);
    ++cases; ++counts[v];
    if (want >= 0 && v != want) ++errors;
    std::uniform_real_distribution<float> u01(0.0f, 1.0f);
    for (int s = 0; s < 40; ++s) {
      float i[3];
      for (int k = 0; k < 3; ++k) {
        const int pick = s < 8 ? (s >> k) & 1 : 2;   // the eight corners of the bounds, then points inside
        i[k] = pick == 0 ? t.imin[k] : pick == 1 ? t.imax[k] : std::fmin(t.imax[k], std::fmax(t.imin[k], t.imin[k] + u01(rng) * (t.imax[k] - t.imin[k])));
      }
      const bool hit = ray_hit(t, i, lo, hi);
      if ((v == kTileAllHit && !hit) || (v == kTileAllMiss && hit)) { ++errors; break; }
    }
  };
  std::mt19937 rng(12345);
  for (const Hand &c : hand) check(c.t, c.lo, c.hi, c.want, rng);
  std::uniform_real_distribution<float> pos(-4.0f, 4.0f), mag(0.05f, 8.0f), wid(0.0f, 0.5f), ext(0.0f, 3.0f);
  for (int n = 0; n < 200000; ++n) {
    TileRays t;
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
      t.o[k] = pos(rng);
      const float a = mag(rng), b = a * (1.0f + wid(rng)), sgn = (rng() & 1u) ? 1.0f : -1.0f;
      t.imin[k] = sgn > 0 ? a : -b; t.imax[k] = sgn > 0 ? b : -a;
      lo[k] = pos(rng);
      hi[k] = lo[k] + ext(rng);
      if ((n & 15) == 0 && k == (n >> 4) % 3) t.o[k] = (n & 16) ? lo[k] : hi[k];   // the origin on a slab
    }
    check(t, lo, hi, -1, rng);
  }
  std::printf("verdicts mutant=%d cases=%llu mixed=%llu allhit=%llu allmiss=%llu verdict_errors=%llu\n", MUT, cases, counts[0], counts[1], counts[2], errors);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc >= 2 && std::strcmp(argv[1], "frame") == 0) {
    const int rc = frame_main(argc, argv);
    if (rc == 2) std::fprintf(stderr, "usage: entry_check frame <rgbbox | irreg | spheres.f32> <cam.f32 | -> <h> <w> [filter] [mutant] [tile_step]\n");
    return rc;
  }
  if (argc >= 2 && std::strcmp(argv[1], "verdicts") == 0) {
    switch (argc > 2 ? std::atoi(argv[2]) : 0) {
    case 1: return verdicts_run<1>();
    case 2: return verdicts_run<2>();
    case 3: return verdicts_run<3>();
    default: return verdicts_run<0>();
    }
  }
  std::fprintf(stderr, "usage: entry_check frame ... | entry_check verdicts [mutant]\n");
  return 2;
}
