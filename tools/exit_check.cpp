// exit_check.cpp -- the exit lists of the pooled kernel's kEntryExit instantiations on the CPU (lane_core.h: exit_tables_path).
// Not a product path, not the oracle.  In the CPU test suite (tests/test_exit_lists_cpu.py).
//
//   build/exit_check frame <rgbbox | irreg | spheres.f32> <cam.f32 | -> <h> <w> [max_depth = 50] [mutant = 0] [dark = 1] [shrink = 0]
// Every pixel's bounce chain is walked with lane_core.h's own arithmetic over the product's own records (rt::make_trav_layout +
// rt::fill_leaf_boxes; the leaf filter as a launch decides it), stopped where the dark stop stops it (dark = 1).  Every BOUNCE ray (a ray that
// starts where a fold has just scattered) is walked twice: from the root, and -- as SHADE does it -- from the exit list of the sphere it leaves,
// decoded from the table exit_tables_path writes: the box test of the list's node E, then E's item and the pair items, or the root when there is no
// list or E's box fails.  Asserted per ray: the SAME multiset of tested leaves from both walks (`set_violations`).  Counted: the bounce rays, their
// items from the root and from the lists (an item is an inner node -- or a pair record -- whose own box the ray passed: one lane of a BOX
// operation), the items of the root walk that are ancestors of the sphere the ray leaves, the rays that started from a list (`lists`), that had a
// list and failed its box (`fallbacks`), the ancestor boxes such rays failed in the root walk (`anc_failed`: one per ray -- below a failed box nothing is tested; `anc_failing_boxes`: every ancestor box the ray would fail, tested on its own), the primary rays' items,
// the spheres with a list, the inner nodes per depth.
// `shrink` (percent): the boxes of the root's inner children, as the root's record holds them, are shrunk about their centres by that much before anything
// is built -- upper boxes that do NOT contain the boxes below them, as a tree taller than its sweeps may have them: such chains must get no list.
// `mutant`: 1 the tables are built without the nesting check, 2 SHADE pushes the list without testing E's box -- each must show up as a violation
// on the case made for it.
//
//   build/exit_check lemma [mutant = 0]
// The lemma of DESIGN.md 3.4c against sampled adversarial rays: boxes E inside A component-wise (shared faces included), origins on the slabs, zero,
// denormal, infinite and NaN direction components: box_hit passes E => box_hit passes A (`lemma_errors`).  mutant 1 drops the nesting on one face.
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

// The walk BOX performs from a set of start items over `rec` (the real records, then the pair records); returns the items expanded, appends the
// tested leaves; `anc` (when given): the items that are in `chain` (the ancestors of one leaf)
unsigned long long walk(const std::vector<float> &rec, const Ray &r, bool filter, std::vector<int32_t> &stack, std::vector<int32_t> &leaves,
                        const std::vector<char> *on_chain = nullptr, unsigned long long *anc = nullptr) {
  unsigned long long items = 0;
  while (!stack.empty()) {
    const int32_t node = stack.back();
    const float *q = &rec[16 * static_cast<size_t>(node)];
    stack.pop_back();
    ++items;
    if (on_chain && (*on_chain)[static_cast<size_t>(node)]) ++*anc;
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
int frame_run(const rt::TravLayout &t, const Cam &cam, int h, int w, int max_depth, bool filter, bool dark, const char *name) {
  const int n_nodes = static_cast<int>(t.nodes64.size() / 16), n_sph = static_cast<int>(t.sph.size() / 4);
  // the tables as the device builds them: one call per path
  std::vector<float> tab(16 * static_cast<size_t>(kExitPairs) + 8 * static_cast<size_t>(n_sph), 0.0f);
  // (the refs as the kernel packs them where the scene fits its 16 bits -- the scenes it renders with lists; plain record indices for larger ones)
  const int ref_mul = (n_nodes + kExitPairs) * (kPsNodeBytes / 8) < 65536 ? kPsNodeBytes / 8 : 1;
  if (n_nodes + kExitPairs >= 65536) return 2;
  for (int p = 0; p < (1 << kExitDmax); ++p) exit_tables_path<MUT == 1 ? 1 : 0>(p, t.root_lo, t.root_hi, t.nodes64.data(), n_nodes, n_sph, tab.data(), ref_mul);
  std::vector<float> rec = t.nodes64;
  rec.insert(rec.end(), tab.begin(), tab.begin() + 16 * kExitPairs);
  const uint32_t *const ent = reinterpret_cast<const uint32_t *>(tab.data() + 16 * kExitPairs);
  // every leaf's ancestors (for the count of ancestor items, and of ancestor boxes failed)
  std::vector<int32_t> parent(static_cast<size_t>(std::max(n_nodes, 1)), -1), leaf_parent(static_cast<size_t>(n_sph), -1);
  std::vector<float> nbox(6 * static_cast<size_t>(std::max(n_nodes, 1)), 0.0f);   // every inner node's own box: the root's, else its slot of its parent's record
  std::memcpy(&nbox[0], t.root_lo, 12); std::memcpy(&nbox[3], t.root_hi, 12);
  for (int i = 0; i < n_nodes; ++i)
    for (int k = 0; k < 2; ++k) {
      int32_t ref8;
      std::memcpy(&ref8, &t.nodes64[16 * static_cast<size_t>(i) + 3 + 4 * k], 4);
      if (ref8 >= 0) {
        parent[static_cast<size_t>(ref8 >> 8)] = i;
        std::memcpy(&nbox[6 * static_cast<size_t>(ref8 >> 8)], &t.nodes64[16 * static_cast<size_t>(i) + 8 * k], 12);
        std::memcpy(&nbox[6 * static_cast<size_t>(ref8 >> 8) + 3], &t.nodes64[16 * static_cast<size_t>(i) + 8 * k + 4], 12);
      } else if (~(ref8 >> 8) < n_sph) leaf_parent[static_cast<size_t>(~(ref8 >> 8))] = i;
    }
  // inner nodes per depth
  std::vector<int> depth_of(static_cast<size_t>(std::max(n_nodes, 1)), 0), per_depth;
  for (int i = 0; i < n_nodes; ++i) {   // (breadth-first numbering: a parent's index is below its children's)
    int d = 0;
    for (int32_t a = parent[static_cast<size_t>(i)]; a >= 0; a = parent[static_cast<size_t>(a)]) ++d;
    if (static_cast<size_t>(d) >= per_depth.size()) per_depth.resize(static_cast<size_t>(d) + 1, 0);
    ++per_depth[static_cast<size_t>(d)];
  }
  std::string depths;
  for (size_t d = 0; d < per_depth.size(); ++d) depths += (d ? "," : "") + std::to_string(per_depth[d]);
  unsigned long long with_list = 0;
  for (int j = 0; j < n_sph; ++j) with_list += (ent[8 * j + 3] & 0xffffu) != 0u;
  unsigned long long bounce = 0, items_root = 0, items_list = 0, items_anc = 0, lists = 0, fallbacks = 0, set_viol = 0, primary = 0, items_primary = 0, pair_items = 0, anc_failed = 0, anc_failed_rays = 0;
#pragma omp parallel
  {
    std::vector<int32_t> stack, la, lb;
    std::vector<char> on_chain(static_cast<size_t>(n_nodes + kExitPairs), 0);
#pragma omp for schedule(dynamic, 4) reduction(+ : bounce, items_root, items_list, items_anc, lists, fallbacks, set_viol, primary, items_primary, pair_items, anc_failed, anc_failed_rays)
    for (int row = 0; row < h; ++row)
      for (int col = 0; col < w; ++col) {
        Ray r = primary_ray(cam, col, row, w, h);
        float lr = 1.0f, lg = 1.0f, lb3 = 1.0f;
        int depth = 0, from = -1;   // from: the sphere the ray leaves (-1: a primary ray)
        for (;;) {
          const bool root_hit = n_nodes > 0 && box_hit(r, t.root_lo[0], t.root_lo[1], t.root_lo[2], t.root_hi[0], t.root_hi[1], t.root_hi[2]);
          if (from >= 0)
            for (int32_t a = leaf_parent[static_cast<size_t>(from)]; a >= 0; a = parent[static_cast<size_t>(a)]) on_chain[static_cast<size_t>(a)] = 1;
          stack.clear(); la.clear();
          if (root_hit) stack.push_back(0);
          unsigned long long anc = 0;
          const unsigned long long it_root = walk(rec, r, filter, stack, la, from >= 0 ? &on_chain : nullptr, &anc);
          if (from >= 0)
            for (int32_t a = leaf_parent[static_cast<size_t>(from)]; a >= 0; a = parent[static_cast<size_t>(a)]) on_chain[static_cast<size_t>(a)] = 0;
          if (from < 0) { ++primary; items_primary += it_root; }
          else {
            ++bounce; items_root += it_root; items_anc += anc;
            // the boxes of the ancestors of the sphere the ray leaves that the ray fails (each tested on its own, whatever its parent's verdict)
            unsigned long long nf = 0;
            for (int32_t a = leaf_parent[static_cast<size_t>(from)]; a >= 0; a = parent[static_cast<size_t>(a)]) {
              const float *b = &nbox[6 * static_cast<size_t>(a)];
              nf += !box_hit(r, b[0], b[1], b[2], b[3], b[4], b[5]);
            }
            anc_failed += nf; anc_failed_rays += nf != 0;
            // as SHADE does it
            const uint32_t *const e = ent + 8 * static_cast<size_t>(from);
            unsigned long long it_list = it_root;
            if ((e[3] & 0xffffu) != 0u) {
              float lo[3], hi[3];
              std::memcpy(lo, e, 12); std::memcpy(hi, e + 4, 12);
              const bool e_hit = MUT == 2 || box_hit(r, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
              stack.clear(); lb.clear();
              if (e_hit) {
                ++lists;
                const uint32_t refs[4] = {e[3] & 0xffffu, e[3] >> 16, e[7] & 0xffffu, e[7] >> 16};
                for (int k = 0; k < 4; ++k)
                  if (refs[k] != 0u) { stack.push_back(static_cast<int32_t>(refs[k] / static_cast<uint32_t>(ref_mul))); pair_items += k > 0; }
              } else {
                ++fallbacks;
                if (root_hit) stack.push_back(0);
              }
              it_list = walk(rec, r, filter, stack, lb);
              std::sort(la.begin(), la.end());
              std::sort(lb.begin(), lb.end());
              set_viol += la != lb;
            }
            items_list += it_list;
          }
          float best = kTMax;
          int bestj = -1;
          for (int32_t j : la) closest_update(sphere_root(r, t.sph[4 * static_cast<size_t>(j)], t.sph[4 * static_cast<size_t>(j) + 1], t.sph[4 * static_cast<size_t>(j) + 2],
                                                          t.sph[4 * static_cast<size_t>(j) + 3]), j, best, bestj);
          float sp[4] = {0.0f, 0.0f, 0.0f, 1.0f}, c[4] = {0.0f, 0.0f, 0.0f, 1.0f};
          if (bestj >= 0) {
            std::memcpy(sp, &t.sph[4 * static_cast<size_t>(bestj)], 16);
            std::memcpy(c, &t.col[4 * static_cast<size_t>(bestj)], 16);
          }
          const bool more = finish_ray_emit(r, best, bestj, sp[0], sp[1], sp[2], sp[3], c[0], c[1], c[2], c[3], lr, lg, lb3, depth, max_depth, [](float, float, float) {});
          if (!more || (dark && light_is_dead(lr, lg, lb3))) break;
          from = bestj;
        }
      }
  }
  std::printf("inner_per_depth=%s ", depths.c_str());
  std::printf("scene=%s n=%d h=%d w=%d max_depth=%d filter=%d dark=%d mutant=%d dmax=%d spheres_with_list=%llu primary=%llu items_primary=%llu bounce=%llu "
              "items_root=%llu items_anc=%llu items_list=%llu pair_items=%llu lists=%llu fallbacks=%llu anc_failed=%llu anc_failing_boxes=%llu set_violations=%llu\n",
              name, n_sph, h, w, max_depth, filter ? 1 : 0, dark ? 1 : 0, MUT, kExitDmax, with_list, primary, items_primary, bounce, items_root, items_anc, items_list,
              pair_items, lists, fallbacks, anc_failed_rays, anc_failed, set_viol);
  return 0;
}

int frame_main(int argc, char **argv) {
  if (argc < 6) return 2;
  const std::string what = argv[2];
  const int h = std::atoi(argv[4]), w = std::atoi(argv[5]);
  const int max_depth = argc > 6 ? std::atoi(argv[6]) : 50;
  const int mutant = argc > 7 ? std::atoi(argv[7]) : 0;
  const bool dark = argc > 8 ? std::atoi(argv[8]) != 0 : true;
  const int shrink = argc > 9 ? std::atoi(argv[9]) : 0;
  if (h <= 0 || w <= 0 || max_depth < 1 || mutant < 0 || mutant > 2) return 2;
  rt::SceneDesc sc;
  const bool named = what == "rgbbox" || what == "irreg";
  if (what == "rgbbox") sc = rt::make_rgbbox();
  else if (what == "irreg") sc = rt::make_floor(100, 600.0f);
  else {
    const std::vector<float> sf = read_floats(argv[2]);
    if (sf.size() < 14 || sf.size() % 7 != 0) {
      std::fprintf(stderr, "exit_check: cannot read %s as n x 7 floats, n >= 2\n", argv[2]);
      return 2;
    }
    sc.spheres.resize(sf.size() / 7);
    std::memcpy(sc.spheres.data(), sf.data(), sf.size() * sizeof(float));
  }
  Cam cam;
  if (std::strcmp(argv[3], "-") == 0) {
    if (!named) return 2;
    const rt::Camera c = rt::scene_camera(sc, h, w);
    static_assert(sizeof(Cam) == sizeof(rt::Camera), "12 floats each");
    std::memcpy(&cam, &c, sizeof cam);
  } else {
    const std::vector<float> cf = read_floats(argv[3]);
    if (cf.size() != 12) {
      std::fprintf(stderr, "exit_check: cannot read %s as 12 floats\n", argv[3]);
      return 2;
    }
    std::memcpy(&cam, cf.data(), sizeof cam);
  }
  const rt::Lbvh bvh = rt::build_lbvh(sc.spheres);
  rt::TravLayout t = rt::make_trav_layout(bvh, 1);
  const rt::LeafBoxConst k = rt::leaf_box_finish(rt::cull_stats(sc.spheres.data(), sc.spheres.size()), sc.spheres.size());
  rt::fill_leaf_boxes(t, k);
  const bool filter = k.ok && rt::leaf_box_camera_ok(k, &cam.ox);
  if (shrink > 0 && !t.nodes64.empty()) {
    for (int s = 0; s < 2; ++s) {
      int32_t ref8;
      std::memcpy(&ref8, &t.nodes64[3 + 4 * s], 4);
      if (ref8 < 0) continue;
      for (int a = 0; a < 3; ++a) {
        float &lo = t.nodes64[8 * s + a], &hi = t.nodes64[8 * s + 4 + a];
        const float cut = 0.005f * static_cast<float>(shrink) * (hi - lo);
        lo += cut; hi -= cut;
      }
    }
  }
  const char *name = named ? what.c_str() : "file";
  switch (mutant) {
  case 1: return frame_run<1>(t, cam, h, w, max_depth, filter, dark, name);
  case 2: return frame_run<2>(t, cam, h, w, max_depth, filter, dark, name);
  default: return frame_run<0>(t, cam, h, w, max_depth, filter, dark, name);
  }
}

// ---- the lemma ----
int lemma_run(int mutant) {
  std::mt19937 rng(20261);
  std::uniform_real_distribution<float> pos(-4.0f, 4.0f), ext(0.0f, 3.0f), grow(0.0f, 1.0f), dir(-1.0f, 1.0f);
  const float inf = kNoHit, specials[] = {0.0f, -0.0f, 1e-42f, -1e-42f, inf, -inf, 1e-30f, -1e30f, std::nanf("")};
  unsigned long long cases = 0, pass_inner = 0, errors = 0;
  for (int n = 0; n < 400000; ++n) {
    float elo[3], ehi[3], alo[3], ahi[3];
    for (int k = 0; k < 3; ++k) {
      elo[k] = pos(rng);
      ehi[k] = elo[k] + ext(rng);
      alo[k] = (rng() & 3u) ? elo[k] - grow(rng) : elo[k];   // (a shared face one time in four)
      ahi[k] = (rng() & 3u) ? ehi[k] + grow(rng) : ehi[k];
    }
    if (mutant == 1) ahi[n % 3] = ehi[n % 3] - 0.25f * (ehi[n % 3] - elo[n % 3]) - 1e-3f;
    for (int s = 0; s < 24; ++s) {
      Ray r = {};
      float o[3], d[3];
      for (int k = 0; k < 3; ++k) {
        const unsigned pick = rng() % 8u;
        // the origin on a face of either box, inside the inner box, or anywhere
        o[k] = pick == 0 ? elo[k] : pick == 1 ? ehi[k] : pick == 2 ? alo[k] : pick == 3 ? ahi[k] : pick < 6 ? elo[k] + grow(rng) * (ehi[k] - elo[k]) : pos(rng) * 2.0f;
        d[k] = (rng() % 3u) == 0u ? specials[rng() % (sizeof specials / sizeof specials[0])] : dir(rng);
      }
      r.ox = o[0]; r.oy = o[1]; r.oz = o[2];
      r.dx = d[0]; r.dy = d[1]; r.dz = d[2];
      ray_derive(r);
      const bool in = box_hit(r, elo[0], elo[1], elo[2], ehi[0], ehi[1], ehi[2]);
      const bool out = box_hit(r, alo[0], alo[1], alo[2], ahi[0], ahi[1], ahi[2]);
      ++cases;
      pass_inner += in;
      errors += in && !out;
    }
  }
  std::printf("lemma mutant=%d cases=%llu pass_inner=%llu lemma_errors=%llu\n", mutant, cases, pass_inner, errors);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc >= 2 && std::strcmp(argv[1], "frame") == 0) {
    const int rc = frame_main(argc, argv);
    if (rc == 2) std::fprintf(stderr, "usage: exit_check frame <rgbbox | irreg | spheres.f32> <cam.f32 | -> <h> <w> [max_depth] [mutant] [dark] [shrink]\n");
    return rc;
  }
  if (argc >= 2 && std::strcmp(argv[1], "lemma") == 0) return lemma_run(argc > 2 ? std::atoi(argv[2]) : 0);
  std::fprintf(stderr, "usage: exit_check frame ... | exit_check lemma [mutant]\n");
  return 2;
}
