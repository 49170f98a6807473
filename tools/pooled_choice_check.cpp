// pooled_choice_check -- rtk::choose_pooled (rt_device.hpp), the one rule that picks the pooled kernel's instantiation, run over the cross
// product of the launch parameters it reads.  Checks that every launch it accepts names a compiled instantiation (rtk::kPooledKeys), that
// every compiled instantiation is reachable, that warm_render_kernels' set is the 34 it has always been, and that rt_context_last_launch's
// `instantiation=` names are the ones the tests and tools read.  The render path's names are also compared with the rule api.cpp used to
// restate by hand: they differ only where that rule named a SOLO kernel that was not launched (four-wave CULL and SPILL launches).
// usage: pooled_choice_check
#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "rt_device.hpp"

using rtk::KParams;

// the name api.cpp used to give a render launch (its own restatement of the choice, before choose_pooled)
static std::string old_render_name(const KParams &p, int waves) {
  const bool single_px = p.solo && p.nframes == 1 && p.order != nullptr && p.deep_class > 0 && p.deep_split == 6 && p.tl_log2 == rtk::kTreeletDepth;
  std::string s = p.px_hdr ? (p.donate ? (p.solo ? "ORD+SOLO+DONATE" : "ORD+DONATE") : (p.solo ? "ORD+SOLO" : "ORD"))
                  : (p.cold && waves == 16) ? (single_px ? "COLD+SOLO" : "COLD")
                  : (p.donate && waves == 16) ? (single_px ? "DONATE+SOLO" : "DONATE") : (single_px ? "SOLO" : "plain");
  return s + (p.cull ? "+CULL" : "") + (p.spill ? "+SPILL" : "");
}

int main() {
  static int order_table[1], px_header[1];
  static unsigned spill_region[1];
  static unsigned char occluded[1];
  std::vector<int> reached(rtk::kNumPooledKeys, 0);
  std::map<std::string, int> names;   // name of an accepted render / rays launch -> count
  long cases = 0, accepted = 0, corrected = 0;
  int fails = 0;
  auto fail = [&](const char *what, const KParams &p, int stats, int waves, int rays) {
    if (++fails <= 20)
      std::printf("FAILED: %s (stats %d waves %d rays %d cull %d spill %d capb %d px_hdr %d donate %d cold %d solo %d order %d deep %d/%d tl %d nframes %d lds %d/%d)\n",
                  what, stats, waves, rays, p.cull, p.spill != nullptr, p.capb, p.px_hdr != nullptr, p.donate, p.cold, p.solo, p.order != nullptr,
                  p.deep_class, p.deep_split, p.tl_log2, p.nframes, p.lds_nodes, p.n_nodes);
  };
  const int capbs[] = {0, rtk::kSpillCapb, rtk::kSpillCapbTest, 512};
  for (int stats = 0; stats < 2; ++stats)
  for (int waves : {2, 4, 8, 12, 16, 20})
  for (int rays : {0, rtk::kRaysColour, rtk::kRaysAny})
  for (int cull = 0; cull < 2; ++cull)
  for (int spill = 0; spill < 4; ++spill)   // 0: no spill region; else one with capb = capbs[spill]
  for (int px = 0; px < 2; ++px)
  for (int donate : {0, 64})
  for (int cold : {0, 3})
  for (int solo = 0; solo < 2; ++solo)
  for (int order = 0; order < 2; ++order)
  for (int deep_class : {0, 3})
  for (int deep_split : {2, 6})
  for (int tl : {rtk::kTreeletDepth, rtk::kTreeletDepth - 1})
  for (int nframes : {1, 2})
  for (int all_lds = 0; all_lds < 2; ++all_lds) {
    KParams p{};
    p.n_nodes = 99; p.n_sph = 100;
    p.lds_nodes = all_lds ? 99 : 40; p.lds_sph = all_lds ? 100 : 0;
    p.cull = cull;
    p.spill = spill ? spill_region : nullptr;
    p.capb = capbs[spill];
    p.px_hdr = px ? px_header : nullptr;
    p.donate = donate; p.cold = cold; p.solo = solo;
    p.order = order ? order_table : nullptr;
    p.deep_class = deep_class; p.deep_split = deep_split; p.tl_log2 = tl;
    p.nframes = nframes;
    p.occluded = occluded;
    p.nrays = 64;
    ++cases;
    rtk::PooledKey k{};
    if (!rtk::choose_pooled(p, stats, waves, rays, &k)) continue;
    ++accepted;
    int idx = -1;
    for (int i = 0; i < rtk::kNumPooledKeys; ++i)
      if (rtk::kPooledKeys[i] == k) idx = i;
    if (idx < 0) { fail("accepted, but no compiled instantiation", p, stats, waves, rays); continue; }
    ++reached[idx];
    if (k.threads != 64 * waves && !(stats && waves != 16 && k.threads == 512)) fail("workgroup size", p, stats, waves, rays);
    if (k.rays != rays || k.stats != (stats != 0) || k.cull != (cull != 0) || (k.spill != 0) != (spill != 0)) fail("flags", p, stats, waves, rays);
    if (stats) continue;
    const std::string name = rtk::pooled_name(k);
    ++names[name];
    if (rays) continue;
    const std::string old = old_render_name(p, waves);
    const bool solo_dropped = waves == 4 && (cull || spill) && old.find("SOLO") != std::string::npos;
    if (solo_dropped) {
      ++corrected;
      const std::string fixed = std::string(cull ? "plain+CULL" : "plain") + (spill ? "+SPILL" : "");
      if (k.solo || name != fixed) fail("corrected name", p, stats, waves, rays);
    } else if (name != old) {
      fail(("name " + name + " against " + old).c_str(), p, stats, waves, rays);
    }
  }
  for (int i = 0; i < rtk::kNumPooledKeys; ++i) {
    for (int j = 0; j < i; ++j)
      if (rtk::kPooledKeys[i] == rtk::kPooledKeys[j]) { std::printf("FAILED: kPooledKeys[%d] repeats kPooledKeys[%d]\n", i, j); ++fails; }
    if (!reached[i]) { std::printf("FAILED: kPooledKeys[%d] (%d threads) is never chosen\n", i, rtk::kPooledKeys[i].threads); ++fails; }
  }
  int warmed = 0;
  for (int i = 0; i < rtk::kNumPooledKeys; ++i) warmed += rtk::pooled_warmed(rtk::kPooledKeys[i]);
  if (rtk::kNumPooledKeys != 64 || warmed != 34) { std::printf("FAILED: %d instantiations, %d warmed (want 64, 34)\n", rtk::kNumPooledKeys, warmed); ++fails; }
  // every name a launch can carry, and no other
  const std::set<std::string> want = {"plain", "SOLO", "COLD", "COLD+SOLO", "DONATE", "DONATE+SOLO", "ORD", "ORD+SOLO", "ORD+DONATE", "ORD+SOLO+DONATE",
                                      "plain+CULL", "SOLO+CULL", "COLD+CULL", "COLD+SOLO+CULL", "DONATE+CULL", "DONATE+SOLO+CULL", "ORD+CULL",
                                      "ORD+SOLO+CULL", "ORD+DONATE+CULL", "ORD+SOLO+DONATE+CULL", "plain+SPILL", "plain+CULL+SPILL", "any", "any+SPILL"};
  std::set<std::string> got;
  for (const auto &kv : names) got.insert(kv.first);
  for (const auto &s : want)
    if (!got.count(s)) { std::printf("FAILED: no launch is named %s\n", s.c_str()); ++fails; }
  for (const auto &s : got)
    if (!want.count(s)) { std::printf("FAILED: unexpected name %s\n", s.c_str()); ++fails; }
  std::printf("pooled_choice_check: %ld cases, %ld accepted, %d instantiations all reachable, %d warmed, %zu names, %ld render names corrected (SOLO on four-wave CULL / SPILL): %s\n",
              cases, accepted, rtk::kNumPooledKeys, warmed, got.size(), corrected, fails ? "FAILED" : "passed");
  return fails ? 1 : 0;
}
