// queue_check.cpp -- plays the tile-queue protocol of the pooled kernel on the CPU.
//
// The kernel's ticket arithmetic lives in rt_device.hpp as __host__ __device__ functions (shard_of, shard_tile,
// shard_tickets, ticket_span, queue_draw); this program drives exactly those with W emulated waves in a random
// interleaving and checks, for many random launch shapes, that
//   * every pixel slot of every position (tile x frame) is handed out exactly once,
//   * positions map to tiles one-to-one (the strips partition the tile grid),
//   * every wave ends with all shards seen dry, having failed at most once per counter,
//   * no counter is touched for a shard whose tickets are all static.
// Host-only (no GPU needed); part of the CPU test suite (tests/test_host_logic.py).
//
//   queue_check [cases [seed]]   the production shapes, then `cases` random launch shapes and as many pixel-ticket lists
//   queue_check extreme          the tile grids of strip images and of the first order's limits (1 x 8192 ... 131072 x 1), each under one counter,
//                                eight strips and eight counters taking turns, with 4096 and with 5120 waves, and as a batch; same checks, and the
//                                strips of a grid narrower than eight tiles must be empty with their counters untouched
//   queue_check span NTILES NFRAMES DS TPT N_DEEP N_SPLIT
//                                no per-slot memory: every ticket of one shard of NTILES x NFRAMES positions once, ticket_span's 32-bit q_next / q_end
//                                against the same formula in uint64_t (the bound of a pooled launch: tiles x frames < 2^26); prints the number of tickets that differ
// (tests/test_frame_edges_cpu.py runs the last two)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "rt_device.hpp"

using namespace rtk;

struct Cfg {
  int tiles_x, tiles_y, ns_log2, nframes, ds, tpt, deep_class, waves, static_first, interleave;
  int cap_log2 = 5;
};

static int run(const Cfg &c, std::mt19937 &rng, bool verbose, int *empty_untouched = nullptr) {
  const int ns = 1 << c.ns_log2;                 // counters
  const int gl2 = c.interleave ? 0 : c.ns_log2;  // log2 of the shards of the GEOMETRY (strips, order table)
  const int gs = 1 << gl2;
  const int ntiles = c.tiles_x * c.tiles_y;
  // a synthetic order table: the identity within each strip + class tables with random deep counts
  std::vector<int> order(static_cast<size_t>(order_table_ints(ntiles)), 0);
  std::vector<int> seen_tile(static_cast<size_t>(ntiles), 0);
  for (int s = 0; s < gs; ++s) {
    const Shard sh = shard_of(s, gl2, c.tiles_x, c.tiles_y);
    for (int k = 0; k < sh.ntiles; ++k) {
      const int tile = shard_tile(sh, k, c.tiles_x);
      if (tile < 0 || tile >= ntiles) { std::printf("tile out of range\n"); return 1; }
      order[static_cast<size_t>(sh.seg + k)] = tile;
      seen_tile[static_cast<size_t>(tile)]++;
    }
    int *tab = order.data() + ntiles + kOrderTableDw * s;
    int acc = 0;
    for (int cl = 0; cl < 8; ++cl) {          // non-decreasing class starts, the last one the tile count
      tab[cl] = acc;
      if (sh.ntiles > acc) acc += static_cast<int>(rng() % static_cast<unsigned>(sh.ntiles - acc + 1)) / (cl < 3 ? 8 : 2);
    }
    tab[0] = 0;
    tab[8] = sh.ntiles;
  }
  for (int t = 0; t < ntiles; ++t)
    if (seen_tile[static_cast<size_t>(t)] != 1) { std::printf("tile %d in %d strips\n", t, seen_tile[static_cast<size_t>(t)]); return 1; }

  QueueConst qc;
  qc.ns_log2 = c.ns_log2; qc.tiles_x = c.tiles_x; qc.tiles_y = c.tiles_y; qc.nframes = c.nframes;
  qc.ds = c.ds; qc.tpt = c.tpt; qc.cap_log2 = c.cap_log2; qc.ntiles = ntiles; qc.interleave = c.interleave;
  const bool deep_on = c.nframes == 1 && c.deep_class > 0;
  qc.order = deep_on ? order.data() : nullptr; qc.deep_class = c.deep_class;
  qc.px = nullptr;
  qc.home_waves = static_cast<unsigned>(c.waves >> c.ns_log2);
  qc.q_static = c.static_first ? qc.home_waves : 0u;

  std::vector<unsigned> counter(static_cast<size_t>(ns), 0u), draws(static_cast<size_t>(ns), 0u);
  std::vector<unsigned char> cover(static_cast<size_t>(ntiles) * c.nframes * 64, 0);
  // waves: workgroup b = w / wpw, wave-in-workgroup = w % wpw; wpw = 4, grid = waves / 4 (a multiple of ns)
  const int wpw = 4, grid = c.waves / wpw;
  struct Wave { unsigned state; bool done; unsigned rank; std::vector<int> fails; };
  std::vector<Wave> wv(static_cast<size_t>(c.waves));
  for (int w = 0; w < c.waves; ++w) {
    const int b = w / wpw, wi = w % wpw;
    wv[static_cast<size_t>(w)].state = queue_state_init(b & (ns - 1), c.static_first != 0);
    wv[static_cast<size_t>(w)].done = false;
    wv[static_cast<size_t>(w)].rank = static_cast<unsigned>(wi) * static_cast<unsigned>(grid >> c.ns_log2) + static_cast<unsigned>(b >> c.ns_log2);
    wv[static_cast<size_t>(w)].fails.assign(static_cast<size_t>(ns), 0);
  }
  std::vector<int> alive(static_cast<size_t>(c.waves));
  for (int w = 0; w < c.waves; ++w) alive[static_cast<size_t>(w)] = w;
  unsigned long long tickets_taken = 0;
  while (!alive.empty()) {
    const size_t pick = rng() % alive.size();
    Wave &W = wv[static_cast<size_t>(alive[pick])];
    TicketSpan sp;
    const bool got = queue_draw(W.state, qc, W.rank, [&](int shard) {
      draws[static_cast<size_t>(shard)]++;
      return counter[static_cast<size_t>(shard)]++;
    }, &sp);
    if (!got) {
      if (((W.state >> 8) & 0xffu) != ((1u << ns) - 1u)) { std::printf("wave left with live shards\n"); return 1; }
      alive[pick] = alive.back();
      alive.pop_back();
      continue;
    }
    tickets_taken++;
    if (sp.q_end <= sp.q_next || sp.q_end > cover.size()) { std::printf("bad span [%u, %u) of %zu\n", sp.q_next, sp.q_end, cover.size()); return 1; }
    // the span lies in the shard the wave is drawing from
    const Shard sh = shard_of(queue_geo_shard(qc, W.state), gl2, c.tiles_x, c.tiles_y);
    if ((sp.q_next >> 6) < static_cast<unsigned>(sh.seg) * 1u || ((sp.q_end - 1) >> 6) >= static_cast<unsigned>(sh.seg + sh.ntiles * c.nframes)) {
      std::printf("span outside its shard\n");
      return 1;
    }
    for (unsigned i = sp.q_next; i < sp.q_end; ++i) {
      if (cover[i]) { std::printf("pixel slot %u handed out twice\n", i); return 1; }
      cover[i] = 1;
    }
  }
  for (size_t i = 0; i < cover.size(); ++i)
    if (!cover[i]) { std::printf("pixel slot %zu never handed out (cfg %d x %d ns %d nf %d ds %d tpt %d dc %d W %d sf %d)\n", i, c.tiles_x, c.tiles_y, ns, c.nframes, c.ds, c.tpt, c.deep_class, c.waves, c.static_first); return 1; }
  // counter draws: successes + at most one failure per wave per shard; none on a shard without dynamic tickets
  for (int s = 0; s < ns; ++s) {
    const int geo = c.interleave ? 0 : s;
    const Shard sh = shard_of(geo, gl2, c.tiles_x, c.tiles_y);
    const int ndeep = queue_ndeep(qc, geo);
    const unsigned n_split = queue_nsplit(qc, ndeep);
    unsigned tk = shard_tickets(static_cast<unsigned>(sh.ntiles) * c.nframes, n_split, static_cast<unsigned>(ndeep), c.ds, c.tpt);
    if (c.interleave) tk = (tk + static_cast<unsigned>(ns) - 1u - static_cast<unsigned>(s)) >> c.ns_log2;
    const unsigned dyn = tk > qc.q_static ? tk - qc.q_static : 0u;
    if (dyn == 0 && draws[static_cast<size_t>(s)] != 0) { std::printf("counter of an all-static shard was drawn from\n"); return 1; }
    if (empty_untouched && sh.ntiles == 0 && draws[static_cast<size_t>(s)] == 0 && counter[static_cast<size_t>(s)] == 0) ++*empty_untouched;
    if (dyn != 0 && (draws[static_cast<size_t>(s)] < dyn || draws[static_cast<size_t>(s)] > dyn + static_cast<unsigned>(c.waves))) {
      std::printf("shard %d: %u draws for %u dynamic tickets and %d waves\n", s, draws[static_cast<size_t>(s)], dyn, c.waves);
      return 1;
    }
  }
  if (verbose) std::printf("ok: %dx%d tiles, %d counter(s)%s, %d frame(s), ds %d, tpt %d, %d waves, static %d: %llu tickets\n", c.tiles_x, c.tiles_y, ns,
                           c.interleave ? " taking turns" : (ns > 1 ? ", a strip each" : ""), c.nframes, c.ds, c.tpt, c.waves, c.static_first, tickets_taken);
  return 0;
}

// Pixel tickets (rt_device.hpp: px_make_header / px_ticket_span through queue_draw): a random list of `npix` pixels cut into the
// five classes at random positions; every list position is handed out exactly once, a ticket of class k covers at most
// 1 << px_log2(k) positions of class k's segment, and every ticket of a class but its last one is full.
static int run_px(std::mt19937 &rng, bool verbose) {
  const int npix = 1 + static_cast<int>(rng() % 20000);
  int pos[kPxClasses + 1];
  pos[0] = 0;
  pos[kPxClasses] = npix;
  for (int k = 1; k < kPxClasses; ++k) pos[k] = static_cast<int>(rng() % static_cast<unsigned>(npix + 1)) / ((rng() & 1) ? 1 : 16);
  for (int k = 1; k < kPxClasses; ++k) if (pos[k] < pos[k - 1]) pos[k] = pos[k - 1];
  int hdr[kPxHdrInts];
  px_make_header(pos, hdr);
  hdr[7] = static_cast<int>(rng() & 1);      // the bulk zipped or not
  QueueConst qc{};
  qc.ns_log2 = (rng() & 1) ? 3 : 0;
  qc.interleave = qc.ns_log2 == 3;
  qc.tiles_x = 1 + static_cast<int>(rng() % 40); qc.tiles_y = 1 + static_cast<int>(rng() % 40); qc.nframes = 1;   // (unused by pixel tickets)
  qc.ds = static_cast<int>(rng() % 7); qc.tpt = static_cast<int>(rng() % 3); qc.cap_log2 = 5; qc.ntiles = qc.tiles_x * qc.tiles_y;
  qc.order = nullptr; qc.deep_class = 0; qc.px = hdr;
  const int waves = 32 * (1 + static_cast<int>(rng() % 40)), ns = 1 << qc.ns_log2;
  const int static_first = static_cast<int>(rng() & 1);
  qc.home_waves = static_cast<unsigned>(waves >> qc.ns_log2);
  qc.q_static = static_first ? qc.home_waves : 0u;
  std::vector<unsigned> counter(static_cast<size_t>(ns), 0u);
  std::vector<unsigned char> cover(static_cast<size_t>(npix), 0);
  const int wpw = 4, grid = waves / wpw;
  struct Wave { unsigned state, rank; };
  std::vector<Wave> wv(static_cast<size_t>(waves));
  std::vector<int> alive(static_cast<size_t>(waves));
  for (int w = 0; w < waves; ++w) {
    const int b = w / wpw, wi = w % wpw;
    wv[static_cast<size_t>(w)].state = queue_state_init(b & (ns - 1), static_first != 0);
    wv[static_cast<size_t>(w)].rank = static_cast<unsigned>(wi) * static_cast<unsigned>(grid >> qc.ns_log2) + static_cast<unsigned>(b >> qc.ns_log2);
    alive[static_cast<size_t>(w)] = w;
  }
  unsigned long long taken = 0;
  while (!alive.empty()) {
    const size_t pick = rng() % alive.size();
    Wave &W = wv[static_cast<size_t>(alive[pick])];
    TicketSpan sp;
    if (!queue_draw(W.state, qc, W.rank, [&](int shard) { return counter[static_cast<size_t>(shard)]++; }, &sp)) {
      alive[pick] = alive.back();
      alive.pop_back();
      continue;
    }
    taken++;
    const int k = static_cast<int>(sp.cls);
    if (k < 0 || k >= kPxClasses || sp.q_end <= sp.q_next || sp.q_next < static_cast<unsigned>(pos[k]) || sp.q_end > static_cast<unsigned>(pos[k + 1]) ||
        sp.q_end - sp.q_next > (1u << px_log2(k)) || (sp.q_end - sp.q_next < (1u << px_log2(k)) && sp.q_end != static_cast<unsigned>(pos[k + 1]))) {
      std::printf("pixel ticket: bad span [%u, %u) of class %d (segment [%d, %d))\n", sp.q_next, sp.q_end, k, pos[k], pos[k + 1]);
      return 1;
    }
    for (unsigned i = sp.q_next; i < sp.q_end; ++i) {
      if (cover[i]) { std::printf("pixel ticket: list position %u handed out twice\n", i); return 1; }
      cover[i] = 1;
    }
  }
  for (int i = 0; i < npix; ++i)
    if (!cover[static_cast<size_t>(i)]) { std::printf("pixel ticket: list position %d never handed out\n", i); return 1; }
  if (taken != static_cast<unsigned long long>(hdr[8 + kPxClasses])) { std::printf("pixel tickets: %llu taken, header says %d\n", taken, hdr[8 + kPxClasses]); return 1; }
  if (verbose) std::printf("ok: pixel tickets, %d pixels, classes at %d %d %d %d, %d counter(s), %d waves, static %d: %llu tickets\n", npix, pos[1], pos[2], pos[3],
                           pos[4], ns, waves, static_first, taken);
  return 0;
}

// The grids of strip images and of the first order's limits (tiles_x x tiles_y), as the launch shapes take them: 16 waves per CU (4096) and twenty (5120)
static int run_extreme() {
  std::mt19937 rng(1u);
  const int grids[][2] = {{1, 8192}, {8192, 1}, {1, 131072}, {131072, 1}, {32768, 2}, {2, 4096}};
  int n = 0;
  for (const auto &g : grids) {
    for (int waves : {4096, 5120}) {
      for (int mode = 0; mode < 3; ++mode) {   // one counter; eight strips; eight counters taking turns
        Cfg c{g[0], g[1], mode ? 3 : 0, 1, 2, 0, 3, waves, 1, mode == 2 ? 1 : 0};
        int empty = 0;
        if (run(c, rng, true, &empty)) return 1;
        // (strips: shard s holds the tile columns [s tiles_x / 8, (s + 1) tiles_x / 8): a grid of fewer than eight columns leaves 8 - tiles_x of them empty)
        const int want = mode == 1 && g[0] < 8 ? 8 - g[0] : 0;
        if (empty != want) { std::printf("%d x %d tiles, mode %d: %d empty untouched shards, expected %d\n", g[0], g[1], mode, empty, want); return 1; }
        ++n;
      }
      // a batch (one counter, two tiles per ticket; no deep tiles: they are a single frame's)
      Cfg b{g[0], g[1], 0, 3, 2, 1, 3, waves, 1, 0};
      if (run(b, rng, true)) return 1;
      ++n;
    }
  }
  std::printf("queue_check: %d extreme cases passed\n", n);
  return 0;
}

// ticket_span in 64 bits: the same three kinds of ticket, no wrap
static void ticket_span64(uint64_t t, uint64_t seg, uint64_t npos, uint64_t n_split, uint64_t n_deep, int ds, int tpt, uint64_t *q_next, uint64_t *q_end) {
  if (t < (n_split << ds)) {
    const uint64_t piece = 64u >> ds;
    *q_next = (seg + (t >> ds)) * 64u + (t & ((uint64_t(1) << ds) - 1u)) * piece;
    *q_end = *q_next + piece;
    return;
  }
  t -= n_split << ds;
  if (t < n_deep - n_split) {
    *q_next = (seg + n_split + t) * 64u;
    *q_end = *q_next + 64u;
    return;
  }
  const uint64_t k0 = n_deep + ((t - (n_deep - n_split)) << tpt);
  const uint64_t k1 = k0 + (uint64_t(1) << tpt) < npos ? k0 + (uint64_t(1) << tpt) : npos;
  *q_next = (seg + k0) * 64u;
  *q_end = (seg + k1) * 64u;
}

static int run_span(int argc, char **argv) {
  if (argc != 8) { std::printf("usage: queue_check span NTILES NFRAMES DS TPT N_DEEP N_SPLIT\n"); return 2; }
  const uint64_t ntiles = std::strtoull(argv[2], nullptr, 10), nframes = std::strtoull(argv[3], nullptr, 10);
  const int ds = std::atoi(argv[4]), tpt = std::atoi(argv[5]);
  const uint64_t n_deep = std::strtoull(argv[6], nullptr, 10), n_split = std::strtoull(argv[7], nullptr, 10);
  const uint64_t npos = ntiles * nframes;
  if (npos == 0 || npos >= (uint64_t(1) << 32) || ds < 0 || ds > 6 || tpt < 0 || tpt > 4 || n_split > n_deep || n_deep > npos) { std::printf("span: bad arguments\n"); return 2; }
  const uint64_t tickets = (n_split << ds) + (n_deep - n_split) + ((npos - n_deep + (uint64_t(1) << tpt) - 1u) >> tpt);
  const unsigned tickets32 = shard_tickets(static_cast<unsigned>(npos), static_cast<unsigned>(n_split), static_cast<unsigned>(n_deep), ds, tpt);
  uint64_t differ = 0, first = 0, covered = 0;
  unsigned got_next = 0, got_end = 0;
  uint64_t want_next = 0, want_end = 0;
  for (uint64_t t = 0; t < tickets; ++t) {
    const TicketSpan sp = ticket_span(static_cast<unsigned>(t), 0u, static_cast<unsigned>(npos), static_cast<unsigned>(n_split), static_cast<unsigned>(n_deep), ds, tpt);
    uint64_t qn, qe;
    ticket_span64(t, 0, npos, n_split, n_deep, ds, tpt, &qn, &qe);
    covered += qe - qn;
    if (sp.q_next != qn || sp.q_end != qe) {
      if (!differ) { first = t; got_next = sp.q_next; got_end = sp.q_end; want_next = qn; want_end = qe; }
      ++differ;
    }
  }
  if (covered != npos * 64u) { std::printf("span: the 64-bit formula covers %llu slots of %llu\n", (unsigned long long)covered, (unsigned long long)(npos * 64u)); return 1; }
  std::printf("span: positions=%llu tickets=%llu tickets32=%u differ=%llu", (unsigned long long)npos, (unsigned long long)tickets, tickets32, (unsigned long long)differ);
  if (differ) std::printf(" first=%llu got=[%u,%u) want=[%llu,%llu)", (unsigned long long)first, got_next, got_end, (unsigned long long)want_next, (unsigned long long)want_end);
  std::printf("\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "extreme") == 0) return run_extreme();
  if (argc > 1 && std::strcmp(argv[1], "span") == 0) return run_span(argc, argv);
  const int cases = argc > 1 ? std::atoi(argv[1]) : 2000;
  const unsigned seed = argc > 2 ? static_cast<unsigned>(std::atoi(argv[2])) : 1u;
  std::mt19937 rng(seed);
  // the production shapes first
  const Cfg fixed[] = {
      {125, 125, 0, 1, 2, 0, 3, 4096, 1, 0},  {125, 125, 3, 1, 2, 0, 3, 4096, 1, 0}, {125, 125, 0, 20, 2, 2, 3, 4096, 1, 0},
      {500, 500, 3, 1, 2, 2, 3, 4096, 1, 0},  {500, 63, 3, 1, 2, 2, 3, 2048, 1, 0},  {250, 250, 0, 1, 2, 2, 3, 4096, 0, 0},
      {1, 1, 0, 1, 2, 0, 3, 4096, 1, 0},      {3, 2, 3, 1, 2, 0, 3, 64, 1, 0},       {25, 25, 3, 1, 0, 0, 0, 1024, 1, 0},
      {125, 125, 3, 1, 2, 0, 3, 4096, 1, 1},  {500, 500, 3, 1, 2, 1, 3, 4096, 1, 1}, {3, 2, 3, 1, 2, 0, 3, 64, 0, 1},
  };
  for (const Cfg &c : fixed)
    if (run(c, rng, true)) return 1;
  for (int i = 0; i < cases; ++i) {
    Cfg c;
    c.tiles_x = 1 + static_cast<int>(rng() % 40);
    c.tiles_y = 1 + static_cast<int>(rng() % 40);
    c.ns_log2 = (rng() & 1) ? 3 : 0;
    c.nframes = (c.ns_log2 == 0 && (rng() % 3) == 0) ? 1 + static_cast<int>(rng() % 5) : 1;
    c.ds = static_cast<int>(rng() % 7);
    c.cap_log2 = static_cast<int>(rng() % 6);
    c.tpt = static_cast<int>(rng() % 5);
    c.deep_class = static_cast<int>(rng() % 5);
    c.waves = 32 * (1 + static_cast<int>(rng() % 40));   // workgroups of 4 waves, a multiple of 8 workgroups
    c.static_first = static_cast<int>(rng() & 1);
    c.interleave = (c.ns_log2 == 3 && (rng() & 1)) ? 1 : 0;
    if (run(c, rng, false)) {
      std::printf("FAILED case %d (seed %u)\n", i, seed);
      return 1;
    }
  }
  for (int i = 0; i < cases; ++i)
    if (run_px(rng, i < 3)) {
      std::printf("FAILED pixel-ticket case %d (seed %u)\n", i, seed);
      return 1;
    }
  std::printf("queue_check: %d random cases + %zu fixed ones passed\n", cases, sizeof(fixed) / sizeof(fixed[0]));
  return 0;
}
