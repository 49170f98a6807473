// The contact clusters' union-find (query_core.h: uf_find / uf_unite, what clusters_hook_kernel runs where the count pass counts) on the host:
// the same text behind a std::atomic<int32_t> policy, relaxed throughout.  Built plain by `make`, and with -fsanitize=thread by the CPU suite
// (tests/test_clusters_cpu.py), which runs it as a stand-alone program.
//   clusters_check threads [T]              T (default 16) threads unite the edges of seeded random graphs, a 10^5 chain in shuffled edge order
//                                           and a clique, each thread a strided share; the roots after a sequential flatten, and after the device's in-place flatten by all threads, must equal a plain
//                                           sequential union-find's (the smallest index of every component).  Exit status 1 where they differ.
//   clusters_check mutants                  three wrong unions and a wrong flatten, each run on the case named for it next to the real
//                                           function: exit status 0 iff that passes every case and every mutant is caught by its own.
//   clusters_check edges <n> <edges.bin> <out.bin> [T]   the roots (n int32) of the graph whose edges are the file's int32 pairs, united by T
//                                           (default 4) threads: the CPU suite compares them with tests/clusters_ref.py.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "query_core.h"

using namespace rtk;
using Edge = std::pair<int32_t, int32_t>;

// the host's atomic-ops policy: every access relaxed, as the device's
struct HostOps {
  std::atomic<int32_t> *parent;
  int32_t load(int32_t x) const { return parent[x].load(std::memory_order_relaxed); }
  void store(int32_t x, int32_t v) const { parent[x].store(v, std::memory_order_relaxed); }
  int32_t cas(int32_t x, int32_t expect, int32_t v) const {
    parent[x].compare_exchange_strong(expect, v, std::memory_order_relaxed, std::memory_order_relaxed);
    return expect;
  }
};

// a plain sequential union-find that links by smaller root: the answer every interleaving must reach
static std::vector<int32_t> sequential_roots(int32_t n, const std::vector<Edge> &edges) {
  std::vector<int32_t> parent(n);
  std::iota(parent.begin(), parent.end(), 0);
  auto find = [&](int32_t x) {
    while (parent[x] != x) x = parent[x];
    return x;
  };
  for (const Edge &e : edges) {
    const int32_t a = find(e.first), b = find(e.second);
    if (a != b) parent[std::max(a, b)] = std::min(a, b);
    for (int32_t x : {e.first, e.second}) {   // full compression, so the plain find above stays short
      const int32_t r = std::min(a, b);
      while (parent[x] != r && parent[x] != x) {
        const int32_t next = parent[x];
        parent[x] = r;
        x = next;
      }
    }
  }
  std::vector<int32_t> root(n);
  for (int32_t i = 0; i < n; ++i) root[i] = find(i);
  return root;
}

static std::vector<int32_t> threaded_roots(int32_t n, const std::vector<Edge> &edges, int nthreads) {
  std::vector<std::atomic<int32_t>> parent(n);
  for (int32_t i = 0; i < n; ++i) parent[i].store(i, std::memory_order_relaxed);
  const HostOps ops{parent.data()};
  std::vector<std::thread> pool;
  for (int t = 0; t < nthreads; ++t)
    pool.emplace_back([&, t] {
      // as a lane of the hook: the root so far is kept while consecutive edges share their first vertex
      int32_t at = -1, mine = -1;
      for (size_t k = t; k < edges.size(); k += nthreads) {
        if (edges[k].first != at) at = mine = edges[k].first;
        const int32_t theirs = uf_find(ops, edges[k].second);
        if (theirs != mine) mine = uf_unite(ops, mine, theirs);
      }
    });
  for (std::thread &th : pool) th.join();
  bool kept = true;   // the invariant every word must have kept
  for (int32_t i = 0; i < n; ++i) kept &= ops.load(i) <= i;
  if (!kept) return std::vector<int32_t>(n, -1);
  // the sequential flatten, kept aside ...
  std::vector<int32_t> root(n);
  for (int32_t i = 0; i < n; ++i) root[i] = uf_root(ops, i);
  // ... and the device's: in place, by all threads at once, each word stored by its owner only
  pool.clear();
  for (int t = 0; t < nthreads; ++t)
    pool.emplace_back([&, t] {
      for (int32_t i = t; i < n; i += nthreads) {
        const int32_t r = uf_root(ops, i);
        if (r != i) ops.store(i, r);
      }
    });
  for (std::thread &th : pool) th.join();
  for (int32_t i = 0; i < n; ++i)
    if (ops.load(i) != root[i]) root[i] = -2;
  return root;
}

static bool same(const char *what, const std::vector<int32_t> &got, const std::vector<int32_t> &want) {
  size_t bad = 0;
  for (size_t i = 0; i < want.size(); ++i) bad += got[i] != want[i];
  size_t clusters = 0;
  for (size_t i = 0; i < want.size(); ++i) clusters += want[i] == (int32_t)i;
  printf("%-28s n=%zu clusters=%zu differ=%zu\n", what, want.size(), clusters, bad);
  return bad == 0;
}

static int run_threads(int nthreads) {
  bool ok = true;
  std::mt19937 rng(20240611u);
  // seeded random graphs around the percolation threshold (m ~ n / 2), sparser and denser
  for (const auto &[n, m] : std::vector<std::pair<int32_t, size_t>>{{1000, 300}, {1000, 500}, {20000, 10000}, {20000, 40000}, {300, 20000}}) {
    std::vector<Edge> edges(m);
    for (Edge &e : edges) {
      const int32_t a = (int32_t)(rng() % (uint32_t)n), b = (int32_t)(rng() % (uint32_t)n);
      e = {std::min(a, b), std::max(a, b)};   // (a == b: a self edge, which unites nothing)
    }
    const std::string what = "random n=" + std::to_string(n) + " m=" + std::to_string(m);
    ok &= same(what.c_str(), threaded_roots(n, edges, nthreads), sequential_roots(n, edges));
  }
  {   // a 10^5 chain, its edges in shuffled order: the deepest trees
    const int32_t n = 100000;
    std::vector<Edge> edges;
    for (int32_t i = 0; i + 1 < n; ++i) edges.push_back({i, i + 1});
    std::shuffle(edges.begin(), edges.end(), rng);
    ok &= same("chain 1e5 shuffled", threaded_roots(n, edges, nthreads), std::vector<int32_t>(n, 0));
  }
  {   // a clique: every thread contends on one word
    const int32_t n = 400;
    std::vector<Edge> edges;
    for (int32_t i = 0; i < n; ++i)
      for (int32_t j = i + 1; j < n; ++j) edges.push_back({i, j});
    ok &= same("clique 400", threaded_roots(n, edges, nthreads), std::vector<int32_t>(n, 0));
  }
  return ok ? 0 : 1;
}

// ---- the mutants: a plain array, and one scripted step of "another lane" between a union's finds and its compare-exchange
struct ScriptOps {
  int32_t *parent;
  std::function<void()> *before_cas;   // run once, ahead of the first cas or hooking store
  void interpose() const {
    if (*before_cas) {
      const std::function<void()> f = std::move(*before_cas);
      *before_cas = nullptr;
      f();
    }
  }
  int *stores_until_script = nullptr;  // or: run it ahead of the store that counts this down to 0
  int32_t load(int32_t x) const { return parent[x]; }
  void store(int32_t x, int32_t v) const {
    if (stores_until_script && --*stores_until_script == 0) interpose();
    parent[x] = v;
  }
  int32_t cas(int32_t x, int32_t expect, int32_t v) const {
    interpose();
    const int32_t seen = parent[x];
    if (seen == expect) parent[x] = v;
    return seen;
  }
};
enum Mutant { kReal = 0, kSmallerUnderLarger, kNoRetry, kHookNonRoot };
static const char *const kMutantName[] = {"uf_unite", "linking smaller under larger", "not retrying a failed CAS", "hooking a non-root"};
static void unite_as(Mutant m, const ScriptOps &a, int32_t x, int32_t y) {
  if (m == kReal) {
    (void)uf_unite(a, x, y);
    return;
  }
  for (;;) {
    if (m != kHookNonRoot) x = uf_find(a, x), y = uf_find(a, y);   // kHookNonRoot: the vertices themselves, whatever hangs them
    if (x == y) return;
    if ((x > y) != (m == kSmallerUnderLarger)) std::swap(x, y);      // y: the one to be hooked
    if (m == kHookNonRoot) {
      a.interpose();
      a.store(y, x);
      return;
    }
    const int32_t seen = a.cas(y, y, x);
    if (seen == y || m == kNoRetry) return;
    y = seen;
  }
}
struct Case {
  const char *name;
  int32_t n;
  std::vector<Edge> before;     // united first, by uf_unite
  Edge racing;                  // the union under test ...
  std::vector<Edge> foreign;    // ... with these united by another lane (uf_unite) between its finds and its hook
};
static bool case_passes(Mutant m, const Case &c) {
  std::vector<int32_t> parent(c.n);
  std::iota(parent.begin(), parent.end(), 0);
  std::function<void()> script;
  const ScriptOps ops{parent.data(), &script};
  std::vector<Edge> all = c.before;
  for (const Edge &e : c.before) unite_as(m, ops, e.first, e.second);
  script = [&] {
    for (const Edge &e : c.foreign) (void)uf_unite(ops, e.first, e.second);
  };
  unite_as(m, ops, c.racing.first, c.racing.second);
  ops.interpose();   // (a union that never reached its hook: the other lane runs afterwards)
  all.push_back(c.racing);
  all.insert(all.end(), c.foreign.begin(), c.foreign.end());
  const std::vector<int32_t> want = sequential_roots(c.n, all);
  for (int32_t i = 0; i < c.n; ++i) {
    if (parent[i] > i) return false;
    int32_t x = i;
    for (int32_t steps = 0; parent[x] != x; x = parent[x])
      if (++steps > c.n) return false;
    if (x != want[i]) return false;
  }
  return true;
}
// The flatten: the chain 0 <- 1 <- 2 <- 3 <- 4 <- 5, vertex 5's lane walking while vertex 3's owner stores its root.  A walk that halves
// (uf_find) re-points 3 at its grandparent BEHIND the owner's store and leaves a non-root in the answer; uf_root stores nothing on the way.
static bool flatten_case_passes(bool halving) {
  std::vector<int32_t> parent = {0, 0, 1, 2, 3, 4};
  std::function<void()> script;
  int countdown = 2;   // (the halving walk's second store is the one to word 3)
  const ScriptOps ops{parent.data(), &script, &countdown};
  script = [&] { parent[3] = 0; };   // vertex 3's owner: its root, stored once
  const int32_t r = halving ? uf_find(ops, 5) : uf_root(ops, 5);
  ops.store(5, r);
  ops.interpose();
  return r == 0 && parent[3] == 0 && parent[5] == 0;
}

static int run_mutants() {
  const Case cases[] = {
      {"", 0, {}, {0, 0}, {}},
      // 0-1 then 1-2: the root must be the smallest index, 0
      {"min_root", 3, {{0, 1}}, {1, 2}, {}},
      // 0-2 races with another lane's 1-2: the cas on 2 fails, and the edge 0-2 must still be united
      {"lost_race", 3, {}, {0, 2}, {{1, 2}}},
      // 1-2 is united, then 0-2: 2 is no root any more; re-pointing it drops 1
      {"overwritten_link", 3, {{1, 2}}, {0, 2}, {}},
  };
  bool ok = true;
  for (int k = 1; k <= 3; ++k) {
    const bool real = case_passes(kReal, cases[k]), mutant = case_passes(static_cast<Mutant>(k), cases[k]);
    printf("case %-17s uf_unite %s; mutant '%s' %s\n", cases[k].name, real ? "passes" : "FAILS", kMutantName[k], mutant ? "NOT CAUGHT" : "caught");
    ok &= real && !mutant;
  }
  const bool real = flatten_case_passes(false), mutant = flatten_case_passes(true);
  printf("case %-17s uf_root %s; mutant '%s' %s\n", "late_halving", real ? "passes" : "FAILS", "halving while flattening",
         mutant ? "NOT CAUGHT" : "caught");
  ok &= real && !mutant;
  return ok ? 0 : 1;
}

static int run_edges(int32_t n, const char *in_path, const char *out_path, int nthreads) {
  FILE *in = fopen(in_path, "rb");
  if (!in) {
    fprintf(stderr, "clusters_check: cannot read %s\n", in_path);
    return 2;
  }
  std::vector<Edge> edges;
  int32_t row[2];
  while (fread(row, sizeof(int32_t), 2, in) == 2) {
    if (row[0] < 0 || row[0] >= n || row[1] < 0 || row[1] >= n) {
      fprintf(stderr, "clusters_check: edge (%d, %d) outside [0, %d)\n", row[0], row[1], n);
      fclose(in);
      return 2;
    }
    edges.push_back({row[0], row[1]});
  }
  fclose(in);
  const std::vector<int32_t> root = threaded_roots(n, edges, nthreads);
  FILE *o = fopen(out_path, "wb");
  if (!o || fwrite(root.data(), sizeof(int32_t), root.size(), o) != root.size()) {
    fprintf(stderr, "clusters_check: cannot write %s\n", out_path);
    return 2;
  }
  fclose(o);
  printf("%zu edges over %d vertices, %d threads\n", edges.size(), n, nthreads);
  return 0;
}

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "threads" && argc <= 3) return run_threads(argc == 3 ? std::max(1, atoi(argv[2])) : 16);
  if (mode == "mutants" && argc == 2) return run_mutants();
  if (mode == "edges" && (argc == 5 || argc == 6)) {
    const int32_t n = atoi(argv[2]);
    if (n < 1) return 2;
    return run_edges(n, argv[3], argv[4], argc == 6 ? std::max(1, atoi(argv[5])) : 4);
  }
  fprintf(stderr, "usage: clusters_check threads [T] | mutants | edges <n> <edges.bin> <out.bin> [T]\n");
  return 2;
}
