// The sphere groups' rule, combine and climb (query_core.h: group_seen, group_combine, group_climb -- what the masked lanes and the derive
// kernel run) on the host, over cases read from a file: the CPU suite holds the numpy restatement (tests/groups_ref.py) equal to this code
// without a GPU.  The file is 32-bit words:
//   P, then P pairs {group word, mask}
//   n, then left[n - 1], right[n - 1], parent[n - 1] (int32, the encoding of rt_prepared_get_bvh: a leaf j is -2 - j, the root's parent < 0),
//   groups[n] in L order, order[n - 1]: the inner nodes in the order in which their climbs are run (a permutation: the result may not
//   depend on it)
// Written: per pair {group_seen, group_combine of the two words}, then the n - 1 node words after every climb.
// usage: groups_check <cases.bin> <out.bin>     (a stand-alone host program: this is the place for a -fsanitize=address,undefined build)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "query_core.h"

using namespace rtk;

namespace {
// plain words on one host thread: the host's memory policy of group_climb
struct HostOps {
  uint32_t *words;
  const int32_t *up;
  uint32_t fetch_or(int32_t v, uint32_t bits) const {
    const uint32_t old = words[v];
    words[v] = old | bits;
    return old;
  }
  int32_t parent(int32_t v) const { return up[v]; }
};
}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: groups_check <cases.bin> <out.bin>\n");
    return 2;
  }
  FILE *in = fopen(argv[1], "rb");
  if (!in) {
    fprintf(stderr, "groups_check: cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<uint32_t> w;
  uint32_t x;
  while (fread(&x, 4, 1, in) == 1) w.push_back(x);
  fclose(in);
  size_t at = 0;
  auto bad = [&](const char *what) {
    fprintf(stderr, "groups_check: malformed file (%s)\n", what);
    return 2;
  };
  if (w.empty()) return bad("empty");
  const size_t P = w[at++];
  if (w.size() < at + 2 * P + 1) return bad("pairs");
  std::vector<uint32_t> out;
  size_t seen = 0;
  for (size_t i = 0; i < P; ++i) {
    const uint32_t g = w[at + 2 * i], m = w[at + 2 * i + 1];
    out.push_back(group_seen(g, m) ? 1u : 0u);
    out.push_back(group_combine(g, m));
    seen += out[2 * i];
  }
  at += 2 * P;
  const size_t n = w[at++];
  if (n < 2 || w.size() != at + 4 * (n - 1) + n) return bad("tree");
  const size_t ni = n - 1;
  std::vector<int32_t> left(ni), right(ni), up(ni), order(ni);
  for (size_t v = 0; v < ni; ++v) {
    left[v] = static_cast<int32_t>(w[at + v]);
    right[v] = static_cast<int32_t>(w[at + ni + v]);
    up[v] = static_cast<int32_t>(w[at + 2 * ni + v]);
    order[v] = static_cast<int32_t>(w[at + 3 * ni + n + v]);
  }
  const uint32_t *groups = &w[at + 3 * ni];
  std::vector<uint32_t> words(ni, 0u);
  const HostOps ops{words.data(), up.data()};
  for (size_t v = 0; v < ni; ++v)
    if (up[v] >= static_cast<int32_t>(ni)) return bad("parent index");
  for (size_t q = 0; q < ni; ++q) {
    const int32_t v = order[q];
    if (v < 0 || static_cast<size_t>(v) >= ni) return bad("node index");
    uint32_t leaf[2] = {0u, 0u};
    const int32_t kids[2] = {left[v], right[v]};
    for (int k = 0; k < 2; ++k)
      if (kids[k] <= -2) {
        const size_t j = static_cast<size_t>(-2 - static_cast<int64_t>(kids[k]));
        if (j >= n) return bad("leaf index");
        leaf[k] = groups[j];
      }
    group_climb(ops, v, group_combine(leaf[0], leaf[1]));
  }
  out.insert(out.end(), words.begin(), words.end());
  FILE *o = fopen(argv[2], "wb");
  if (!o || fwrite(out.data(), sizeof(uint32_t), out.size(), o) != out.size()) {
    fprintf(stderr, "groups_check: cannot write %s\n", argv[2]);
    return 2;
  }
  fclose(o);
  printf("%zu pairs (%zu seen), a tree of %zu spheres: root word %08x\n", P, seen, n, words[0]);
  return 0;
}
