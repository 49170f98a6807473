// The host-side predicates behind the ENTRY kernels of the pooled family (rt_device.hpp), printed for tests/test_batch_trim_cpu.py: no HIP runtime calls.
//   batch_trim_check keys                               every compiled key: "<name> threads=.. all_lds=.. ... entry_ok=0|1"
//   batch_trim_check flags LEAF_BOX DARK                "const=0|1": may the launch take a kernel that has both flags compiled in?
//   batch_trim_check colbytes NODES SPH CAPB CAPL PLANES     "bytes=<pooled_col_lds_bytes> wave=<bytes of one wave's region>"
//   batch_trim_check fits COL_LDS_BYTES LIMIT           "fits=0|1"
//   batch_trim_check bits MODE LEAF_BOX DARK COL_LDS_BYTES LIMIT COL_LDS     "entry=<the ENTRY template value> mode=.. col_lds=.. rt_flags=.."
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rt_device.hpp"

int main(int argc, char **argv) {
  using namespace rtk;
  auto arg = [&](int i) { return i < argc ? std::atoll(argv[i]) : 0ll; };
  if (argc >= 2 && !std::strcmp(argv[1], "keys")) {
    for (int i = 0; i < kNumPooledKeys; ++i) {
      const PooledKey &k = kPooledKeys[i];
      std::printf("%s threads=%d all_lds=%d stats=%d solo=%d tail=%d ord=%d cull=%d spill=%d rays=%d presort=%d leaf_box=%d entry_ok=%d\n", pooled_name(k).c_str(), k.threads,
                  k.all_lds, k.stats, k.solo, k.tail, k.ord, k.cull, k.spill, k.rays, pooled_presort(k), pooled_leaf_box(k), pooled_entry_ok(k));
    }
    return 0;
  }
  if (argc == 4 && !std::strcmp(argv[1], "flags")) {
    std::printf("const=%d\n", pooled_entry_flags_const((int)arg(2), (int)arg(3)));
    return 0;
  }
  if (argc == 7 && !std::strcmp(argv[1], "colbytes")) {
    std::printf("bytes=%zu wave=%zu\n", pooled_col_lds_bytes((int)arg(2), (int)arg(3), (int)arg(4), (int)arg(5), (int)arg(6)),
                pooled_wave_dw((int)arg(6), (int)arg(4), (int)arg(5)) * sizeof(unsigned));
    return 0;
  }
  if (argc == 4 && !std::strcmp(argv[1], "fits")) {
    std::printf("fits=%d\n", pooled_col_fits((size_t)arg(2), (size_t)arg(3)));
    return 0;
  }
  if (argc == 8 && !std::strcmp(argv[1], "bits")) {
    const int e = pooled_entry_bits((int)arg(2), (int)arg(3), (int)arg(4), (size_t)arg(5), (size_t)arg(6), arg(7) != 0);
    std::printf("entry=%d mode=%d col_lds=%d rt_flags=%d\n", e, e & kEntryModeMask, (e & kEntryColLds) != 0, (e & kEntryRtFlags) != 0);
    return 0;
  }
  std::fprintf(stderr, "usage: batch_trim_check keys | flags L D | colbytes NODES SPH CAPB CAPL PLANES | fits BYTES LIMIT | bits MODE L D BYTES LIMIT COL\n");
  return 2;
}
