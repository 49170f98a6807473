// The host-side predicates behind the kernels that have the twenty-wave shape's constants compiled in (rt_device.hpp: pooled_wide_plan, pooled_wide_ok), printed
// for tests/test_wide_const_cpu.py: no HIP runtime calls.
//   wide_const_check plan WAVES WGS_PER_CU LDS_NODES LDS_SPH RAY_PLANES     "wide=0|1": may a launch of this shape take such a kernel?
//   wide_const_check keys                                                   every compiled key: "<name> threads=.. ... wide_ok=0|1" (has it the twin?)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rt_device.hpp"

int main(int argc, char **argv) {
  using namespace rtk;
  auto arg = [&](int i) { return i < argc ? std::atoi(argv[i]) : 0; };
  if (argc == 7 && !std::strcmp(argv[1], "plan")) {
    std::printf("wide=%d\n", pooled_wide_plan(arg(2), arg(3), arg(4), arg(5), arg(6)));
    return 0;
  }
  if (argc == 2 && !std::strcmp(argv[1], "keys")) {
    for (int i = 0; i < kNumPooledKeys; ++i) {
      const PooledKey &k = kPooledKeys[i];
      std::printf("%s threads=%d all_lds=%d stats=%d solo=%d tail=%d ord=%d cull=%d spill=%d rays=%d wide_ok=%d\n", pooled_name(k).c_str(), k.threads, k.all_lds, k.stats,
                  k.solo, k.tail, k.ord, k.cull, k.spill, k.rays, pooled_wide_ok(k));
    }
    return 0;
  }
  std::fprintf(stderr, "usage: wide_const_check plan WAVES WGS LDS_NODES LDS_SPH PLANES | keys\n");
  return 2;
}
