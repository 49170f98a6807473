# Builds the MI355X-native render library and its checker.
#   make            -> raytracers_amd/libray_mi355x.so  (HIP, gfx950) + tools
#   make oracle     -> oracle/build/liboracle.so        (CPU oracle, test infrastructure)
# -ffp-contract=off is load-bearing on both host and device: parity is bit-exact fp32.
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
CSRC    := raytracers_amd/csrc
OBJ     := build/obj
LIB     := raytracers_amd/libray_mi355x.so
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wextra -Wno-unused-parameter
HOSTFLAGS := -O2 -std=c++17 -fPIC -ffp-contract=off -Wall -Wextra

all: $(LIB) tools oracle

$(OBJ)/render_kernels.o: $(CSRC)/render_kernels.hip $(CSRC)/lane_core.h $(CSRC)/rt_device.hpp $(CSRC)/treelet.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJ)/query_kernels.o: $(CSRC)/query_kernels.hip $(CSRC)/query_core.h $(CSRC)/query_device.hpp $(CSRC)/lane_core.h $(CSRC)/rt_device.hpp $(CSRC)/treelet.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJ)/bvh_build.o: $(CSRC)/bvh_build.hip $(CSRC)/rt_device.hpp $(CSRC)/lane_core.h $(CSRC)/treelet.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJ)/api.o: $(CSRC)/api.cpp $(CSRC)/rt_internal.hpp $(CSRC)/rt_device.hpp $(CSRC)/rt_host.hpp $(CSRC)/lane_core.h include/rt_mi355x.h $(CSRC)/treelet.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJ)/api_queries.o: $(CSRC)/api_queries.cpp $(CSRC)/rt_internal.hpp $(CSRC)/query_device.hpp $(CSRC)/rt_device.hpp $(CSRC)/rt_host.hpp $(CSRC)/lane_core.h include/rt_mi355x.h $(CSRC)/treelet.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJ)/futhark_shim.o: $(CSRC)/futhark_shim.cpp $(CSRC)/rt_internal.hpp $(CSRC)/rt_device.hpp $(CSRC)/rt_host.hpp $(CSRC)/lane_core.h include/ray.h include/rt_mi355x.h $(CSRC)/treelet.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJ)/multi_gpu.o: $(CSRC)/multi_gpu.cpp $(CSRC)/rt_internal.hpp $(CSRC)/rt_device.hpp $(CSRC)/rt_host.hpp include/rt_mi355x.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJ)/host_build.o: $(CSRC)/host_build.cpp $(CSRC)/rt_host.hpp $(CSRC)/lane_core.h $(CSRC)/treelet.h
	@mkdir -p $(OBJ)
	$(CXX) $(HOSTFLAGS) -c $< -o $@

# (librccl is NOT linked: multi_gpu.cpp loads it on demand, so a single-GPU host needs no RCCL)
$(LIB): $(OBJ)/render_kernels.o $(OBJ)/query_kernels.o $(OBJ)/bvh_build.o $(OBJ)/api.o $(OBJ)/api_queries.o $(OBJ)/futhark_shim.o $(OBJ)/multi_gpu.o $(OBJ)/host_build.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -ldl

# native harness (our own bench front-end; the reference's futhark/main.c links the same way)
build/rtbench: tools/rtbench.c include/ray.h include/rt_mi355x.h $(LIB)
	@mkdir -p build
	$(CC) -O2 -std=gnu99 -Wall -Iinclude -o $@ tools/rtbench.c -Lraytracers_amd -lray_mi355x -Wl,-rpath,'$$ORIGIN/../raytracers_amd' -lm

build/wavesim: tools/wavesim.cpp $(CSRC)/lane_core.h $(CSRC)/rt_host.hpp $(OBJ)/host_build.o
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -fopenmp -I$(CSRC) -o $@ tools/wavesim.cpp $(OBJ)/host_build.o

# microbenchmark behind the bench line's measured peaks (tools/gpu_issue_peak.sh runs it)
build/issue_peak: tools/issue_peak.hip
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-inline-asm -o $@ $<

build/hip_touch: tools/hip_touch.hip
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O2 -o $@ $<

# the pooled kernel's tile-queue protocol (rt_device.hpp) played on the CPU; in the CPU test suite
# (`queue_check extreme`: the tile grids of strip images, 1 x 8192 ... 131072 x 1; `queue_check span NTILES NFRAMES DS TPT N_DEEP N_SPLIT`: every ticket's
# 32-bit span against the formula in 64 bits, no per-slot memory -- the bound tiles x frames < 2^26; tests/test_frame_edges_cpu.py)
build/queue_check: tools/queue_check.cpp $(CSRC)/rt_device.hpp $(CSRC)/lane_core.h $(CSRC)/treelet.h
	@mkdir -p build
	$(HIPCC) -O2 -std=c++17 -Wall -I$(CSRC) -o $@ $<

# the choice of the pooled kernel's instantiation (rt_device.hpp: choose_pooled) over its inputs, against the compiled set; in the CPU test suite
build/pooled_choice_check: tools/pooled_choice_check.cpp $(CSRC)/rt_device.hpp $(CSRC)/lane_core.h $(CSRC)/treelet.h
	@mkdir -p build
	$(HIPCC) -O2 -std=c++17 -Wall -I$(CSRC) -o $@ $<

# the predicates behind the ENTRY kernels (rt_device.hpp: pooled_entry_ok, pooled_entry_flags_const, pooled_col_fits, pooled_entry_bits) printed for the CPU test suite
build/batch_trim_check: tools/batch_trim_check.cpp $(CSRC)/rt_device.hpp $(CSRC)/lane_core.h $(CSRC)/treelet.h
	@mkdir -p build
	$(HIPCC) -O2 -std=c++17 -Wall -I$(CSRC) -o $@ $<

# the predicates behind the kernels with the twenty-wave shape's constants compiled in (rt_device.hpp: pooled_wide_plan, pooled_wide_ok) printed for the CPU test suite
build/wide_const_check: tools/wide_const_check.cpp $(CSRC)/rt_device.hpp $(CSRC)/lane_core.h $(CSRC)/treelet.h
	@mkdir -p build
	$(HIPCC) -O2 -std=c++17 -Wall -I$(CSRC) -o $@ $<

# the DONATE instantiation's mailbox protocol (render_kernels.hip) as a model, random interleavings; in the CPU test suite
build/donate_check: tools/donate_check.cpp
	@mkdir -p build
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ $<

# design tool + CPU check of the treelet numbering / masks (treelet.h) against a plain depth-first walk; in the CPU test suite
build/treelet_probe: tools/treelet_probe.cpp $(CSRC)/lane_core.h $(CSRC)/treelet.h $(CSRC)/rt_host.hpp $(OBJ)/host_build.o
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -I$(CSRC) -o $@ tools/treelet_probe.cpp $(OBJ)/host_build.o

# the inequalities behind the CULL instantiations (lane_core.h: cull_limit) hammered with the product's binary32 code against __float128; in the CPU test suite
build/cull_bound_check: tools/cull_bound_check.cpp $(CSRC)/lane_core.h $(CSRC)/rt_host.hpp $(OBJ)/host_build.o
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -fopenmp -I$(CSRC) -o $@ tools/cull_bound_check.cpp $(OBJ)/host_build.o -lquadmath

# whole renders at the limits of the culling guards: the host's decision and constants, and every ray chain walked un-culled and under the
# strongest limit any traversal order could apply (cases: tests/edge_cull.py); in the CPU test suite
build/cull_guard_check: tools/cull_guard_check.cpp $(CSRC)/lane_core.h $(CSRC)/rt_host.hpp $(OBJ)/host_build.o
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -I$(CSRC) -o $@ tools/cull_guard_check.cpp $(OBJ)/host_build.o

# the render path's dark stop (lane_core.h: light_is_dead): every pixel's chain walked in full and stopped where SHADE would stop it -- pixels
# compared, rays / box tests / sphere tests of both; in the CPU test suite
build/dark_stop_check: tools/dark_stop_check.cpp $(CSRC)/lane_core.h $(CSRC)/rt_host.hpp $(OBJ)/host_build.o
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -I$(CSRC) -o $@ tools/dark_stop_check.cpp $(OBJ)/host_build.o

# the leaf's own box of the pooled records (lane_core.h: leaf_box_eps): every chain of a frame walked over the product's records unfiltered and
# filtered -- sphere tests of both, accepted roots lost, pixels compared -- and the claim behind the margin hammered against __float128, with the
# shrunk boxes that must be found; in the CPU test suite
build/leaf_box_check: tools/leaf_box_check.cpp $(CSRC)/lane_core.h $(CSRC)/rt_host.hpp $(OBJ)/host_build.o
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -fopenmp -I$(CSRC) -o $@ tools/leaf_box_check.cpp $(OBJ)/host_build.o -lquadmath

# the box test of the proximity queries (query_core.h: box_may_hold) hammered with host-built boxes and __float128; in the CPU test suite
build/proximity_bound_check: tools/proximity_bound_check.cpp $(CSRC)/query_core.h $(CSRC)/lane_core.h $(CSRC)/rt_host.hpp $(OBJ)/host_build.o
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -fopenmp -I$(CSRC) -o $@ tools/proximity_bound_check.cpp $(OBJ)/host_build.o -lquadmath

# the node test of the box queries (query_core.h: box_may_meet) hammered with host-built boxes and __float128; in the CPU test suite
build/box_query_bound_check: tools/box_query_bound_check.cpp $(CSRC)/query_core.h $(CSRC)/lane_core.h $(CSRC)/rt_host.hpp $(OBJ)/host_build.o
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -fopenmp -I$(CSRC) -o $@ tools/box_query_bound_check.cpp $(OBJ)/host_build.o -lquadmath

# the node test of the plane-set queries (query_core.h: planes_may_meet) and the gap's error bound hammered with host-built boxes and __float128;
# in the CPU test suite
build/plane_query_bound_check: tools/plane_query_bound_check.cpp $(CSRC)/query_core.h $(CSRC)/lane_core.h $(CSRC)/rt_host.hpp $(OBJ)/host_build.o
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -fopenmp -I$(CSRC) -o $@ tools/plane_query_bound_check.cpp $(OBJ)/host_build.o -lquadmath

# the culling guards in two stages (statistics + finish) against the one-pass function, and the device's reduction of the statistics
# modelled on the host (random partitions and merge orders); in the CPU test suite
build/cull_stats_check: tools/cull_stats_check.cpp $(CSRC)/rt_host.hpp $(OBJ)/host_build.o
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -I$(CSRC) -o $@ tools/cull_stats_check.cpp $(OBJ)/host_build.o

# the per-tile entry lists of the ENTRY instantiations (lane_core.h: tile_rays / tile_verdict / tile_frontier / tile_entry): every primary ray of a frame walked
# from the root and from its tile's list over the product's records -- tested leaves of both compared, items saved per cap counted -- tile verdicts against
# sampled rays, and three mutants that must be found; in the CPU test suite
build/entry_check: tools/entry_check.cpp $(CSRC)/lane_core.h $(CSRC)/rt_host.hpp $(OBJ)/host_build.o
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -fopenmp -I$(CSRC) -o $@ tools/entry_check.cpp $(OBJ)/host_build.o

# the exit lists of the kEntryExit kernels on the CPU: every bounce ray of a frame from the root and from the list of the sphere it leaves,
# over the product's records and the tables exit_tables_path writes; the lemma against sampled rays; two mutants that must be found; in the CPU test suite
build/exit_check: tools/exit_check.cpp $(CSRC)/lane_core.h $(CSRC)/rt_host.hpp $(OBJ)/host_build.o
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -fopenmp -I$(CSRC) -o $@ tools/exit_check.cpp $(OBJ)/host_build.o

# box_hit_presorted on operands picked by the ray's sign offsets out of a sign-ordered record (lane_core.h) against box_hit_interval; in the CPU test suite
build/box_presorted_check: tools/box_presorted_check.cpp $(CSRC)/lane_core.h
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -I$(CSRC) -o $@ tools/box_presorted_check.cpp

# the sphere casts' per-sphere rule (query_core.h: sweep_contact) over cases read from a file, tau and kind written as bits; in the CPU test suite
build/sweep_check: tools/sweep_check.cpp $(CSRC)/query_core.h $(CSRC)/lane_core.h
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -I$(CSRC) -o $@ tools/sweep_check.cpp

# the along-ray queries' per-sphere rule (query_core.h: sweep_contact_roots) over the same case files: kind, tau and the two roots written as
# bits, kind and tau held equal to sweep_contact's; in the CPU test suite
build/along_check: tools/along_check.cpp $(CSRC)/query_core.h $(CSRC)/lane_core.h
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -I$(CSRC) -o $@ tools/along_check.cpp

# the sphere groups' rule, combine and climb (query_core.h: group_seen / group_combine / group_climb) over pairs and a tree read from a file, the
# node words written out; in the CPU test suite.  build/asan/groups_check: the same program under -fsanitize=address,undefined (host code
# only, stand-alone)
build/groups_check: tools/groups_check.cpp $(CSRC)/query_core.h $(CSRC)/lane_core.h
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -I$(CSRC) -o $@ tools/groups_check.cpp

build/asan/groups_check: tools/groups_check.cpp $(CSRC)/query_core.h $(CSRC)/lane_core.h
	@mkdir -p build/asan
	$(CXX) -O1 -g -std=c++17 -ffp-contract=off -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) -o $@ tools/groups_check.cpp

# the contact clusters' union-find (query_core.h: uf_find / uf_unite) behind std::atomic: threads uniting random graphs, a shuffled chain and
# a clique against a sequential union-find, and four mutants each caught by its case; in the CPU test suite, which also builds and runs
# build/tsan/clusters_check, the same program under -fsanitize=thread (host code only, stand-alone)
build/clusters_check: tools/clusters_check.cpp $(CSRC)/query_core.h $(CSRC)/lane_core.h
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -I$(CSRC) -pthread -o $@ tools/clusters_check.cpp

build/tsan/clusters_check: tools/clusters_check.cpp $(CSRC)/query_core.h $(CSRC)/lane_core.h
	@mkdir -p build/tsan
	/opt/rocm/lib/llvm/bin/clang++ -O1 -std=c++17 -ffp-contract=off -Wall -Wextra $(TSAN) -I$(CSRC) -pthread -o $@ tools/clusters_check.cpp

# one bounce of a ray path (query_core.h: path_bounce behind sphere_root and rehit_full, what paths_kernel runs when a fold ends) over cases read
# from a file, the outcome and the new loop variables written as bits; in the CPU test suite
build/path_check: tools/path_check.cpp $(CSRC)/query_core.h $(CSRC)/lane_core.h
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -I$(CSRC) -o $@ tools/path_check.cpp

# the pooled kernel's loop on emulated lanes with the culling rule: tests saved, pixels kept; in the CPU test suite
build/cull_pooled: tools/cull_pooled.cpp $(CSRC)/lane_core.h $(CSRC)/rt_host.hpp $(OBJ)/host_build.o
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -I$(CSRC) -o $@ tools/cull_pooled.cpp $(OBJ)/host_build.o

# host threads sharing one context and one prepared scene (the context lock): the plain build is in the GPU test suite ...
build/ctx_threads: tools/ctx_threads.cpp include/ray.h include/rt_mi355x.h $(LIB)
	@mkdir -p build
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -pthread -o $@ tools/ctx_threads.cpp -Lraytracers_amd -lray_mi355x -Wl,-rpath,'$$ORIGIN/../raytracers_amd'

# ... and the same program over the library's HOST code built with -fsanitize=thread (device code and the HIP runtime are not
# instrumented): build/tsan/libray_mi355x.so + build/tsan/ctx_threads, run on a GPU box by tools/gpu.sh tsan
TSAN := -fsanitize=thread -g
build/tsan/ctx_threads: tools/ctx_threads.cpp $(CSRC)/api.cpp $(CSRC)/api_queries.cpp $(CSRC)/futhark_shim.cpp $(CSRC)/multi_gpu.cpp $(CSRC)/host_build.cpp $(OBJ)/render_kernels.o $(OBJ)/query_kernels.o $(OBJ)/bvh_build.o
	@mkdir -p build/tsan
	$(HIPCC) $(HIPFLAGS) $(TSAN) -c $(CSRC)/api.cpp -o build/tsan/api.o
	$(HIPCC) $(HIPFLAGS) $(TSAN) -c $(CSRC)/api_queries.cpp -o build/tsan/api_queries.o
	$(HIPCC) $(HIPFLAGS) $(TSAN) -c $(CSRC)/futhark_shim.cpp -o build/tsan/futhark_shim.o
	$(HIPCC) $(HIPFLAGS) $(TSAN) -c $(CSRC)/multi_gpu.cpp -o build/tsan/multi_gpu.o
	/opt/rocm/lib/llvm/bin/clang++ $(HOSTFLAGS) $(TSAN) -c $(CSRC)/host_build.cpp -o build/tsan/host_build.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(TSAN) -o build/tsan/libray_mi355x.so $(OBJ)/render_kernels.o $(OBJ)/query_kernels.o $(OBJ)/bvh_build.o build/tsan/api.o build/tsan/api_queries.o build/tsan/futhark_shim.o build/tsan/multi_gpu.o build/tsan/host_build.o -ldl
	/opt/rocm/lib/llvm/bin/clang++ -O1 -std=c++17 $(TSAN) -Iinclude -pthread -o $@ tools/ctx_threads.cpp -Lbuild/tsan -lray_mi355x -Wl,-rpath,'$$ORIGIN'

# ... and once more with the locks compiled out (-DRT_NO_CONTEXT_LOCK): what the sanitizer says about the library WITHOUT them (the control run)
build/tsan_nolock/ctx_threads: tools/ctx_threads.cpp $(CSRC)/api.cpp $(CSRC)/api_queries.cpp $(CSRC)/futhark_shim.cpp $(CSRC)/multi_gpu.cpp $(CSRC)/host_build.cpp $(OBJ)/render_kernels.o $(OBJ)/query_kernels.o $(OBJ)/bvh_build.o
	@mkdir -p build/tsan_nolock
	$(HIPCC) $(HIPFLAGS) $(TSAN) -DRT_NO_CONTEXT_LOCK -c $(CSRC)/api.cpp -o build/tsan_nolock/api.o
	$(HIPCC) $(HIPFLAGS) $(TSAN) -DRT_NO_CONTEXT_LOCK -c $(CSRC)/api_queries.cpp -o build/tsan_nolock/api_queries.o
	$(HIPCC) $(HIPFLAGS) $(TSAN) -DRT_NO_CONTEXT_LOCK -c $(CSRC)/futhark_shim.cpp -o build/tsan_nolock/futhark_shim.o
	$(HIPCC) $(HIPFLAGS) $(TSAN) -DRT_NO_CONTEXT_LOCK -c $(CSRC)/multi_gpu.cpp -o build/tsan_nolock/multi_gpu.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(TSAN) -o build/tsan_nolock/libray_mi355x.so $(OBJ)/render_kernels.o $(OBJ)/query_kernels.o $(OBJ)/bvh_build.o build/tsan_nolock/api.o build/tsan_nolock/api_queries.o build/tsan_nolock/futhark_shim.o build/tsan_nolock/multi_gpu.o build/tsan/host_build.o -ldl
	/opt/rocm/lib/llvm/bin/clang++ -O1 -std=c++17 $(TSAN) -Iinclude -pthread -o $@ tools/ctx_threads.cpp -Lbuild/tsan_nolock -lray_mi355x -Wl,-rpath,'$$ORIGIN'

# the view-order sorts (tile order, pixel list + header, first order: launch_tile_order / launch_px_order / launch_first_order of the library) on
# cases from a file, every buffer between guards, and a view's arrays after rendered frames (white box); in the GPU test suite (tests/test_view_order_gpu.py)
build/view_order_check: tools/view_order_check.cpp $(CSRC)/rt_internal.hpp $(CSRC)/rt_device.hpp $(CSRC)/rt_host.hpp $(CSRC)/lane_core.h $(CSRC)/treelet.h include/rt_mi355x.h $(LIB)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -Iinclude -o $@ tools/view_order_check.cpp -Lraytracers_amd -lray_mi355x -Wl,-rpath,'$$ORIGIN/../raytracers_amd'

build/first_call_probe: tools/first_call_probe.c include/ray.h $(LIB)
	@mkdir -p build
	$(CC) -O2 -std=gnu99 -Wall -Iinclude -o $@ tools/first_call_probe.c -Lraytracers_amd -lray_mi355x -Wl,-rpath,'$$ORIGIN/../raytracers_amd'

tools: build/first_call_probe build/ctx_threads build/rtbench build/issue_peak build/queue_check build/pooled_choice_check build/batch_trim_check build/wide_const_check build/donate_check build/treelet_probe build/hip_touch build/cull_bound_check build/cull_guard_check build/dark_stop_check build/leaf_box_check build/entry_check build/exit_check build/cull_pooled build/cull_stats_check build/proximity_bound_check build/box_query_bound_check build/plane_query_bound_check build/box_presorted_check build/sweep_check build/along_check build/groups_check build/path_check build/clusters_check build/view_order_check

oracle:
	$(MAKE) -s -C oracle

clean:
	rm -rf build $(LIB)
	$(MAKE) -C oracle clean

.PHONY: all tools oracle clean
