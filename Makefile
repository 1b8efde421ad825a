# Build of the MI355X RANSAC pose engine (gfx950).  `make` builds librsc.so (HIP kernels + C ABI),
# the oracle (test infrastructure) and the host-emulation test libraries.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PKG = orb-slam2-optimized_amd
CSRC = $(PKG)/csrc
LIBDIR = $(PKG)/lib
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math \
           -fno-gpu-flush-denormals-to-zero -Wall -Wno-unused-function -Wno-unused-variable
HDRS = include/rsc.h $(wildcard $(CSRC)/*.h)

all: $(LIBDIR)/librsc.so $(LIBDIR)/librsc_spin1.so oracle hostemu frameproj_emu kfproj_emu facade_test facade_proj_test \
     facade_loopproj_test facade_voc_test chase_mirror_test bowvoc_emu localproj_emu facade_localproj_test lastproj_emu \
     facade_lastproj_test facade_triang_test arena_test viewimage_test rounds_test seed_window_test triang_emu fusekf_emu facade_fusekf_test ref_dbow2 \
     mpupdate_emu facade_mpupdate_test stereo_emu facade_stereo_test localba_emu localba_test facade_localba_test \
     scan_bound_test

include $(CSRC)/objs.mk
OBJS = $(RSC_OBJS:%=$(LIBDIR)/%.o)

$(LIBDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/%.o: $(CSRC)/%.cpp $(HDRS)
	mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

# kernels.hip with the compiler's kernel-resource remarks kept beside the object; anything else the compiler says
# (warnings) is shown as usual, without source excerpts (registers, scratch and
# waves per SIMD of every kernel as built: tests/test_cpu_round_args_resources.py)
$(LIBDIR)/kernels.o: $(CSRC)/kernels.hip $(HDRS)
	mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -fno-caret-diagnostics -c $< -o $@ \
		2> $(LIBDIR)/kernels.resources.txt || { cat $(LIBDIR)/kernels.resources.txt >&2; exit 1; }
	@grep -v 'Rpass-analysis=kernel-resource-usage' $(LIBDIR)/kernels.resources.txt >&2 || true

# mpupdate.hip likewise (registers, LDS and occupancy of the two MapPoint-update kernels: DESIGN.md §2.15)
$(LIBDIR)/mpupdate.o: $(CSRC)/mpupdate.hip $(HDRS)
	mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -fno-caret-diagnostics -c $< -o $@ \
		2> $(LIBDIR)/mpupdate.resources.txt || { cat $(LIBDIR)/mpupdate.resources.txt >&2; exit 1; }
	@grep -v 'Rpass-analysis=kernel-resource-usage' $(LIBDIR)/mpupdate.resources.txt >&2 || true

# stereo.hip likewise (the match and cut kernels of ComputeStereoMatches: DESIGN.md §2.16)
$(LIBDIR)/stereo.o: $(CSRC)/stereo.hip $(HDRS)
	mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -fno-caret-diagnostics -c $< -o $@ \
		2> $(LIBDIR)/stereo.resources.txt || { cat $(LIBDIR)/stereo.resources.txt >&2; exit 1; }
	@grep -v 'Rpass-analysis=kernel-resource-usage' $(LIBDIR)/stereo.resources.txt >&2 || true

# localba.hip likewise (the stage kernels of LocalBundleAdjustment: DESIGN.md §2.17)
$(LIBDIR)/localba.o: $(CSRC)/localba.hip $(HDRS)
	mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -fno-caret-diagnostics -c $< -o $@ \
		2> $(LIBDIR)/localba.resources.txt || { cat $(LIBDIR)/localba.resources.txt >&2; exit 1; }
	@grep -v 'Rpass-analysis=kernel-resource-usage' $(LIBDIR)/localba.resources.txt >&2 || true

$(LIBDIR)/librsc.so: $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $^

# TEST-ONLY variant: the split eigen stage's hand-off waits give up after one poll, so the fault path
# (split_wait -> fault word -> RSC_ERR_INTERNAL) runs on the device (tests/test_gpu_fault.py)
$(LIBDIR)/kernels_spin1.o: $(CSRC)/kernels.hip $(HDRS)
	mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -DRSC_SPLIT_SPIN_LIMIT=1 -c $< -o $@

$(LIBDIR)/librsc_spin1.so: $(OBJS:%/kernels.o=%/kernels_spin1.o)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $^

FACADE_TESTS = facade_test facade_proj_test facade_loopproj_test facade_localproj_test facade_lastproj_test \
               facade_triang_test facade_fusekf_test facade_voc_test facade_mpupdate_test facade_stereo_test facade_localba_test

$(FACADE_TESTS): %: $(LIBDIR)/%

$(FACADE_TESTS:%=$(LIBDIR)/%): $(LIBDIR)/%: tests/cpp/%.cpp $(CSRC)/facade/*.hpp $(LIBDIR)/librsc.so
	g++ -O2 -std=c++17 -Iinclude -I$(CSRC)/facade -o $@ $< -L$(LIBDIR) -lrsc -Wl,-rpath,'$$ORIGIN'

# the LocalBundleAdjustment facade test also compiles the host restatement it compares against
$(LIBDIR)/facade_localba_test: tests/localba_emu/localba_emu.cpp $(CSRC)/rsc_localba.h

# TEST-ONLY host programs: tridiag_qr with and without the mirror() / any_lane() hooks of its
# rotation sink (tests/test_cpu_chase_mirror.py); the second build runs under the host sanitizers
chase_mirror_test: $(LIBDIR)/chase_mirror_test $(LIBDIR)/chase_mirror_test_san

HOSTFLAGS = -O2 -std=c++17 -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-unknown-pragmas

$(LIBDIR)/chase_mirror_test: tests/cpp/chase_mirror_test.cpp $(CSRC)/rsc_core.h
	mkdir -p $(LIBDIR)
	g++ $(HOSTFLAGS) -o $@ $<

$(LIBDIR)/chase_mirror_test_san: tests/cpp/chase_mirror_test.cpp $(CSRC)/rsc_core.h
	mkdir -p $(LIBDIR)
	g++ $(HOSTFLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ $<

# TEST-ONLY host programs: the staging-arena cursor against the matchers' former offset arithmetic
# (tests/test_cpu_arena.py); the second build runs under the host sanitizers
arena_test: $(LIBDIR)/arena_test $(LIBDIR)/arena_test_san

$(LIBDIR)/arena_test: tests/cpp/arena_test.cpp $(CSRC)/rsc_arena.h
	mkdir -p $(LIBDIR)
	g++ $(HOSTFLAGS) -o $@ $<

$(LIBDIR)/arena_test_san: tests/cpp/arena_test.cpp $(CSRC)/rsc_arena.h
	mkdir -p $(LIBDIR)
	g++ $(HOSTFLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ $<

# TEST-ONLY host programs: the view-image builder and the views' shared argument checks against the view
# builders' former offset arithmetic (tests/test_cpu_viewimage.py); the second build runs under the host sanitizers
viewimage_test: $(LIBDIR)/viewimage_test $(LIBDIR)/viewimage_test_san

VIEWIMAGE_DEPS = tests/cpp/viewimage_test.cpp $(CSRC)/rsc_viewimage.h $(CSRC)/rsc_arena.h include/rsc.h

$(LIBDIR)/viewimage_test: $(VIEWIMAGE_DEPS)
	mkdir -p $(LIBDIR)
	g++ $(HOSTFLAGS) -o $@ $<

$(LIBDIR)/viewimage_test_san: $(VIEWIMAGE_DEPS)
	mkdir -p $(LIBDIR)
	g++ $(HOSTFLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ $<

# TEST-ONLY host programs: the drivers' bookkeeping (rsc_rounds.h) against the former driver loops
# (tests/test_cpu_rounds.py); the second build runs under the host sanitizers
rounds_test: $(LIBDIR)/rounds_test $(LIBDIR)/rounds_test_san

ROUNDS_DEPS = tests/cpp/rounds_test.cpp $(CSRC)/rsc_rounds.h $(CSRC)/rsc_engine.h include/rsc.h

$(LIBDIR)/rounds_test: $(ROUNDS_DEPS)
	mkdir -p $(LIBDIR)
	g++ $(HOSTFLAGS) -o $@ $<

$(LIBDIR)/rounds_test_san: $(ROUNDS_DEPS)
	mkdir -p $(LIBDIR)
	g++ $(HOSTFLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ $<

# TEST-ONLY host programs: the closed form of srand(seed)'s window (rsc_core.h rng_seed_word) against
# the Schrage loop, and RngStream's seed mark and lazily worked-out window (tests/test_cpu_seed_window.py);
# the second build runs under the host sanitizers
seed_window_test: $(LIBDIR)/seed_window_test $(LIBDIR)/seed_window_test_san

SEED_WINDOW_DEPS = tests/cpp/seed_window_test.cpp $(CSRC)/rsc_core.h $(CSRC)/rsc_engine.h

$(LIBDIR)/seed_window_test: $(SEED_WINDOW_DEPS)
	mkdir -p $(LIBDIR)
	g++ $(HOSTFLAGS) -o $@ $<

$(LIBDIR)/seed_window_test_san: $(SEED_WINDOW_DEPS)
	mkdir -p $(LIBDIR)
	g++ $(HOSTFLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ $<

# TEST-ONLY host programs: the continue rule of the PnP scan's two-segment counting (rsc_scanbound.h) over every
# (N, PPT, min_inliers, count) (tests/test_cpu_scan_bound.py); the second build runs under the host sanitizers
scan_bound_test: $(LIBDIR)/scan_bound_test $(LIBDIR)/scan_bound_test_san

SCAN_BOUND_DEPS = tests/cpp/scan_bound_test.cpp $(CSRC)/rsc_scanbound.h $(CSRC)/rsc_core.h

$(LIBDIR)/scan_bound_test: $(SCAN_BOUND_DEPS)
	mkdir -p $(LIBDIR)
	g++ $(HOSTFLAGS) -o $@ $<

$(LIBDIR)/scan_bound_test_san: $(SCAN_BOUND_DEPS)
	mkdir -p $(LIBDIR)
	g++ $(HOSTFLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ $<

# TEST-ONLY host program: the sequential LocalBundleAdjustment restatement (tests/localba_emu) on four scenes of
# its own (tests/test_cpu_localba.py); the second build runs under the host sanitizers
localba_test: $(LIBDIR)/localba_test $(LIBDIR)/localba_test_san

LOCALBA_DEPS = tests/cpp/localba_test.cpp tests/localba_emu/localba_emu.cpp $(CSRC)/rsc_localba.h $(CSRC)/rsc_poseopt.h \
               $(CSRC)/rsc_core.h $(CSRC)/rsc_math.h include/rsc.h

$(LIBDIR)/localba_test: $(LOCALBA_DEPS)
	mkdir -p $(LIBDIR)
	g++ $(HOSTFLAGS) -o $@ $<

$(LIBDIR)/localba_test_san: $(LOCALBA_DEPS)
	mkdir -p $(LIBDIR)
	g++ $(HOSTFLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ $<

oracle:
	$(MAKE) -s -C oracle

# TEST-ONLY: the reference's own DBoW2 around our driver (oracle/Makefile `ref`), where a reference tree exists
ref_dbow2:
	$(MAKE) -s -C oracle ref

hostemu:
	$(MAKE) -s -C tests/hostemu

frameproj_emu:
	$(MAKE) -s -C tests/frameproj_emu

kfproj_emu:
	$(MAKE) -s -C tests/kfproj_emu

bowvoc_emu:
	$(MAKE) -s -C tests/bowvoc_emu

localproj_emu:
	$(MAKE) -s -C tests/localproj_emu

lastproj_emu:
	$(MAKE) -s -C tests/lastproj_emu

triang_emu:
	$(MAKE) -s -C tests/triang_emu

fusekf_emu:
	$(MAKE) -s -C tests/fusekf_emu

mpupdate_emu:
	$(MAKE) -s -C tests/mpupdate_emu

stereo_emu:
	$(MAKE) -s -C tests/stereo_emu

localba_emu:
	$(MAKE) -s -C tests/localba_emu

clean:
	rm -rf $(LIBDIR) oracle/build oracle/_ref tests/hostemu/build tests/frameproj_emu/build tests/kfproj_emu/build tests/bowvoc_emu/build \
	       tests/localproj_emu/build tests/lastproj_emu/build tests/triang_emu/build tests/fusekf_emu/build tests/mpupdate_emu/build \
	       tests/stereo_emu/build tests/localba_emu/build

.PHONY: localba_emu localba_test facade_localba_test
.PHONY: all oracle ref_dbow2 hostemu frameproj_emu kfproj_emu bowvoc_emu localproj_emu lastproj_emu triang_emu fusekf_emu mpupdate_emu stereo_emu facade_stereo_test facade_mpupdate_test facade_fusekf_test facade_localproj_test facade_lastproj_test facade_triang_test facade_test facade_proj_test facade_loopproj_test \
        facade_voc_test chase_mirror_test arena_test viewimage_test rounds_test seed_window_test scan_bound_test clean
