# Top-level build: the gfx950 engine (libjfgpu.so), the host CLI, the oracle.
#   make            -> engine + CLI + oracle
#   make engine     -> jellyfish_amd/lib/libjfgpu.so   (hipcc cross-compiles without a GPU)
#   make kernel-harness -> tests/kernels/_build/libjfgpu_kt.so   (the stage tests' library; not product)
#   make kernel-harness-nword -> tests/kernels/_build/libjfgpu_ktn.so   (the same for the keys of three and four words)
#   make kernel-harness-bloom-keys -> tests/kernels/_build/libjfgpu_ktbk.so   (P1b of the Bloom insert for keys of two to four words)
HIPCC    ?= hipcc
CXX      ?= g++
ARCH     ?= gfx950
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-result
CSRC     := jellyfish_amd/csrc
LIBDIR   := jellyfish_amd/lib

all: engine cli oracle

engine: $(LIBDIR)/libjfgpu.so

$(LIBDIR)/libjfgpu.so: $(wildcard $(CSRC)/*.hip) $(wildcard $(CSRC)/*.hpp) $(wildcard $(CSRC)/*.inl) include/jfgpu.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(CSRC)/jfgpu.hip -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib

# test infrastructure, not product: the engine's translation unit plus entry points that launch one stage of the
# partitioned insert path alone (tests/kernels/stage_harness.hip; tests/test_gpu_stage_*.py)
KTDIR    := tests/kernels/_build
kernel-harness: $(KTDIR)/libjfgpu_kt.so

$(KTDIR)/libjfgpu_kt.so: tests/kernels/stage_harness.hip $(wildcard $(CSRC)/*.hip) $(wildcard $(CSRC)/*.hpp) $(wildcard $(CSRC)/*.inl) include/jfgpu.h
	@mkdir -p $(KTDIR)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ tests/kernels/stage_harness.hip -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib

# ... and the stages of the partitioned insert of three- and four-word keys (tests/kernels/stage_harness_nword.hip;
# tests/test_gpu_stage_nword.py)
kernel-harness-nword: $(KTDIR)/libjfgpu_ktn.so

$(KTDIR)/libjfgpu_ktn.so: tests/kernels/stage_harness_nword.hip $(wildcard $(CSRC)/*.hip) $(wildcard $(CSRC)/*.hpp) $(wildcard $(CSRC)/*.inl) include/jfgpu.h
	@mkdir -p $(KTDIR)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ tests/kernels/stage_harness_nword.hip -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib

# ... and P1b of the partitioned Bloom insert for keys of two to four words (tests/kernels/stage_harness_bloom_keys.hip;
# tests/test_gpu_stage_bloom_p1_keys.py)
kernel-harness-bloom-keys: $(KTDIR)/libjfgpu_ktbk.so

$(KTDIR)/libjfgpu_ktbk.so: tests/kernels/stage_harness_bloom_keys.hip $(wildcard $(CSRC)/*.hip) $(wildcard $(CSRC)/*.hpp) $(wildcard $(CSRC)/*.inl) include/jfgpu.h
	@mkdir -p $(KTDIR)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ tests/kernels/stage_harness_bloom_keys.hip -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib

cli: bin/jellyfish-amd

bin/jellyfish-amd: $(wildcard jellyfish_amd/cli/*.cc) $(wildcard jellyfish_amd/include/jellyfish_amd/*.hpp) include/jfgpu.h $(LIBDIR)/libjfgpu.so
	@mkdir -p bin
	@if [ -f jellyfish_amd/cli/jellyfish_amd.cc ]; then \
	  $(CXX) -O2 -std=c++17 -Wall -Iinclude -Ijellyfish_amd/include -o $@ jellyfish_amd/cli/jellyfish_amd.cc -L$(LIBDIR) -ljfgpu -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -pthread; \
	fi

oracle:
	$(MAKE) -C oracle all

clean:
	rm -rf $(LIBDIR) bin oracle/_build $(KTDIR)
.PHONY: all engine cli oracle clean kernel-harness kernel-harness-nword kernel-harness-bloom-keys
