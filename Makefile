# Builds libdwpa22000.so (HIP for gfx950 + host C++) in-tree, and the CPU parity oracle (test infrastructure).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CXXFLAGS ?= -O3 -std=c++17 -fPIC -Wall -Wno-unused-function
SRC := dwpa_amd/csrc
OBJ := build/obj
LIB := dwpa_amd/lib/libdwpa22000.so
HDRS := $(wildcard $(SRC)/*.hpp) include/dwpa22000.h
OBJS := $(OBJ)/kernels.o $(OBJ)/rules_dev.o $(OBJ)/engine.o $(OBJ)/m22000_host.o $(OBJ)/crack.o $(OBJ)/rules.o \
        $(OBJ)/pbkdf2_module.o $(OBJ)/pbkdf2_hsaco.o $(OBJ)/host_crypto.o $(OBJ)/host_check.o \
        $(OBJ)/mask.o $(OBJ)/mask_dev.o $(OBJ)/crack_common.o $(OBJ)/hybrid_dev.o \
        $(OBJ)/combi_dev.o $(OBJ)/chain.o $(OBJ)/chain_dev.o $(OBJ)/chain_rules_dev.o \
        $(OBJ)/crack_range.o $(OBJ)/markov.o $(OBJ)/markov_dev.o $(OBJ)/table.o $(OBJ)/table_dev.o \
        $(OBJ)/assoc.o $(OBJ)/assoc_dev.o
LLVM := /opt/rocm/lib/llvm/bin
ISSUE_RULE ?= sched=1:alt:orig:asmnop,before_half
# 1: the two work-queue PBKDF2 kernels keep their cold words in LDS (pbkdf2_dev.hpp pbkdf2_lane_lds); 0: the plain lane
QUEUE_LDS ?= 1

all: $(LIB) oracle

$(OBJ)/%.o: $(SRC)/%.hip $(HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -Iinclude -c $< -o $@

$(OBJ)/%.o: $(SRC)/%.cpp $(HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -Iinclude -c $< -o $@

# product PBKDF2 kernel: hipcc -> gfx950 asm -> VALU issue pass -> code object -> embedded byte array
build/pbkdf2/pbkdf2_gfx950.s: $(SRC)/pbkdf2_gfx950.hip $(SRC)/pbkdf2_dev.hpp $(SRC)/crypto_dev.hpp
	@mkdir -p build/pbkdf2
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 --cuda-device-only -DDWPA_QUEUE_LDS=$(QUEUE_LDS) -S $< -o $@

PBKDF2_QUEUE_KERNELS := k_pbkdf2_gfx950_q+k_pbkdf2_gfx950_mg_q
PBKDF2_KERNELS := k_pbkdf2_gfx950+k_pbkdf2_gfx950_ms+k_pbkdf2_gfx950_mg+k_pbkdf2_gfx950_p+k_pbkdf2_gfx950_ms_p+k_pbkdf2_gfx950_mg_p+k_pbkdf2_gfx950_q+k_pbkdf2_gfx950_mg_q

# the pass fails closed (an instruction it cannot model stops the build) ...
build/pbkdf2/pbkdf2_issue.s: build/pbkdf2/pbkdf2_gfx950.s $(SRC)/gen/issue_pass.py Makefile
	python3 $(SRC)/gen/issue_pass.py $< $@ $(PBKDF2_KERNELS) $(ISSUE_RULE)

# ... and every scheduled loop must compute the compiler's results (tools/issue_equiv.py) before the code object links
build/pbkdf2/issue_equiv.ok: build/pbkdf2/pbkdf2_gfx950.s build/pbkdf2/pbkdf2_issue.s tools/issue_equiv.py
	python3 tools/issue_equiv.py $< $(PBKDF2_KERNELS) $(ISSUE_RULE) 2
	@touch $@

# ... and the LDS work-queue kernels must fit (64 VGPRs, no scratch, 8 waves per SIMD, 16 KiB LDS, five no-return LDS
# xors and no memory access in the loop): a kernel that spills is not linked
build/pbkdf2/queue_lds_gate.ok: build/pbkdf2/pbkdf2_issue.s tools/kernel_asm.py
ifeq ($(QUEUE_LDS),1)
	python3 tools/kernel_asm.py gate $< $(PBKDF2_QUEUE_KERNELS)
endif
	@touch $@

build/pbkdf2/pbkdf2_gfx950.hsaco: build/pbkdf2/pbkdf2_issue.s build/pbkdf2/issue_equiv.ok build/pbkdf2/queue_lds_gate.ok
	$(LLVM)/clang -target amdgcn-amd-amdhsa -mcpu=$(ARCH) -c $< -o build/pbkdf2/pbkdf2_issue.o
	$(LLVM)/ld.lld -shared build/pbkdf2/pbkdf2_issue.o -o $@

build/pbkdf2/pbkdf2_hsaco.cpp: build/pbkdf2/pbkdf2_gfx950.hsaco $(SRC)/gen/embed.py
	python3 $(SRC)/gen/embed.py $< $@ pbkdf2_gfx950_hsaco

$(OBJ)/pbkdf2_hsaco.o: build/pbkdf2/pbkdf2_hsaco.cpp
	@mkdir -p $(OBJ)
	$(HIPCC) $(CXXFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	@mkdir -p dwpa_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -lz -lpthread

oracle:
	$(MAKE) -s -C oracle

asm: $(SRC)/kernels.hip $(SRC)/mask_dev.hip $(SRC)/hybrid_dev.hip $(SRC)/combi_dev.hip $(SRC)/chain_dev.hip \
     $(SRC)/chain_rules_dev.hip $(SRC)/rules_dev.hip $(SRC)/markov_dev.hip $(SRC)/table_dev.hip $(SRC)/assoc_dev.hip $(HDRS)
	@mkdir -p build/asm
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -Iinclude -c $< -o build/asm/kernels.o -save-temps=obj -Rpass-analysis=kernel-resource-usage
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -Iinclude -c $(SRC)/mask_dev.hip -o build/asm/mask_dev.o -save-temps=obj -Rpass-analysis=kernel-resource-usage
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -Iinclude -c $(SRC)/hybrid_dev.hip -o build/asm/hybrid_dev.o -save-temps=obj -Rpass-analysis=kernel-resource-usage
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -Iinclude -c $(SRC)/combi_dev.hip -o build/asm/combi_dev.o -save-temps=obj -Rpass-analysis=kernel-resource-usage
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -Iinclude -c $(SRC)/chain_dev.hip -o build/asm/chain_dev.o -save-temps=obj -Rpass-analysis=kernel-resource-usage
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -Iinclude -c $(SRC)/chain_rules_dev.hip -o build/asm/chain_rules_dev.o -save-temps=obj -Rpass-analysis=kernel-resource-usage
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -Iinclude -c $(SRC)/rules_dev.hip -o build/asm/rules_dev.o -save-temps=obj -Rpass-analysis=kernel-resource-usage
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -Iinclude -c $(SRC)/markov_dev.hip -o build/asm/markov_dev.o -save-temps=obj -Rpass-analysis=kernel-resource-usage
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -Iinclude -c $(SRC)/table_dev.hip -o build/asm/table_dev.o -save-temps=obj -Rpass-analysis=kernel-resource-usage
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -Iinclude -c $(SRC)/assoc_dev.hip -o build/asm/assoc_dev.o -save-temps=obj -Rpass-analysis=kernel-resource-usage

clean:
	rm -rf build $(LIB)
	$(MAKE) -s -C oracle clean

.PHONY: all oracle clean asm

tools: tools/bin/valu_peak tools/bin/pbkdf2_lab tools/bin/valu_lat tools/bin/valu_peak64 tools/bin/inflate_bench \
       tools/bin/inflate_check tools/bin/item_queue_check tools/bin/rules_fuzz_asan tools/bin/clock_idle \
       tools/bin/inflate_check_tsan tools/bin/tail_placement tools/bin/parse_fuzz_asan tools/bin/host_check_fuzz_asan tools/bin/host_pbkdf2_paths tools/bin/vgpr_bank \
       tools/bin/mask_fuzz_asan tools/bin/chain_fuzz_asan tools/bin/range_cursor_check tools/bin/markov_fuzz_asan \
       tools/bin/table_fuzz_asan tools/bin/assoc_fuzz_asan

tools/bin/valu_lat: tools/valu_lat.hip
	@mkdir -p tools/bin
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -o $@ $<

tools/bin/pbkdf2_lab: tools/pbkdf2_lab.hip dwpa_amd/csrc/crypto_dev.hpp
	@mkdir -p tools/bin
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -o $@ $<

tools/bin/valu_peak: tools/valu_peak.hip
	@mkdir -p tools/bin
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -o $@ $<

.PHONY: tools

tools/bin/valu_peak64: tools/valu_peak64.hip
	@mkdir -p tools/bin
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -o $@ $<

tools/bin/inflate_bench: tools/inflate_bench.cpp $(SRC)/dict_reader.hpp $(SRC)/inflate.hpp $(SRC)/pinflate.hpp $(SRC)/m22000_host.cpp \
                         $(SRC)/m22000_host.hpp
	@mkdir -p tools/bin
	g++ -O3 -std=c++17 -Iinclude -I$(SRC) -o $@ tools/inflate_bench.cpp $(SRC)/m22000_host.cpp -lz -lpthread

tools/bin/inflate_check: tools/inflate_check.cpp $(SRC)/inflate.hpp $(SRC)/pinflate.hpp
	@mkdir -p tools/bin
	g++ -O3 -std=c++17 -Wall -I$(SRC) -o $@ tools/inflate_check.cpp -lz -lpthread

tools/bin/item_queue_check: tools/item_queue_check.cpp $(SRC)/dict_reader.hpp $(SRC)/inflate.hpp $(SRC)/pinflate.hpp \
                            $(SRC)/m22000_host.cpp $(SRC)/m22000_host.hpp
	@mkdir -p tools/bin
	g++ -O2 -std=c++17 -Wall -Iinclude -I$(SRC) -o $@ tools/item_queue_check.cpp $(SRC)/m22000_host.cpp -lz -lpthread

# host fuzz of the rule engine under AddressSanitizer + UBSan (host code only: -fsanitize after -Xarch_host)
tools/bin/rules_fuzz_asan: tools/rules_fuzz.cpp $(SRC)/rules.cpp $(SRC)/rules.hpp $(SRC)/rules_apply.hpp
	@mkdir -p tools/bin
	$(HIPCC) -O1 -g -std=c++17 -Iinclude -I$(SRC) -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
	    -o $@ tools/rules_fuzz.cpp $(SRC)/rules.cpp

# host fuzz of the mask language (parser, keyspace, candidates) under AddressSanitizer + UBSan: mask.cpp alone
tools/bin/mask_fuzz_asan: tools/mask_fuzz.cpp $(SRC)/mask.cpp $(SRC)/mask.hpp include/dwpa22000.h
	@mkdir -p tools/bin
	$(HIPCC) -O1 -g -std=c++17 -Iinclude -I$(SRC) -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
	    -o $@ tools/mask_fuzz.cpp $(SRC)/mask.cpp

# host fuzz of the Markov model (loader, thresholded keyspace, candidates, table image) under AddressSanitizer + UBSan
tools/bin/markov_fuzz_asan: tools/markov_fuzz.cpp $(SRC)/markov.cpp $(SRC)/markov.hpp $(SRC)/mask.cpp $(SRC)/mask.hpp \
                            $(SRC)/dict_reader.hpp $(SRC)/m22000_host.cpp $(SRC)/m22000_host.hpp include/dwpa22000.h
	@mkdir -p tools/bin
	$(HIPCC) -O1 -g -std=c++17 -Iinclude -I$(SRC) -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
	    -o $@ tools/markov_fuzz.cpp $(SRC)/markov.cpp $(SRC)/mask.cpp $(SRC)/m22000_host.cpp -lz -lpthread

# host fuzz of the table attack (parser, saturating counts, index, candidates) under AddressSanitizer + UBSan:
# table.cpp alone
tools/bin/table_fuzz_asan: tools/table_fuzz.cpp $(SRC)/table.cpp $(SRC)/table.hpp include/dwpa22000.h
	@mkdir -p tools/bin
	$(HIPCC) -O1 -g -std=c++17 -Iinclude -I$(SRC) -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
	    -o $@ tools/table_fuzz.cpp $(SRC)/table.cpp

# the association attack's host side (file parser, single generator, nets, entries, start[], candidates) over the
# fixtures and random plans under AddressSanitizer + UBSan: assoc.cpp with the rule engine and the line parser
tools/bin/assoc_fuzz_asan: tools/assoc_fuzz.cpp $(SRC)/assoc.cpp $(SRC)/assoc.hpp $(SRC)/rules.cpp $(SRC)/rules.hpp \
                           $(SRC)/rules_apply.hpp $(SRC)/dict_reader.hpp $(SRC)/m22000_host.cpp $(SRC)/m22000_host.hpp
	@mkdir -p tools/bin
	$(HIPCC) -O1 -g -std=c++17 -Iinclude -I$(SRC) -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
	    -o $@ tools/assoc_fuzz.cpp $(SRC)/assoc.cpp $(SRC)/rules.cpp $(SRC)/m22000_host.cpp -lz -lpthread

# host fuzz of the chain attack's keyspace / split arithmetic under AddressSanitizer + UBSan: chain.cpp alone
tools/bin/chain_fuzz_asan: tools/chain_fuzz.cpp $(SRC)/chain.cpp $(SRC)/chain.hpp include/dwpa22000.h
	@mkdir -p tools/bin
	$(HIPCC) -O1 -g -std=c++17 -Iinclude -I$(SRC) -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
	    -o $@ tools/chain_fuzz.cpp $(SRC)/chain.cpp

tools/bin/parse_fuzz_asan: tools/parse_fuzz.cpp $(SRC)/m22000_host.cpp $(SRC)/m22000_host.hpp $(SRC)/tables.hpp
	@mkdir -p tools/bin
	$(HIPCC) -O1 -g -std=c++17 -Iinclude -I$(SRC) -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
	    -o $@ tools/parse_fuzz.cpp $(SRC)/m22000_host.cpp

# host fuzz of the host backend's check path under AddressSanitizer + UBSan (the engine's thread pool stubbed)
tools/bin/host_check_fuzz_asan: tools/host_check_fuzz.cpp $(SRC)/host_check.cpp $(SRC)/host_crypto.cpp \
                                $(SRC)/host_crypto.hpp $(SRC)/m22000_host.cpp $(SRC)/m22000_host.hpp $(SRC)/engine.hpp
	@mkdir -p tools/bin
	$(HIPCC) -O1 -g -std=c++17 -Iinclude -I$(SRC) -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
	    -o $@ tools/host_check_fuzz.cpp $(SRC)/host_check.cpp $(SRC)/host_crypto.cpp $(SRC)/m22000_host.cpp -lpthread

# one thread's time per call of each host PBKDF2 loop (SHA-NI 1/2/4 chains, AVX-512 1/2/3 registers, scalar)
tools/bin/host_pbkdf2_paths: tools/host_pbkdf2_paths.cpp $(SRC)/host_crypto.cpp $(SRC)/host_crypto.hpp
	@mkdir -p tools/bin
	$(HIPCC) -O3 -std=c++17 -Iinclude -I$(SRC) -o $@ tools/host_pbkdf2_paths.cpp

tools/bin/clock_idle: tools/clock_idle.hip
	@mkdir -p tools/bin
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -o $@ $<

tools/bin/vgpr_bank: tools/vgpr_bank.hip
	@mkdir -p tools/bin
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -o $@ $<

tools/bin/tail_placement: tools/tail_placement.hip
	@mkdir -p tools/bin
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -o $@ $<

# the parallel inflate (loader thread + workers + the reader) under ThreadSanitizer
tools/bin/inflate_check_tsan: tools/inflate_check.cpp $(SRC)/inflate.hpp $(SRC)/pinflate.hpp
	@mkdir -p tools/bin
	g++ -O1 -g -std=c++17 -Wall -I$(SRC) -fsanitize=thread -DDWPA_PINFLATE_LOAD_STEP=16384 -o $@ tools/inflate_check.cpp \
	    -lz -lpthread

# the range attacks' shared cursor (crack_cursor.hpp) with concurrent takers under ThreadSanitizer
tools/bin/range_cursor_check: tools/range_cursor_check.cpp $(SRC)/crack_cursor.hpp
	@mkdir -p tools/bin
	g++ -O1 -g -std=c++17 -Wall -I$(SRC) -fsanitize=thread -o $@ tools/range_cursor_check.cpp -lpthread
