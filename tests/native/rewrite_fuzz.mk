# TEST INFRASTRUCTURE ONLY: memory-safety + differential driver for the rewrite core
# (nex_amd/csrc/rewrite_core.hpp), built by tests/test_rewrite_core.py with
# `make -f rewrite_fuzz.mk rewrite_fuzz`. Host code only: -Xarch_host keeps the
# sanitizers off the gfx950 side of the compile, as match_fuzz.mk beside it does.
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../nex_amd/csrc
rewrite_fuzz: rewrite_fuzz.cpp $(CSRC)/rewrite_core.hpp $(CSRC)/checksum_core.hpp $(CSRC)/frame_core.hpp ../../include/nexg.h
	@mkdir -p build
	$(HIPCC) -O1 -g -std=c++17 -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-omit-frame-pointer -c rewrite_fuzz.cpp -o build/rewrite_fuzz.o
	$(HIPCC) --offload-arch=gfx950 -fsanitize=address,undefined -fno-gpu-sanitize build/rewrite_fuzz.o -o $@
