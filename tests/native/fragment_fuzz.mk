# TEST INFRASTRUCTURE ONLY: memory-safety + differential driver for the fragmentation core
# (nex_amd/csrc/fragment_core.hpp), built by tests/test_fragment_core.py with
# `make -f fragment_fuzz.mk fragment_fuzz`. Host code only: -Xarch_host keeps the
# sanitizers off the gfx950 side of the compile, as encap_fuzz.mk beside it does.
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../nex_amd/csrc
fragment_fuzz: fragment_fuzz.cpp $(CSRC)/fragment_core.hpp $(CSRC)/encap_core.hpp $(CSRC)/frame_core.hpp ../../include/nexg.h
	@mkdir -p build
	$(HIPCC) -O1 -g -std=c++17 -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-omit-frame-pointer -c fragment_fuzz.cpp -o build/fragment_fuzz.o
	$(HIPCC) --offload-arch=gfx950 -fsanitize=address,undefined -fno-gpu-sanitize build/fragment_fuzz.o -o $@
