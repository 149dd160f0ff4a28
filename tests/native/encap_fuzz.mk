# TEST INFRASTRUCTURE ONLY: memory-safety + differential driver for the encapsulation core
# (nex_amd/csrc/encap_core.hpp), built by tests/test_encap_core.py with
# `make -f encap_fuzz.mk encap_fuzz`. Host code only: -Xarch_host keeps the
# sanitizers off the gfx950 side of the compile, as rewrite_fuzz.mk beside it does.
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../nex_amd/csrc
encap_fuzz: encap_fuzz.cpp $(CSRC)/encap_core.hpp $(CSRC)/frame_core.hpp ../../include/nexg.h
	@mkdir -p build
	$(HIPCC) -O1 -g -std=c++17 -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-omit-frame-pointer -c encap_fuzz.cpp -o build/encap_fuzz.o
	$(HIPCC) --offload-arch=gfx950 -fsanitize=address,undefined -fno-gpu-sanitize build/encap_fuzz.o -o $@
