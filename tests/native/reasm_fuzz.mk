# TEST INFRASTRUCTURE ONLY: the reassembly pass's two stand-alone host programs.
#   reasm_fuzz          memory-safety + differential driver for the reassembly core
#                       (nex_amd/csrc/reasm_core.hpp), built by tests/test_reasm_core.py with
#                       `make -f reasm_fuzz.mk reasm_fuzz`. Host code only: -Xarch_host keeps the
#                       sanitizers off the gfx950 side of the compile, as fragment_fuzz.mk does.
#   reasm_layout_test   ReasmPlanLayout against include/nexg.h's formula (tests/test_reasm_layout.py)
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../nex_amd/csrc
reasm_fuzz: reasm_fuzz.cpp $(CSRC)/reasm_core.hpp $(CSRC)/fragment_core.hpp $(CSRC)/encap_core.hpp $(CSRC)/frame_core.hpp ../../include/nexg.h
	@mkdir -p build
	$(HIPCC) -O1 -g -std=c++17 -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-omit-frame-pointer -c reasm_fuzz.cpp -o build/reasm_fuzz.o
	$(HIPCC) --offload-arch=gfx950 -fsanitize=address,undefined -fno-gpu-sanitize build/reasm_fuzz.o -o $@

reasm_layout_test: reasm_layout_test.cpp $(CSRC)/workspace_layout.hpp ../../include/nexg.h
	g++ -O1 -std=c++17 -Wall -Werror -o $@ reasm_layout_test.cpp
