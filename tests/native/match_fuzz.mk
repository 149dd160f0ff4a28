# TEST INFRASTRUCTURE ONLY: memory-safety + differential driver for the match core
# (nex_amd/csrc/match_core.hpp), built by tests/test_match_core.py with
# `make -f match_fuzz.mk match_fuzz`. Host code only: -Xarch_host keeps the
# sanitizers off the gfx950 side of the compile, as the parse_fuzz rule of the
# Makefile beside it does.
HIPCC ?= /opt/rocm/bin/hipcc
match_fuzz: match_fuzz.cpp ../../nex_amd/csrc/match_core.hpp ../../include/nexg.h
	@mkdir -p build
	$(HIPCC) -O1 -g -std=c++17 -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-omit-frame-pointer -c match_fuzz.cpp -o build/match_fuzz.o
	$(HIPCC) --offload-arch=gfx950 -fsanitize=address,undefined -fno-gpu-sanitize build/match_fuzz.o -o $@
