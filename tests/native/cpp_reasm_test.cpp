// TEST INFRASTRUCTURE ONLY: the C++ host API's reassembly (include/nexg.hpp
// Engine::reassemble_plan / reassemble / reassemble_held / reassemble_bufs) on
// the frames tests/test_cpp_reasm.py writes, one hex frame per line ("-" = empty
// frame).
//   --link: no device; the wrappers are instantiated and linked, the struct
//           size and the workspace layout are checked
//   --gpu <file>: align 1, then align 16: "W <align> <frames> <output frames>
//           <total> <held>", per input frame "R <status> <kind> <hdr_len>
//           <flags> <members> <data_len> <out> <head>", per output frame "F
//           <offset> <src> <hex>", per held frame "H <index>"
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "nexg.hpp"
#include "../../nex_amd/csrc/workspace_layout.hpp"

static std::vector<uint8_t> hex(const std::string& s) {
    std::vector<uint8_t> b;
    if (s == "-") return b;
    for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
    return b;
}

static int run_gpu(const char* path) {
    std::vector<std::vector<uint8_t>> frames;
    std::ifstream in(path);
    for (std::string line; std::getline(in, line);)
        if (!line.empty()) frames.push_back(hex(line));
    nexg::Engine eng(0);
    for (uint32_t align : {1u, 16u}) {
        const auto r = eng.reassemble_bufs(frames, align);
        printf("W %u %zu %zu %llu %zu\n", align, r.rows.size(), r.lengths.size(), (unsigned long long)r.offsets.back(), r.held.size());
        for (const nexg_reasm& x : r.rows)
            printf("R %u %u %u %u %u %u %u %u\n", x.status, x.kind, x.hdr_len, x.flags, x.members, x.data_len, x.out, x.head);
        for (size_t f = 0; f < r.lengths.size(); f++) {
            printf("F %llu %u ", (unsigned long long)r.offsets[f], r.src[f]);
            if (r.lengths[f] == 0) printf("-");
            for (uint32_t k = 0; k < r.lengths[f]; k++) printf("%02x", r.data[r.offsets[f] + k]);
            printf("\n");
        }
        for (uint32_t i : r.held) printf("H %u\n", i);
    }
    return 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(nexg_reasm) == 16, "include/nexg.h");
    if (argc >= 3 && std::string(argv[1]) == "--gpu") {
        try {
            return run_gpu(argv[2]);
        } catch (const std::exception& e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    // --link: take the wrappers' addresses so they are instantiated and must link
    auto p1 = &nexg::Engine::reassemble_plan;
    auto p2 = &nexg::Engine::reassemble;
    auto p3 = &nexg::Engine::reassemble_held;
    auto p4 = &nexg::Engine::reassemble_bufs;
    int layout = 0;
    for (uint64_t count : {0ull, 1ull, 256ull, 257ull, 65536ull, 65537ull, 1ull << 24, 0xFFFFFFFFull}) {
        const nexg::ReasmPlanLayout w = nexg::ReasmPlanLayout::from(count);
        layout += w.bytes == nexg_reasm_plan_workspace(count) && w.info % 16 == 0 && w.info >= nexg_flow_sort_workspace(count) &&
                  w.tile_heads + 4 * w.tiles <= w.bytes && nexg_reasm_held_workspace(count) == nexg_select_workspace(count);
    }
    printf("link ok %d %d\n", (p1 != nullptr) + (p2 != nullptr) + (p3 != nullptr) + (p4 != nullptr), layout);
    return 0;
}
