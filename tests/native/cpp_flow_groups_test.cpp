// TEST INFRASTRUCTURE ONLY: the C++ host API's per-flow counters
// (include/nexg.hpp nexg::FlowGroup, Engine::flow_sort / flow_groups /
// flow_group_bufs) on the frames tests/test_gpu_flow_groups.py writes, one hex
// frame per line ("-" = empty frame).
//   --link: no device; the wrappers are instantiated and linked, and the
//           header's struct size, field offsets and workspace helpers are printed
//   --gpu <file>: with strict + VLAN parse, for the default option and for
//           symmetric: "O <option> <count> <groups>", per group
//           "G <hash hex> <kind> <proto> <flags8> <first> <packets> <bytes> <mixed> <first_index>",
//           then "I" and the frame numbers in sorted order, then "M" and every
//           frame's group number
#include <cstddef>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "nexg.hpp"

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
    nexg::ParseOption vlan;
    vlan.unwrap_vlan = true;
    const nexg::FlowOption opts[2] = {nexg::FlowOption(), nexg::FlowOption().symmetric()};
    for (int oi = 0; oi < 2; oi++) {
        const auto f = eng.flow_group_bufs(frames, opts[oi], vlan, nexg::ParseMode::Strict);
        printf("O %d %zu %zu\n", oi, f.order.size(), f.groups.size());
        for (const nexg::FlowGroup& g : f.groups)
            printf("G %08x %u %u %u %u %u %llu %u %u\n", g.hash, g.kind, g.proto, g.flags8, g.first, g.packets,
                   (unsigned long long)g.bytes, g.mixed, g.first_index);
        printf("I");
        for (uint32_t i : f.order) printf(" %u", i);
        printf("\nM");
        for (uint32_t g : f.group_of) printf(" %u", g);
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(nexg::FlowGroup) == 32, "include/nexg.h");
    if (argc >= 3 && std::string(argv[1]) == "--gpu") {
        try {
            return run_gpu(argv[2]);
        } catch (const std::exception& e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    // --link: take the wrappers' addresses so they are instantiated and must link
    auto p1 = &nexg::Engine::flow_sort;
    auto p2 = &nexg::Engine::flow_groups;
    auto p3 = &nexg::Engine::flow_group_bufs;
    printf("link ok %d\n", (p1 != nullptr) + (p2 != nullptr) + (p3 != nullptr));
    printf("struct %zu hash %zu kind %zu proto %zu flags8 %zu reserved %zu first %zu packets %zu bytes %zu mixed %zu "
           "first_index %zu\n",
           sizeof(nexg_flow_group), offsetof(nexg_flow_group, hash), offsetof(nexg_flow_group, kind),
           offsetof(nexg_flow_group, proto), offsetof(nexg_flow_group, flags8), offsetof(nexg_flow_group, reserved),
           offsetof(nexg_flow_group, first), offsetof(nexg_flow_group, packets), offsetof(nexg_flow_group, bytes),
           offsetof(nexg_flow_group, mixed), offsetof(nexg_flow_group, first_index));
    for (int i = 2; i < argc; i++) {
        const uint64_t n = std::stoull(argv[i]);
        printf("workspace %llu %llu %llu\n", (unsigned long long)n, (unsigned long long)nexg_flow_sort_workspace(n),
               (unsigned long long)nexg_flow_groups_workspace(n));
    }
    return 0;
}
