// TEST INFRASTRUCTURE ONLY: the C++ host API's flow rows and flow-affine
// partition (include/nexg.hpp nexg::FlowOption, Engine::flow / flow_partition /
// flow_bufs) on the frames tests/test_cpp_flow.py writes, one hex frame per
// line ("-" = empty frame).
//   --link: no device; the wrappers are instantiated and linked, the header's
//           struct sizes, the option builder and the workspace helper are checked
//   --gpu <file>: with strict + VLAN parse and 8 buckets, for the default
//           option and for symmetric: "O <option> <count>", per frame
//           "R <hash hex> <kind> <proto> <swapped> <bucket>", then "I" and the
//           frame numbers in bucket order, then "B" and bucket_first
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
        const auto f = eng.flow_bufs(frames, 8, opts[oi], vlan, nexg::ParseMode::Strict);
        printf("O %d %zu\n", oi, f.flows.size());
        for (size_t i = 0; i < f.flows.size(); i++)
            printf("R %08x %u %u %u %u\n", f.flows[i].hash, f.flows[i].kind, f.flows[i].proto, f.flows[i].swapped, f.bucket[i]);
        printf("I");
        for (uint32_t i : f.index) printf(" %u", i);
        printf("\nB");
        for (uint64_t b : f.bucket_first) printf(" %llu", (unsigned long long)b);
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(nexg_flow) == 8 && sizeof(nexg_flow_option) == 48, "include/nexg.h");
    if (argc >= 3 && std::string(argv[1]) == "--gpu") {
        try {
            return run_gpu(argv[2]);
        } catch (const std::exception& e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    // --link: take the wrappers' addresses so they are instantiated and must link
    auto p1 = &nexg::Engine::flow;
    auto p2 = &nexg::Engine::flow_partition;
    auto p3 = &nexg::Engine::flow_bufs;
    std::array<uint8_t, 40> k{};
    k[39] = 7;
    const nexg::FlowOption o = nexg::FlowOption().symmetric().no_ports().key(k).no_ports(false);
    printf("link ok %d %u %u %llu %llu %llu\n", (p1 != nullptr) + (p2 != nullptr) + (p3 != nullptr), o.get().flags,
           o.get().key[39], (unsigned long long)nexg_flow_partition_workspace(65793, 8),
           (unsigned long long)nexg_flow_partition_workspace(65793, 256),
           (unsigned long long)nexg_flow_partition_workspace(0, 1));
    return 0;
}
