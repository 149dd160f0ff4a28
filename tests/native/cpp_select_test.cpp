// TEST INFRASTRUCTURE ONLY: the C++ host API's frame selection and gather
// (include/nexg.hpp nexg::Filter, Engine::select / gather_plan / gather /
// gather_rows / select_bufs) on the frames tests/test_cpp_select.py writes, one
// hex frame per line ("-" = empty frame).
//   --link: no device; the wrappers are instantiated and linked, the header's
//           constants, struct sizes and the builder's validation are checked
//   --gpu <file>: for each of the three filters below, with strict + VLAN parse
//           and align 1, 4, 16: "F <filter> <align> <count> <total>", then per
//           selected frame "S <index> <rule> <offset> <length> <flags hex> <bytes hex>"
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

static std::vector<nexg::Filter> filters() {
    std::vector<nexg::Filter> f(3);
    // TCP SYNs to 10/8, UDP port 53 or 5353, a failed L4 checksum, IPv6 from 2001:db8::/32
    f[0].tcp(0x12, 0x02).dst_net4({10, 0, 0, 0}, 8);
    f[0].udp().any_port(53);
    f[0].udp().any_port(5353);
    f[0].bad_checksum_l4();
    f[0].any().src_net6({0x20, 0x01, 0x0d, 0xb8}, 32);
    f[1].udp().length(0, 100).invert();
    f[2].status(NEXG_ERR_TRUNCATED).any().proto(58);
    return f;
}

static int run_gpu(const char* path) {
    std::vector<std::vector<uint8_t>> frames;
    std::ifstream in(path);
    for (std::string line; std::getline(in, line);)
        if (!line.empty()) frames.push_back(hex(line));
    nexg::Engine eng(0);
    nexg::ParseOption vlan;
    vlan.unwrap_vlan = true;
    const auto fl = filters();
    for (size_t fi = 0; fi < fl.size(); fi++)
        for (uint32_t align : {1u, 4u, 16u}) {
            const auto s = eng.select_bufs(frames, fl[fi], vlan, nexg::ParseMode::Strict, align);
            printf("F %zu %u %zu %llu\n", fi, align, s.index.size(), (unsigned long long)s.data.size());
            for (size_t k = 0; k < s.index.size(); k++) {
                printf("S %u %u %llu %u %08x ", s.index[k], s.rule[k], (unsigned long long)s.offsets[k], s.lengths[k],
                       s.records[k].flags);
                for (uint64_t j = s.offsets[k]; j < s.offsets[k + 1]; j++) printf("%02x", s.data[j]);
                printf("\n");
            }
        }
    return 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(nexg_rule) == 64 && sizeof(nexg_filter) == 1032, "include/nexg.h");
    if (argc >= 3 && std::string(argv[1]) == "--gpu") {
        try {
            return run_gpu(argv[2]);
        } catch (const std::exception& e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    // --link: take the wrappers' addresses so they are instantiated and must link
    auto p1 = &nexg::Engine::select;
    auto p2 = &nexg::Engine::gather_plan;
    auto p3 = &nexg::Engine::gather;
    auto p4 = &nexg::Engine::gather_rows;
    auto p5 = &nexg::Engine::select_bufs;
    const auto fl = filters();
    int ok = 0, refused = 0;
    for (const auto& f : fl) ok += nexg_filter_check(&f.get()) == NEXG_OK;
    try {
        nexg::Filter bad;
        bad.any().any_port(2, 1);  // lo > hi
        (void)bad.get();
    } catch (const nexg::Error&) {
        refused++;
    }
    try {
        nexg::Filter bad;
        bad.any().src_net4({10, 0, 0, 0}, 33);
        (void)bad.get();
    } catch (const nexg::Error&) {
        refused++;
    }
    try {
        (void)nexg::Filter().get();  // no rule
    } catch (const nexg::Error&) {
        refused++;
    }
    printf("link ok %d %u %d %d %llu %llu\n", (p1 != nullptr) + (p2 != nullptr) + (p3 != nullptr) + (p4 != nullptr) + (p5 != nullptr),
           fl[0].f.n_rules, ok, refused, (unsigned long long)nexg_select_workspace(65793),
           (unsigned long long)nexg_gather_plan_workspace(65793));
    return 0;
}
