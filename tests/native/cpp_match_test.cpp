// TEST INFRASTRUCTURE ONLY: the C++ host API's fixed-string match
// (include/nexg.hpp nexg::PatternSet, Engine::match / match_select /
// match_bufs) on the frames tests/test_cpp_match.py writes, one hex frame per
// line ("-" = empty frame).
//   --link: no device; the wrappers are instantiated and linked, the header's
//           constants, struct sizes and the builder's validation are checked
//   --gpu <file>: for each of the two sets below, with strict + VLAN parse:
//           "M <set> <frames> <selected>", per frame "R <mask hex> <first_off>
//           <first_pat>", per selected frame "S <index> <offset> <length>"
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

static std::vector<nexg::PatternSet> sets() {
    std::vector<nexg::PatternSet> s(2);
    // payloads: "host:" in any case, a leading "GET ", "mark" starting at bytes 20..22
    s[0].nocase("hOsT:", 5).prefix("GET ", 4).add("mark", 4, 0, 20, 22);
    // whole frames: the first six bytes 01..06, "xyz" anywhere
    s[1].add(std::string("\x01\x02\x03\x04\x05\x06", 6), 0, 0, 0).add("xyz", 3).frame();
    return s;
}
// what match_select is asked for per set: any, all, none
static const uint32_t kMasks[2][3] = {{0x5, 0, 0x2}, {0, 0x3, 0}};

static int run_gpu(const char* path) {
    std::vector<std::vector<uint8_t>> frames;
    std::ifstream in(path);
    for (std::string line; std::getline(in, line);)
        if (!line.empty()) frames.push_back(hex(line));
    nexg::Engine eng(0);
    nexg::ParseOption vlan;
    vlan.unwrap_vlan = true;
    const auto ps = sets();
    for (size_t si = 0; si < ps.size(); si++) {
        const auto m = eng.match_bufs(frames, ps[si], kMasks[si][0], kMasks[si][1], kMasks[si][2], vlan, nexg::ParseMode::Strict);
        printf("M %zu %zu %zu\n", si, m.rows.size(), m.index.size());
        for (const auto& r : m.rows) printf("R %08x %u %u\n", r.mask, r.first_off, r.first_pat);
        for (size_t k = 0; k < m.index.size(); k++)
            printf("S %u %llu %u\n", m.index[k], (unsigned long long)m.offsets[k], m.lengths[k]);
    }
    return 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(nexg_pattern) == 32 && sizeof(nexg_patterns) == 1032 && sizeof(nexg_match) == 8, "include/nexg.h");
    if (argc >= 3 && std::string(argv[1]) == "--gpu") {
        try {
            return run_gpu(argv[2]);
        } catch (const std::exception& e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    // --link: take the wrappers' addresses so they are instantiated and must link
    auto p1 = &nexg::Engine::match;
    auto p2 = &nexg::Engine::match_select;
    auto p3 = &nexg::Engine::match_bufs;
    const auto ps = sets();
    int ok = 0, refused = 0;
    for (const auto& s : ps) ok += nexg_patterns_check(&s.get()) == NEXG_OK;
    try {
        (void)nexg::PatternSet().get();  // no pattern
    } catch (const nexg::Error&) {
        refused++;
    }
    try {
        nexg::PatternSet bad;
        bad.add("ab", 2, 0, 5, 4);  // off_lo > off_hi
        (void)bad.get();
    } catch (const nexg::Error&) {
        refused++;
    }
    try {
        nexg::PatternSet bad;
        bad.add("ab", 2, 0x2);  // an unknown pattern flag
        (void)bad.get();
    } catch (const nexg::Error&) {
        refused++;
    }
    try {
        nexg::PatternSet bad;
        bad.add("ab", 2);
        bad.s.pat[0].reserved[9] = 1;
        (void)bad.get();
    } catch (const nexg::Error&) {
        refused++;
    }
    try {
        nexg::PatternSet bad;
        bad.add("ab", 2);
        bad.s.pat[0].bytes[2] = 'c';  // a byte past len
        (void)bad.get();
    } catch (const nexg::Error&) {
        refused++;
    }
    try {
        nexg::PatternSet bad;
        bad.add("ab", 2);
        bad.s.flags = 0x2;  // an unknown set flag
        (void)bad.get();
    } catch (const nexg::Error&) {
        refused++;
    }
    try {
        nexg::PatternSet().add("0123456789abcdefg", 17);  // 17 bytes
    } catch (const nexg::Error&) {
        refused++;
    }
    try {
        nexg::PatternSet().add("", 0);  // no byte
    } catch (const nexg::Error&) {
        refused++;
    }
    try {
        nexg::PatternSet full;
        for (int i = 0; i < 33; i++) full.add("x", 1);  // the 33rd
    } catch (const nexg::Error&) {
        refused++;
    }
    printf("link ok %d %u %u %d %d %llu\n", (p1 != nullptr) + (p2 != nullptr) + (p3 != nullptr), ps[0].s.n_patterns,
           ps[1].s.flags, ok, refused, (unsigned long long)nexg_match_select_workspace(65793));
    return 0;
}
