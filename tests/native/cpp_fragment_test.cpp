// TEST INFRASTRUCTURE ONLY: the C++ host API's fragmentation (include/nexg.hpp
// nexg::FragOption, Engine::fragment_plan / fragment / fragment_bufs) on the
// frames tests/test_cpp_fragment.py writes, one hex frame per line ("-" = empty
// frame).
//   --link: no device; the wrappers are instantiated and linked, the struct
//           sizes, the workspace layout and the builder's validation are checked
//   --gpu <file>: mtu 576 with align 1, then mtu 1500 under IGNORE_DF with align
//           16: "W <mtu> <align> <frames> <output frames> <total>", per input
//           frame "R <status> <kind> <hdr_len> <pieces> <piece_data> <first>",
//           per output frame "F <offset> <src> <hex>"
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
    const nexg::FragOption options[2] = {nexg::FragOption(576), nexg::FragOption(1500).ignore_df().align(16)};
    for (const nexg::FragOption& o : options) {
        const auto r = eng.fragment_bufs(frames, o);
        printf("W %u %u %zu %zu %llu\n", o.o.mtu, o.o.align, r.rows.size(), r.lengths.size(), (unsigned long long)r.offsets.back());
        for (const nexg_fragged& x : r.rows) printf("R %u %u %u %u %u %u\n", x.status, x.kind, x.hdr_len, x.pieces, x.piece_data, x.first);
        for (size_t f = 0; f < r.lengths.size(); f++) {
            printf("F %llu %u ", (unsigned long long)r.offsets[f], r.src[f]);
            if (r.lengths[f] == 0) printf("-");
            for (uint32_t k = 0; k < r.lengths[f]; k++) printf("%02x", r.data[r.offsets[f] + k]);
            printf("\n");
        }
    }
    return 0;
}

template <class F>
static int refuses(F f) {
    try {
        f();
    } catch (const nexg::Error&) {
        return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(nexg_frag_option) == 16 && sizeof(nexg_fragged) == 16, "include/nexg.h");
    if (argc >= 3 && std::string(argv[1]) == "--gpu") {
        try {
            return run_gpu(argv[2]);
        } catch (const std::exception& e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    // --link: take the wrappers' addresses so they are instantiated and must link
    auto p1 = &nexg::Engine::fragment_plan;
    auto p2 = &nexg::Engine::fragment;
    auto p3 = &nexg::Engine::fragment_bufs;
    int ok = 0, refused = 0, layout = 0;
    ok += nexg_frag_option_check(&nexg::FragOption(68).get()) == NEXG_OK;
    ok += nexg_frag_option_check(&nexg::FragOption(65535).ignore_df().align(16).get()) == NEXG_OK;
    ok += nexg::FragOption(1500).ignore_df().ignore_df(false).get().flags == 0;
    refused += refuses([] { (void)nexg::FragOption(67).get(); });              // below RFC 791's minimum
    refused += refuses([] { (void)nexg::FragOption(65536).get(); });           // past the total length field
    refused += refuses([] { (void)nexg::FragOption(1500).align(2).get(); });
    refused += refuses([] { (void)nexg::FragOption(1500).align(0).get(); });
    refused += refuses([] { (void)nexg::FragOption(1500).align(32).get(); });
    refused += refuses([] { nexg::FragOption o(1500); o.o.flags = 2; (void)o.get(); });     // unknown flag
    refused += refuses([] { nexg::FragOption o(1500); o.o.reserved = 1; (void)o.get(); });
    // the workspace's regions against the header's size: aligned, disjoint, in bounds
    for (uint64_t count : {0ull, 1ull, 256ull, 257ull, 65536ull, 65537ull, 1ull << 24, 0xFFFFFFFFull}) {
        const nexg::FragPlanLayout w = nexg::FragPlanLayout::from(count);
        const uint64_t table = 8u * ((w.tiles + 255u) / 256u * 256u);  // each table: whole scan steps of 256 tiles
        layout += w.bytes == nexg_fragment_plan_workspace(count) && w.tile_frames % 8 == 0 && w.tile_bytes % 8 == 0 &&
                  w.frames_total % 8 == 0 && w.tile_frames + 8 * w.tiles <= w.tile_bytes && w.tile_bytes + 8 * w.tiles <= w.frames_total &&
                  w.frames_total + 8 <= w.bytes && table >= 8 * w.tiles;
    }
    printf("link ok %d %d %d %d\n", (p1 != nullptr) + (p2 != nullptr) + (p3 != nullptr), ok, refused, layout);
    return 0;
}
