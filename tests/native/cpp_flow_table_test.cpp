// TEST INFRASTRUCTURE ONLY: the flow table across batches through the C header
// and the C++ host API (include/nexg.h nexg_flow_entry / the table workspace
// helper, nex_amd/csrc/workspace_layout.hpp FlowTableLayout, include/nexg.hpp
// nexg::FlowEntry, Engine::flow_table_merge / flow_table_bufs).
//   --link [n_in n_groups]...: no device; the wrappers are instantiated and
//           linked; the struct's size and field offsets are printed, and per
//           pair "workspace <n_in> <n_groups> <bytes>" from the header's helper and
//           "layout <n_in> <n_groups> <positions> <tiles> <mark> <tile_first> <bytes>" from the layout
//   --gpu <file> <size>...: the frames of <file> (one hex frame per line, "-" =
//           empty frame) cut into batches of the sizes given (the last takes
//           the rest), parsed strict + VLAN and merged one after the other,
//           epoch = the batch number, for the default option and for
//           symmetric: per batch "T <option> <epoch> <entries>", per entry
//           "E <hash hex> <kind> <proto> <flags8> <reserved> <key hex> <last_epoch> <packets> <bytes>",
//           then "S" and every group's slot, then "M" and every frame's group
#include <cstddef>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../nex_amd/csrc/workspace_layout.hpp"
#include "nexg.hpp"

static std::vector<uint8_t> hex(const std::string& s) {
    std::vector<uint8_t> b;
    if (s == "-") return b;
    for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
    return b;
}

static int run_gpu(const char* path, const std::vector<size_t>& sizes) {
    std::vector<std::vector<uint8_t>> frames;
    std::ifstream in(path);
    for (std::string line; std::getline(in, line);)
        if (!line.empty()) frames.push_back(hex(line));
    nexg::Engine eng(0);
    nexg::ParseOption vlan;
    vlan.unwrap_vlan = true;
    const nexg::FlowOption opts[2] = {nexg::FlowOption(), nexg::FlowOption().symmetric()};
    for (int oi = 0; oi < 2; oi++) {
        std::vector<nexg::FlowEntry> table;
        size_t at = 0;
        for (size_t b = 0; b <= sizes.size(); b++) {
            const size_t end = b < sizes.size() && at + sizes[b] < frames.size() ? at + sizes[b] : frames.size();
            const std::vector<std::vector<uint8_t>> batch(frames.begin() + at, frames.begin() + end);
            at = end;
            const auto u = eng.flow_table_bufs(table, batch, (uint32_t)b, 0, opts[oi], vlan, nexg::ParseMode::Strict);
            table = u.table;
            printf("T %d %zu %zu\n", oi, b, table.size());
            for (const nexg::FlowEntry& e : table) {
                printf("E %08x %u %u %u %u ", e.hash, e.kind, e.proto, e.flags8, e.reserved);
                for (uint8_t k : e.key) printf("%02x", k);
                printf(" %u %llu %llu\n", e.last_epoch, (unsigned long long)e.packets, (unsigned long long)e.bytes);
            }
            printf("S");
            for (uint32_t s : u.slot) printf(" %u", s);
            printf("\nM");
            for (uint32_t g : u.group_of) printf(" %u", g);
            printf("\n");
            if (at == frames.size()) break;
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(nexg::FlowEntry) == 64, "include/nexg.h");
    if (argc >= 3 && std::string(argv[1]) == "--gpu") {
        try {
            std::vector<size_t> sizes;
            for (int i = 3; i < argc; i++) sizes.push_back(std::stoull(argv[i]));
            return run_gpu(argv[2], sizes);
        } catch (const std::exception& e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    // --link: take the wrappers' addresses so they are instantiated and must link
    auto p1 = &nexg::Engine::flow_table_merge;
    auto p2 = &nexg::Engine::flow_table_bufs;
    printf("link ok %d\n", (p1 != nullptr) + (p2 != nullptr));
    printf("struct %zu hash %zu kind %zu proto %zu flags8 %zu reserved %zu key %zu last_epoch %zu packets %zu bytes %zu\n",
           sizeof(nexg_flow_entry), offsetof(nexg_flow_entry, hash), offsetof(nexg_flow_entry, kind),
           offsetof(nexg_flow_entry, proto), offsetof(nexg_flow_entry, flags8), offsetof(nexg_flow_entry, reserved),
           offsetof(nexg_flow_entry, key), offsetof(nexg_flow_entry, last_epoch), offsetof(nexg_flow_entry, packets),
           offsetof(nexg_flow_entry, bytes));
    printf("mixed %u align %zu\n", NEXG_FLOW_ENTRY_MIXED, alignof(nexg_flow_entry));
    for (int i = 2; i + 1 < argc; i += 2) {
        const uint64_t n_in = std::stoull(argv[i]), n_groups = std::stoull(argv[i + 1]);
        const nexg::FlowTableLayout w = nexg::FlowTableLayout::from(n_in, n_groups);
        printf("workspace %llu %llu %llu\n", (unsigned long long)n_in, (unsigned long long)n_groups,
               (unsigned long long)nexg_flow_table_workspace(n_in, n_groups));
        printf("layout %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)n_in, (unsigned long long)n_groups,
               (unsigned long long)w.positions, (unsigned long long)w.tiles, (unsigned long long)w.mark,
               (unsigned long long)w.tile_first, (unsigned long long)w.bytes);
    }
    return 0;
}
