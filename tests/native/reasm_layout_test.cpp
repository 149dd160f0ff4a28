// TEST INFRASTRUCTURE ONLY: nex_amd/csrc/workspace_layout.hpp's ReasmPlanLayout
// against nexg_reasm_plan_workspace of include/nexg.h, on the host (g++, no
// HIP); tests/test_reasm_layout.py runs it.
//
// For every count: the layout's `bytes` is what the header's formula returns;
// the sort's workspace starts at 0 and ends before the first region; a region
// starts on its element's size (the 32-B classifications on 16 B); the regions,
// each with the element count its kernels index, lie inside the workspace and
// do not overlap. nexg_reasm_held_workspace is TileCountLayout's. Prints
// "bytes <count> <bytes>" per count, one line per failure and "ok <checks>" at
// the end; exit status 1 on any failure.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../nex_amd/csrc/workspace_layout.hpp"

namespace {

struct Region {
    const char* name;
    uint64_t offset, align, elem, n;
};

int failures = 0;
uint64_t checks = 0;

void expect(bool ok, const char* what, uint64_t count) {
    checks++;
    if (ok) return;
    failures++;
    printf("FAIL %s (count %llu)\n", what, (unsigned long long)count);
}

}  // namespace

int main() {
    const uint64_t counts[] = {0, 1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 65535, 65536, 65537,
                               65793, 262143, 262144, 262145, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFEull, 0xFFFFFFFFull};
    for (uint64_t count : counts) {
        const uint64_t tiles = (count + 255u) / 256u;
        const nexg::ReasmPlanLayout w = nexg::ReasmPlanLayout::from(count);
        printf("bytes %llu %llu\n", (unsigned long long)count, (unsigned long long)w.bytes);
        expect(w.tiles == tiles, "tiles", count);
        expect(w.bytes == nexg_reasm_plan_workspace(count), "bytes differ from the header's formula", count);
        expect(w.sort == 0 && nexg::FlowSortLayout::from(count).bytes == nexg_flow_sort_workspace(count), "sort", count);
        std::vector<Region> regions = {
            {"sort", w.sort, 8, 1, nexg_flow_sort_workspace(count)},
            {"info", w.info, 16, 32, count},
            {"key_idfo", w.key_idfo, 8, 8, count},
            {"key_hash", w.key_hash, 8, 8, count},
            {"mark", w.mark, 8, 8, count},
            {"tile_bb", w.tile_bb, 8, 8, tiles},
            {"tile_frames", w.tile_frames, 8, 8, tiles},
            {"tile_bytes", w.tile_bytes, 8, 8, tiles},
            {"totals", w.totals, 8, 8, 4},
            {"order", w.order, 4, 4, count},
            {"out_len", w.out_len, 4, 4, count},
            {"starts", w.starts, 4, 4, count},
            {"tile_heads", w.tile_heads, 4, 4, tiles},
        };
        for (const Region& r : regions) {
            expect(r.offset % r.align == 0, r.name, count);             // aligned
            expect(r.offset + r.elem * r.n <= w.bytes, r.name, count);  // in bounds
        }
        std::sort(regions.begin(), regions.end(), [](const Region& a, const Region& b) {
            return a.offset != b.offset ? a.offset < b.offset : a.n < b.n;  // an empty region may share its start
        });
        for (size_t i = 1; i < regions.size(); i++)
            expect(regions[i - 1].offset + regions[i - 1].elem * regions[i - 1].n <= regions[i].offset, regions[i].name,
                   count);  // disjoint
        expect(nexg::TileCountLayout::from(count).bytes == nexg_reasm_held_workspace(count), "held workspace", count);
    }
    printf("ok %llu\n", (unsigned long long)checks);
    return failures ? 1 : 0;
}
