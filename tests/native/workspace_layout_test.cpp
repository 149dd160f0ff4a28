// TEST INFRASTRUCTURE ONLY: nex_amd/csrc/workspace_layout.hpp against the size
// formulas of include/nexg.h, on the host (g++, no HIP).
//
// For every count and bucket count below: a layout's `bytes` is what the
// matching nexg_*_workspace returns; a region of u64 starts on 8 B and a region
// of u32 on 4 B; the regions, each with the element count its kernels index
// (stated here on its own: tiles of 1024 frames, chunks of 1024 counters, tiles
// of 256 sorted positions or frames), lie inside the workspace and do not overlap.
// Prints one line per failure and "ok <checks>" at the end; exit status 1 on any failure.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../nex_amd/csrc/workspace_layout.hpp"

namespace {

struct Region {
    const char* name;
    uint64_t offset, elem, n;
};

int failures = 0;
uint64_t checks = 0;

void expect(bool ok, const char* layout, const char* what, uint64_t count, uint32_t buckets) {
    checks++;
    if (ok) return;
    failures++;
    printf("FAIL %s: %s (count %llu, buckets %u)\n", layout, what, (unsigned long long)count, buckets);
}

void check(const char* layout, uint64_t count, uint32_t buckets, uint64_t bytes, uint64_t want_bytes,
           std::vector<Region> regions) {
    expect(bytes == want_bytes, layout, "bytes differ from the header's formula", count, buckets);
    for (const Region& r : regions) {
        expect(r.offset % r.elem == 0, layout, r.name, count, buckets);               // aligned to its element
        expect(r.offset + r.elem * r.n <= bytes, layout, r.name, count, buckets);  // in bounds
    }
    std::sort(regions.begin(), regions.end(), [](const Region& a, const Region& b) {
        return a.offset != b.offset ? a.offset < b.offset : a.n < b.n;  // an empty region may share its start
    });
    for (size_t i = 1; i < regions.size(); i++)
        expect(regions[i - 1].offset + regions[i - 1].elem * regions[i - 1].n <= regions[i].offset, layout,
               regions[i].name, count, buckets);  // disjoint
}

}  // namespace

int main() {
    const uint64_t counts[] = {0, 1, 255, 256, 257, 1023, 1024, 1025, 65793, 0xFFFFFFFFull};
    const uint32_t bucket_counts[] = {1, 2, 3, 255, 256};
    for (uint64_t count : counts) {
        const uint64_t tiles1024 = (count + 1023u) / 1024u, tiles256 = (count + 255u) / 256u;
        for (uint32_t buckets : bucket_counts) {
            const nexg::FlowPartLayout w = nexg::FlowPartLayout::from(count, buckets);
            const uint64_t counters = tiles1024 * buckets, chunks = (counters + 1023u) / 1024u;
            expect(w.tiles == tiles1024 && w.counters == counters && w.chunks == chunks, "FlowPartLayout",
                   "tiles, counters, chunks", count, buckets);
            check("FlowPartLayout", count, buckets, w.bytes, nexg_flow_partition_workspace(count, buckets),
                  {{"total", w.total, 8, 1}, {"sums", w.sums, 4, chunks}, {"hist", w.hist, 4, counters}});
        }
        {
            const nexg::FlowSortLayout w = nexg::FlowSortLayout::from(count);
            const uint64_t counters = tiles1024 * 256u, chunks = (counters + 1023u) / 1024u;
            expect(w.tiles == tiles1024 && w.counters == counters && w.chunks == chunks, "FlowSortLayout",
                   "tiles, counters, chunks", count, 256);
            check("FlowSortLayout", count, 256, w.bytes, nexg_flow_sort_workspace(count),
                  {{"total", w.total, 8, 1}, {"sums", w.sums, 4, chunks}, {"hist", w.hist, 4, counters},
                   {"ping", w.ping, 8, count}, {"pong", w.pong, 8, count}});
        }
        {
            const nexg::FlowGroupsLayout w = nexg::FlowGroupsLayout::from(count);
            expect(w.tiles == tiles256, "FlowGroupsLayout", "tiles", count, 0);
            check("FlowGroupsLayout", count, 0, w.bytes, nexg_flow_groups_workspace(count),
                  {{"totals", w.totals, 8, 2}, {"tile_bytes", w.tile_bytes, 8, tiles256}, {"mark", w.mark, 8, count},
                   {"tile_heads", w.tile_heads, 4, tiles256}, {"tile_brk", w.tile_brk, 4, tiles256},
                   {"starts", w.starts, 4, count}});
        }
        // the tile tables of the compactions and the plans: k_tile_scan touches
        // `tiles` entries; the total goes to the caller's own slot, or (the
        // fragment plan's frame total) to the first 8 spare bytes
        for (uint64_t want : {nexg_select_workspace(count), nexg_decap_select_workspace(count),
                              nexg_match_select_workspace(count)}) {
            const nexg::TileCountLayout w = nexg::TileCountLayout::from(count);
            expect(w.tiles == tiles256, "TileCountLayout", "tiles", count, 0);
            check("TileCountLayout", count, 0, w.bytes, want, {{"tile_count", w.tile_count, 4, tiles256}});
        }
        for (uint64_t want : {nexg_gather_plan_workspace(count), nexg_encap_plan_workspace(count)}) {
            const nexg::TileSumLayout w = nexg::TileSumLayout::from(count);
            expect(w.tiles == tiles256, "TileSumLayout", "tiles", count, 0);
            check("TileSumLayout", count, 0, w.bytes, want, {{"tile_sum", w.tile_sum, 8, tiles256}});
        }
        {
            const nexg::FragPlanLayout w = nexg::FragPlanLayout::from(count);
            expect(w.tiles == tiles256, "FragPlanLayout", "tiles", count, 0);
            check("FragPlanLayout", count, 0, w.bytes, nexg_fragment_plan_workspace(count),
                  {{"tile_frames", w.tile_frames, 8, tiles256}, {"tile_bytes", w.tile_bytes, 8, tiles256},
                   {"frames_total", w.frames_total, 8, 1}});
        }
    }
    printf("ok %llu\n", (unsigned long long)checks);
    return failures ? 1 : 0;
}
