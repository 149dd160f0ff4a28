// workspace_layout.hpp — where the regions of a caller's workspace start.
//
// include/nexg.h gives each workspace's size (the nexg_*_workspace inlines, a C
// header other people compile); the structs here name the regions inside and
// give their byte offsets, and the launchers that take a workspace take every
// pointer from them. tests/native/workspace_layout_test.cpp holds the two
// against each other: equal sizes, regions aligned, disjoint and in bounds
// (FlowTableLayout: tests/test_flow_table_layout.py, through
// tests/native/cpp_flow_table_test.cpp).
// Plain host code: <stdint.h> and nexg.h only.
#pragma once
#include <stdint.h>

#include "../../include/nexg.h"

namespace nexg {

template <typename T>
inline T* region(void* workspace, uint64_t offset) {
    return reinterpret_cast<T*>(static_cast<char*>(workspace) + offset);
}

// nexg_select_workspace, nexg_decap_select_workspace and
// nexg_match_select_workspace (the order-preserving compactions): one u32 per
// 256-frame tile, rounded up to whole scan steps of 256 tiles, and 16 spare bytes
struct TileCountLayout {
    uint64_t tiles;
    uint64_t tile_count;  // u32[tiles]
    uint64_t bytes;
    static TileCountLayout from(uint64_t count) {
        TileCountLayout w;
        w.tiles = (count + 255u) / 256u;
        w.tile_count = 0;
        w.bytes = 4u * ((w.tiles + 255u) / 256u * 256u) + 16u;
        return w;
    }
};

// nexg_gather_plan_workspace and nexg_encap_plan_workspace (the two plans):
// one u64 per 256-frame tile, rounded up the same way, and 16 spare bytes
struct TileSumLayout {
    uint64_t tiles;
    uint64_t tile_sum;  // u64[tiles]
    uint64_t bytes;
    static TileSumLayout from(uint64_t count) {
        TileSumLayout w;
        w.tiles = (count + 255u) / 256u;
        w.tile_sum = 0;
        w.bytes = 8u * ((w.tiles + 255u) / 256u * 256u) + 16u;
        return w;
    }
};

// nexg_fragment_plan_workspace: two u64 per 256-frame tile, each table rounded
// up to whole scan steps of 256 tiles, then the output frames' total in the
// first 8 of the 16 spare bytes
struct FragPlanLayout {
    uint64_t tiles;
    uint64_t tile_frames;   // u64[tiles]
    uint64_t tile_bytes;    // u64[tiles]
    uint64_t frames_total;  // u64[1]
    uint64_t bytes;
    static FragPlanLayout from(uint64_t count) {
        FragPlanLayout w;
        w.tiles = (count + 255u) / 256u;
        const uint64_t table = 8u * ((w.tiles + 255u) / 256u * 256u);
        w.tile_frames = 0;
        w.tile_bytes = table;
        w.frames_total = 2u * table;
        w.bytes = 2u * table + 16u;
        return w;
    }
};

// nexg_flow_partition_workspace: the scan's total, one u32 per chunk of 1024
// counters (an even number of slots, so the counters start on 8 B), then the
// buckets x tiles counters, bucket-major
struct FlowPartLayout {
    static constexpr uint32_t kChunk = 1024u;  // counters per chunk of the scan
    uint64_t tiles, counters, chunks;
    uint64_t total;  // u64[1]
    uint64_t sums;   // u32[chunks]
    uint64_t hist;   // u32[counters]
    uint64_t bytes;
    static FlowPartLayout from(uint64_t count, uint32_t buckets) {
        FlowPartLayout w;
        w.tiles = (count + NEXG_FLOW_TILE - 1u) / NEXG_FLOW_TILE;
        w.counters = w.tiles * buckets;
        w.chunks = (w.counters + kChunk - 1u) / kChunk;
        w.total = 0;
        w.sums = 8u;
        w.hist = w.sums + 4u * ((w.chunks + 1u) & ~(uint64_t)1u);
        w.bytes = w.hist + 4u * w.counters;
        return w;
    }
};

// nexg_flow_sort_workspace: the partition's at 256 buckets (a whole number of
// 8 B), then two buffers of `count` (hash, index) pairs
struct FlowSortLayout : FlowPartLayout {
    uint64_t ping, pong;  // u64[count] each
    static FlowSortLayout from(uint64_t count) {
        FlowSortLayout w;
        static_cast<FlowPartLayout&>(w) = FlowPartLayout::from(count, 256u);
        w.ping = w.bytes;
        w.pong = w.ping + 8u * count;
        w.bytes = w.pong + 8u * count;
        return w;
    }
};

// nexg_flow_groups_workspace: the 8-B regions first, the u32 tables (an even
// number of slots each) behind them
struct FlowGroupsLayout {
    uint64_t tiles;       // of 256 sorted positions
    uint64_t totals;      // u64[2]: breaks, bytes
    uint64_t tile_bytes;  // u64[tiles]
    uint64_t mark;        // u64[count]
    uint64_t tile_heads;  // u32[tiles]
    uint64_t tile_brk;    // u32[tiles]
    uint64_t starts;      // u32[count]
    uint64_t bytes;
    static FlowGroupsLayout from(uint64_t count) {
        FlowGroupsLayout w;
        w.tiles = (count + 255u) / 256u;
        const uint64_t even_tiles = (w.tiles + 1u) & ~(uint64_t)1u;
        w.totals = 0;
        w.tile_bytes = 16u;
        w.mark = w.tile_bytes + 8u * w.tiles;
        w.tile_heads = w.mark + 8u * count;
        w.tile_brk = w.tile_heads + 4u * even_tiles;
        w.starts = w.tile_brk + 4u * even_tiles;
        w.bytes = w.starts + 4u * ((count + 1u) & ~(uint64_t)1u);
        return w;
    }
};

// nexg_reasm_plan_workspace: the sort's workspace (rounded up to 16 B), the
// 32-B classifications, the 8-B regions, then the u32 tables (an even number
// of slots each)
struct ReasmPlanLayout {
    uint64_t tiles;        // of 256 frames, and of 256 sorted positions
    uint64_t sort;         // FlowSortLayout::from(count)
    uint64_t info;         // 32 B per frame, 16-B aligned
    uint64_t key_idfo;     // u64[count]: id << 13 | fo in the low word
    uint64_t key_hash;     // u64[count]: the hash in the low word
    uint64_t mark;         // u64[count]
    uint64_t tile_bb;      // u64[tiles]: breaks | bad << 32
    uint64_t tile_frames;  // u64[tiles]
    uint64_t tile_bytes;   // u64[tiles]
    uint64_t totals;       // u64[4]: groups, breaks | bad << 32, output frames, spare
    uint64_t order;        // u32[count]
    uint64_t out_len;      // u32[count]
    uint64_t starts;       // u32[count]
    uint64_t tile_heads;   // u32[tiles]
    uint64_t bytes;
    static ReasmPlanLayout from(uint64_t count) {
        ReasmPlanLayout w;
        w.tiles = (count + 255u) / 256u;
        const uint64_t even = (count + 1u) & ~(uint64_t)1u, even_tiles = (w.tiles + 1u) & ~(uint64_t)1u;
        w.sort = 0;
        w.info = (FlowSortLayout::from(count).bytes + 15u) & ~(uint64_t)15u;
        w.key_idfo = w.info + 32u * count;
        w.key_hash = w.key_idfo + 8u * count;
        w.mark = w.key_hash + 8u * count;
        w.tile_bb = w.mark + 8u * count;
        w.tile_frames = w.tile_bb + 8u * w.tiles;
        w.tile_bytes = w.tile_frames + 8u * w.tiles;
        w.totals = w.tile_bytes + 8u * w.tiles;
        w.order = w.totals + 32u;
        w.out_len = w.order + 4u * even;
        w.starts = w.out_len + 4u * even;
        w.tile_heads = w.starts + 4u * even;
        w.bytes = w.tile_heads + 4u * even_tiles;
        return w;
    }
};

// nexg_flow_table_workspace: a u64 per position of the merged order, then a
// u32 per 256-position tile (an even number of slots)
struct FlowTableLayout {
    uint64_t positions;   // n_in + n_groups
    uint64_t tiles;       // of 256 merged positions
    uint64_t mark;        // u64[positions]
    uint64_t tile_first;  // u32[tiles]
    uint64_t bytes;
    static FlowTableLayout from(uint64_t n_in, uint64_t n_groups) {
        FlowTableLayout w;
        w.positions = n_in + n_groups;
        w.tiles = (w.positions + 255u) / 256u;
        w.mark = 0;
        w.tile_first = 8u * w.positions;
        w.bytes = w.tile_first + 4u * ((w.tiles + 1u) & ~(uint64_t)1u);
        return w;
    }
};

}  // namespace nexg
