// nexg_internal.hpp — host-side launch interfaces shared between the kernel
// translation units and the C ABI (nexg_api.hip). Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nexg.h"

namespace nexg {

struct ParseArgs {
    const uint8_t* data;
    uint64_t data_bytes;
    const uint64_t* offsets;
    const uint32_t* lengths;
    uint32_t stride;
    uint64_t count;
    uint32_t opt_flags;
    uint32_t ip_offset;
    void* out;
    uint32_t tile_order = 0;  // fixed-stride tiles: 0 in grid order, 1 XCD-contiguous
    uint32_t hints = 0;       // NEXG_FRAMES_* (include/nexg.h)
    uint32_t* tail = nullptr; // TwoPass tail-sum hand-off (count entries) for outputs
                              // narrower than 4 B per frame; null -> the output itself
    uint64_t* stamps = nullptr;  // k_parse_span<..., TIMING>: 8 clock stamps per workgroup
    uint8_t* grouped_heads = nullptr;  // span kernel, NEXG_OUT_GROUPED run as SPARSE at the code offset: head bytes
                                       // (all NEXG_GROUPED_TILE_RUN: exceptions in one run per 256-frame tile)
    const uint64_t* off_bases = nullptr;  // NEXG_FRAMES_OFFSETS32 over 4 GiB: one full offset per 256 frames
};

// Kernel variants of the parse path, as choose_parse_variant
// returns them. (NEXG_OUT_SLICE stages any other layout in a per-lane 128-B
// window, k_parse<1, ...>: launch_slice picks it, no variant names it.)
enum class ParseVariant {
    TileStride64,   // fixed 64-B stride: coalesced tile staging into LDS
    TileStride,     // fixed stride (multiple of 16, <= 128): tile staging
    TwoPass,        // any layout: k_tail_sums (bytes past 80) + k_parse_lane80
    SpanTile,       // packed layouts: 16-KiB sub-tiles through LDS + chunk prefix sums
};

hipError_t launch_parse(ParseVariant v, const ParseArgs& a, int out_kind, hipStream_t s);
// nexg_probe_span_clock: the span kernel's stamped instance (grouped output)
hipError_t launch_span_clock(const ParseArgs& a, hipStream_t s);
// TwoPass hands each frame's tail sum to pass 2 through its own output
// element; outputs narrower than 4 B need a.tail (count u32) instead.
inline bool parse_needs_tail(ParseVariant v, int out_kind) {
    return v == ParseVariant::TwoPass &&
           (out_kind == NEXG_OUT_VERDICT || out_kind == NEXG_OUT_SPARSE || out_kind == NEXG_OUT_GROUPED);
}
uint32_t tile_order_for(const ParseArgs& a);
uint32_t build_tile_order();
uint32_t l4_build_tile_order();
uint32_t probe_tile_order();
uint32_t build_lds_pad();  // dynamic LDS of the udp_ping builds (workgroups per CU)
ParseVariant choose_parse_variant(const ParseArgs& a);

// Tile handled by this workgroup. Workgroups are dispatched to the 8 XCDs
// round-robin (blockIdx % 8).
//  order 0: grid order, tile = b.
//  order 1: each XCD one contiguous eighth of the batch, tile = (b % 8) * (nb / 8) + b / 8.
//  order K >= 2: XCD-local runs of K consecutive tiles, the runs dealt to the
//    XCDs round-robin — XCD x's i-th workgroup takes tile (i / K * 8 + x) * K + i % K.
//    At any moment each XCD streams its own K-tile run of the batch instead of
//    every eighth tile (profiles/r04/tile_order/: K = 16 over 16-KiB tiles is
//    5-7 % faster than grid order at 1 and 3.25 GiB; K = 4 is 5 % slower).
// Workgroups past the last whole group of 8 (order 1) or 8K (order K) keep grid
// order, so the map is a bijection on [0, nb) for every grid size.
__host__ __device__ __forceinline__ uint64_t tile_of(uint32_t b, uint32_t nb, uint32_t order) {
    if (!order) return b;
    if (order & 0x80000000u) {  // CU-affine runs (measurement order "cuR", round 6): XCD-local runs of
        // 32 R tiles in which the XCD's c-th workgroup of a dispatch round (CU c of 32 at launch)
        // takes R consecutive tiles: tile c R + j for the run's (32 j + c)-th workgroup
        const uint32_t R = order & 0x7FFFFFFFu;
        if (R == 0 || R > (nb >> 8)) return b;  // no whole run of 8 x 32 R
        const uint32_t K = 32u * R;
        const uint32_t whole = nb / (8u * K) * (8u * K);
        if (b >= whole) return b;
        const uint32_t i = b >> 3, x = b & 7u, l = i % K;
        return ((uint64_t)(i / K) * 8u + x) * K + (uint64_t)(l % 32u) * R + l / 32u;
    }
    if (order == 1u) {
        const uint32_t q = nb >> 3;
        return b >= (q << 3) ? b : (uint64_t)(b & 7u) * q + (b >> 3);
    }
    const uint32_t K = order;
    if (K > (nb >> 3)) return b;  // no whole group (and 8K cannot overflow below)
    const uint32_t whole = nb / (8u * K) * (8u * K);
    if (b >= whole) return b;
    const uint32_t i = b >> 3, x = b & 7u;
    return ((uint64_t)(i / K) * 8u + x) * K + i % K;
}
__device__ __forceinline__ uint64_t tile_index(uint32_t order) { return tile_of(blockIdx.x, gridDim.x, order); }

hipError_t launch_checksum(const ParseArgs& a, uint32_t skipword, uint16_t* out, hipStream_t s);

hipError_t launch_sparse_expand(const ParseArgs& a, const uint8_t* sparse, nexg_desc* out, bool grouped,
                                hipStream_t s);

hipError_t launch_recompute(const ParseArgs& a, uint32_t which, nexg_fixup* out, hipStream_t s);

// nexg_rewrite_batch (nexg_rewrite.hip); `actions` has passed check_actions (rewrite_core.hpp)
hipError_t launch_rewrite(const ParseArgs& a, const nexg_actions& actions, const uint8_t* action_index,
                          nexg_rewritten* out, hipStream_t s);

hipError_t launch_decode_options(const ParseArgs& a, const nexg_record* recs, nexg_options* out,
                                 hipStream_t s);

// nexg_decap_batch / nexg_decap_select (nexg_decap.hip). workspace: as
// nexg_decap_select_workspace sizes it (workspace_layout.hpp TileCountLayout),
// left holding the tiles' exclusive scan.
hipError_t launch_decap(const ParseArgs& a, const nexg_record* recs, uint32_t which, uint32_t vxlan_port,
                        nexg_tunnel* tunnels, uint64_t* inner_off, uint32_t* inner_len, hipStream_t s);
hipError_t launch_decap_select(const nexg_tunnel* tunnels, const uint64_t* inner_off, const uint32_t* inner_len,
                               uint64_t count, uint32_t inner_mask, uint32_t* out_index, uint64_t* out_off,
                               uint32_t* out_len, uint64_t* out_count, void* workspace, hipStream_t s);

// nexg_encap_plan / nexg_encap_frames (nexg_encap.hip). The specs travel as a
// kernel argument in the form encap_core.hpp's prepare_tunnels gives them.
// workspace: as nexg_encap_plan_workspace sizes it (workspace_layout.hpp
// TileSumLayout), left holding the tiles' exclusive scan.
struct EncapSet;
hipError_t launch_encap_plan(const ParseArgs& a, const EncapSet& set, const uint8_t* tunnel_index, uint32_t align,
                             uint64_t* out_offsets, uint32_t* out_len, void* workspace, hipStream_t s);
hipError_t launch_encap_frames(const ParseArgs& a, const EncapSet& set, const uint8_t* tunnel_index, const nexg_flow* flows,
                               const uint64_t* out_offsets, uint8_t* out_data, uint64_t out_cap, nexg_encapped* rows,
                               hipStream_t s);

// nexg_fragment_plan / nexg_fragment_frames (nexg_fragment.hip); the option has
// passed check_frag_option (fragment_core.hpp). workspace: as
// nexg_fragment_plan_workspace sizes it (workspace_layout.hpp FragPlanLayout),
// left holding the tiles' exclusive scans.
hipError_t launch_fragment_plan(const ParseArgs& a, uint32_t mtu, uint32_t flags, uint32_t align, uint32_t* out_first,
                                uint64_t* out_bytes, nexg_fragged* rows, void* workspace, hipStream_t s);
hipError_t launch_fragment_frames(const ParseArgs& a, uint32_t mtu, uint32_t flags, uint32_t align, const uint32_t* out_first,
                                  const uint64_t* out_bytes, uint64_t out_count, uint64_t* out_offsets, uint32_t* out_len,
                                  uint32_t* out_src, uint8_t* out_data, uint64_t out_cap, hipStream_t s);

// nexg_dns_batch / nexg_dns_entries (nexg_dns.hip). tile_first: one u64 per
// 256-frame tile + 1, left holding the tiles' exclusive scan and the total.
hipError_t launch_dns(const ParseArgs& a, const nexg_record* recs, uint32_t any_udp, uint32_t port, nexg_dns* out,
                      uint64_t* tile_first, hipStream_t s);
hipError_t launch_dns_entries(const ParseArgs& a, const nexg_dns* dns, const uint64_t* tile_first,
                              nexg_dns_entry* entries, uint64_t cap, hipStream_t s);

// nexg_select_batch / nexg_gather_* (nexg_select.hip). The filter travels as a
// kernel argument in the form the kernel tests with: addresses as big-endian
// word values with their prefix masks applied, ranges packed lo | hi << 16.
struct SelRule {  // 96 bytes
    uint32_t flags_mask, flags_value, tests;
    uint32_t misc;  // ip_proto | tcp_mask << 8 | tcp_value << 16 | family << 24
    uint32_t sport, dport, length, pad;
    uint32_t src[4], src_mask[4], dst[4], dst_mask[4];
};
struct SelFilter {
    uint32_t n_rules, invert;
    uint32_t need;  // kSelNeed*: which record dwords / frame bytes some rule reads
    uint32_t pad;
    SelRule rule[NEXG_FILTER_MAX_RULES];
};
// nullptr when the filter is valid (then *out, if given, is filled), else what is wrong with it
const char* prepare_filter(const nexg_filter* f, SelFilter* out);
// workspace: as nexg_select_workspace (workspace_layout.hpp TileCountLayout) and
// nexg_gather_plan_workspace (TileSumLayout) size it, left holding the tiles'
// exclusive scan
hipError_t launch_select(const ParseArgs& a, const nexg_record* recs, const SelFilter& f, uint32_t* out_index,
                         uint64_t* out_off, uint32_t* out_len, uint8_t* out_rule, uint64_t* out_count,
                         void* workspace, hipStream_t s);
hipError_t launch_gather_plan(const ParseArgs& a, uint32_t align, uint64_t* out_offsets, uint32_t* out_len,
                              void* workspace, hipStream_t s);
hipError_t launch_gather_frames(const ParseArgs& a, const uint64_t* out_offsets, uint8_t* out_data, uint64_t out_cap,
                                hipStream_t s);
hipError_t launch_gather_rows(const void* rows, uint32_t row_bytes, uint64_t rows_count, const uint32_t* index,
                              uint64_t n, void* out, hipStream_t s);

// nexg_match_batch / nexg_match_select (nexg_match.hip). The set travels as a
// kernel argument in the form match_core.hpp gives it. workspace: as
// nexg_match_select_workspace sizes it (workspace_layout.hpp TileCountLayout),
// left holding the tiles' exclusive scan.
struct MatchSet;
hipError_t launch_match(const ParseArgs& a, const nexg_record* recs, const MatchSet& s, nexg_match* out, hipStream_t st);
hipError_t launch_match_select(const ParseArgs& a, const nexg_match* rows, uint32_t any_mask, uint32_t all_mask,
                               uint32_t none_mask, uint32_t* out_index, uint64_t* out_off, uint32_t* out_len,
                               uint64_t* out_count, void* workspace, hipStream_t s);

// nexg_flow_batch / nexg_flow_partition (nexg_flow.hip). The Toeplitz key
// travels as a kernel argument: its 40 bytes as ten big-endian word values.
// workspace: as nexg_flow_partition_workspace lays it out.
struct FlowKey {
    uint32_t w[10];
};
hipError_t launch_flow(const ParseArgs& a, const nexg_record* recs, uint32_t opt, const FlowKey& key, nexg_flow* out,
                       hipStream_t s);
hipError_t launch_flow_partition(const ParseArgs& a, const nexg_flow* flows, uint32_t buckets, uint32_t* out_index,
                                 uint64_t* out_off, uint32_t* out_len, uint64_t* bucket_first, void* workspace,
                                 hipStream_t s);
// nexg_flow_sort / nexg_flow_groups (nexg_flow.hip); the workspaces as
// nexg_flow_sort_workspace / nexg_flow_groups_workspace lay them out
hipError_t launch_flow_sort(const nexg_flow* flows, uint64_t count, uint32_t* out_index, void* workspace, hipStream_t s);
// The sort's four passes over any rows (`count` u64, the 32-bit key in the low
// word), from the table's order (start nullptr) or from the order a chain
// before left in `start` (which may be out_index): a sort by two keys is two
// chains, the minor key first. The workspace is nexg_flow_sort_workspace's.
hipError_t launch_radix_sort(const void* rows, const uint32_t* start, uint64_t count, uint32_t* out_index, void* workspace,
                             hipStream_t s);

// nexg_reasm_plan / nexg_reasm_frames / nexg_reasm_held (nexg_reasm.hip).
// workspace: as nexg_reasm_plan_workspace (workspace_layout.hpp
// ReasmPlanLayout) and nexg_select_workspace (TileCountLayout) size it.
hipError_t launch_reasm_plan(const ParseArgs& a, uint32_t align, uint32_t* out_first, uint64_t* out_bytes, nexg_reasm* rows,
                             void* workspace, hipStream_t s);
hipError_t launch_reasm_frames(const ParseArgs& a, uint32_t align, const nexg_reasm* rows, const uint32_t* out_first,
                               const uint64_t* out_bytes, uint64_t out_count, uint64_t* out_offsets, uint32_t* out_len,
                               uint32_t* out_src, uint8_t* out_data, uint64_t out_cap, hipStream_t s);
hipError_t launch_reasm_held(const ParseArgs& a, const nexg_reasm* rows, uint32_t* out_index, uint64_t* out_off,
                             uint32_t* out_len, uint64_t* out_count, void* workspace, hipStream_t s);
hipError_t launch_flow_groups(const ParseArgs& a, const nexg_record* recs, const nexg_flow* flows, uint32_t opt,
                              const uint32_t* order, nexg_flow_group* out, uint64_t groups_cap, uint32_t* out_group,
                              uint64_t* out_count, void* workspace, hipStream_t s);
// nexg_flow_table_merge (nexg_flow.hip); the workspace as nexg_flow_table_workspace lays it out.
// n_in and n_groups are below 2^31.
hipError_t launch_flow_table_merge(const ParseArgs& a, const nexg_record* recs, uint32_t opt, const nexg_flow_group* groups,
                                   uint64_t n_groups, const nexg_flow_entry* table_in, uint64_t n_in, uint32_t epoch,
                                   uint32_t min_epoch, nexg_flow_entry* table_out, uint64_t table_cap, uint32_t* out_slot,
                                   uint64_t* out_count, void* workspace, hipStream_t s);

hipError_t launch_probe_stream(const uint8_t* data, uint64_t tiles, uint32_t mode, void* out, hipStream_t s);
hipError_t launch_probe_latency(uint32_t* buf, uint32_t lines, uint32_t start, uint32_t steps, uint32_t loaded_wgs,
                                uint32_t rounds, uint64_t* out, hipStream_t s);

hipError_t launch_build_udp4_tuples(const nexg_udp4_build& p, const nexg_udp4_tuple* tuples, uint8_t* out,
                                    uint32_t out_stride, hipStream_t s);
hipError_t launch_build_udp4(const nexg_udp4_build& p, uint8_t* out, uint32_t out_stride,
                             hipStream_t s);

hipError_t launch_build_udp6(const nexg_udp6_build& p, uint8_t* out, uint32_t out_stride,
                             hipStream_t s);

hipError_t launch_build_tcp(const nexg_tcp_build& p, uint8_t* out, uint32_t out_stride, hipStream_t s);
hipError_t launch_build_icmp_echo(const nexg_icmp_echo_build& p, uint8_t* out, uint32_t out_stride,
                                  hipStream_t s);

hipError_t launch_build_arp(const nexg_arp_build& p, uint8_t* out, uint32_t out_stride, hipStream_t s);
hipError_t launch_build_ndp_ns(const nexg_ndp_ns_build& p, uint8_t* out, uint32_t out_stride, hipStream_t s);

hipError_t launch_gen_lengths(int workload, uint64_t seed, uint64_t first, uint64_t count,
                              uint32_t* lengths, hipStream_t s);
hipError_t launch_gen_frames(int workload, uint64_t seed, uint64_t first, uint64_t count,
                             uint8_t* data, const uint64_t* offsets, uint32_t stride,
                             hipStream_t s);
hipError_t launch_gen_udp4_params(uint64_t seed, uint64_t first, uint64_t count,
                                  uint32_t* src_ip, uint32_t* dst_ip, uint16_t* sport,
                                  uint16_t* dport, uint16_t* ip_id, hipStream_t s);

}  // namespace nexg
