// nexg_encap.hip — nexg_encap_plan / nexg_encap_frames: every frame of a table
// copied behind an outer Ethernet / IP / UDP + VXLAN or GRE header
// (include/nexg.h; the per-frame rule is encap_core.hpp). The other direction
// of nexg_decap.hip, and a match-action table's second action half: rule j of
// a filter gets tunnel j through tunnel_index.
//
// Plan: one lane per frame gives the output length; the tile sums, their scan
// and the lanes' prefixes are the gather plan's shape on the same primitives
// (table_kernels.hpp: block_sum, k_tile_scan<uint64_t>, block_excl_scan).
//
// Fill: frame-centric. A quarter wave (16 lanes) owns a frame, 16 frames per
// workgroup. The lanes take the frame's aligned 16-B output chunks round
// robin, so a step of the group is 256 contiguous output bytes (two cache
// lines) and, off by the phase between source and destination, 256 to 272
// contiguous source bytes; the source address of a chunk follows from the
// frame's offset alone. A quarter wave rather than a whole one: the outer
// frame of a 64-B inner frame is 8 chunks and that of a 1500-B one 97, so 16
// lanes are busy on the shortest frame and loop six times on an MTU frame,
// four chunks' loads in flight per lane, where 64 lanes would idle three
// quarters of the wave on the traffic mixes' most frequent length. The specs
// (2 KiB) travel as the kernel's first argument and are copied from the
// kernel-argument segment into LDS by two vector loads per lane (indexing the
// argument itself by a lane's spec number would copy it to scratch): a frame
// needs eight of its spec's dwords in every lane and the header dwords in the
// three to six lanes that hold header chunks.
// The UDP checksum is summed from the chunks as they are copied, reduced over
// the group by four shuffles, and the header chunks leave last. No atomics, no
// workspace, no scratch; the output is never read.
#include "encap_core.hpp"
#include "table_kernels.hpp"

namespace nexg {

static_assert(sizeof(nexg_tunnel_spec) == 96 && sizeof(nexg_tunnels) == 8 + 16 * 96, "nexg_tunnel_spec is 96 bytes (include/nexg.h)");
static_assert(sizeof(nexg_encapped) == 8, "nexg_encapped is 8 bytes (include/nexg.h)");

// ---- plan ------------------------------------------------------------------------------

struct EncapPlanSet {
    uint32_t n;
    uint32_t meta[NEXG_ENCAP_MAX_TUNNELS];  // EncapTpl.meta
};

// frame idx's output length rounded up to the alignment (a power of two); 0 past the table
__device__ __forceinline__ uint32_t encap_padded(const ParseArgs& a, const EncapPlanSet& s, const uint8_t* tunnel_index,
                                                 uint64_t idx, uint32_t align, uint32_t& out_len) {
    out_len = 0;
    if (idx >= a.count) return 0u;
    uint64_t off;
    uint32_t len;
    const bool ext = frame_extent(a, idx, off, len);
    const uint32_t t = tunnel_index ? (uint32_t)NEXG_GLOBAL(uint8_t, tunnel_index)[idx] : 0u;
    uint32_t meta = 0;
    for (uint32_t r = 0; r < s.n; r++)  // uniform: the set stays in scalar registers
        if (t == r) meta = s.meta[r];
    const EncapShape sh = encap_shape(t < s.n, meta, ext, len);
    out_len = sh.H + sh.m;
    return (out_len + align - 1u) & ~(align - 1u);
}

__global__ __launch_bounds__(256) void k_encap_plan_sum(ParseArgs a, EncapPlanSet s, const uint8_t* tunnel_index,
                                                        uint32_t align, uint64_t* tile_sum) {
    __shared__ uint32_t s_w[4];
    uint32_t out_len;
    const uint64_t sum = block_sum(encap_padded(a, s, tunnel_index, (uint64_t)blockIdx.x * kTile + threadIdx.x, align, out_len), s_w);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = sum;  // < 2^24 + pads
}

__global__ __launch_bounds__(256) void k_encap_plan_write(ParseArgs a, EncapPlanSet s, const uint8_t* tunnel_index,
                                                          uint32_t align, const uint64_t* tile_base, uint64_t* out_offsets,
                                                          uint32_t* out_len) {
    __shared__ uint32_t s_w[4];
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    uint32_t len, total;
    const uint32_t before = block_excl_scan(encap_padded(a, s, tunnel_index, idx, align, len), s_w, total);
    if (idx >= a.count) return;
    out_offsets[idx] = tile_base[blockIdx.x] + before;
    if (out_len) out_len[idx] = len;
}

hipError_t launch_encap_plan(const ParseArgs& a, const EncapSet& set, const uint8_t* tunnel_index, uint32_t align,
                             uint64_t* out_offsets, uint32_t* out_len, void* workspace, hipStream_t st) {
    EncapPlanSet s{};
    s.n = set.n;
    for (uint32_t i = 0; i < set.n; i++) s.meta[i] = set.t[i].meta;
    const TileSumLayout w = TileSumLayout::from(a.count);
    const uint64_t tiles = w.tiles;
    uint64_t* tile_sum = region<uint64_t>(workspace, w.tile_sum);
    if (tiles) hipLaunchKernelGGL(k_encap_plan_sum, dim3((uint32_t)tiles), dim3(kTile), 0, st, a, s, tunnel_index, align, tile_sum);
    hipLaunchKernelGGL(k_tile_scan<uint64_t>, dim3(1), dim3(kTile), 0, st, tile_sum, tiles, out_offsets + a.count);
    if (tiles)
        hipLaunchKernelGGL(k_encap_plan_write, dim3((uint32_t)tiles), dim3(kTile), 0, st, a, s, tunnel_index, align, tile_sum,
                           out_offsets, out_len);
    return hipGetLastError();
}

// ---- fill ------------------------------------------------------------------------------

constexpr uint32_t kEncapGroups = kTile / kEncapLanes;  // frames per workgroup

// out_offsets is caller memory: whatever it holds, a frame's stores lie in
// [out_offsets[i], min(out_offsets[i + 1], out_offsets[i] + its length + 15,
// out_cap)) (encap_range), its chunk loop is bounded by its own length, and every source
// byte read lies inside a frame whose extent frame_extent accepted (the body
// is encap_core.hpp's encap_group_lane, which the host driver runs too).
__global__ __launch_bounds__(256) void k_encap_frames(EncapSet s, ParseArgs a, const uint8_t* tunnel_index,
                                                      const nexg_flow* flows, const uint64_t* out_offsets, uint8_t* out_data,
                                                      uint64_t out_cap, nexg_encapped* rows) {
    // the first explicit argument lies at byte 0 of the kernel-argument segment
    __shared__ uint32_t s_set[sizeof(EncapSet) / 4u];
    const auto* karg = (const __attribute__((address_space(4))) uint32_t*)__builtin_amdgcn_kernarg_segment_ptr();
    for (uint32_t k = threadIdx.x; k < sizeof(EncapSet) / 4u; k += kTile) s_set[k] = karg[k];
    __syncthreads();
    const uint32_t lane = threadIdx.x & (kEncapLanes - 1u);
    const uint64_t idx = (uint64_t)blockIdx.x * kEncapGroups + threadIdx.x / kEncapLanes;
    EncapJob j{};
    j.live = idx < a.count;  // a group past the table runs on with no chunk
    j.index = (uint32_t)idx;
    if (j.live) {
        const auto* oo = NEXG_GLOBAL(uint64_t, out_offsets);
        j.lo = oo[idx];
        j.next = oo[idx + 1];
        uint64_t off;
        j.ext = frame_extent(a, idx, off, j.len);
        j.src = reinterpret_cast<uint64_t>(a.data) + off;
        if (tunnel_index) j.t = NEXG_GLOBAL(uint8_t, tunnel_index)[idx];
    }
    const nexg_encapped row = encap_group_lane(
        reinterpret_cast<const EncapTpl*>(&s_set[offsetof(EncapSet, t) / 4u]), s.n, j, out_cap, out_data, lane,
        [&] { return NEXG_GLOBAL(uint32_t, flows)[2u * idx]; },  // nexg_flow.hash
        [](uint32_t v) {
#pragma unroll
            for (int d = kEncapLanes / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, kEncapLanes);
            return v;
        });
    if (j.live && rows && lane == 0) rows[idx] = row;
}

hipError_t launch_encap_frames(const ParseArgs& a, const EncapSet& set, const uint8_t* tunnel_index, const nexg_flow* flows,
                               const uint64_t* out_offsets, uint8_t* out_data, uint64_t out_cap, nexg_encapped* rows,
                               hipStream_t st) {
    if (a.count == 0) return hipSuccess;
    const uint64_t blocks = (a.count + kEncapGroups - 1) / kEncapGroups;
    hipLaunchKernelGGL(k_encap_frames, dim3((uint32_t)blocks), dim3(kTile), 0, st, set, a, tunnel_index, flows, out_offsets,
                       out_data, out_cap, rows);
    return hipGetLastError();
}

}  // namespace nexg
