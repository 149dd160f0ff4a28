// nexg_fragment.hip — nexg_fragment_plan / nexg_fragment_frames: every IPv4
// frame of a table over an MTU cut into RFC 791 fragments (include/nexg.h; the
// per-frame rule is fragment_core.hpp). The first one-to-many pass: a frame
// gives 0..8183 output frames.
//
// Plan: one lane per frame reads the four header words that decide the shape
// and gives the frame's output frames and padded output bytes; each of the two
// is summed per tile, scanned over the tiles and prefixed within the tile on
// the primitives the encap and gather plans use (table_kernels.hpp: block_sum,
// k_tile_scan<uint64_t>, block_excl_scan). The rows leave with the prefixes.
//
// Fill: encap's geometry. A quarter wave (16 lanes) owns an input frame, 16
// frames per workgroup, and loops over the frame's output frames; a piece's
// aligned 16-B output chunks go round robin over the lanes exactly as an
// encapsulated frame's do (encap_core.hpp's encap_copy / encap_finish: a piece
// is a header in front of a run of source bytes). The header is read once per
// frame into LDS as the pieces' two templates (piece 0; the pieces behind it,
// options that are not copied turned into NOPs) with their word sums, so a
// piece costs three patches and three additions for its checksum. A group
// writes its frame's table entries 16 at a time after the bytes. A frame with
// thousands of pieces keeps its group busy while the workgroup's other groups
// wait at the end: correct and bounded, not fast. No atomics, no workspace, no
// scratch; the output is never read.
#include "fragment_core.hpp"
#include "table_kernels.hpp"
#include "workspace_layout.hpp"

namespace nexg {

static_assert(sizeof(nexg_frag_option) == 16 && sizeof(nexg_fragged) == 16, "nexg_frag_option, nexg_fragged are 16 bytes (include/nexg.h)");

struct FragOpt {
    uint32_t mtu, flags, align;
};

// ---- plan ------------------------------------------------------------------------------

// frame idx's shape, output frames and padded output bytes; none past the table
__device__ __forceinline__ FragShape frag_planned(const ParseArgs& a, const FragOpt& o, uint64_t idx, uint32_t& bytes) {
    bytes = 0;
    if (idx >= a.count) return FragShape{};
    uint64_t off;
    uint32_t len;
    const bool ext = frame_extent(a, idx, off, len);
    const FragShape s = frag_shape(ext, len, reinterpret_cast<uint64_t>(a.data) + (ext ? off : 0u), o.mtu, o.flags);
    bytes = frag_out_bytes(s, len, o.align);
    return s;
}

__global__ __launch_bounds__(256) void k_fragment_plan_sum(ParseArgs a, FragOpt o, uint64_t* tile_frames, uint64_t* tile_bytes) {
    __shared__ uint32_t s_f[4], s_b[4];
    uint32_t bytes;
    const FragShape s = frag_planned(a, o, (uint64_t)blockIdx.x * kTile + threadIdx.x, bytes);
    const uint64_t frames = block_sum(s.n, s_f);     // <= 256 * 8183
    const uint64_t total = block_sum(bytes, s_b);    // < 2^28
    if (threadIdx.x == 0) {
        tile_frames[blockIdx.x] = frames;
        tile_bytes[blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(256) void k_fragment_plan_write(ParseArgs a, FragOpt o, const uint64_t* tile_frames,
                                                             const uint64_t* tile_bytes, const uint64_t* frames_total,
                                                             uint32_t* out_first, uint64_t* out_bytes, nexg_fragged* rows) {
    __shared__ uint32_t s_f[4], s_b[4];
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    uint32_t bytes, total;
    const FragShape s = frag_planned(a, o, idx, bytes);
    const uint32_t f_before = block_excl_scan(s.n, s_f, total);
    const uint32_t b_before = block_excl_scan(bytes, s_b, total);
    if (idx >= a.count) return;
    const uint32_t first = (uint32_t)tile_frames[blockIdx.x] + f_before;
    out_first[idx] = first;
    out_bytes[idx] = tile_bytes[blockIdx.x] + b_before;
    if (rows) rows[idx] = frag_row(s, first);
    // the total in 64 bits decides: 2^32 - 1 says that the output frames do not fit the 32-bit prefixes
    if (idx == a.count - 1u) out_first[a.count] = *frames_total >= 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)*frames_total;
}

hipError_t launch_fragment_plan(const ParseArgs& a, uint32_t mtu, uint32_t flags, uint32_t align, uint32_t* out_first,
                                uint64_t* out_bytes, nexg_fragged* rows, void* workspace, hipStream_t st) {
    const FragOpt o{mtu, flags, align};
    const FragPlanLayout w = FragPlanLayout::from(a.count);
    const uint64_t tiles = w.tiles;
    if (!tiles) {  // no workspace then
        hipError_t e = hipMemsetAsync(out_first, 0, 4, st);
        if (e == hipSuccess) e = hipMemsetAsync(out_bytes, 0, 8, st);
        return e;
    }
    uint64_t* tile_frames = region<uint64_t>(workspace, w.tile_frames);
    uint64_t* tile_bytes = region<uint64_t>(workspace, w.tile_bytes);
    uint64_t* frames_total = region<uint64_t>(workspace, w.frames_total);
    hipLaunchKernelGGL(k_fragment_plan_sum, dim3((uint32_t)tiles), dim3(kTile), 0, st, a, o, tile_frames, tile_bytes);
    hipLaunchKernelGGL(k_tile_scan<uint64_t>, dim3(1), dim3(kTile), 0, st, tile_frames, tiles, frames_total);
    hipLaunchKernelGGL(k_tile_scan<uint64_t>, dim3(1), dim3(kTile), 0, st, tile_bytes, tiles, out_bytes + a.count);
    hipLaunchKernelGGL(k_fragment_plan_write, dim3((uint32_t)tiles), dim3(kTile), 0, st, a, o, tile_frames, tile_bytes,
                       frames_total, out_first, out_bytes, rows);
    return hipGetLastError();
}

// ---- fill ------------------------------------------------------------------------------

constexpr uint32_t kFragGroups = kTile / kFragLanes;  // input frames per workgroup

// The body is fragment_core.hpp's three phases, which the host driver runs too;
// the bounds they keep against out_first, out_bytes and out_cap are stated there.
__global__ __launch_bounds__(256) void k_fragment_frames(ParseArgs a, FragOpt o, const uint32_t* out_first,
                                                         const uint64_t* out_bytes, FragOut out) {
    __shared__ FragHdr s_hdr[kFragGroups];
    const uint32_t lane = threadIdx.x & (kFragLanes - 1u), g = threadIdx.x / kFragLanes;
    const uint64_t idx = (uint64_t)blockIdx.x * kFragGroups + g;
    FragJob j{};
    j.live = idx < a.count;  // a group past the table runs on with no output frame
    j.index = (uint32_t)idx;
    FragShape s{};
    if (j.live) {
        const auto* of = NEXG_GLOBAL(uint32_t, out_first);
        const auto* ob = NEXG_GLOBAL(uint64_t, out_bytes);
        j.first = of[idx];
        j.first_end = of[idx + 1];
        j.lo = ob[idx];
        j.next = ob[idx + 1];
        uint64_t off;
        j.ext = frame_extent(a, idx, off, j.len);
        j.src = reinterpret_cast<uint64_t>(a.data) + (j.ext ? off : 0u);  // a rejected extent's offset is any number
        s = frag_shape(j.ext, j.len, j.src, o.mtu, o.flags);
    }
    frag_stage(j, s, s_hdr[g], lane);
    __syncthreads();
    if (lane == 0u) frag_walk(s, s_hdr[g]);
    __syncthreads();
    frag_fill(j, s, s_hdr[g], o.align, out, lane);
    if (j.live && lane == 0u && idx == a.count - 1u) out.offsets[out.count] = j.next;  // out_bytes[count]
}

hipError_t launch_fragment_frames(const ParseArgs& a, uint32_t mtu, uint32_t flags, uint32_t align, const uint32_t* out_first,
                                  const uint64_t* out_bytes, uint64_t out_count, uint64_t* out_offsets, uint32_t* out_len,
                                  uint32_t* out_src, uint8_t* out_data, uint64_t out_cap, hipStream_t st) {
    if (a.count == 0) return hipMemcpyAsync(out_offsets + out_count, out_bytes, 8, hipMemcpyDeviceToDevice, st);
    const FragOpt o{mtu, flags, align};
    const FragOut out{out_offsets, out_len, out_src, out_data, out_cap, out_count};
    const uint64_t blocks = (a.count + kFragGroups - 1) / kFragGroups;
    hipLaunchKernelGGL(k_fragment_frames, dim3((uint32_t)blocks), dim3(kTile), 0, st, a, o, out_first, out_bytes, out);
    return hipGetLastError();
}

}  // namespace nexg
