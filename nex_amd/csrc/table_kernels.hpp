// table_kernels.hpp — what the passes that write a frame table share
// (nexg_select.hip, nexg_flow.hip): a frame's table entry as the table gives
// it, and the one-workgroup scan of per-tile values.
#pragma once

#include "parse_kernels.hpp"

namespace nexg {

// off(i) and len(i) as the table gives them (frame_extent's reads, without its
// clamp: the selected table repeats the input's entries); false for an extent
// nexg_parse_batch reports as NEXG_ERR_BAD_EXTENT
__device__ __forceinline__ bool table_extent(const ParseArgs& a, uint64_t idx, uint64_t& off, uint64_t& l64) {
    if (a.offsets && !a.lengths && (a.hints & NEXG_FRAMES_OFFSETS32)) {
        const auto* op = NEXG_GLOBAL(uint32_t, a.offsets);
        const uint32_t o0 = op[idx], o1 = op[idx + 1];
        uint64_t b = 0;
        if (a.off_bases) b = NEXG_GLOBAL(uint64_t, a.off_bases)[idx >> 8];
        off = b + (uint32_t)(o0 - (uint32_t)b);
        l64 = (uint32_t)(o1 - o0);
    } else if (a.offsets && !a.lengths) {
        const auto* op = NEXG_GLOBAL(uint64_t, a.offsets);
        const uint64_t o0 = op[idx], o1 = op[idx + 1];
        off = o0;
        l64 = o1 - o0;
    } else if (a.offsets) {
        off = table_off(a, idx, idx);
        l64 = NEXG_GLOBAL(uint32_t, a.lengths)[idx];
    } else {
        off = idx * (uint64_t)a.stride;
        l64 = a.lengths ? (uint64_t)NEXG_GLOBAL(uint32_t, a.lengths)[idx] : (uint64_t)a.stride;
    }
    return !(l64 > 65535u || off > a.data_bytes || l64 > a.data_bytes - off);
}

// one workgroup: per-tile values become their exclusive scan in place, 256
// tiles per step (a wave scan, the four wave totals through LDS, a running
// carry); one lane stores the total
template <typename T>
__global__ __launch_bounds__(256) void k_tile_scan(T* tile, uint64_t tiles, uint64_t* out_total) {
    __shared__ T s_w[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    uint64_t carry = 0;
    for (uint64_t c = 0; c < tiles; c += kTile) {
        const T v = c + t < tiles ? tile[c + t] : (T)0;
        T x = v;  // inclusive scan within the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const T y = __shfl_up(x, d, 64);
            if (lane >= (uint32_t)d) x += y;
        }
        if (lane == 63u) s_w[wv] = x;
        __syncthreads();
        T below = 0;
        for (uint32_t k = 0; k < wv; k++) below += s_w[k];
        const T total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        if (c + t < tiles) tile[c + t] = (T)carry + below + x - v;
        carry += total;
        __syncthreads();  // s_w is rewritten by the next step
    }
    if (t == 0) *out_total = carry;
}

}  // namespace nexg
