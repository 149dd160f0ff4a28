// table_kernels.hpp — what the second passes share (nexg_decap.hip,
// nexg_dns.hip, nexg_select.hip, nexg_flow.hip, ...): the record's fields by
// dword, a frame's table entry as the table gives it, frame bytes as
// big-endian words, the 256-lane workgroup's scan / count / sum, the
// one-workgroup scan of per-tile values, and on top of those the
// order-preserving compaction of a frame table (decap_select, select).
#pragma once

#include <cstddef>

#include "parse_kernels.hpp"
#include "workspace_layout.hpp"

namespace nexg {

// ---- nexg_record by dword (include/nexg.h) ---------------------------------------------

constexpr uint32_t kRecFlags = 0, kRecPayload = 1, kRecL3 = 3, kRecIpWord = 5, kRecProto = 6, kRecSrc = 7, kRecDst = 8,
                   kRecPorts = 11, kRecL4Type = 12;
static_assert(offsetof(nexg_record, flags) == 4 * kRecFlags, "flags");
static_assert(offsetof(nexg_record, payload_off) == 4 * kRecPayload && offsetof(nexg_record, payload_len) == 4 * kRecPayload + 2,
              "payload_off | payload_len << 16");
static_assert(offsetof(nexg_record, l3_off) == 4 * kRecL3, "l3_off in the low half");
static_assert(offsetof(nexg_record, ip_word) == 4 * kRecIpWord, "ip_word");
static_assert(offsetof(nexg_record, ip_proto) == 4 * kRecProto + 1, "ip_proto in byte 1");
static_assert(offsetof(nexg_record, ip_src) == 4 * kRecSrc && offsetof(nexg_record, ip_dst) == 4 * kRecDst, "ip_src, ip_dst");
static_assert(offsetof(nexg_record, src_port) == 4 * kRecPorts && offsetof(nexg_record, dst_port) == 4 * kRecPorts + 2,
              "src_port | dst_port << 16");
static_assert(offsetof(nexg_record, l4_type) == 4 * kRecL4Type + 2, "l4_type in byte 2");

// quarter Q (16 B) of a record, and dword K of the record out of the quarter
// that holds it (another quarter does not compile)
template <uint32_t Q>
struct RecQuarter {
    uint4 v;
};
template <uint32_t Q>
__device__ __forceinline__ RecQuarter<Q> rec_quarter(const nexg_record* r) {
    return {load16<true>(reinterpret_cast<const uint8_t*>(r) + 16u * Q)};
}
template <uint32_t K>
__device__ __forceinline__ uint32_t rec_dw(const RecQuarter<K / 4u>& q) {
    return K % 4u == 0u ? q.v.x : K % 4u == 1u ? q.v.y : K % 4u == 2u ? q.v.z : q.v.w;
}

__device__ __forceinline__ uint32_t rec_status(uint32_t flags) { return (flags >> NEXG_STATUS_SHIFT) & 7u; }
__device__ __forceinline__ void rec_payload(uint32_t dw, uint32_t& off, uint32_t& len) { off = dw & 0xFFFFu, len = dw >> 16; }
__device__ __forceinline__ uint32_t rec_l3(uint32_t dw) { return dw & 0xFFFFu; }
__device__ __forceinline__ uint32_t rec_proto(uint32_t dw) { return (dw >> 8) & 0xFFu; }
__device__ __forceinline__ uint32_t rec_sport(uint32_t dw) { return dw & 0xFFFFu; }
__device__ __forceinline__ uint32_t rec_dport(uint32_t dw) { return dw >> 16; }
__device__ __forceinline__ uint32_t rec_l4_type(uint32_t dw) { return (dw >> 16) & 0xFFu; }

// ---- frames ------------------------------------------------------------------------------

// off(i) and len(i) as the table gives them (frame_extent's reads, without its
// clamp: the selected table repeats the input's entries); false for an extent
// nexg_parse_batch reports as NEXG_ERR_BAD_EXTENT.
// A second reader beside parse_kernels.hpp's frame_extent, on purpose. One
// reader in frame_extent's five-branch wording, with frame_extent as it plus
// the clamp, kept every parse kernel's code but made nexg_flow_table_merge
// 0.7 to 0.85 % slower (k_merge_write; profiles/table_skeletons/README.md),
// and this wording inside frame_extent changes the parse kernels. A change to
// the over-4-GiB base arithmetic has to be made in both.
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

// The `bytes` (1..4 N) frame bytes at byte address A as N big-endian words, byte
// 0 on top of w[0] (past `bytes`: 0, or what the last dword loaded holds); a
// lane with `on` false loads nothing and gets zeros. They come as the N + 1
// covering aligned dwords, funnel-shifted into place in registers. Every dword
// loaded holds a wanted byte, so the loads stay inside the frame's own 16-byte
// blocks. (`on` apart from `bytes`: with a constant count the gates of all but
// the last dword fold to `on` alone.)
template <uint32_t N>
__device__ __forceinline__ void frame_be_words(uint64_t A, bool on, uint32_t bytes, uint32_t (&w)[N]) {
    const uint32_t sh = (uint32_t)A & 3u, span = on ? sh + bytes : 0u;  // bytes from the first aligned dword
    const auto* dw = NEXG_GLOBAL(uint32_t, reinterpret_cast<const void*>(A & ~3ull));
    uint32_t d[N + 1];
#pragma unroll
    for (uint32_t k = 0; k < N + 1; k++) d[k] = 4u * k < span ? dw[k] : 0u;
#pragma unroll
    for (uint32_t j = 0; j < N; j++) w[j] = __builtin_bswap32(__builtin_amdgcn_alignbyte(d[j + 1], d[j], sh));
}

// ---- the 256-lane workgroup (four waves) ---------------------------------------------------
// Each of the three below contains one barrier, so all 256 lanes call it: a
// lane past the batch takes part with 0 / false and returns after the call,
// never before. The caller owns the __shared__ s_w[4], and the barrier that a
// second call with the same s_w needs in front of it.

// the lane's exclusive prefix of v within the workgroup, and the workgroup's total
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* s_w, T& total) {
    const uint32_t wv = threadIdx.x >> 6;
    const T x = wave_incl_scan(v);
    if ((threadIdx.x & 63u) == 63u) s_w[wv] = x;
    __syncthreads();
    T below = 0;
    for (uint32_t k = 0; k < wv; k++) below += s_w[k];
    total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return below + x - v;
}

// the number of lanes with pred, and for such a lane its rank among them (by
// ballot, popcount and mbcnt)
struct BlockCount {
    uint32_t rank, total;
};
__device__ __forceinline__ BlockCount block_count(bool pred, uint32_t* s_w) {
    const uint32_t wv = threadIdx.x >> 6;
    const uint64_t m = __ballot(pred);
    if ((threadIdx.x & 63u) == 0u) s_w[wv] = (uint32_t)__builtin_popcountll(m);
    __syncthreads();
    uint32_t below = 0;
    for (uint32_t k = 0; k < wv; k++) below += s_w[k];
    return {below + lanes_below(m), s_w[0] + s_w[1] + s_w[2] + s_w[3]};
}

// the workgroup's sum of x (each wave's by xor shuffles), in 64 bits
__device__ __forceinline__ uint64_t block_sum(uint32_t x, uint32_t* s_w) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    return (uint64_t)s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// one workgroup: per-tile values become their exclusive scan in place, 256
// tiles per step with a running carry; lane 0 stores the total after the loop
// (out_total may be tile + tiles: that slot is never read)
template <typename T>
__global__ __launch_bounds__(256) void k_tile_scan(T* tile, uint64_t tiles, uint64_t* out_total) {
    __shared__ T s_w[4];
    const uint32_t t = threadIdx.x;
    uint64_t carry = 0;
    for (uint64_t c = 0; c < tiles; c += kTile) {
        const T v = c + t < tiles ? tile[c + t] : (T)0;
        T total;
        const T before = block_excl_scan(v, s_w, total);
        if (c + t < tiles) tile[c + t] = (T)carry + before;
        carry += total;
        __syncthreads();  // s_w is rewritten by the next step
    }
    if (t == 0) *out_total = carry;
}

// ---- order-preserving compaction of a frame table ------------------------------------------
// Count per 256-frame tile (block_count), scan of the tile counts
// (k_tile_scan), scatter by rank: positions come from ballots, mbcnt ranks and
// scans alone, so a run repeats bit for bit. A pass is its selector S, a struct
// that travels by value as the kernel argument (what it holds stays in scalar
// registers) and provides
//   uint64_t count() const                    the frames of the input table (host and device)
//   struct Picked                             what pick() worked out and entry() wants again; may be empty
//   bool pick(idx, Picked&) const             is frame idx < count() selected; the only part the count kernel runs
//   void entry(idx, picked, off, len) const   the selected frame's entry of the output table
//   static constexpr bool kTagged             whether the pass has the optional per-frame output out_tag (one byte
//                                             per selected frame, select's out_rule); if so
//   uint8_t tag(picked) const                 the selected frame's byte of it
// The workspace is TileCountLayout's, left holding the tiles' exclusive scan.

template <typename S>
__global__ __launch_bounds__(256) void k_compact_count(S s, uint32_t* tile_count) {
    __shared__ uint32_t s_w[4];
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    typename S::Picked p;
    const bool sel = idx < s.count() && s.pick(idx, p);
    const uint32_t total = block_count(sel, s_w).total;
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

template <typename S>
__global__ __launch_bounds__(256) void k_compact_scatter(S s, const uint32_t* tile_base, uint32_t* out_index,
                                                         uint64_t* out_off, uint32_t* out_len, uint8_t* out_tag) {
    __shared__ uint32_t s_w[4];
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    typename S::Picked p;
    const bool sel = idx < s.count() && s.pick(idx, p);
    const uint32_t rank = block_count(sel, s_w).rank;
    if (!sel) return;
    // rank < the number selected <= count: inside the outputs' capacity (checked
    // all the same: a caller rewriting what pick() reads or the workspace
    // between the passes must not turn into a store out of bounds)
    const uint64_t k = (uint64_t)tile_base[blockIdx.x] + rank;
    if (k >= s.count()) return;
    uint64_t off;
    uint32_t len;
    s.entry(idx, p, off, len);
    out_index[k] = (uint32_t)idx;
    out_off[k] = off;
    out_len[k] = len;
    if constexpr (S::kTagged)
        if (out_tag) out_tag[k] = s.tag(p);
}

// an empty table launches the scan alone: *out_count = 0
template <typename S>
hipError_t launch_compact(const S& sel, uint32_t* out_index, uint64_t* out_off, uint32_t* out_len, uint8_t* out_tag,
                          uint64_t* out_count, void* workspace, hipStream_t s) {
    const TileCountLayout w = TileCountLayout::from(sel.count());
    uint32_t* tile_count = region<uint32_t>(workspace, w.tile_count);
    if (w.tiles) hipLaunchKernelGGL(k_compact_count<S>, dim3((uint32_t)w.tiles), dim3(kTile), 0, s, sel, tile_count);
    hipLaunchKernelGGL(k_tile_scan<uint32_t>, dim3(1), dim3(kTile), 0, s, tile_count, w.tiles, out_count);
    if (w.tiles)
        hipLaunchKernelGGL(k_compact_scatter<S>, dim3((uint32_t)w.tiles), dim3(kTile), 0, s, sel, tile_count, out_index,
                           out_off, out_len, out_tag);
    return hipGetLastError();
}

}  // namespace nexg
