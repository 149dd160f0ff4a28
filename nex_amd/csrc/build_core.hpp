// build_core.hpp — what the builder kernels (nexg_build.hip: one lane per frame;
// nexg_build_probe.hip: probe batches from a template) and their launchers
// share: the tile geometry and epilogue, the header emitters, the LDS / global
// frame writers, the shared-payload helpers and the host-side launch helpers.
#pragma once

#include "frame_core.hpp"
#include "nexg_internal.hpp"

namespace nexg {

constexpr uint32_t kBuildTile = 256;       // frames per workgroup (one per lane)
constexpr uint32_t kBuildMaxStride = 128;  // largest frame stride an LDS tile holds

// ------------------------------------------------------------------- host

// Frames go through an LDS tile and leave as 16-B stores: the stride fits a
// tile and the output is 16-B aligned. Else every lane writes global memory.
inline bool build_staged(const uint8_t* out, uint32_t out_stride) {
    return out_stride <= kBuildMaxStride && (reinterpret_cast<uint64_t>(out) & 15u) == 0;
}

// Tiles of `tile` frames that cover `count` frames (no overflow at any count)
constexpr uint64_t build_tile_count(uint64_t count, uint32_t tile) { return count / tile + (count % tile != 0); }

// One workgroup per tile, all in one grid: at most 2^32 - 1 tiles
inline hipError_t build_grid(uint64_t count, uint32_t tile, dim3& grid) {
    const uint64_t tiles = build_tile_count(count, tile);
    if (tiles > 0xFFFFFFFFull) return hipErrorInvalidValue;
    grid = dim3((uint32_t)tiles);
    return hipSuccess;
}

// Dynamic LDS of a workgroup whose tile needs tile_lds bytes so that `wgs`
// workgroups share a CU's 160 KiB (1 KiB each left for static LDS and the
// allocation granule), within a workgroup's 64 KiB; wgs 0: the tile alone.
inline uint32_t build_lds_for_wgs(uint32_t tile_lds, uint32_t wgs) {
    const uint32_t cap = wgs ? 160u * 1024u / wgs - 1024u : 0u;
    return tile_lds > cap ? tile_lds : cap < 65536u ? cap : 65536u;
}

// ---- tcp_ping / icmp_ping arguments: k_build_l4 (nexg_build.hip) and the
// probe templates made from them (nexg_build_probe.hip)
enum { kL4Tcp = 6, kL4Icmp = 1 };

struct L4Args {
    nexg_ip_build ip;
    // TCP
    const uint16_t* sport;
    const uint16_t* dport;
    const uint32_t* seq;
    const uint32_t* ack;
    uint32_t def_seq, def_ack;
    uint16_t def_sport, def_dport, window, urg;
    uint32_t flags;
    uint32_t opt_padded;  // bytes, multiple of 4, <= 40
    uint32_t opt_sum;     // BE word sum of the padded options
    uint8_t options[40];
    // ICMP
    const uint16_t* ident;
    const uint16_t* seqno;
    uint16_t def_ident, def_seqno;
    uint32_t icmp_type, icmp_code;
    // shared
    const uint8_t* payload;
    uint32_t payload_len;
    uint64_t count;
    uint8_t* out;
    uint32_t out_stride;
    uint32_t tile_order;  // tile_index order (nexg_internal.hpp), as k_build_udp4
};

// A probe batch (one source, a destination per frame, nothing else per frame)
// through the template kernels of nexg_build_probe.hip: false when the shape
// is not theirs (the per-lane builder takes it), else e is the launch's status.
bool try_probe_udp6(const nexg_udp6_build& p, uint8_t* out, uint32_t out_stride, hipStream_t s, hipError_t& e);
bool try_probe_l4(const L4Args& l, int kind, uint8_t* out, uint32_t out_stride, hipStream_t s, hipError_t& e);

// ----------------------------------------------------------------- device

// Phase timing of the builders' workgroups (measurement builds only:
// -DNEXG_PROBE_TIMING=1, tools/probe_timing.py): thread 0 of workgroup b
// stores s_memtime at phase k into g_build_stamps[8 b + k] (k = 6, 7:
// s_memrealtime at entry and exit); the product library has none of it.
// A device variable lives in one translation unit's code object, so such a
// build compiles both builder sources as one unit (see nexg_build.hip's end).
#ifndef NEXG_PROBE_TIMING
#define NEXG_PROBE_TIMING 0
#endif
#if NEXG_PROBE_TIMING
constexpr uint32_t kStampWgs = 1u << 18;
__device__ uint64_t g_build_stamps[8u * kStampWgs];
#define NEXG_BUILD_STAMP(k)                                                                    \
    do {                                                                                       \
        if (threadIdx.x == 0 && blockIdx.x < kStampWgs)                                        \
            g_build_stamps[8u * blockIdx.x + (k)] = (k) >= 6 ? __builtin_amdgcn_s_memrealtime()  \
                                                             : __builtin_amdgcn_s_memtime();   \
    } while (0)
#else
#define NEXG_BUILD_STAMP(k) do { } while (0)
#endif

// The tile of TILE frames this workgroup builds, one frame per lane
template <uint32_t TILE>
struct BuildTile {
    uint64_t first;  // the tile's first frame
    // order: tile_index's (nexg_internal.hpp); a literal 0 folds to blockIdx.x
    __device__ __forceinline__ explicit BuildTile(uint32_t order) {
        NEXG_BUILD_STAMP(0);
        NEXG_BUILD_STAMP(6);
        first = tile_index(order) * TILE;
    }
    // this lane's frame (in the batch when threadIdx.x < frames(count))
    __device__ __forceinline__ uint64_t lane() const { return first + threadIdx.x; }
    // the tile's frames: TILE, or what is left of a batch of `count`. (Apart
    // from the constructor so that a kernel reads `count` where it needs it:
    // as a constructor argument its load moved in front of tile_index.)
    __device__ __forceinline__ uint32_t frames(uint64_t count) const {
        const uint64_t left = count - first;
        return left < TILE ? (uint32_t)left : TILE;
    }
};

// tile copy-out shared by the builders: `bytes` staged contiguously in LDS
// leave a workgroup of WG threads as 16-B non-temporal stores (+ byte tail of
// a partial tile). Non-temporal: the udp_ping build of 16M frames takes 0.132
// instead of 0.165 ms with identical HBM traffic (PMC).
template <uint32_t WG>
__device__ __forceinline__ void build_copy_out(const uint8_t* smem, uint8_t* T, uint32_t bytes) {
    const uint32_t tid = threadIdx.x;
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    for (uint32_t c = tid; c < bytes / 16u; c += WG)
        __builtin_nontemporal_store(reinterpret_cast<const v4u*>(smem)[c], reinterpret_cast<v4u*>(T) + c);
    const uint32_t tail = bytes & ~15u;
    if (tid < bytes - tail) T[tail + tid] = smem[tail + tid];
}

// measurement builds: the stores issued, then (after their completion) done
__device__ __forceinline__ void build_stamp_exit() {
#if NEXG_PROBE_TIMING
    NEXG_BUILD_STAMP(4);
    __builtin_amdgcn_s_waitcnt(0x0F70);
    NEXG_BUILD_STAMP(5);
    NEXG_BUILD_STAMP(7);
#endif
}

// The per-lane builders' epilogue, every lane's frame written: a staged tile
// (nf frames of `stride` bytes in smem) goes out to its place in the batch's `out`
template <bool STAGED, uint32_t TILE>
__device__ __forceinline__ void build_finish(const uint8_t* smem, const BuildTile<TILE>& t, uint32_t nf, uint8_t* out,
                                             uint32_t stride) {
    NEXG_BUILD_STAMP(1);
    if (STAGED) {
        __syncthreads();
        NEXG_BUILD_STAMP(2);
        NEXG_BUILD_STAMP(3);
        build_copy_out<TILE>(smem, out + t.first * stride, nf * stride);
    }
    build_stamp_exit();
}

__device__ __forceinline__ uint32_t bswap16(uint32_t v) { return ((v & 0xFFu) << 8) | ((v >> 8) & 0xFFu); }

// Per-frame parameter or the batch default. The array is read as a global
// (address-space 1) pointer: written as `per ? per[i] : def` with def in the
// kernel arguments, the compiler selected between the two addresses and issued
// flat loads (counted on both vmcnt and lgkmcnt) for every parameter.
template <class T>
__device__ __forceinline__ uint32_t per_or_def(const T* per, uint64_t i, uint32_t def) {
    return per ? (uint32_t)NEXG_GLOBAL(T, per)[i] : def;
}

// Loads of one batch-wide value (the shared source, the small payload) by every
// lane of every workgroup: through the scalar cache (constant address space,
// s_load), not as vector loads of one line that every workgroup of the grid
// sends to that line's L2 channel. p is 4-B aligned.
typedef const __attribute__((address_space(4))) uint32_t* uniform_u32_ptr;
__device__ __forceinline__ uniform_u32_ptr uniform_u32(const void* p) {
    return reinterpret_cast<uniform_u32_ptr>(reinterpret_cast<uintptr_t>(p));
}

// ---- header emitters: halfwords in memory order (low byte first) -----------

// Halfword k (0..2) of frame i's 6-B address (read bytewise: any alignment),
// or of the batch default
__device__ __forceinline__ uint32_t mac_halfword(const uint8_t* per, const uint8_t (&def)[6], uint64_t i, int k) {
    return per_or_def(per, i * 6 + 2 * k, def[2 * k]) | (per_or_def(per, i * 6 + 2 * k + 1, def[2 * k + 1]) << 8);
}

// Ethernet header, hw[0..7): destination, source, EtherType (as it lies in memory)
template <int NH>
__device__ __forceinline__ void emit_eth(uint32_t (&hw)[NH], const uint8_t* dst_mac, const uint8_t (&def_dst)[6],
                                         const uint8_t* src_mac, const uint8_t (&def_src)[6], uint64_t i,
                                         uint32_t ethertype_le) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        hw[k] = mac_halfword(dst_mac, def_dst, i, k);
        hw[3 + k] = mac_halfword(src_mac, def_src, i, k);
    }
    hw[6] = ethertype_le;
}

// Frame i's addresses as AW dwords (4-B aligned, network order as loaded); the
// source per frame, or one for the whole batch (`shared`: a uniform branch)
template <uint32_t AW>
__device__ __forceinline__ void load_addrs(const uint8_t* src_ip, const uint8_t* dst_ip, bool shared, uint64_t i,
                                           uint32_t (&sw)[AW], uint32_t (&dw)[AW]) {
#pragma unroll
    for (uint32_t k = 0; k < AW; k++) dw[k] = NEXG_GLOBAL(uint32_t, dst_ip)[AW * i + k];
    if (shared) {
#pragma unroll
        for (uint32_t k = 0; k < AW; k++) sw[k] = uniform_u32(src_ip)[k];
    } else {
#pragma unroll
        for (uint32_t k = 0; k < AW; k++) sw[k] = NEXG_GLOBAL(uint32_t, src_ip)[AW * i + k];
    }
}

// IPv6 header behind Ethernet, hw[7..27) (ipv6.rs:50-75): version 6, traffic
// class, flow label (low 20 bits), payload length, next header, hop limit,
// source, destination
template <int NH>
__device__ __forceinline__ void emit_ipv6(uint32_t (&hw)[NH], uint32_t tc, uint32_t flow_label, uint32_t payload_len,
                                          uint32_t next, uint32_t hop_limit, const uint32_t (&sw)[4],
                                          const uint32_t (&dw)[4]) {
    const uint32_t fl = flow_label & 0xFFFFFu;
    hw[7] = ((6u << 4) | (tc >> 4)) | ((((tc & 0xFu) << 4) | (fl >> 16)) << 8);
    hw[8] = ((fl >> 8) & 0xFFu) | ((fl & 0xFFu) << 8);
    hw[9] = bswap16(payload_len);
    hw[10] = next | (hop_limit << 8);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        hw[11 + 2 * k] = sw[k] & 0xFFFFu; hw[12 + 2 * k] = sw[k] >> 16;
        hw[19 + 2 * k] = dw[k] & 0xFFFFu; hw[20 + 2 * k] = dw[k] >> 16;
    }
}

// ---- frame writers -----------------------------------------------------------

// Frame header given as NH (odd) little-endian halfwords of its bytes, written
// to LDS at an even offset d0: (NH-1)/2 dword writes + 1 halfword write, the
// dword run shifted by one halfword when d0 = 2 mod 4.
template <int NH>
__device__ __forceinline__ void lds_put_halfwords(uint8_t* smem, uint32_t d0, const uint32_t (&hw)[NH]) {
    static_assert(NH % 2 == 1, "odd halfword count");
    const bool al = (d0 & 2u) == 0;
    const uint32_t b32 = al ? d0 : d0 + 2u;
#pragma unroll
    for (int m = 0; m < NH / 2; m++) {
        const uint32_t v = al ? (hw[2 * m] | (hw[2 * m + 1] << 16)) : (hw[2 * m + 1] | (hw[2 * m + 2] << 16));
        *reinterpret_cast<uint32_t*>(smem + b32 + 4u * m) = v;
    }
    *reinterpret_cast<uint16_t*>(smem + (al ? d0 + 2u * (NH - 1) : d0)) = (uint16_t)(al ? hw[NH - 1] : hw[0]);
}

// N (even) halfwords at an even offset e: dword writes, the run shifted by a
// halfword (one 2-B write at each end) when e = 2 mod 4
template <int N>
__device__ __forceinline__ void lds_put_even_run(uint8_t* smem, uint32_t e, const uint32_t (&hw)[N]) {
    static_assert(N % 2 == 0, "even halfword count");
    if ((e & 2u) == 0) {
#pragma unroll
        for (int m = 0; m < N / 2; m++)
            *reinterpret_cast<uint32_t*>(smem + e + 4u * m) = hw[2 * m] | (hw[2 * m + 1] << 16);
    } else {
        *reinterpret_cast<uint16_t*>(smem + e) = (uint16_t)hw[0];
#pragma unroll
        for (int m = 0; m < N / 2 - 1; m++)
            *reinterpret_cast<uint32_t*>(smem + e + 2u + 4u * m) = hw[2 * m + 1] | (hw[2 * m + 2] << 16);
        *reinterpret_cast<uint16_t*>(smem + e + 2u * (N - 1)) = (uint16_t)hw[N - 1];
    }
}

// NH (odd) halfwords of frame bytes at any LDS offset d0. Even d0:
// lds_put_halfwords. Odd d0 (odd frame strides): the first byte alone, the
// next 2 NH - 2 bytes re-paired into halfwords at the even offset d0 + 1
// (dword writes), the last byte alone — instead of 2 NH byte writes.
template <int NH>
__device__ __forceinline__ void lds_put_frame_hw(uint8_t* smem, uint32_t d0, const uint32_t (&hw)[NH]) {
    if ((d0 & 1u) == 0) {
        lds_put_halfwords<NH>(smem, d0, hw);
        return;
    }
    uint32_t sh[NH - 1];
#pragma unroll
    for (int k = 0; k < NH - 1; k++) sh[k] = (hw[k] >> 8) | ((hw[k + 1] & 0xFFu) << 8);
    smem[d0] = (uint8_t)hw[0];
    lds_put_even_run<NH - 1>(smem, d0 + 1u, sh);
    smem[d0 + 2u * NH - 1u] = (uint8_t)(hw[NH - 1] >> 8);
}

// halfword v (memory order: low byte first) at LDS/global byte offset p
__device__ __forceinline__ void put_hw(uint8_t* base, uint32_t p, uint32_t v, bool odd) {
    if (odd) {
        base[p] = (uint8_t)v;
        base[p + 1] = (uint8_t)(v >> 8);
    } else {
        *reinterpret_cast<uint16_t*>(base + p) = (uint16_t)v;
    }
}

// Where the lane of frame i writes it: at byte d0 = lane x stride of the LDS
// tile when STAGED, else at its own place in the global output (a 64-bit
// product: frame index and stride have no common bound).
struct FrameAt {
    uint8_t* base;
    uint32_t d0;
};
template <bool STAGED>
__device__ __forceinline__ FrameAt frame_at(uint8_t* smem, uint8_t* out, uint64_t i, uint32_t stride) {
    return STAGED ? FrameAt{smem, threadIdx.x * stride} : FrameAt{out + i * stride, 0u};
}

// The frame's NH header halfwords at byte d0 of base:
template <bool STAGED, int NH>
__device__ __forceinline__ void put_frame_head(uint8_t* base, uint32_t d0, const uint32_t (&hw)[NH]) {
    if (STAGED) {
        lds_put_frame_hw<NH>(base, d0, hw);  // dword writes at either parity of d0
    } else {  // consecutive byte stores: the compiler merges them into wide (unaligned) global stores
        uint8_t* d = base + d0;
#pragma unroll
        for (int k = 0; k < NH; k++) {
            d[2 * k] = (uint8_t)hw[k];
            d[2 * k + 1] = (uint8_t)(hw[k] >> 8);
        }
    }
}
// ... and the zeros from the frame's end (flen bytes) to the stride: a staged
// tile leaves whole, while direct writes touch the frame's own bytes only
template <bool STAGED>
__device__ __forceinline__ void put_frame_gap(uint8_t* base, uint32_t d0, uint32_t stride, uint32_t flen) {
    if (STAGED)
        for (uint32_t k = flen; k < stride; k++) base[d0 + k] = 0;
}
// The whole frame: header halfwords, n bytes of `run` behind them, the gap
template <bool STAGED, int NH>
__device__ __forceinline__ void put_frame(uint8_t* base, uint32_t d0, uint32_t stride, const uint32_t (&hw)[NH],
                                          const uint8_t* run, uint32_t n) {
    put_frame_head<STAGED, NH>(base, d0, hw);
    for (uint32_t k = 0; k < n; k++) base[d0 + 2u * NH + k] = run[k];
    put_frame_gap<STAGED>(base, d0, stride, 2u * NH + n);
}

// ---- shared payload ----------------------------------------------------------

// BE word sum of the shared payload (it starts at an even L4 offset), once
// per workgroup: all threads call it together; 0 without a barrier when the
// payload is empty (udp_ping's case), so the empty build pays nothing
__device__ __forceinline__ uint32_t shared_payload_sum(const uint8_t* pl, uint32_t n, uint32_t* s) {
    if (n == 0) return 0u;  // kernel argument: uniform over the workgroup
    if (threadIdx.x == 0) *s = 0;
    __syncthreads();
    uint32_t ps = 0;
    for (uint32_t k = 2u * threadIdx.x; k < n; k += 2u * kBuildTile)
        ps += ((uint32_t)pl[k] << 8) | (k + 1 < n ? (uint32_t)pl[k + 1] : 0u);
    if (ps) atomicAdd(s, ps);
    __syncthreads();
    return *s;
}

// A shared payload of at most kSmallPay bytes (icmp_ping's "hello"): every
// lane loads the same dwords (uniform addresses: scalar loads, no barrier)
// and sums them itself, instead of shared_payload_sum's per-workgroup global
// loads, LDS atomic and two barriers in front of every tile.
constexpr uint32_t kSmallPay = 64;
struct SmallPayload {
    uint32_t w[kSmallPay / 4];  // payload byte k = byte k & 3 of w[k >> 2] (bytes past n: 0)
    // k a compile-time index (unrolled loops): no dynamically indexed private array
    __device__ __forceinline__ uint32_t byte(uint32_t k) const { return (w[k >> 2] >> (8u * (k & 3u))) & 0xFFu; }
};

__device__ __forceinline__ void load_small_payload(const uint8_t* pl, uint32_t n, SmallPayload& sp, uint32_t& be_sum) {
    if (n == 0) {  // uniform; pl may be NULL
#pragma unroll
        for (uint32_t k = 0; k < kSmallPay / 4; k++) sp.w[k] = 0;
        be_sum = 0;
        return;
    }
    const uint64_t a = reinterpret_cast<uint64_t>(pl);
    const uint32_t sh = (uint32_t)(a & 3u);
    const uniform_u32_ptr src = uniform_u32(reinterpret_cast<const void*>(a & ~3ull));
    const uint32_t nw = (sh + n + 3u) >> 2;
    uint32_t raw[kSmallPay / 4 + 1];
#pragma unroll
    for (uint32_t k = 0; k < kSmallPay / 4 + 1; k++) raw[k] = src[k < nw ? k : nw - 1u];  // clamped: none past n
    // one empty asm over all 17: the loads issue together, one wait (per-value
    // statements let the compiler sink each load next to its own wait)
    asm volatile("" : "+s"(raw[0]), "+s"(raw[1]), "+s"(raw[2]), "+s"(raw[3]), "+s"(raw[4]), "+s"(raw[5]),
                 "+s"(raw[6]), "+s"(raw[7]), "+s"(raw[8]), "+s"(raw[9]), "+s"(raw[10]), "+s"(raw[11]),
                 "+s"(raw[12]), "+s"(raw[13]), "+s"(raw[14]), "+s"(raw[15]), "+s"(raw[16]));
    static_assert(kSmallPay / 4 + 1 == 17, "the asm above names every raw dword");
#pragma unroll
    for (uint32_t k = 0; k < kSmallPay / 4 + 1; k++) raw[k] = k < nw ? raw[k] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < kSmallPay / 4; k++) {  // realigned to the payload's first byte, masked to n
        const uint32_t x = __builtin_amdgcn_alignbyte(raw[k + 1], raw[k], sh);
        sp.w[k] = 4u * k + 4u <= n ? x : 4u * k >= n ? 0u : x & ((1u << (8u * (n - 4u * k))) - 1u);
    }
    uint32_t s = 0;  // BE words from the payload's start (an even L4 offset), odd tail byte high
#pragma unroll
    for (uint32_t k = 0; k < kSmallPay / 4; k++)  // two BE halfwords per dword (bytes past n are 0)
        s += bswap16(sp.w[k] & 0xFFFFu) + bswap16(sp.w[k] >> 16);
    be_sum = s;
}

// The small payload's words into LDS (s_w, 16 dwords) for byte copies with a
// run-time count: every wave writes the same (uniform) values itself, so no
// barrier is needed before its own reads (a wave's LDS operations execute in
// order). A byte loop over the uniform words in registers was a private array
// with a dynamic index (scratch), and 64 compile-time guarded stores cost 128
// scalar instructions per wave.
__device__ __forceinline__ void stage_small_payload(const SmallPayload& sp, uint32_t* s_w) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSmallPay / 4; k++) v = lane == k ? sp.w[k] : v;
    if (lane < kSmallPay / 4) s_w[lane] = v;
}

}  // namespace nexg
