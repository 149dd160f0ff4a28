// nexg_flow.hip — flow keys, the Toeplitz RSS hash and the flow-affine
// partition on gfx950 (include/nexg.h; an extension: the reference has no flow
// notion). nexg_flow_batch is a second pass over a batch already parsed with
// NEXG_OUT_RECORD that gives every frame an 8-byte flow row; nexg_flow_partition
// is one stable radix pass over those rows with up to 256 buckets (a histogram
// per 1024-frame tile, a hierarchical scan of the histograms, a scatter), the
// select's count / scan / scatter shape with P counters per tile instead of one.
#include "table_kernels.hpp"

namespace nexg {

static_assert(sizeof(nexg_flow) == 8, "nexg_flow is 8 bytes (include/nexg.h)");
static_assert(sizeof(nexg_flow_option) == 48, "nexg_flow_option is 48 bytes (include/nexg.h)");

// ---- flow rows -----------------------------------------------------------------------

constexpr uint32_t kFlowNibbles = 72;  // 36 key bytes at most

// k_flow: one lane per frame. The hash is linear over GF(2), so it is the XOR
// of one table entry per 4-bit nibble of the key bytes: s_tab[p][n] = the XOR
// of the key windows K[4p + k, 4p + k + 32) over the set bits k of n. The
// table (72 x 16 words, 4.5 KiB) is built per workgroup from the ten key words
// (4.5 entries per lane, 4 shift / select / XOR steps each); a lookup reads
// one of 16 consecutive words, so the 64 lanes of a wave touch 16 distinct
// banks at most and lanes with equal nibbles share a broadcast: no bank
// conflict, where a 256-entry byte table would see the lanes' random bytes
// collide, and the bit-serial form costs three VALU steps per key bit (864 for
// an IPv6 frame with ports against 72 lookups). Per lane: 48 B of its record
// (the three 16-B quarters that hold flags / l3_off, ip_word / ip_proto /
// ip_src, ip_dst / the ports), for an IPv6 frame its two addresses as
// big-endian words (frame_be_words of table_kernels.hpp), and one 8-B
// non-temporal store; consecutive lanes write consecutive rows. Words no lane
// of the wave has (the IPv6 words in a wave of IPv4 frames) are skipped by
// wave-uniform branches; a lane with a shorter key looks up nibble 0 there,
// whose entry is 0.
__global__ __launch_bounds__(256) void k_flow(ParseArgs a, const nexg_record* recs, uint32_t opt, FlowKey key,
                                              nexg_flow* out) {
    typedef uint32_t v2u __attribute__((ext_vector_type(2)));
    __shared__ uint32_t s_key[10];
    __shared__ uint32_t s_tab[kFlowNibbles * 16u];
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < 10; k++)
        if (t == k) s_key[k] = key.w[k];
    __syncthreads();
    for (uint32_t e = t; e < kFlowNibbles * 16u; e += kTile) {
        const uint32_t p = e >> 4, n = e & 15u, wi = p >> 3, sh = (p & 7u) * 4u;  // a nibble lies inside one key word
        const uint64_t kk = (uint64_t)s_key[wi] << 32 | s_key[wi + 1];            // wi <= 8
        uint32_t v = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (n & (8u >> k)) v ^= (uint32_t)((kk << (sh + k)) >> 32);
        s_tab[e] = v;
    }
    __syncthreads();
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + t;
    if (idx >= a.count) return;
    const RecQuarter<0> q0 = rec_quarter<0>(recs + idx);
    const RecQuarter<1> q1 = rec_quarter<1>(recs + idx);
    const RecQuarter<2> q2 = rec_quarter<2>(recs + idx);
    uint64_t off, l64;
    const bool ext = table_extent(a, idx, off, l64);
    const uint32_t flags = rec_dw<kRecFlags>(q0), l3 = rec_l3(rec_dw<kRecL3>(q0)), ip_word = rec_dw<kRecIpWord>(q1),
                   proto = rec_proto(rec_dw<kRecProto>(q1)), ports_dw = rec_dw<kRecPorts>(q2);
    const bool ok = rec_status(flags) == 0u;
    const bool v4 = ok && (flags & NEXG_L_IPV4) != 0u;
    // the record is caller memory: the header must lie inside the frame's own extent before any load
    const bool v6 = ok && !v4 && (flags & NEXG_L_IPV6) != 0u && ext && (uint64_t)l3 + 40u <= l64;
    const bool has = v4 || v6;
    const bool l4 = has && (flags & (NEXG_L_TCP | NEXG_L_UDP)) != 0u && !(opt & NEXG_FLOW_NO_PORTS) &&
                    !(v4 && (ip_word & 0x3FFFu) != 0u);
    uint32_t S[4] = {v4 ? rec_dw<kRecSrc>(q1) : 0u, 0u, 0u, 0u}, D[4] = {v4 ? rec_dw<kRecDst>(q2) : 0u, 0u, 0u, 0u};
    if (__ballot(v6) != 0ull) {
        uint32_t a6[8];  // the source, then the destination
        frame_be_words(reinterpret_cast<uint64_t>(a.data) + off + l3 + 8u, v6, 32u, a6);
#pragma unroll
        for (uint32_t j = 0; j < 4; j++)
            if (v6) S[j] = a6[j], D[j] = a6[j + 4];
    }
    uint32_t sport = l4 ? rec_sport(ports_dw) : 0u, dport = l4 ? rec_dport(ports_dw) : 0u;
    // NEXG_FLOW_SYMMETRIC: (source address, src_port) > (destination address, dst_port) as byte strings
    bool gt = sport > dport, decided = false;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++)
        if (!decided && S[j] != D[j]) gt = S[j] > D[j], decided = true;
    const bool swapped = has && (opt & NEXG_FLOW_SYMMETRIC) && gt;
    if (swapped) {
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t x = S[j];
            S[j] = D[j], D[j] = x;
        }
        const uint32_t x = sport;
        sport = dport, dport = x;
    }
    const uint32_t ports = sport << 16 | dport;
    // the key bytes as big-endian words: 2 or 3 (IPv4), 8 or 9 (IPv6)
    const uint32_t W[9] = {S[0], v6 ? S[1] : D[0], v6 ? S[2] : ports, v6 ? S[3] : 0u, v6 ? D[0] : 0u,
                           v6 ? D[1] : 0u, v6 ? D[2] : 0u, v6 ? D[3] : 0u, v6 ? ports : 0u};
    uint32_t h = 0;
#pragma unroll
    for (uint32_t j = 0; j < 9; j++) {
        const bool mine = j < 2u ? has : j == 2u ? (v6 || l4) : j < 8u ? v6 : (v6 && l4);
        if (__ballot(mine) == 0ull) continue;  // wave-uniform
#pragma unroll
        for (uint32_t q = 0; q < 8; q++) h ^= s_tab[(8u * j + q) * 16u + ((W[j] >> (28u - 4u * q)) & 15u)];
    }
    const uint32_t kind = v4 ? (l4 ? NEXG_FLOW_IPV4_L4 : NEXG_FLOW_IPV4) : v6 ? (l4 ? NEXG_FLOW_IPV6_L4 : NEXG_FLOW_IPV6)
                                                                             : NEXG_FLOW_NONE;
    const uint32_t tail = has ? kind | proto << 8 | (swapped ? 1u << 16 : 0u) : 0u;
    __builtin_nontemporal_store(v2u{has ? h : 0u, tail}, reinterpret_cast<v2u*>(out) + idx);
}

hipError_t launch_flow(const ParseArgs& a, const nexg_record* recs, uint32_t opt, const FlowKey& key, nexg_flow* out,
                       hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    const uint64_t blocks = (a.count + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_flow, dim3((uint32_t)blocks), dim3(kTile), 0, s, a, recs, opt, key, out);
    return hipGetLastError();
}

// ---- partition -------------------------------------------------------------------------

constexpr uint32_t kPartTile = NEXG_FLOW_TILE;  // frames per workgroup: each of the 4 waves owns 256 consecutive
constexpr uint32_t kPartRounds = kPartTile / kTile;  // frames and takes them 64 at a time
constexpr uint32_t kScanChunk = 1024;
static_assert(kPartTile == 4u * 64u * kPartRounds, "four waves, whole rounds");

// the lanes of the wave whose frame is valid and falls into this lane's bucket:
// one ballot per bucket bit
__device__ __forceinline__ uint64_t bucket_peers(uint32_t b, bool valid, uint32_t nbits) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {
        if (k < nbits) {  // uniform
            const bool bit = (b >> k) & 1u;
            const uint64_t bb = __ballot(bit);
            m &= bit ? bb : ~bb;
        }
    }
    return m;
}

// Phase A of both kernels: the wave's histogram of its 256 frames in its own
// LDS row (zeroed before), one leader lane per bucket and round adding the
// bucket's peer count. The LDS serves a wave's accesses in program order, so
// the next round's leader reads what this round's stored. bk[r] keeps the
// lane's bucket of round r (0xFFFFFFFF past the table) for phase C.
__device__ __forceinline__ void wave_hist(const nexg_flow* flows, uint64_t count, uint32_t P, uint32_t nbits,
                                          uint64_t first, volatile uint32_t* row, uint32_t (&bk)[kPartRounds]) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t r = 0; r < kPartRounds; r++) {
        const uint64_t idx = first + 64u * r + lane;
        const bool valid = idx < count;
        const uint32_t b = valid ? NEXG_GLOBAL(uint32_t, flows)[idx * 2u] % P : 0u;
        bk[r] = valid ? b : 0xFFFFFFFFu;
        const uint64_t m = bucket_peers(b, valid, nbits);
        const uint32_t cnt = (uint32_t)__builtin_popcountll(m);
        if (valid && lanes_below(m) == cnt - 1u) row[b] += cnt;
    }
}

// hist[b * T + tile] = the number of the tile's frames in bucket b
__global__ __launch_bounds__(256) void k_part_count(const nexg_flow* flows, uint64_t count, uint32_t P, uint32_t nbits,
                                                    uint64_t T, uint32_t* hist) {
    __shared__ uint32_t s_w[4][256];
    const uint32_t t = threadIdx.x, wv = t >> 6;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) s_w[k][t] = 0u;
    __syncthreads();
    uint32_t bk[kPartRounds];
    wave_hist(flows, count, P, nbits, (uint64_t)blockIdx.x * kPartTile + (uint64_t)wv * (kPartTile / 4u), s_w[wv], bk);
    __syncthreads();
    if (t < P) hist[(uint64_t)t * T + blockIdx.x] = s_w[0][t] + s_w[1][t] + s_w[2][t] + s_w[3][t];
}

// the hierarchical scan of the n = P * T counters: sums of 1024-counter chunks,
// (block_sum), k_tile_scan over the chunk sums, then each chunk's own exclusive
// scan (block_excl_scan) on top of its base. No workgroup waits for another.
__global__ __launch_bounds__(256) void k_chunk_sums(const uint32_t* v, uint64_t n, uint32_t* sums) {
    __shared__ uint32_t s_w[4];
    const uint64_t base = (uint64_t)blockIdx.x * kScanChunk;
    uint32_t x = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanChunk / kTile; k++) {
        const uint64_t i = base + k * kTile + threadIdx.x;
        if (i < n) x += v[i];
    }
    const uint32_t sum = (uint32_t)block_sum(x, s_w);
    if (threadIdx.x == 0) sums[blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void k_chunk_apply(uint32_t* v, uint64_t n, const uint32_t* sums) {
    __shared__ uint32_t s_w[4];
    const uint64_t base = (uint64_t)blockIdx.x * kScanChunk;
    uint32_t carry = sums[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < kScanChunk / kTile; k++) {
        const uint64_t i = base + k * kTile + threadIdx.x;
        uint32_t total;
        const uint32_t before = block_excl_scan(i < n ? v[i] : 0u, s_w, total);
        if (i < n) v[i] = carry + before;
        carry += total;
        __syncthreads();  // s_w is rewritten by the next step
    }
}

// k_part_scatter: phase A again (the histogram of each wave's 256 frames), then
// lane b turns bucket b's four wave counts into the waves' first positions
// inside the tile's own bucket order (a workgroup scan of the 256 bucket
// totals) and keeps the distance from there to the bucket's scanned global
// base; each wave walks its rounds once more: a frame's position in the tile's
// order is its bucket's running position in the wave's row plus its rank among
// the round's peers below it, and the bucket's last peer advances the row
// (frames of a bucket are thereby numbered by wave, round and lane, which is
// their index order). The frame's number and bucket are parked at that
// position in LDS, and after one more barrier consecutive lanes take
// consecutive positions: a bucket's frames of this tile leave as one run of
// consecutive entries per output array (128 entries long at 8 buckets, 4 at
// 256) instead of one isolated store per frame and array.
__global__ __launch_bounds__(256) void k_part_scatter(ParseArgs a, const nexg_flow* flows, uint32_t P, uint32_t nbits,
                                                      uint64_t T, const uint32_t* base, uint32_t* out_index,
                                                      uint64_t* out_off, uint32_t* out_len, uint64_t* bucket_first) {
    __shared__ uint32_t s_w[4][256];
    __shared__ uint32_t s_ord[kPartTile];  // frame number in the tile | bucket << 16, in the tile's bucket order
    __shared__ uint32_t s_delta[256];      // global position - position in the tile's order, per bucket
    __shared__ uint32_t s_ws[4];
    const uint32_t t = threadIdx.x, wv = t >> 6, lane = t & 63u;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) s_w[k][t] = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kPartRounds; k++) s_ord[k * kTile + t] = 0xFFFFFFFFu;
    __syncthreads();
    const uint64_t tile0 = (uint64_t)blockIdx.x * kPartTile;
    uint32_t bk[kPartRounds];
    wave_hist(flows, a.count, P, nbits, tile0 + (uint64_t)wv * (kPartTile / 4u), s_w[wv], bk);
    __syncthreads();
    {
        uint32_t c[4], tot = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) c[k] = s_w[k][t], tot += c[k];  // 0 for t >= P
        uint32_t frames;
        uint32_t run = block_excl_scan(tot, s_ws, frames);  // the bucket's first position in the tile's order
        const uint32_t b0 = t < P ? base[(uint64_t)t * T + blockIdx.x] : 0u;
        s_delta[t] = b0 - run;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            s_w[k][t] = run;
            run += c[k];
        }
        if (blockIdx.x == 0 && t < P) bucket_first[t] = b0;  // tile 0's base: the frames in the buckets below
        if (blockIdx.x == 0 && t == 0) bucket_first[P] = a.count;
    }
    __syncthreads();
    volatile uint32_t* row = s_w[wv];
#pragma unroll
    for (uint32_t r = 0; r < kPartRounds; r++) {
        const bool valid = bk[r] != 0xFFFFFFFFu;
        const uint32_t b = valid ? bk[r] : 0u;
        const uint64_t m = bucket_peers(b, valid, nbits);
        if (valid) {
            const uint32_t cnt = (uint32_t)__builtin_popcountll(m), rank = lanes_below(m);
            const uint32_t lp = row[b] + rank;
            if (rank == cnt - 1u) row[b] = lp + 1u;
            if (lp < kPartTile) s_ord[lp] = (wv * (kPartTile / 4u) + 64u * r + lane) | b << 16;  // always: the counts are this kernel's own
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kPartRounds; r++) {
        const uint32_t j = r * kTile + t, e = s_ord[j];
        if (e != 0xFFFFFFFFu) {
            const uint64_t idx = tile0 + (e & 0xFFFFu);
            const uint32_t pos = j + s_delta[e >> 16];
            uint64_t off, l64;
            table_extent(a, idx, off, l64);
            // pos < count by construction (checked all the same: flows and the
            // workspace are caller memory, and a caller rewriting them between
            // the passes must not turn into a store out of bounds)
            if (pos < a.count) {
                out_index[pos] = (uint32_t)idx;
                if (out_off) {
                    out_off[pos] = off;
                    out_len[pos] = l64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)l64;
                }
            }
        }
    }
}

hipError_t launch_flow_partition(const ParseArgs& a, const nexg_flow* flows, uint32_t buckets, uint32_t* out_index,
                                 uint64_t* out_off, uint32_t* out_len, uint64_t* bucket_first, void* workspace,
                                 hipStream_t s) {
    if (a.count == 0) return hipMemsetAsync(bucket_first, 0, 8u * ((uint64_t)buckets + 1u), s);
    const uint64_t T = (a.count + kPartTile - 1) / kPartTile, n = T * buckets;
    const uint64_t chunks = (n + kScanChunk - 1) / kScanChunk;
    // the workspace as nexg_flow_partition_workspace lays it out
    uint64_t* total = static_cast<uint64_t*>(workspace);
    uint32_t* sums = reinterpret_cast<uint32_t*>(total + 1);
    uint32_t* hist = sums + ((chunks + 1u) & ~1ull);
    const uint32_t nbits = buckets > 1u ? 32u - (uint32_t)__builtin_clz(buckets - 1u) : 0u;
    hipLaunchKernelGGL(k_part_count, dim3((uint32_t)T), dim3(kTile), 0, s, flows, a.count, buckets, nbits, T, hist);
    hipLaunchKernelGGL(k_chunk_sums, dim3((uint32_t)chunks), dim3(kTile), 0, s, hist, n, sums);
    hipLaunchKernelGGL(k_tile_scan<uint32_t>, dim3(1), dim3(kTile), 0, s, sums, chunks, total);
    hipLaunchKernelGGL(k_chunk_apply, dim3((uint32_t)chunks), dim3(kTile), 0, s, hist, n, sums);
    hipLaunchKernelGGL(k_part_scatter, dim3((uint32_t)T), dim3(kTile), 0, s, a, flows, buckets, nbits, T, hist, out_index,
                       out_off, out_len, bucket_first);
    return hipGetLastError();
}

}  // namespace nexg
