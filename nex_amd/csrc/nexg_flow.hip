// nexg_flow.hip — flow keys, the Toeplitz RSS hash and the flow-affine
// partition on gfx950 (include/nexg.h; an extension: the reference has no flow
// notion). nexg_flow_batch is a second pass over a batch already parsed with
// NEXG_OUT_RECORD that gives every frame an 8-byte flow row; nexg_flow_partition
// is one stable radix pass over those rows with up to 256 buckets (a histogram
// per 1024-frame tile, a hierarchical scan of the histograms, a scatter), the
// select's count / scan / scatter shape with P counters per tile instead of one.
// nexg_flow_sort is four such passes over the 32-bit hash with 256 buckets (a
// stable LSD radix sort of (hash, index) pairs), and nexg_flow_groups reduces
// the sorted batch to one row per run of equal hashes by prefix sums.
// nexg_flow_table_merge keeps a table of flow entries across batches: a
// merge-path merge of the table with a batch's groups, both ascending by hash.
#include "table_kernels.hpp"
#include "workspace_layout.hpp"

namespace nexg {

static_assert(sizeof(nexg_flow) == 8, "nexg_flow is 8 bytes (include/nexg.h)");
static_assert(sizeof(nexg_flow_option) == 48, "nexg_flow_option is 48 bytes (include/nexg.h)");
static_assert(sizeof(nexg_flow_group) == 32, "nexg_flow_group is 32 bytes (include/nexg.h)");

// ---- flow rows -----------------------------------------------------------------------

constexpr uint32_t kFlowNibbles = 72;  // 36 key bytes at most

// A frame's flow key as nexg_flow_batch documents it (include/nexg.h): which
// frames have a flow, the IPv4 fragment rule, the IPv6 addresses out of the
// frame, the symmetric exchange. k_flow hashes the words; k_group_mark compares
// them. Per lane: 48 B of its record (the three 16-B quarters that hold flags /
// l3_off, ip_word / ip_proto / ip_src, ip_dst / the ports) and, for an IPv6
// frame, its two addresses as big-endian words (frame_be_words of
// table_kernels.hpp). A lane with `on` false loads nothing and has no flow.
// ext / l64: table_extent's verdict and len(idx) (false / 0 without `on`).
struct FlowKeyWords {
    uint32_t W[9];         // the key bytes as big-endian words: 2 or 3 (IPv4), 8 or 9 (IPv6); 0 past the key
    uint32_t kind, proto;  // NEXG_FLOW_*; record.ip_proto, 0 without a flow
    bool has, v6, l4, swapped;
};
__device__ __forceinline__ FlowKeyWords flow_key_words(const ParseArgs& a, const nexg_record* recs, uint64_t idx, bool on,
                                                       uint32_t opt, bool& ext, uint64_t& l64) {
    RecQuarter<0> q0{make_uint4(0u, 0u, 0u, 0u)};
    RecQuarter<1> q1{make_uint4(0u, 0u, 0u, 0u)};
    RecQuarter<2> q2{make_uint4(0u, 0u, 0u, 0u)};
    uint64_t off = 0;
    l64 = 0;
    ext = false;
    if (on) {
        q0 = rec_quarter<0>(recs + idx);
        q1 = rec_quarter<1>(recs + idx);
        q2 = rec_quarter<2>(recs + idx);
        ext = table_extent(a, idx, off, l64);
    }
    const uint32_t flags = rec_dw<kRecFlags>(q0), l3 = rec_l3(rec_dw<kRecL3>(q0)), ip_word = rec_dw<kRecIpWord>(q1),
                   proto = rec_proto(rec_dw<kRecProto>(q1)), ports_dw = rec_dw<kRecPorts>(q2);
    const bool ok = on && rec_status(flags) == 0u;
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
    const uint32_t kind = v4 ? (l4 ? NEXG_FLOW_IPV4_L4 : NEXG_FLOW_IPV4) : v6 ? (l4 ? NEXG_FLOW_IPV6_L4 : NEXG_FLOW_IPV6)
                                                                             : NEXG_FLOW_NONE;
    return {{S[0], v6 ? S[1] : D[0], v6 ? S[2] : ports, v6 ? S[3] : 0u, v6 ? D[0] : 0u, v6 ? D[1] : 0u, v6 ? D[2] : 0u,
             v6 ? D[3] : 0u, v6 ? ports : 0u},
            kind, has ? proto : 0u, has, v6, l4, swapped};
}

// k_flow: one lane per frame. The hash is linear over GF(2), so it is the XOR
// of one table entry per 4-bit nibble of the key bytes: s_tab[p][n] = the XOR
// of the key windows K[4p + k, 4p + k + 32) over the set bits k of n. The
// table (72 x 16 words, 4.5 KiB) is built per workgroup from the ten key words
// (4.5 entries per lane, 4 shift / select / XOR steps each); a lookup reads
// one of 16 consecutive words, so the 64 lanes of a wave touch 16 distinct
// banks at most and lanes with equal nibbles share a broadcast: no bank
// conflict, where a 256-entry byte table would see the lanes' random bytes
// collide, and the bit-serial form costs three VALU steps per key bit (864 for
// an IPv6 frame with ports against 72 lookups). Per lane: flow_key_words'
// loads and one 8-B non-temporal store; consecutive lanes write consecutive
// rows. Words no lane of the wave has (the IPv6 words in a wave of IPv4
// frames) are skipped by wave-uniform branches; a lane with a shorter key
// looks up nibble 0 there, whose entry is 0.
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
    bool ext;
    uint64_t l64;
    const FlowKeyWords kw = flow_key_words(a, recs, idx, true, opt, ext, l64);
    const bool has = kw.has, v6 = kw.v6, l4 = kw.l4;
    const uint32_t(&W)[9] = kw.W;
    uint32_t h = 0;
#pragma unroll
    for (uint32_t j = 0; j < 9; j++) {
        const bool mine = j < 2u ? has : j == 2u ? (v6 || l4) : j < 8u ? v6 : (v6 && l4);
        if (__ballot(mine) == 0ull) continue;  // wave-uniform
#pragma unroll
        for (uint32_t q = 0; q < 8; q++) h ^= s_tab[(8u * j + q) * 16u + ((W[j] >> (28u - 4u * q)) & 15u)];
    }
    const uint32_t tail = kw.kind | kw.proto << 8 | (kw.swapped ? 1u << 16 : 0u);
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
static_assert(kScanChunk == FlowPartLayout::kChunk, "the workspace holds one sum per chunk of the scan");

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
// bucket(idx) is how a lane gets its bucket: PartBucket for the partition,
// SortDigit (below) for a pass of the sort.
struct PartBucket {
    const nexg_flow* flows;
    uint32_t P;
    __device__ __forceinline__ uint32_t operator()(uint64_t idx) const { return NEXG_GLOBAL(uint32_t, flows)[idx * 2u] % P; }
};

template <typename Bucket>
__device__ __forceinline__ void wave_hist(const Bucket& bucket, uint64_t count, uint32_t nbits, uint64_t first,
                                          volatile uint32_t* row, uint32_t (&bk)[kPartRounds]) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t r = 0; r < kPartRounds; r++) {
        const uint64_t idx = first + 64u * r + lane;
        const bool valid = idx < count;
        const uint32_t b = valid ? bucket(idx) : 0u;
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
    wave_hist(PartBucket{flows, P}, count, nbits, (uint64_t)blockIdx.x * kPartTile + (uint64_t)wv * (kPartTile / 4u),
              s_w[wv], bk);
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

// the scan's three kernels over the n counters of `hist`, in place
static void launch_counter_scan(uint32_t* hist, uint64_t n, uint32_t* sums, uint64_t* total, hipStream_t s) {
    const uint64_t chunks = (n + kScanChunk - 1) / kScanChunk;
    const dim3 gC((uint32_t)chunks), b(kTile);
    hipLaunchKernelGGL(k_chunk_sums, gC, b, 0, s, hist, n, sums);
    hipLaunchKernelGGL(k_tile_scan<uint32_t>, dim3(1), b, 0, s, sums, chunks, total);
    hipLaunchKernelGGL(k_chunk_apply, gC, b, 0, s, hist, n, sums);
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
// 256) instead of one isolated store per frame and array. tile_bucket_order is
// all of that up to the parked order (s_ord, s_delta), for the partition and
// for the sort's passes alike; it returns the lane's bucket's global base.
template <typename Bucket>
__device__ __forceinline__ uint32_t tile_bucket_order(const Bucket& bucket, uint64_t count, uint32_t P, uint32_t nbits,
                                                      uint64_t T, const uint32_t* base, uint32_t (*s_w)[256],
                                                      uint32_t* s_ord, uint32_t* s_delta, uint32_t* s_ws) {
    const uint32_t t = threadIdx.x, wv = t >> 6, lane = t & 63u;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) s_w[k][t] = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kPartRounds; k++) s_ord[k * kTile + t] = 0xFFFFFFFFu;
    __syncthreads();
    const uint64_t tile0 = (uint64_t)blockIdx.x * kPartTile;
    uint32_t bk[kPartRounds];
    wave_hist(bucket, count, nbits, tile0 + (uint64_t)wv * (kPartTile / 4u), s_w[wv], bk);
    __syncthreads();
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
    return b0;
}

__global__ __launch_bounds__(256) void k_part_scatter(ParseArgs a, const nexg_flow* flows, uint32_t P, uint32_t nbits,
                                                      uint64_t T, const uint32_t* base, uint32_t* out_index,
                                                      uint64_t* out_off, uint32_t* out_len, uint64_t* bucket_first) {
    __shared__ uint32_t s_w[4][256];
    __shared__ uint32_t s_ord[kPartTile];  // frame number in the tile | bucket << 16, in the tile's bucket order
    __shared__ uint32_t s_delta[256];      // global position - position in the tile's order, per bucket
    __shared__ uint32_t s_ws[4];
    const uint32_t t = threadIdx.x;
    const uint64_t tile0 = (uint64_t)blockIdx.x * kPartTile;
    const uint32_t b0 = tile_bucket_order(PartBucket{flows, P}, a.count, P, nbits, T, base, s_w, s_ord, s_delta, s_ws);
    if (blockIdx.x == 0 && t < P) bucket_first[t] = b0;  // tile 0's base: the frames in the buckets below
    if (blockIdx.x == 0 && t == 0) bucket_first[P] = a.count;
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
    const FlowPartLayout w = FlowPartLayout::from(a.count, buckets);
    const uint64_t T = w.tiles;
    uint32_t* hist = region<uint32_t>(workspace, w.hist);
    const uint32_t nbits = buckets > 1u ? 32u - (uint32_t)__builtin_clz(buckets - 1u) : 0u;
    hipLaunchKernelGGL(k_part_count, dim3((uint32_t)T), dim3(kTile), 0, s, flows, a.count, buckets, nbits, T, hist);
    launch_counter_scan(hist, w.counters, region<uint32_t>(workspace, w.sums), region<uint64_t>(workspace, w.total), s);
    hipLaunchKernelGGL(k_part_scatter, dim3((uint32_t)T), dim3(kTile), 0, s, a, flows, buckets, nbits, T, hist, out_index,
                       out_off, out_len, bucket_first);
    return hipGetLastError();
}

// ---- sort --------------------------------------------------------------------------------
// Four passes of the partition's count / scan / scatter with 256 buckets, one
// per byte of the hash from the lowest up: a stable LSD radix sort. What moves
// is a (hash, index) pair in one u64 (hash low, frame number high); the first
// pass makes the pairs from the flow rows, the last stores the frame numbers
// alone. The workspace is the partition's at 256 buckets, then two buffers of
// `count` pairs (nexg_flow_sort_workspace).

// kOrdered (with kFirst): the chain starts from the order a chain before it
// left, not from the table's: position k holds frame order[k] (an entry past
// the table stands for key 0), which is how a sort by two keys is two chains.
template <bool kFirst, bool kOrdered = false>
struct SortDigit {
    const void* src;  // kFirst: the rows, the key their low word; else the pairs the pass before stored
    const uint32_t* order;  // kOrdered only
    uint64_t count;
    uint32_t shift;
    __device__ __forceinline__ uint64_t pair(uint64_t idx) const {
        if constexpr (kFirst && kOrdered) {
            const uint64_t i = order[idx];
            const uint64_t v = i < count ? NEXG_GLOBAL(uint64_t, src)[i] : 0ull;
            return (v & 0xFFFFFFFFull) | i << 32;
        } else {
            const uint64_t v = NEXG_GLOBAL(uint64_t, src)[idx];
            return kFirst ? (v & 0xFFFFFFFFull) | idx << 32 : v;
        }
    }
    __device__ __forceinline__ uint32_t operator()(uint64_t idx) const { return ((uint32_t)pair(idx) >> shift) & 255u; }
};

// k_part_count with the pass's digit as the bucket
template <bool kFirst, bool kOrdered = false>
__global__ __launch_bounds__(256) void k_sort_count(const void* src, const uint32_t* order, uint64_t count, uint32_t shift,
                                                    uint64_t T, uint32_t* hist) {
    __shared__ uint32_t s_w[4][256];
    const uint32_t t = threadIdx.x, wv = t >> 6;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) s_w[k][t] = 0u;
    __syncthreads();
    uint32_t bk[kPartRounds];
    wave_hist(SortDigit<kFirst, kOrdered>{src, order, count, shift}, count, 8u, (uint64_t)blockIdx.x * kPartTile + (uint64_t)wv * (kPartTile / 4u),
              s_w[wv], bk);
    __syncthreads();
    hist[(uint64_t)t * T + blockIdx.x] = s_w[0][t] + s_w[1][t] + s_w[2][t] + s_w[3][t];
}

// k_part_scatter's shape: a digit's pairs of this tile leave as one run of
// consecutive 8-B entries (kLast: 4-B frame numbers). A pair is loaded a second
// time for the store (its tile's 8 KiB were read a moment ago); whatever the
// source holds by then, the position comes from the parked order and is
// checked against `count`.
template <bool kFirst, bool kLast, bool kOrdered = false>
__global__ __launch_bounds__(256) void k_sort_scatter(const void* src, const uint32_t* order, uint64_t count, uint32_t shift,
                                                      uint64_t T, const uint32_t* base, uint64_t* dst, uint32_t* out_index) {
    __shared__ uint32_t s_w[4][256];
    __shared__ uint32_t s_ord[kPartTile];
    __shared__ uint32_t s_delta[256];
    __shared__ uint32_t s_ws[4];
    const uint32_t t = threadIdx.x;
    const uint64_t tile0 = (uint64_t)blockIdx.x * kPartTile;
    const SortDigit<kFirst, kOrdered> digit{src, order, count, shift};
    tile_bucket_order(digit, count, 256u, 8u, T, base, s_w, s_ord, s_delta, s_ws);
#pragma unroll
    for (uint32_t r = 0; r < kPartRounds; r++) {
        const uint32_t j = r * kTile + t, e = s_ord[j];
        if (e != 0xFFFFFFFFu) {
            const uint64_t pair = digit.pair(tile0 + (e & 0xFFFFu));
            const uint32_t pos = j + s_delta[e >> 16];
            if (pos < count) {
                if (kLast)
                    out_index[pos] = (uint32_t)(pair >> 32);
                else
                    dst[pos] = pair;
            }
        }
    }
}

// rows: `count` u64, the 32-bit key in the low word. start: nullptr, or the
// order the chain starts from (it may be out_index: the first pass reads it,
// the last writes).
hipError_t launch_radix_sort(const void* rows, const uint32_t* start, uint64_t count, uint32_t* out_index, void* workspace,
                             hipStream_t s) {
    if (count == 0) return hipSuccess;
    const FlowSortLayout w = FlowSortLayout::from(count);
    const uint64_t T = w.tiles;
    uint32_t* hist = region<uint32_t>(workspace, w.hist);
    uint64_t* ping = region<uint64_t>(workspace, w.ping);
    uint64_t* pong = region<uint64_t>(workspace, w.pong);
    const dim3 gT((uint32_t)T), b(kTile);
    for (uint32_t pass = 0; pass < 4; pass++) {
        const void* src = pass == 0 ? rows : (pass & 1u) ? ping : pong;
        uint64_t* dst = (pass & 1u) ? pong : ping;
        const uint32_t shift = 8u * pass;
        if (pass == 0 && start)
            hipLaunchKernelGGL((k_sort_count<true, true>), gT, b, 0, s, src, start, count, shift, T, hist);
        else if (pass == 0)
            hipLaunchKernelGGL(k_sort_count<true>, gT, b, 0, s, src, start, count, shift, T, hist);
        else
            hipLaunchKernelGGL(k_sort_count<false>, gT, b, 0, s, src, start, count, shift, T, hist);
        launch_counter_scan(hist, w.counters, region<uint32_t>(workspace, w.sums), region<uint64_t>(workspace, w.total), s);
        if (pass == 0 && start)
            hipLaunchKernelGGL((k_sort_scatter<true, false, true>), gT, b, 0, s, src, start, count, shift, T, hist, dst, out_index);
        else if (pass == 0)
            hipLaunchKernelGGL((k_sort_scatter<true, false>), gT, b, 0, s, src, start, count, shift, T, hist, dst, out_index);
        else if (pass < 3)
            hipLaunchKernelGGL((k_sort_scatter<false, false>), gT, b, 0, s, src, start, count, shift, T, hist, dst, out_index);
        else
            hipLaunchKernelGGL((k_sort_scatter<false, true>), gT, b, 0, s, src, start, count, shift, T, hist, dst, out_index);
    }
    return hipGetLastError();
}

hipError_t launch_flow_sort(const nexg_flow* flows, uint64_t count, uint32_t* out_index, void* workspace, hipStream_t s) {
    return launch_radix_sort(flows, nullptr, count, out_index, workspace, s);
}

// ---- groups ------------------------------------------------------------------------------
// One row per run of equal hashes in the sorted order. k_group_mark gives
// every sorted position a head flag (the hash differs from the position
// before, or position 0), a break flag (same hash, another key) and its
// frame's length, and scans the three inside its 256-position tile; one
// workgroup scans the tiles' totals (k_tile_scan, once per value);
// k_group_place numbers the groups and notes where each starts; k_group_rows,
// one lane per group, takes the differences of the prefixes at the group's
// start and at the next group's. Every step is per position or per group: the
// sizes of the groups do not enter.

// what k_group_mark leaves per position: the exclusive in-tile prefixes of the
// lengths (at most 255 x 65535 < 2^24), of the breaks and of the heads (at
// most 255 each), and the head flag
constexpr uint32_t kMarkBrk = 24, kMarkHeads = 32, kMarkHead = 40;
// the three values in one u64 for the tile's scan: 256 x 65535 < 2^24, then two
// counts of at most 256
constexpr uint32_t kSumBrk = 24, kSumHeads = 34;

__device__ __forceinline__ bool flow_keys_differ(const FlowKeyWords& x, const FlowKeyWords& y) {
    uint32_t d = (x.kind ^ y.kind) | (x.proto ^ y.proto);
#pragma unroll
    for (uint32_t j = 0; j < 9; j++) d |= x.W[j] ^ y.W[j];
    return d != 0u;
}

// `order` is caller memory: an entry past the table stands for a frame with an
// all-zero flow row, no key and length 0, and nothing is loaded for it. The
// key of the position before is recomputed, not exchanged: a lane needs it only
// when the two hashes are equal.
__global__ __launch_bounds__(256) void k_group_mark(ParseArgs a, const nexg_record* recs, const nexg_flow* flows,
                                                    uint32_t opt, const uint32_t* order, uint64_t* mark,
                                                    uint32_t* tile_heads, uint32_t* tile_brk, uint64_t* tile_bytes) {
    __shared__ uint64_t s_w[4];
    const uint64_t k = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    const bool in = k < a.count, prev = in && k > 0;
    const uint32_t i = in ? order[k] : 0xFFFFFFFFu, j = prev ? order[k - 1] : 0xFFFFFFFFu;
    const bool vi = in && i < a.count, vj = prev && j < a.count;
    const uint32_t hi = vi ? NEXG_GLOBAL(uint32_t, flows)[(uint64_t)i * 2u] : 0u;
    const uint32_t hj = vj ? NEXG_GLOBAL(uint32_t, flows)[(uint64_t)j * 2u] : 0u;
    const bool head = in && (!prev || hi != hj);
    bool ext, ext_j;
    uint64_t l64, l64_j;
    const FlowKeyWords ki = flow_key_words(a, recs, i, vi, opt, ext, l64);
    const FlowKeyWords kj = flow_key_words(a, recs, j, vj && !head, opt, ext_j, l64_j);
    const bool brk = in && !head && flow_keys_differ(ki, kj);
    const uint64_t len = ext ? l64 : 0u;  // <= 65535 with a valid extent
    uint64_t total;
    const uint64_t before = block_excl_scan(len | (uint64_t)brk << kSumBrk | (uint64_t)head << kSumHeads, s_w, total);
    if (in)
        mark[k] = (before & 0xFFFFFFull) | ((before >> kSumBrk) & 0xFFull) << kMarkBrk |
                  ((before >> kSumHeads) & 0xFFull) << kMarkHeads | (uint64_t)head << kMarkHead;
    if (threadIdx.x == 0) {
        tile_bytes[blockIdx.x] = total & 0xFFFFFFull;
        tile_brk[blockIdx.x] = (uint32_t)(total >> kSumBrk) & 0x3FFu;
        tile_heads[blockIdx.x] = (uint32_t)(total >> kSumHeads);
    }
}

// the group number of every position (the heads at and before it, less one),
// stored by frame number, and each group's first position
__global__ __launch_bounds__(256) void k_group_place(uint64_t count, const uint32_t* order, const uint64_t* mark,
                                                     const uint32_t* tile_heads, uint32_t* starts, uint32_t* out_group) {
    const uint64_t k = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    if (k >= count) return;
    const uint64_t m = mark[k];
    const uint32_t head = (uint32_t)(m >> kMarkHead) & 1u;
    const uint32_t g = tile_heads[blockIdx.x] + ((uint32_t)(m >> kMarkHeads) & 0xFFu) + head - 1u;
    // g <= k by construction; checked all the same, as the workspace is caller memory
    if (head && g < count) starts[g] = (uint32_t)k;
    if (out_group) {
        const uint32_t i = order[k];
        if (i < count) out_group[i] = g;
    }
}

__global__ __launch_bounds__(256) void k_group_rows(uint64_t count, const nexg_flow* flows,
                                                    const uint32_t* order, const uint64_t* mark, const uint32_t* tile_brk,
                                                    const uint64_t* tile_bytes, const uint64_t* totals,
                                                    const uint32_t* starts, const uint64_t* out_count, nexg_flow_group* out,
                                                    uint64_t cap) {
    const uint64_t g = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    uint64_t G = *out_count;
    if (G > count) G = count;
    if (g >= G || g >= cap) return;
    // positions out of the workspace are clamped before they index anything
    uint64_t first = starts[g], next = g + 1 < G ? starts[g + 1] : count;
    if (first >= count) first = count - 1u;
    if (next > count) next = count;
    const uint64_t m0 = mark[first];
    uint64_t bytes0 = tile_bytes[first >> 8] + (m0 & 0xFFFFFFull), bytes1 = totals[1];
    uint32_t brk0 = tile_brk[first >> 8] + ((uint32_t)(m0 >> kMarkBrk) & 0xFFu), brk1 = (uint32_t)totals[0];
    if (next < count) {
        const uint64_t m1 = mark[next];
        bytes1 = tile_bytes[next >> 8] + (m1 & 0xFFFFFFull);
        brk1 = tile_brk[next >> 8] + ((uint32_t)(m1 >> kMarkBrk) & 0xFFu);
    }
    const uint32_t fi = order[first];
    const uint64_t row = fi < count ? NEXG_GLOBAL(uint64_t, flows)[fi] : 0ull;
    const uint64_t bytes = bytes1 - bytes0;
    const uint32_t mixed = brk1 - brk0;
    uint4* o = reinterpret_cast<uint4*>(out + g);
    o[0] = make_uint4((uint32_t)row, ((uint32_t)(row >> 32) & 0xFFFFu) | (mixed != 0u ? 1u << 16 : 0u), (uint32_t)first,
                      (uint32_t)(next - first));
    o[1] = make_uint4((uint32_t)bytes, (uint32_t)(bytes >> 32), mixed, fi);
}

hipError_t launch_flow_groups(const ParseArgs& a, const nexg_record* recs, const nexg_flow* flows, uint32_t opt,
                              const uint32_t* order, nexg_flow_group* out, uint64_t groups_cap, uint32_t* out_group,
                              uint64_t* out_count, void* workspace, hipStream_t s) {
    const uint64_t count = a.count;
    if (count == 0) return hipMemsetAsync(out_count, 0, 8, s);
    const FlowGroupsLayout w = FlowGroupsLayout::from(count);
    const uint64_t tiles = w.tiles;
    uint64_t* totals = region<uint64_t>(workspace, w.totals);  // breaks, bytes
    uint64_t* tile_bytes = region<uint64_t>(workspace, w.tile_bytes);
    uint64_t* mark = region<uint64_t>(workspace, w.mark);
    uint32_t* tile_heads = region<uint32_t>(workspace, w.tile_heads);
    uint32_t* tile_brk = region<uint32_t>(workspace, w.tile_brk);
    uint32_t* starts = region<uint32_t>(workspace, w.starts);
    const dim3 gT((uint32_t)tiles), b(kTile);
    hipLaunchKernelGGL(k_group_mark, gT, b, 0, s, a, recs, flows, opt, order, mark, tile_heads, tile_brk, tile_bytes);
    hipLaunchKernelGGL(k_tile_scan<uint32_t>, dim3(1), b, 0, s, tile_heads, tiles, out_count);
    hipLaunchKernelGGL(k_tile_scan<uint32_t>, dim3(1), b, 0, s, tile_brk, tiles, totals);
    hipLaunchKernelGGL(k_tile_scan<uint64_t>, dim3(1), b, 0, s, tile_bytes, tiles, totals + 1);
    hipLaunchKernelGGL(k_group_place, gT, b, 0, s, count, order, mark, tile_heads, starts, out_group);
    const uint64_t rows = groups_cap < count ? groups_cap : count;
    if (rows)
        hipLaunchKernelGGL(k_group_rows, dim3((uint32_t)((rows + kTile - 1) / kTile)), b, 0, s, count, flows, order,
                           mark, tile_brk, tile_bytes, totals, starts, out_count, out, groups_cap);
    return hipGetLastError();
}

// ---- table -------------------------------------------------------------------------------
// The flow table across batches: table_out = the union of table_in and one
// batch's groups, both ascending by hash (nexg_flow_table_merge, include/nexg.h).
// A merge-path merge. The merged order is by hash, a table entry before the
// group of the same hash. k_merge_mark, one workgroup per 256 positions of it:
// two lanes find where the tile starts and ends in the two arrays (one binary
// search along a diagonal each, the only dependent chains of global loads);
// the two runs' hashes (256 in all) are staged in LDS; every element is ranked
// against the other run there, which gives its position in the tile and whether
// its hash is in both; the "leaves an entry" flags (a kept table entry, a group
// with a new hash) are scanned in position order. k_tile_scan turns the tiles'
// totals into their first slots and gives *out_count. k_merge_write, one lane
// per position, builds the entry of a surviving position (table entry + group,
// key recompute and compare) and stores it as four 16-B stores; a group
// stores its entry's slot. No atomics.

static_assert(sizeof(nexg_flow_entry) == 64, "nexg_flow_entry is 64 bytes (include/nexg.h)");
static_assert(offsetof(nexg_flow_entry, kind) == 4 && offsetof(nexg_flow_entry, flags8) == 6 &&
                  offsetof(nexg_flow_entry, key) == 8 && offsetof(nexg_flow_entry, last_epoch) == 44 &&
                  offsetof(nexg_flow_entry, packets) == 48 && offsetof(nexg_flow_entry, bytes) == 56,
              "the entry by dword: hash, kind | proto << 8 | flags8 << 16, 9 key dwords, last_epoch, packets, bytes");
static_assert(offsetof(nexg_flow_group, flags8) == 6 && offsetof(nexg_flow_group, packets) == 12 &&
                  offsetof(nexg_flow_group, bytes) == 16 && offsetof(nexg_flow_group, first_index) == 28,
              "the group by dword: hash, kind | proto << 8 | flags8 << 16, first, packets, bytes, mixed, first_index");

// what k_merge_mark leaves per position, in one u64: the source in the low
// word (a table index, or a group index with kSrcGroup), in the high word the
// exclusive in-tile prefix of the survivors (at most 255) and three flags
constexpr uint32_t kSrcGroup = 1u << 31;
constexpr uint32_t kAuxLive = 1u << 16;   // leaves an entry
constexpr uint32_t kAuxBoth = 1u << 17;   // the hash is in the table and in the groups
constexpr uint32_t kAuxValid = 1u << 18;  // some element took the position (always, with ascending inputs)

constexpr uint32_t kEntryDw = sizeof(nexg_flow_entry) / 4u, kGroupDw = sizeof(nexg_flow_group) / 4u;

// the number of table entries among the first d positions of the merged order:
// the least i with A[i].hash > B[d - 1 - i].hash. lo <= i <= hi throughout, so
// every index is inside its array whatever the arrays hold.
__device__ __forceinline__ uint32_t merge_split(const nexg_flow_entry* A, uint32_t nA, const nexg_flow_group* B,
                                                uint32_t nB, uint32_t d) {
    uint32_t lo = d > nB ? d - nB : 0u, hi = d < nA ? d : nA;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        const uint32_t ha = NEXG_GLOBAL(uint32_t, A)[(uint64_t)mid * kEntryDw];
        const uint32_t hb = NEXG_GLOBAL(uint32_t, B)[(uint64_t)(d - 1u - mid) * kGroupDw];
        if (ha <= hb)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo;
}

// the number of s[0, n) below h (kIncl: at or below h), s ascending
template <bool kIncl>
__device__ __forceinline__ uint32_t lds_rank(const uint32_t* s, uint32_t n, uint32_t h) {
    uint32_t lo = 0, len = n;
    while (len) {
        const uint32_t half = len / 2u, v = s[lo + half];
        if (kIncl ? v <= h : v < h)
            lo += half + 1u, len -= half + 1u;
        else
            len = half;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_merge_mark(const nexg_flow_entry* A, uint32_t nA, const nexg_flow_group* B,
                                                    uint32_t nB, uint32_t min_epoch, uint64_t* mark,
                                                    uint32_t* tile_first) {
    __shared__ uint32_t s_ha[kTile], s_hb[kTile];  // the tile's table hashes and group hashes
    __shared__ uint32_t s_src[kTile], s_aux[kTile];  // by position in the tile
    __shared__ uint32_t s_split[2], s_edge[4], s_w[4];
    const uint32_t t = threadIdx.x;
    const uint64_t N = (uint64_t)nA + nB;
    const uint32_t d0 = blockIdx.x * kTile;
    const uint32_t cnt = N - d0 < kTile ? (uint32_t)(N - d0) : kTile;
    if (t == 0u || t == 64u) s_split[t >> 6] = merge_split(A, nA, B, nB, d0 + (t ? cnt : 0u));
    s_aux[t] = 0u;
    __syncthreads();
    // a0 <= min(d0, nA) and d0 - a0 <= nB by merge_split's bounds
    const uint32_t a0 = s_split[0], b0 = d0 - a0;
    uint32_t na = s_split[1] - a0;
    // inputs that are not ascending can make the two searches disagree: any split with
    // a0 + na <= nA and b0 + nb <= nB keeps the loads inside the arrays
    if (na > cnt) na = nA - a0 < cnt ? nA - a0 : cnt;
    const uint32_t nb = cnt - na;
    // one element per lane: the tile's table entries, then its groups
    const bool isA = t < na, isB = !isA && t < cnt;
    uint32_t h = 0, last = 0;
    if (isA) {
        const auto* e = NEXG_GLOBAL(uint32_t, A) + (uint64_t)(a0 + t) * kEntryDw;
        h = e[0], last = e[11];
        s_ha[t] = h;
    } else if (isB) {
        h = NEXG_GLOBAL(uint32_t, B)[(uint64_t)(b0 + t - na) * kGroupDw];
        s_hb[t - na] = h;
    }
    // the tie across a tile border: an entry that is the tile's last position has its
    // group as the next tile's first, so the neighbours' hashes are looked at as well
    if (t == 0u) {
        const bool prev = a0 > 0u, next = b0 + nb < nB;
        s_edge[0] = prev, s_edge[1] = prev ? NEXG_GLOBAL(uint32_t, A)[(uint64_t)(a0 - 1u) * kEntryDw] : 0u;
        s_edge[2] = next, s_edge[3] = next ? NEXG_GLOBAL(uint32_t, B)[(uint64_t)(b0 + nb) * kGroupDw] : 0u;
    }
    __syncthreads();
    if (isA) {
        const uint32_t r = lds_rank<false>(s_hb, nb, h);  // groups below: the entry goes before its group
        const bool both = r < nb ? s_hb[r] == h : (s_edge[2] != 0u && s_edge[3] == h);
        const bool live = both || last >= min_epoch;
        s_src[t + r] = a0 + t;  // t + r < na + nb
        s_aux[t + r] = kAuxValid | (live ? kAuxLive : 0u) | (both ? kAuxBoth : 0u);
    } else if (isB) {
        const uint32_t j = t - na, r = lds_rank<true>(s_ha, na, h);  // entries at or below
        const bool both = r > 0u ? s_ha[r - 1u] == h : (s_edge[0] != 0u && s_edge[1] == h);
        s_src[j + r] = kSrcGroup | (b0 + j);
        s_aux[j + r] = kAuxValid | (both ? kAuxBoth : kAuxLive);
    }
    __syncthreads();
    const uint32_t aux = s_aux[t];
    uint32_t total;
    const uint32_t before = block_excl_scan((aux & kAuxLive) ? 1u : 0u, s_w, total);
    if (t < cnt) mark[(uint64_t)d0 + t] = (uint64_t)(aux | before) << 32 | ((aux & kAuxValid) ? s_src[t] : 0u);
    if (t == 0u) tile_first[blockIdx.x] = total;
}

// Every index out of the workspace (caller memory) is checked against its
// array before it is used, and the slot against `cap`.
__global__ __launch_bounds__(256) void k_merge_write(ParseArgs a, const nexg_record* recs, uint32_t opt,
                                                     const nexg_flow_entry* A, uint32_t nA, const nexg_flow_group* B,
                                                     uint32_t nB, uint32_t epoch, const uint64_t* mark,
                                                     const uint32_t* tile_first, nexg_flow_entry* out, uint64_t cap,
                                                     uint32_t* out_slot) {
    const uint64_t N = (uint64_t)nA + nB, p = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    const uint64_t m = p < N ? mark[p] : 0ull;
    const uint32_t src = (uint32_t)m, aux = (uint32_t)(m >> 32), idx = src & ~kSrcGroup;
    const bool valid = (aux & kAuxValid) != 0u, both = (aux & kAuxBoth) != 0u;
    const bool fromB = valid && (src & kSrcGroup) != 0u && idx < nB, fromA = valid && !(src & kSrcGroup) && idx < nA;
    uint64_t slot = (uint64_t)tile_first[blockIdx.x] + (aux & 0xFFFFu);
    if (fromB) {
        if (both) slot -= 1u;  // its entry is the position before, which survives
        if (out_slot) out_slot[idx] = (uint32_t)slot;
    }
    const bool store = (fromA || fromB) && (aux & kAuxLive) != 0u && slot < cap;
    // the group of a matched entry is the next position: entry `idx` at position p has p - idx groups before it
    const uint32_t gi = fromB ? idx : (uint32_t)(p - idx);
    const bool with_group = store && (fromB || (both && p >= idx && p - idx < nB));
    uint4 g0 = make_uint4(0u, 0u, 0u, 0u), g1 = g0;
    if (with_group) {
        g0 = load16(reinterpret_cast<const uint8_t*>(B + gi));
        g1 = load16(reinterpret_cast<const uint8_t*>(B + gi) + 16u);
    }
    bool ext;
    uint64_t l64;
    const uint32_t fi = g1.w;
    const FlowKeyWords kw = flow_key_words(a, recs, fi, with_group && fi < a.count, opt, ext, l64);
    uint32_t K[9];
#pragma unroll
    for (uint32_t j = 0; j < 9; j++) K[j] = __builtin_bswap32(kw.W[j]);  // the key bytes in memory order
    const uint32_t tag = kw.kind | kw.proto << 8;
    uint4 e0, e1, e2, e3;
    if (fromB) {
        e0 = make_uint4(g0.x, tag | (g0.y & (NEXG_FLOW_ENTRY_MIXED << 16)), K[0], K[1]);
        e1 = make_uint4(K[2], K[3], K[4], K[5]);
        e2 = make_uint4(K[6], K[7], K[8], epoch);
        e3 = make_uint4(g0.w, 0u, g1.x, g1.y);
    } else {
        e0 = e1 = e2 = e3 = make_uint4(0u, 0u, 0u, 0u);
        if (store) {
            const uint8_t* e = reinterpret_cast<const uint8_t*>(A + idx);
            e0 = load16(e), e1 = load16(e + 16u), e2 = load16(e + 32u), e3 = load16(e + 48u);
        }
        if (with_group) {
            const uint32_t differ = ((e0.y ^ tag) & 0xFFFFu) | (e0.z ^ K[0]) | (e0.w ^ K[1]) | (e1.x ^ K[2]) | (e1.y ^ K[3]) |
                                    (e1.z ^ K[4]) | (e1.w ^ K[5]) | (e2.x ^ K[6]) | (e2.y ^ K[7]) | (e2.z ^ K[8]);
            e0.y |= (g0.y & (NEXG_FLOW_ENTRY_MIXED << 16)) | (differ ? NEXG_FLOW_ENTRY_MIXED << 16 : 0u);
            e2.w = epoch;
            const uint64_t packets = ((uint64_t)e3.y << 32 | e3.x) + g0.w;
            const uint64_t bytes = ((uint64_t)e3.w << 32 | e3.z) + ((uint64_t)g1.y << 32 | g1.x);
            e3 = make_uint4((uint32_t)packets, (uint32_t)(packets >> 32), (uint32_t)bytes, (uint32_t)(bytes >> 32));
        }
    }
    if (store) {
        uint4* o = reinterpret_cast<uint4*>(out + slot);
        o[0] = e0, o[1] = e1, o[2] = e2, o[3] = e3;
    }
}

hipError_t launch_flow_table_merge(const ParseArgs& a, const nexg_record* recs, uint32_t opt, const nexg_flow_group* groups,
                                   uint64_t n_groups, const nexg_flow_entry* table_in, uint64_t n_in, uint32_t epoch,
                                   uint32_t min_epoch, nexg_flow_entry* table_out, uint64_t table_cap, uint32_t* out_slot,
                                   uint64_t* out_count, void* workspace, hipStream_t s) {
    if (n_in + n_groups == 0) return hipMemsetAsync(out_count, 0, 8, s);
    const FlowTableLayout w = FlowTableLayout::from(n_in, n_groups);
    uint64_t* mark = region<uint64_t>(workspace, w.mark);
    uint32_t* tile_first = region<uint32_t>(workspace, w.tile_first);
    const dim3 gT((uint32_t)w.tiles), b(kTile);
    hipLaunchKernelGGL(k_merge_mark, gT, b, 0, s, table_in, (uint32_t)n_in, groups, (uint32_t)n_groups, min_epoch, mark,
                       tile_first);
    hipLaunchKernelGGL(k_tile_scan<uint32_t>, dim3(1), b, 0, s, tile_first, w.tiles, out_count);
    hipLaunchKernelGGL(k_merge_write, gT, b, 0, s, a, recs, opt, table_in, (uint32_t)n_in, groups, (uint32_t)n_groups, epoch,
                       mark, tile_first, table_out, table_cap, out_slot);
    return hipGetLastError();
}

}  // namespace nexg
