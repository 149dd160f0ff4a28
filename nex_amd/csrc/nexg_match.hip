// nexg_match.hip — fixed-string match on frame bytes and the selection by its
// rows on gfx950 (include/nexg.h; an extension: the reference has no payload
// search). k_match streams every region byte from HBM once and tests up to 32
// patterns at every start position behind a two-byte prefilter; the per-frame
// rule (region, fold, occurrence, row) is match_core.hpp's, which the host
// driver tests/native/match_fuzz.cpp runs too. k_match_count / k_tile_scan /
// k_match_scatter compact the frame table by the rows' masks in order. That is
// table_kernels.hpp's compaction written out: as the selector MatchPick of
// launch_compact the pass measured 0.7 to 1 % slower (the count kernel, which
// reads a count, a pointer and three masks, got the whole ParseArgs as its
// argument; profiles/table_skeletons/README.md), so it keeps its own kernels.
#include "match_core.hpp"
#include "table_kernels.hpp"
#include "workspace_layout.hpp"

namespace nexg {

static_assert(sizeof(nexg_pattern) == 32, "nexg_pattern is 32 bytes (include/nexg.h)");
static_assert(sizeof(nexg_patterns) == 8 + 32 * 32, "nexg_patterns is 1032 bytes (include/nexg.h)");
static_assert(sizeof(nexg_match) == 8, "nexg_match is 8 bytes (include/nexg.h)");
static_assert(sizeof(MatchPat) == 24 && sizeof(MatchSet) == 8 + 32 * 24, "the set as a kernel argument");

struct MatchArgs {
    ParseArgs a;
    const nexg_record* recs;
    MatchSet s;  // by value: under 1 KB of the 4-KB argument segment, no device copy
};

constexpr uint32_t kStarts = 16;  // start positions per work item

// k_match: one 256-lane workgroup per 256-frame tile.
//   1. every lane builds one row of the prefilter tables in LDS: T0[b] = the
//      patterns whose byte 0 can be b, T1[b] the same for byte 1 (all patterns
//      of length 1), both cases entered for the letters of a NOCASE pattern.
//      The patterns themselves go to LDS as well: a lane reads the ones its
//      prefilter lets through, at an index that differs from lane to lane.
//   2. lane t stages frame t's region: its absolute start address and length,
//      and the number of work items it makes, kStarts start positions each;
//      the tile's exclusive scan of those counts says which frame an item
//      belongs to.
//   3. lanes take the items t, t + 256, ...: a binary search of the scan finds
//      the frame, frame_be_words<8> fetches the <= 31 bytes the 16 starts can
//      touch as covering aligned dwords (each holds a region byte, so the
//      loads stay inside the frame's own 16-B blocks), and for every start
//      the 16-byte window is funnel-shifted out of those registers. Bytes past
//      the region may hold anything: match_at's length test leaves them out.
//   4. a lane's hits for one item are OR-ed / min-ed in registers, then into
//      the frame's LDS accumulators with one atomicOr and one atomicMin: the
//      result does not depend on the order of arrival. No global atomics.
//   5. after a barrier lane t stores frame t's 8-byte row.
__global__ __launch_bounds__(256) void k_match(MatchArgs p, nexg_match* out) {
    __shared__ uint32_t s_T0[256], s_T1[256];
    __shared__ uint32_t s_pat[NEXG_MATCH_MAX_PATTERNS][6];
    __shared__ uint64_t s_src[kTile];       // absolute address of the region's first byte
    __shared__ uint32_t s_n[kTile];         // region length
    __shared__ uint32_t s_start[kTile];     // region start inside the frame
    __shared__ uint32_t s_item[kTile + 1];  // exclusive scan of the frames' item counts
    __shared__ uint32_t s_mask[kTile], s_first[kTile];
    __shared__ uint32_t s_w[4];
    const uint32_t t = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * kTile;
    const uint32_t nf = p.a.count - first < kTile ? (uint32_t)(p.a.count - first) : kTile;
    const uint32_t np = p.s.n;

    {  // 1. the prefilter row of byte value t (the pattern loop is uniform: the set stays in scalar registers)
        uint32_t r0 = 0u, r1 = 0u;
        for (uint32_t i = 0; i < np; i++) {
            const MatchPat& P = p.s.pat[i];
            const uint32_t L = P.meta & 0xFFu;
            const bool nocase = ((P.meta >> 8) & NEXG_PAT_NOCASE) != 0u;
            const uint32_t b = nocase ? match_fold(t) : t;
            if (b == P.w[0] >> 24) r0 |= 1u << i;
            if (L == 1u || b == ((P.w[0] >> 16) & 0xFFu)) r1 |= 1u << i;
            const uint32_t k = t & 7u;  // lanes 8 i .. 8 i + 5 copy pattern i's six dwords
            if ((t >> 3) == i && k < 6u)
                s_pat[i][k] = k == 0u ? P.w[0] : k == 1u ? P.w[1] : k == 2u ? P.w[2] : k == 3u ? P.w[3] : k == 4u ? P.meta : P.win;
        }
        s_T0[t] = r0;
        s_T1[t] = r1;
    }

    // 2. the regions
    uint32_t items = 0u;
    if (t < nf) {
        const uint64_t idx = first + t;
        uint64_t off;
        uint32_t len, start, n, fl = 0u, pl = 0u;
        frame_extent(p.a, idx, off, len);  // len 0 for a bad extent or a length above 65535
        if (!(p.s.flags & NEXG_MATCH_FRAME)) {
            const auto* rw = NEXG_GLOBAL(uint32_t, p.recs) + idx * 16u;
            fl = rw[kRecFlags];
            pl = rw[kRecPayload];
        }
        match_region(p.s.flags, len, fl, pl, start, n);
        s_src[t] = reinterpret_cast<uint64_t>(p.a.data) + off + start;
        s_n[t] = n;
        s_start[t] = start;
        items = (n + kStarts - 1u) / kStarts;  // <= 4096
    }
    s_mask[t] = 0u;
    s_first[t] = kMatchNoKey;
    uint32_t total;
    const uint32_t before = block_excl_scan(items, s_w, total);  // its barrier also covers step 1 and the stores above
    s_item[t] = before;
    if (t == 0) s_item[kTile] = total;
    __syncthreads();

    // 3. the items
    for (uint32_t it = t; it < total; it += kTile) {
        uint32_t l = 0, h = nf;  // the last frame f with s_item[f] <= it: the one that owns the item
        while (h - l > 1u) {
            const uint32_t mid = (l + h) >> 1;
            if (s_item[mid] <= it) l = mid;
            else h = mid;
        }
        const uint32_t f = l, n = s_n[f], q0 = (it - s_item[f]) * kStarts;
        if (q0 >= n) continue;  // cannot happen with a consistent stage; bounds the loads all the same
        const uint32_t bytes = n - q0 < 31u ? n - q0 : 31u;
        uint32_t w[8];
        frame_be_words<8>(s_src[f] + q0, true, bytes, w);
        uint32_t hit = 0u, key = kMatchNoKey;
        const uint32_t fo = s_start[f] + q0;
#pragma unroll
        for (uint32_t j = 0; j < kStarts; j++) {
            const uint32_t q = q0 + j;
            if (q >= n) break;
            const uint32_t wi = j >> 2, sh = 8u * (j & 3u);
            uint32_t ww[4];
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) ww[i] = sh ? (w[wi + i] << sh) | (w[wi + i + 1] >> (32u - sh)) : w[wi + i];
            uint32_t cand = s_T0[ww[0] >> 24] & s_T1[(ww[0] >> 16) & 0xFFu];
            if (!cand) continue;
            uint32_t wf[4];
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) wf[i] = match_fold4(ww[i]);
            while (cand) {
                const uint32_t i = (uint32_t)__builtin_ctz(cand);
                cand &= cand - 1u;
                const MatchPat P{{s_pat[i][0], s_pat[i][1], s_pat[i][2], s_pat[i][3]}, s_pat[i][4], s_pat[i][5]};
                if (!match_at(P, ww, wf, q, n)) continue;
                hit |= 1u << i;
                const uint32_t k = match_key(fo + j, i);
                key = k < key ? k : key;
            }
        }
        if (hit) {  // 4.
            atomicOr(&s_mask[f], hit);
            atomicMin(&s_first[f], key);
        }
    }
    __syncthreads();

    // 5. the rows
    if (t < nf) {
        const nexg_match r = match_row(s_mask[t], s_first[t]);
        uint2 v;
        v.x = r.mask;
        v.y = (uint32_t)r.first_off | (uint32_t)r.first_pat << 16 | (uint32_t)r.reserved << 24;
        reinterpret_cast<uint2*>(out)[first + t] = v;
    }
}

hipError_t launch_match(const ParseArgs& a, const nexg_record* recs, const MatchSet& s, nexg_match* out, hipStream_t st) {
    const uint64_t tiles = (a.count + kTile - 1) / kTile;
    if (!tiles) return hipSuccess;
    MatchArgs p{a, recs, s};
    hipLaunchKernelGGL(k_match, dim3((uint32_t)tiles), dim3(kTile), 0, st, p, out);
    return hipGetLastError();
}

// ---- selection by the rows ---------------------------------------------------------

struct MatchSel {
    uint32_t any_mask, all_mask, none_mask;
};

__device__ __forceinline__ bool row_selected(const nexg_match* rows, uint64_t idx, const MatchSel& m) {
    return match_selected(NEXG_GLOBAL(uint32_t, rows)[idx * 2u], m.any_mask, m.all_mask, m.none_mask);
}

__global__ __launch_bounds__(256) void k_match_count(uint64_t count, const nexg_match* rows, MatchSel m,
                                                     uint32_t* tile_count) {
    __shared__ uint32_t s_w[4];
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    const bool sel = idx < count && row_selected(rows, idx, m);
    const uint32_t total = block_count(sel, s_w).total;
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_match_scatter(ParseArgs a, const nexg_match* rows, MatchSel m,
                                                       const uint32_t* tile_base, uint32_t* out_index, uint64_t* out_off,
                                                       uint32_t* out_len) {
    __shared__ uint32_t s_w[4];
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    const bool sel = idx < a.count && row_selected(rows, idx, m);
    const uint32_t rank = block_count(sel, s_w).rank;
    if (!sel) return;
    // rank < the number selected <= count: inside the outputs' capacity (checked
    // all the same: a caller rewriting the rows or the workspace between the
    // passes must not turn into a store out of bounds)
    const uint64_t k = (uint64_t)tile_base[blockIdx.x] + rank;
    if (k >= a.count) return;
    uint64_t off, l64;
    table_extent(a, idx, off, l64);
    out_index[k] = (uint32_t)idx;
    out_off[k] = off;
    out_len[k] = l64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)l64;
}

hipError_t launch_match_select(const ParseArgs& a, const nexg_match* rows, uint32_t any_mask, uint32_t all_mask,
                               uint32_t none_mask, uint32_t* out_index, uint64_t* out_off, uint32_t* out_len,
                               uint64_t* out_count, void* workspace, hipStream_t s) {
    const TileCountLayout w = TileCountLayout::from(a.count);
    const uint64_t tiles = w.tiles;
    uint32_t* tile_count = region<uint32_t>(workspace, w.tile_count);
    const MatchSel m{any_mask, all_mask, none_mask};
    if (tiles) hipLaunchKernelGGL(k_match_count, dim3((uint32_t)tiles), dim3(kTile), 0, s, a.count, rows, m, tile_count);
    hipLaunchKernelGGL(k_tile_scan<uint32_t>, dim3(1), dim3(kTile), 0, s, tile_count, tiles, out_count);
    if (tiles)
        hipLaunchKernelGGL(k_match_scatter, dim3((uint32_t)tiles), dim3(kTile), 0, s, a, rows, m, tile_count, out_index,
                           out_off, out_len);
    return hipGetLastError();
}

}  // namespace nexg
