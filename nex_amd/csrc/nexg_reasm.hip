// nexg_reasm.hip — nexg_reasm_plan / nexg_reasm_frames / nexg_reasm_held: the
// IPv4 fragments of a frame table put back together (include/nexg.h; the
// per-frame rules are reasm_core.hpp). The first many-to-one pass: a group of
// input frames, found by sorting, becomes one output frame.
//
// Plan. k_reasm_classify, one lane per frame, keeps the frame's class and key
// (ReasmInfo) and its two sort keys. Two chains of the flow sort's radix passes
// (launch_radix_sort, nexg_flow.hip) order the frames by (hash,
// identification, fo, frame number), frames that are no fragments last.
// k_reasm_mark gives every sorted position its head / break / bad flags
// (reasm_mark) and scans them inside its 256-position tile; k_tile_scan scans
// the tiles' totals; k_reasm_place notes where each run starts; k_reasm_rows,
// one lane per position, takes the differences of the prefixes at its run's
// start and at the next run's (k_group_rows' scheme: the sizes of the runs do
// not enter), reads the run's two ends and writes its frame's row and output
// length. Then the fragment plan's two scans in frame order (block_sum,
// k_tile_scan<uint64_t>, block_excl_scan) give out_first and out_bytes, and
// k_reasm_part_out hands a PART its head's output frame.
//
// Fill: the fragment fill's geometry. A quarter wave owns an input frame, 16
// frames per workgroup; reasm_core.hpp's three phases. No atomics, no
// workspace, no scratch; the output is never read.
#include "reasm_core.hpp"
#include "table_kernels.hpp"
#include "workspace_layout.hpp"

namespace nexg {

static_assert(sizeof(nexg_reasm) == 16, "nexg_reasm is 16 bytes (include/nexg.h)");
static_assert(offsetof(nexg_reasm, members) == 4 && offsetof(nexg_reasm, data_len) == 6 && offsetof(nexg_reasm, out) == 8 &&
                  offsetof(nexg_reasm, head) == 12,
              "the row by dword: status | kind << 8 | hdr_len << 16 | flags << 24, members | data_len << 16, out, head");

// ---- plan ------------------------------------------------------------------------------

__device__ __forceinline__ ReasmInfo load_info(const ReasmInfo* info, uint64_t i) {
    const uint4 a = load16<true>(reinterpret_cast<const uint8_t*>(info + i));
    const uint4 b = load16<true>(reinterpret_cast<const uint8_t*>(info + i) + 16u);
    return {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}

__global__ __launch_bounds__(256) void k_reasm_classify(ParseArgs a, ReasmInfo* info, uint64_t* key_idfo, uint64_t* key_hash) {
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    if (idx >= a.count) return;
    uint64_t off;
    uint32_t len;
    const bool ext = frame_extent(a, idx, off, len);
    const ReasmClass c = reasm_classify(ext, len, reinterpret_cast<uint64_t>(a.data) + (ext ? off : 0u));
    const ReasmInfo x = reasm_info(c, ext ? len : 0u);
    uint4* o = reinterpret_cast<uint4*>(info + idx);
    o[0] = make_uint4(x.hash, x.idfo, x.shape, x.d);
    o[1] = make_uint4(x.src, x.dst, x.proto, x.len);
    key_idfo[idx] = x.idfo;
    key_hash[idx] = x.hash;
}

// what k_reasm_mark leaves per position: the exclusive in-tile prefixes of the
// heads, the breaks and the bad flags (at most 255 each), and the head flag
constexpr uint32_t kRmBrk = 10, kRmBad = 20, kRmHead = 30;

__device__ __forceinline__ uint64_t rm_bb(uint32_t packed) {  // breaks | bad << 32
    return (uint64_t)((packed >> kRmBrk) & 0x3FFu) | (uint64_t)((packed >> kRmBad) & 0x3FFu) << 32;
}

__global__ __launch_bounds__(256) void k_reasm_mark(uint64_t count, const ReasmInfo* info, const uint32_t* order, uint64_t* mark,
                                                    uint32_t* tile_heads, uint64_t* tile_bb) {
    __shared__ uint32_t s_w[4];
    const uint64_t k = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    const bool in = k < count, prev = in && k > 0;
    const uint32_t i = in ? order[k] : 0xFFFFFFFFu, j = prev ? order[k - 1] : 0xFFFFFFFFu;
    // an entry past the table (the sort's own output never is) stands for a frame that is no fragment
    const ReasmInfo none{0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u, 0u};
    const ReasmInfo xi = in && i < count ? load_info(info, i) : none;
    const ReasmInfo xj = prev && j < count ? load_info(info, j) : none;
    const ReasmMark m = reasm_mark(xi, prev, xj);
    const uint32_t v = in ? (uint32_t)m.head | (uint32_t)m.brk << kRmBrk | (uint32_t)m.bad << kRmBad : 0u;
    uint32_t total;
    const uint32_t before = block_excl_scan(v, s_w, total);
    if (in) mark[k] = (uint64_t)(before | (uint32_t)m.head << kRmHead) | (uint64_t)i << 32;
    if (threadIdx.x == 0) {
        tile_heads[blockIdx.x] = total & 0x3FFu;
        tile_bb[blockIdx.x] = rm_bb(total);
    }
}

__global__ __launch_bounds__(256) void k_reasm_place(uint64_t count, const uint64_t* mark, const uint32_t* tile_heads,
                                                     uint32_t* starts) {
    const uint64_t k = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    if (k >= count) return;
    const uint32_t m = (uint32_t)mark[k];
    if (!((m >> kRmHead) & 1u)) return;
    const uint32_t g = tile_heads[blockIdx.x] + (m & 0x3FFu);
    if (g < count) starts[g] = (uint32_t)k;  // g <= k by construction
}

// the breaks and bad flags before position p (p < count), breaks | bad << 32
__device__ __forceinline__ uint64_t rm_before(const uint64_t* mark, const uint64_t* tile_bb, uint64_t p) {
    return tile_bb[p >> 8] + rm_bb((uint32_t)mark[p]);
}

// One lane per sorted position: its frame's row, without `out`, and its output
// length. Positions out of the workspace are clamped before they index
// anything, as in k_group_rows.
__global__ __launch_bounds__(256) void k_reasm_rows(uint64_t count, const ReasmInfo* info, const uint32_t* order,
                                                    const uint64_t* mark, const uint32_t* tile_heads, const uint64_t* tile_bb,
                                                    const uint64_t* totals, const uint32_t* starts, nexg_reasm* rows,
                                                    uint32_t* out_len) {
    const uint64_t k = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    if (k >= count) return;
    const uint32_t i = order[k];
    if (i >= count) return;
    const ReasmInfo x = load_info(info, i);
    uint4 row;
    uint32_t olen = 0;
    if (!info_frag(x)) {
        const uint32_t status = (x.shape >> 16) & 0xFFu, kind = x.shape >> 24;
        row = make_uint4(status | kind << 8, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu);
        olen = x.len;
    } else {
        const uint32_t m = (uint32_t)mark[k];
        uint64_t G = totals[0];
        if (G > count) G = count;
        uint64_t g = (uint64_t)tile_heads[blockIdx.x] + (m & 0x3FFu) + ((m >> kRmHead) & 1u);
        g = g ? g - 1u : 0u;
        if (g >= G) g = G ? G - 1u : 0u;
        uint64_t first = starts[g], next = g + 1u < G ? starts[g + 1u] : count;
        if (first > k) first = k;
        if (next <= k || next > count) next = k + 1u;
        const uint64_t b0 = rm_before(mark, tile_bb, first), b1 = next < count ? rm_before(mark, tile_bb, next) : totals[1];
        // the flag of `first` itself is the run's own: a head's bad flag (fo != 0); its break flag is never set
        const uint32_t brk = (uint32_t)b1 - (uint32_t)b0, bad = (uint32_t)(b1 >> 32) - (uint32_t)(b0 >> 32);
        const uint32_t ih = order[first], il = order[next - 1u];
        const ReasmInfo none{0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u, 0u};
        const ReasmInfo xh = ih < count ? load_info(info, ih) : none, xl = il < count ? load_info(info, il) : none;
        uint32_t D;
        const bool complete = reasm_complete(brk, bad, xh, xl, D) && info_frag(xh) && info_frag(xl);
        const bool head = complete && k == first;
        const uint32_t kind = complete ? (head ? NEXG_REASM_HEAD : NEXG_REASM_PART) : NEXG_REASM_HELD;
        const uint32_t members = (uint32_t)(next - first);
        row = make_uint4(NEXG_FRAME_OK | kind << 8 | info_hl(x) << 16 | (brk ? NEXG_REASM_COLLISION << 24 : 0u),
                         head ? (members & 0xFFFFu) | D << 16 : 0u, 0xFFFFFFFFu, complete ? ih : 0xFFFFFFFFu);
        olen = head ? 14u + info_hl(x) + D : 0u;
    }
    reinterpret_cast<uint4*>(rows)[i] = row;
    out_len[i] = olen;
}

// frame idx's output frames (0 or 1) and padded output bytes, from its row's kind and its output length
__device__ __forceinline__ uint32_t reasm_planned(uint64_t count, const nexg_reasm* rows, const uint32_t* out_len, uint32_t align,
                                                  uint64_t idx, uint32_t& bytes) {
    bytes = 0;
    if (idx >= count) return 0u;
    const uint32_t kind = (NEXG_GLOBAL(uint32_t, rows)[idx * 4u] >> 8) & 0xFFu;
    if (kind != NEXG_REASM_PASS && kind != NEXG_REASM_HEAD) return 0u;
    bytes = frag_pad(out_len[idx], align);
    return 1u;
}

__global__ __launch_bounds__(256) void k_reasm_plan_sum(uint64_t count, const nexg_reasm* rows, const uint32_t* out_len,
                                                        uint32_t align, uint64_t* tile_frames, uint64_t* tile_bytes) {
    __shared__ uint32_t s_f[4], s_b[4];
    uint32_t bytes;
    const uint32_t n = reasm_planned(count, rows, out_len, align, (uint64_t)blockIdx.x * kTile + threadIdx.x, bytes);
    const uint64_t frames = block_sum(n, s_f);
    const uint64_t total = block_sum(bytes, s_b);  // < 2^25
    if (threadIdx.x == 0) {
        tile_frames[blockIdx.x] = frames;
        tile_bytes[blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(256) void k_reasm_plan_write(uint64_t count, nexg_reasm* rows, const uint32_t* out_len,
                                                          uint32_t align, const uint64_t* tile_frames,
                                                          const uint64_t* tile_bytes, const uint64_t* frames_total,
                                                          uint32_t* out_first, uint64_t* out_bytes) {
    __shared__ uint32_t s_f[4], s_b[4];
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    uint32_t bytes, total;
    const uint32_t n = reasm_planned(count, rows, out_len, align, idx, bytes);
    const uint32_t f_before = block_excl_scan(n, s_f, total);
    const uint32_t b_before = block_excl_scan(bytes, s_b, total);
    if (idx >= count) return;
    const uint32_t first = (uint32_t)tile_frames[blockIdx.x] + f_before;
    out_first[idx] = first;
    out_bytes[idx] = tile_bytes[blockIdx.x] + b_before;
    if (n) rows[idx].out = first;
    if (idx == count - 1u) out_first[count] = (uint32_t)*frames_total;  // at most count
}

__global__ __launch_bounds__(256) void k_reasm_part_out(uint64_t count, nexg_reasm* rows, const uint32_t* out_first) {
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    if (idx >= count) return;
    const uint32_t kind = (NEXG_GLOBAL(uint32_t, rows)[idx * 4u] >> 8) & 0xFFu;
    if (kind != NEXG_REASM_PART) return;
    const uint32_t h = NEXG_GLOBAL(uint32_t, rows)[idx * 4u + 3u];
    if (h < count) rows[idx].out = out_first[h];
}

hipError_t launch_reasm_plan(const ParseArgs& a, uint32_t align, uint32_t* out_first, uint64_t* out_bytes, nexg_reasm* rows,
                             void* workspace, hipStream_t st) {
    const uint64_t count = a.count;
    if (!count) {  // no workspace then
        hipError_t e = hipMemsetAsync(out_first, 0, 4, st);
        if (e == hipSuccess) e = hipMemsetAsync(out_bytes, 0, 8, st);
        return e;
    }
    const ReasmPlanLayout w = ReasmPlanLayout::from(count);
    ReasmInfo* info = region<ReasmInfo>(workspace, w.info);
    uint64_t* key_idfo = region<uint64_t>(workspace, w.key_idfo);
    uint64_t* key_hash = region<uint64_t>(workspace, w.key_hash);
    uint64_t* mark = region<uint64_t>(workspace, w.mark);
    uint64_t* tile_bb = region<uint64_t>(workspace, w.tile_bb);
    uint64_t* tile_frames = region<uint64_t>(workspace, w.tile_frames);
    uint64_t* tile_bytes = region<uint64_t>(workspace, w.tile_bytes);
    uint64_t* totals = region<uint64_t>(workspace, w.totals);
    uint32_t* order = region<uint32_t>(workspace, w.order);
    uint32_t* olen = region<uint32_t>(workspace, w.out_len);
    uint32_t* starts = region<uint32_t>(workspace, w.starts);
    uint32_t* tile_heads = region<uint32_t>(workspace, w.tile_heads);
    void* sort_ws = region<char>(workspace, w.sort);
    const dim3 gT((uint32_t)w.tiles), b(kTile), one(1);
    hipLaunchKernelGGL(k_reasm_classify, gT, b, 0, st, a, info, key_idfo, key_hash);
    hipError_t e = launch_radix_sort(key_idfo, nullptr, count, order, sort_ws, st);
    if (e != hipSuccess) return e;
    e = launch_radix_sort(key_hash, order, count, order, sort_ws, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_reasm_mark, gT, b, 0, st, count, info, order, mark, tile_heads, tile_bb);
    hipLaunchKernelGGL(k_tile_scan<uint32_t>, one, b, 0, st, tile_heads, w.tiles, totals);
    hipLaunchKernelGGL(k_tile_scan<uint64_t>, one, b, 0, st, tile_bb, w.tiles, totals + 1);
    hipLaunchKernelGGL(k_reasm_place, gT, b, 0, st, count, mark, tile_heads, starts);
    hipLaunchKernelGGL(k_reasm_rows, gT, b, 0, st, count, info, order, mark, tile_heads, tile_bb, totals, starts, rows, olen);
    hipLaunchKernelGGL(k_reasm_plan_sum, gT, b, 0, st, count, rows, olen, align, tile_frames, tile_bytes);
    hipLaunchKernelGGL(k_tile_scan<uint64_t>, one, b, 0, st, tile_frames, w.tiles, totals + 2);
    hipLaunchKernelGGL(k_tile_scan<uint64_t>, one, b, 0, st, tile_bytes, w.tiles, out_bytes + count);
    hipLaunchKernelGGL(k_reasm_plan_write, gT, b, 0, st, count, rows, olen, align, tile_frames, tile_bytes, totals + 2,
                       out_first, out_bytes);
    hipLaunchKernelGGL(k_reasm_part_out, gT, b, 0, st, count, rows, out_first);
    return hipGetLastError();
}

// ---- fill ------------------------------------------------------------------------------

constexpr uint32_t kReasmGroups = kTile / kReasmLanes;  // input frames per workgroup

// The body is reasm_core.hpp's three phases, which the host driver runs too;
// the bounds they keep against rows, out_first, out_bytes and out_cap are
// stated there.
__global__ __launch_bounds__(256) void k_reasm_frames(ParseArgs a, const nexg_reasm* rows, const uint32_t* out_first,
                                                      const uint64_t* out_bytes, FragOut out) {
    __shared__ FragHdr s_hdr[kReasmGroups];
    const uint32_t lane = threadIdx.x & (kReasmLanes - 1u), g = threadIdx.x / kReasmLanes;
    const uint64_t idx = (uint64_t)blockIdx.x * kReasmGroups + g;
    ReasmJob j{};
    j.live = idx < a.count;  // a group past the table runs on with nothing to write
    j.index = (uint32_t)idx;
    ReasmClass c{};
    if (j.live) {
        const auto* of = NEXG_GLOBAL(uint32_t, out_first);
        const auto* ob = NEXG_GLOBAL(uint64_t, out_bytes);
        const uint4 row = load16<true>(reinterpret_cast<const uint8_t*>(rows + idx));
        j.kind = (row.x >> 8) & 0xFFu;
        j.data_len = row.y >> 16;
        j.head_hl = (row.x >> 16) & 0xFFu;
        j.first = of[idx];
        j.first_end = of[idx + 1];
        uint64_t h = idx;
        j.named = true;
        if (j.kind == NEXG_REASM_PART) {
            h = row.w;
            j.named = h < a.count;
            if (j.named) j.head_hl = (NEXG_GLOBAL(uint32_t, rows)[h * 4u] >> 16) & 0xFFu;
        }
        if (j.named) {
            j.lo = ob[h];
            j.next = ob[h + 1];
        }
        uint64_t off;
        j.ext = frame_extent(a, idx, off, j.len);
        j.src = reinterpret_cast<uint64_t>(a.data) + (j.ext ? off : 0u);  // a rejected extent's offset is any number
        c = reasm_classify(j.ext, j.len, j.src);
    }
    reasm_stage(j, c, s_hdr[g], lane);
    __syncthreads();
    if (lane == 0u) reasm_sum(j, c, s_hdr[g]);
    __syncthreads();
    reasm_fill(j, c, s_hdr[g], out, lane);
    if (j.live && lane == 0u && idx == a.count - 1u) out.offsets[out.count] = NEXG_GLOBAL(uint64_t, out_bytes)[a.count];
}

hipError_t launch_reasm_frames(const ParseArgs& a, uint32_t align, const nexg_reasm* rows, const uint32_t* out_first,
                               const uint64_t* out_bytes, uint64_t out_count, uint64_t* out_offsets, uint32_t* out_len,
                               uint32_t* out_src, uint8_t* out_data, uint64_t out_cap, hipStream_t st) {
    (void)align;  // the plan put it into out_bytes
    if (a.count == 0) return hipMemcpyAsync(out_offsets + out_count, out_bytes, 8, hipMemcpyDeviceToDevice, st);
    const FragOut out{out_offsets, out_len, out_src, out_data, out_cap, out_count};
    const uint64_t blocks = (a.count + kReasmGroups - 1) / kReasmGroups;
    hipLaunchKernelGGL(k_reasm_frames, dim3((uint32_t)blocks), dim3(kTile), 0, st, a, rows, out_first, out_bytes, out);
    return hipGetLastError();
}

// ---- held --------------------------------------------------------------------------------

// nexg_reasm_held: table_kernels.hpp's compaction with the row's kind as the selector
struct HeldPick {
    ParseArgs a;
    const nexg_reasm* rows;
    struct Picked {};
    static constexpr bool kTagged = false;
    NEXG_HD uint64_t count() const { return a.count; }
    __device__ __forceinline__ bool pick(uint64_t idx, Picked&) const {
        return ((NEXG_GLOBAL(uint32_t, rows)[idx * 4u] >> 8) & 0xFFu) == NEXG_REASM_HELD;
    }
    __device__ __forceinline__ void entry(uint64_t idx, const Picked&, uint64_t& off, uint32_t& len) const {
        uint64_t l64;
        table_extent(a, idx, off, l64);
        len = l64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)l64;
    }
};

hipError_t launch_reasm_held(const ParseArgs& a, const nexg_reasm* rows, uint32_t* out_index, uint64_t* out_off,
                             uint32_t* out_len, uint64_t* out_count, void* workspace, hipStream_t s) {
    return launch_compact(HeldPick{a, rows}, out_index, out_off, out_len, nullptr, out_count, workspace, s);
}

}  // namespace nexg
