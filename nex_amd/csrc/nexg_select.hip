// nexg_select.hip — frame selection by rule and gather on gfx950
// (include/nexg.h; an extension: the reference has no filter). A pass over a
// batch already parsed with NEXG_OUT_RECORD that tests each frame's record
// against up to 16 rules and compacts the matching frames' table entries in
// order (table_kernels.hpp's compaction; the rule is select_rule), then the
// gather that copies the selected frames into one dense buffer and compacts
// per-frame rows by the selected index.
#include "table_kernels.hpp"

namespace nexg {

static_assert(sizeof(nexg_rule) == 64, "nexg_rule is 64 bytes (include/nexg.h)");
static_assert(sizeof(nexg_filter) == 8 + 16 * 64, "nexg_filter is 1032 bytes (include/nexg.h)");
static_assert(sizeof(SelRule) == 96, "SelRule is 96 bytes");

// SelFilter.need: what some rule of the filter reads
constexpr uint32_t kSelNeedProto = 1u, kSelNeedSrc4 = 2u, kSelNeedDst4 = 4u, kSelNeedPorts = 8u, kSelNeedTcp = 16u,
                   kSelNeedV6 = 32u;

// ---- host: validation and the kernel's form of the filter ----------------------

static void prefix_words(const uint8_t* addr, uint32_t bits, uint32_t width, uint32_t* w, uint32_t* m) {
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t lo = 32u * k;  // first prefix bit of this word
        const uint32_t nb = 32u * k >= width || bits <= lo ? 0u : (bits - lo >= 32u ? 32u : bits - lo);
        m[k] = nb == 0u ? 0u : nb == 32u ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> nb);
        const uint32_t v = (uint32_t)addr[4 * k] << 24 | (uint32_t)addr[4 * k + 1] << 16 |
                           (uint32_t)addr[4 * k + 2] << 8 | (uint32_t)addr[4 * k + 3];
        w[k] = v & m[k];
    }
}

const char* prepare_filter(const nexg_filter* f, SelFilter* out) {
    if (!f) return "NULL filter";
    if (f->n_rules == 0 || f->n_rules > NEXG_FILTER_MAX_RULES) return "filter: n_rules must be 1..16";
    if (f->flags & ~NEXG_FILTER_INVERT) return "filter: unknown flag bits";
    SelFilter o{};
    o.n_rules = f->n_rules;
    o.invert = f->flags & NEXG_FILTER_INVERT;
    for (uint32_t i = 0; i < f->n_rules; i++) {
        const nexg_rule& r = f->rules[i];
        const uint32_t t = r.tests;
        if (t & ~NEXG_RULE_ALL) return "rule: unknown test bits";
        if (r.reserved != 0) return "rule: reserved must be 0";
        if ((t & NEXG_RULE_ANY_PORT) && (t & (NEXG_RULE_SRC_PORT | NEXG_RULE_DST_PORT)))
            return "rule: ANY_PORT excludes SRC_PORT and DST_PORT";
        if ((t & NEXG_RULE_ANY_PORT) && (r.dport_lo || r.dport_hi)) return "rule: ANY_PORT needs dport_lo = dport_hi = 0";
        if ((t & (NEXG_RULE_SRC_PORT | NEXG_RULE_ANY_PORT)) && r.sport_lo > r.sport_hi) return "rule: sport_lo > sport_hi";
        if ((t & NEXG_RULE_DST_PORT) && r.dport_lo > r.dport_hi) return "rule: dport_lo > dport_hi";
        if ((t & NEXG_RULE_LENGTH) && r.len_lo > r.len_hi) return "rule: len_lo > len_hi";
        const uint32_t addr = t & (NEXG_RULE_SRC_ADDR | NEXG_RULE_DST_ADDR | NEXG_RULE_ANY_ADDR);
        if ((t & NEXG_RULE_ANY_ADDR) && (t & (NEXG_RULE_SRC_ADDR | NEXG_RULE_DST_ADDR)))
            return "rule: ANY_ADDR excludes SRC_ADDR and DST_ADDR";
        if ((t & NEXG_RULE_ANY_ADDR) && r.dst_bits) return "rule: ANY_ADDR needs dst_bits = 0";
        const uint32_t width = r.family == 4 ? 32u : 128u;
        if (addr) {
            if (r.family != 4 && r.family != 6) return "rule: address test with a family other than 4 or 6";
            if ((t & (NEXG_RULE_SRC_ADDR | NEXG_RULE_ANY_ADDR)) && r.src_bits > width) return "rule: src_bits above the family's width";
            if ((t & NEXG_RULE_DST_ADDR) && r.dst_bits > width) return "rule: dst_bits above the family's width";
        }
        SelRule& d = o.rule[i];
        d.flags_mask = r.flags_mask;
        d.flags_value = r.flags_value;
        d.tests = t;
        d.misc = (uint32_t)r.ip_proto | (uint32_t)r.tcp_mask << 8 | (uint32_t)r.tcp_value << 16 |
                 (uint32_t)(addr ? r.family : 0) << 24;
        d.sport = (uint32_t)r.sport_lo | (uint32_t)r.sport_hi << 16;
        d.dport = (uint32_t)r.dport_lo | (uint32_t)r.dport_hi << 16;
        d.length = (uint32_t)r.len_lo | (uint32_t)r.len_hi << 16;
        if (t & (NEXG_RULE_SRC_ADDR | NEXG_RULE_ANY_ADDR)) prefix_words(r.src, r.src_bits, width, d.src, d.src_mask);
        if (t & NEXG_RULE_DST_ADDR) prefix_words(r.dst, r.dst_bits, width, d.dst, d.dst_mask);
        if (t & NEXG_RULE_PROTO) o.need |= kSelNeedProto;
        if (t & (NEXG_RULE_SRC_PORT | NEXG_RULE_DST_PORT | NEXG_RULE_ANY_PORT)) o.need |= kSelNeedPorts;
        if (t & NEXG_RULE_TCP_FLAGS) o.need |= kSelNeedTcp;
        if (addr && r.family == 6) o.need |= kSelNeedV6;
        if (addr && r.family == 4) {
            if (t & (NEXG_RULE_SRC_ADDR | NEXG_RULE_ANY_ADDR)) o.need |= kSelNeedSrc4;
            if (t & (NEXG_RULE_DST_ADDR | NEXG_RULE_ANY_ADDR)) o.need |= kSelNeedDst4;
        }
    }
    if (out) *out = o;
    return nullptr;
}

// ---- select ----------------------------------------------------------------------

__device__ __forceinline__ bool in_range(uint32_t v, uint32_t lohi) { return v >= (lohi & 0xFFFFu) && v <= (lohi >> 16); }

__device__ __forceinline__ bool prefix4(const uint32_t* a, const uint32_t* w, const uint32_t* m) {
    return (((a[0] & m[0]) ^ w[0]) | ((a[1] & m[1]) ^ w[1]) | ((a[2] & m[2]) ^ w[2]) | ((a[3] & m[3]) ^ w[3])) == 0u;
}

// One lane's verdict: the lowest matching rule, or NEXG_RULE_NONE. The filter is
// a kernel argument and the rule loop is wave-uniform, so the rules stay in
// scalar registers. Only the record dwords some rule tests are loaded (f.need),
// and frame bytes (the two IPv6 addresses, by frame_be_words) only under a
// family-6 rule, only by lanes whose header is whole inside their own frame.
__device__ __forceinline__ uint32_t select_rule(const ParseArgs& a, const nexg_record* recs, const SelFilter& f,
                                                uint64_t idx, uint64_t& off, uint32_t& len32) {
    uint64_t l64;
    const bool ext = table_extent(a, idx, off, l64);
    len32 = l64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)l64;
    const auto* rw = NEXG_GLOBAL(uint32_t, recs) + idx * 16u;
    const uint32_t flags = rw[kRecFlags];
    const bool ok = rec_status(flags) == 0u;
    uint32_t proto = 0, src4 = 0, dst4 = 0, ports = 0, tcpf = 0;
    if (f.need & kSelNeedProto) proto = rec_proto(rw[kRecProto]);
    if (f.need & kSelNeedSrc4) src4 = rw[kRecSrc];
    if (f.need & kSelNeedDst4) dst4 = rw[kRecDst];
    if (f.need & kSelNeedPorts) ports = rw[kRecPorts];
    if (f.need & kSelNeedTcp) tcpf = rec_l4_type(rw[kRecL4Type]);
    const bool l4 = ok && (flags & (NEXG_L_TCP | NEXG_L_UDP)) != 0u;
    const bool v4 = ok && (flags & NEXG_L_IPV4) != 0u;
    bool v6 = false;
    uint32_t a6[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the IPv6 source, then the destination
    if (f.need & kSelNeedV6) {
        const uint32_t l3 = rec_l3(rw[kRecL3]);
        v6 = ok && ext && (flags & NEXG_L_IPV6) != 0u && (uint64_t)l3 + 40u <= l64;
        frame_be_words(reinterpret_cast<uint64_t>(a.data) + off + l3 + 8u, v6, 32u, a6);
    }
    const uint32_t *s6 = a6, *d6 = a6 + 4;
    const uint32_t s4[4] = {src4, 0, 0, 0}, d4[4] = {dst4, 0, 0, 0};
    uint32_t hit = NEXG_RULE_NONE;
    for (uint32_t r = 0; r < f.n_rules; r++) {
        const SelRule& R = f.rule[r];
        const uint32_t t = R.tests, fam = R.misc >> 24;
        bool m = (flags & R.flags_mask) == R.flags_value;
        if (t & NEXG_RULE_PROTO) m = m && ok && (flags & (NEXG_L_IPV4 | NEXG_L_IPV6)) != 0u && proto == (R.misc & 0xFFu);
        if (t & NEXG_RULE_SRC_PORT) m = m && l4 && in_range(rec_sport(ports), R.sport);
        if (t & NEXG_RULE_DST_PORT) m = m && l4 && in_range(rec_dport(ports), R.dport);
        if (t & NEXG_RULE_ANY_PORT) m = m && l4 && (in_range(rec_sport(ports), R.sport) || in_range(rec_dport(ports), R.sport));
        if (t & (NEXG_RULE_SRC_ADDR | NEXG_RULE_DST_ADDR | NEXG_RULE_ANY_ADDR)) {
            const bool six = fam == 6u;
            m = m && (six ? v6 : v4);
            const uint32_t* S = six ? s6 : s4;
            const uint32_t* D = six ? d6 : d4;
            if (t & NEXG_RULE_SRC_ADDR) m = m && prefix4(S, R.src, R.src_mask);
            if (t & NEXG_RULE_DST_ADDR) m = m && prefix4(D, R.dst, R.dst_mask);
            if (t & NEXG_RULE_ANY_ADDR) m = m && (prefix4(S, R.src, R.src_mask) || prefix4(D, R.src, R.src_mask));
        }
        if (t & NEXG_RULE_TCP_FLAGS)
            m = m && ok && (flags & NEXG_L_TCP) != 0u && (tcpf & ((R.misc >> 8) & 0xFFu)) == ((R.misc >> 16) & 0xFFu);
        if (t & NEXG_RULE_LENGTH) m = m && len32 <= 0xFFFFu && in_range(len32, R.length);
        if (m && hit == NEXG_RULE_NONE) hit = r;
    }
    return hit;
}

// nexg_select_batch: table_kernels.hpp's compaction with this selector. Off, len
// and the verdict all come from the one select_rule call of pick().
struct SelectPick {
    ParseArgs a;
    const nexg_record* recs;
    SelFilter f;
    struct Picked {
        uint64_t off = 0;
        uint32_t len = 0, hit = NEXG_RULE_NONE;
    };
    static constexpr bool kTagged = true;  // out_rule
    NEXG_HD uint64_t count() const { return a.count; }
    __device__ __forceinline__ bool pick(uint64_t idx, Picked& p) const {
        p.hit = select_rule(a, recs, f, idx, p.off, p.len);
        return (p.hit != NEXG_RULE_NONE) != (f.invert != 0u);
    }
    __device__ __forceinline__ void entry(uint64_t, const Picked& p, uint64_t& off, uint32_t& len) const {
        off = p.off, len = p.len;
    }
    __device__ __forceinline__ uint8_t tag(const Picked& p) const { return (uint8_t)(f.invert ? NEXG_RULE_NONE : p.hit); }
};

hipError_t launch_select(const ParseArgs& a, const nexg_record* recs, const SelFilter& f, uint32_t* out_index,
                         uint64_t* out_off, uint32_t* out_len, uint8_t* out_rule, uint64_t* out_count, void* workspace,
                         hipStream_t s) {
    return launch_compact(SelectPick{a, recs, f}, out_index, out_off, out_len, out_rule, out_count, workspace, s);
}

// ---- gather plan -------------------------------------------------------------------

// copied(k) rounded up to the alignment (a power of two); 0 past the table
__device__ __forceinline__ uint32_t plan_padded(const ParseArgs& a, uint64_t idx, uint32_t align, uint32_t& copied) {
    copied = 0;
    if (idx >= a.count) return 0u;
    uint64_t off;
    frame_extent(a, idx, off, copied);  // length 0 for a bad extent or a length above 65535
    return (copied + align - 1u) & ~(align - 1u);
}

__global__ __launch_bounds__(256) void k_plan_sum(ParseArgs a, uint32_t align, uint64_t* tile_sum) {
    __shared__ uint32_t s_w[4];
    uint32_t copied;
    const uint64_t sum = block_sum(plan_padded(a, (uint64_t)blockIdx.x * kTile + threadIdx.x, align, copied), s_w);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = sum;  // < 2^24 + pads
}

__global__ __launch_bounds__(256) void k_plan_write(ParseArgs a, uint32_t align, const uint64_t* tile_base,
                                                    uint64_t* out_offsets, uint32_t* out_len) {
    __shared__ uint32_t s_w[4];
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    uint32_t copied, total;
    const uint32_t before = block_excl_scan(plan_padded(a, idx, align, copied), s_w, total);
    if (idx >= a.count) return;
    out_offsets[idx] = tile_base[blockIdx.x] + before;
    if (out_len) out_len[idx] = copied;
}

hipError_t launch_gather_plan(const ParseArgs& a, uint32_t align, uint64_t* out_offsets, uint32_t* out_len,
                              void* workspace, hipStream_t s) {
    const TileSumLayout w = TileSumLayout::from(a.count);
    const uint64_t tiles = w.tiles;
    uint64_t* tile_sum = region<uint64_t>(workspace, w.tile_sum);
    if (tiles) hipLaunchKernelGGL(k_plan_sum, dim3((uint32_t)tiles), dim3(kTile), 0, s, a, align, tile_sum);
    hipLaunchKernelGGL(k_tile_scan<uint64_t>, dim3(1), dim3(kTile), 0, s, tile_sum, tiles, out_offsets + a.count);
    if (tiles)
        hipLaunchKernelGGL(k_plan_write, dim3((uint32_t)tiles), dim3(kTile), 0, s, a, align, tile_sum, out_offsets,
                           out_len);
    return hipGetLastError();
}

// ---- gather copy ---------------------------------------------------------------------

// k_gather_frames: one workgroup per 256-frame tile of the selected table. The
// tile owns the output bytes [B, E) = [out_offsets[first], out_offsets[first +
// nf]), E clamped to out_cap. Its frames' output offsets relative to B, source
// offsets and copied lengths are staged in LDS; lanes then own the aligned
// 16-B output chunks that overlap [B, E), 256 at a time. A lane finds the
// frame that holds its chunk's first byte by a binary search of the relative
// offsets.
//   fast path: the chunk lies whole inside the tile's range and inside one
//     frame's slot [off(f), off(f + 1)): up to 16 source bytes come as the
//     covering aligned dwords (every dword loaded holds a wanted byte, so the
//     loads stay inside the frame's own 16-B blocks), are byte-aligned in
//     registers, the pad tail is zeroed, and the chunk leaves as one aligned
//     non-temporal 16-B store.
//   slow path: a chunk that straddles frames (frames shorter than 16 B,
//     zero-length frames, unaligned frame boundaries) or the tile's edges is
//     assembled byte by byte; whole chunks still leave as one 16-B store, the
//     partial chunks at the tile's two edges (shared with the neighbour tiles,
//     or cut by out_cap) as byte stores of the tile's own bytes only.
// out_offsets is caller memory: whatever it holds, every store lies in
// [B, min(E, out_cap)), every source byte read lies inside a frame whose extent
// frame_extent accepted, and the chunk loop is bounded by out_cap.
__global__ __launch_bounds__(256) void k_gather_frames(ParseArgs a, const uint64_t* out_offsets, uint8_t* out_data,
                                                       uint64_t out_cap) {
    __shared__ uint32_t s_rel[kTile + 1];  // output offset of frame f relative to B; [nf] = E - B
    __shared__ uint32_t s_len[kTile];      // copied(f)
    __shared__ uint64_t s_src[kTile];      // off(f) in a.data
    const uint64_t first = (uint64_t)blockIdx.x * kTile;
    const uint32_t nf = a.count - first < kTile ? (uint32_t)(a.count - first) : kTile;
    const uint32_t t = threadIdx.x;
    const auto* oo = NEXG_GLOBAL(uint64_t, out_offsets);
    const uint64_t B = oo[first], E0 = oo[first + nf];
    const uint64_t E = E0 < out_cap ? E0 : out_cap;
    if (E <= B) return;  // uniform: nothing of this tile below out_cap
    if (t < nf) {
        uint64_t off;
        uint32_t len;
        frame_extent(a, first + t, off, len);
        const uint64_t o = oo[first + t];
        s_rel[t] = o < B ? 0u : o - B > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)(o - B);
        s_len[t] = len;
        s_src[t] = off;
    }
    if (t == 0) s_rel[nf] = E0 - B > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)(E0 - B);
    __syncthreads();
    const uint64_t base = reinterpret_cast<uint64_t>(a.data);
    const uint64_t c0 = B >> 4, c1 = (E + 15u) >> 4;  // chunks [c0, c1)
    for (uint64_t c = c0 + t; c < c1; c += kTile) {
        const uint64_t lo = c * 16u < B ? B : c * 16u, hi = c * 16u + 16u > E ? E : c * 16u + 16u;
        const uint64_t p64 = lo - B;
        const uint32_t p = p64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)p64;
        // the last frame f of the tile with rel[f] <= p (rel[0] = 0 <= p)
        uint32_t l = 0, h = nf;
        while (h - l > 1u) {
            const uint32_t mid = (l + h) >> 1;
            if (s_rel[mid] <= p) l = mid;
            else h = mid;
        }
        uint32_t f = l;
        const bool whole = hi - lo == 16u;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (whole && p64 + 16u <= s_rel[f + 1]) {
            const uint32_t q = p - s_rel[f], len = s_len[f];
            const uint32_t n = q >= len ? 0u : len - q >= 16u ? 16u : len - q;  // source bytes of this chunk
            if (n) {
                const uint64_t A = base + s_src[f] + q;
                const uint32_t sh = (uint32_t)A & 3u;
                const auto* dw = NEXG_GLOBAL(uint32_t, reinterpret_cast<const void*>(A & ~3ull));
                uint32_t d[5];
                if (n == 16u) {
                    const u32x4a4 w = __builtin_nontemporal_load(NEXG_GLOBAL(u32x4a4, reinterpret_cast<const void*>(A & ~3ull)));
                    d[0] = w.x, d[1] = w.y, d[2] = w.z, d[3] = w.w;
                    d[4] = sh ? dw[4] : 0u;
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < 5; k++) d[k] = 4u * k < sh + n ? dw[k] : 0u;
                }
                uint32_t w[4];
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    w[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], sh);
                    const uint32_t keep = n <= 4u * j ? 0u : n - 4u * j >= 4u ? 0xFFFFFFFFu : (1u << (8u * (n - 4u * j))) - 1u;
                    w[j] &= keep;
                }
                v = u32x4{w[0], w[1], w[2], w[3]};
            }
            __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(out_data + c * 16u));
            continue;
        }
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        for (uint64_t j = lo; j < hi; j++) {
            const uint64_t pj64 = j - B;
            const uint32_t pj = pj64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)pj64;
            while (f + 1u < nf && s_rel[f + 1] <= pj) f++;
            const uint32_t q = pj - s_rel[f];
            const uint32_t b = pj >= s_rel[f] && q < s_len[f] ? NEXG_GLOBAL(uint8_t, a.data)[s_src[f] + q] : 0u;
            if (whole) w[(j & 15u) >> 2] |= b << (8u * (j & 3u));
            else out_data[j] = (uint8_t)b;
        }
        if (whole) __builtin_nontemporal_store(u32x4{w[0], w[1], w[2], w[3]}, reinterpret_cast<u32x4*>(out_data + c * 16u));
    }
}

hipError_t launch_gather_frames(const ParseArgs& a, const uint64_t* out_offsets, uint8_t* out_data, uint64_t out_cap,
                                hipStream_t s) {
    const uint64_t tiles = (a.count + kTile - 1) / kTile;
    if (!tiles || !out_cap) return hipSuccess;
    hipLaunchKernelGGL(k_gather_frames, dim3((uint32_t)tiles), dim3(kTile), 0, s, a, out_offsets, out_data, out_cap);
    return hipGetLastError();
}

// ---- gather rows ---------------------------------------------------------------------

// ROW bytes per row, moved in pieces of P = min(ROW, 16) bytes: one lane per
// piece, the ROW / P lanes of a row are consecutive, so a wave stores one
// contiguous run
template <uint32_t ROW>
__global__ __launch_bounds__(256) void k_gather_rows(const void* rows, uint64_t rows_count, const uint32_t* index,
                                                     uint64_t n, void* out) {
    constexpr uint32_t P = ROW < 16u ? ROW : 16u, PER = ROW / P;
    typedef uint32_t piece __attribute__((ext_vector_type(P / 4u)));
    const uint64_t g = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    const uint64_t k = g / PER, part = g % PER;
    if (k >= n) return;
    const uint64_t i = NEXG_GLOBAL(uint32_t, index)[k];
    piece v = {};
    if (i < rows_count) v = NEXG_GLOBAL(piece, rows)[i * PER + part];
    __builtin_nontemporal_store(v, reinterpret_cast<piece*>(out) + g);
}

hipError_t launch_gather_rows(const void* rows, uint32_t row_bytes, uint64_t rows_count, const uint32_t* index,
                              uint64_t n, void* out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t pieces = n * (row_bytes < 16u ? 1u : row_bytes / 16u);
    const dim3 grid((uint32_t)((pieces + kTile - 1) / kTile)), block(kTile);
    switch (row_bytes) {
    case 4: hipLaunchKernelGGL(k_gather_rows<4>, grid, block, 0, s, rows, rows_count, index, n, out); break;
    case 8: hipLaunchKernelGGL(k_gather_rows<8>, grid, block, 0, s, rows, rows_count, index, n, out); break;
    case 16: hipLaunchKernelGGL(k_gather_rows<16>, grid, block, 0, s, rows, rows_count, index, n, out); break;
    case 32: hipLaunchKernelGGL(k_gather_rows<32>, grid, block, 0, s, rows, rows_count, index, n, out); break;
    case 64: hipLaunchKernelGGL(k_gather_rows<64>, grid, block, 0, s, rows, rows_count, index, n, out); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace nexg
