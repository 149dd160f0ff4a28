// reasm_core.hpp — the per-frame core of nexg_reasm_plan / nexg_reasm_frames
// (k_reasm_*, nexg_reasm.hip): IPv4 reassembly as include/nexg.h states it. The
// kernels run it on gfx950; the test-only host driver
// (tests/native/reasm_fuzz.cpp) runs the very same code on the CPU, one call
// per lane and phase.
//
// Plan side: reasm_classify reads the header words that decide a frame's class
// and key (each a big-endian u16 from the one or two aligned dwords that hold
// it, behind the length check that places it inside the frame), reasm_hash is
// the Toeplitz hash of the key without the identification, ReasmInfo is what
// the plan keeps per frame (32 B) and reasm_mark what a sorted position says
// about itself given the position before it.
//
// Fill side: a frame belongs to a group of kReasmLanes lanes, as in
// fragment_core.hpp, and every copy is an EncapFrame that leaves through
// encap_copy / encap_finish: aligned 16-B output chunks round robin over the
// lanes, the source funnel-shifted to the destination's phase. A PASS frame is
// a payload without a header; a HEAD is its own header (staged by frag_stage as
// a template with total length, flags / offset and checksum zero, patched from
// the row) in front of its own data; a PART is a payload that starts in the
// middle of the head's output frame. Chunks that straddle two members' data
// leave as byte stores of each member's own bytes.
#pragma once

#include "fragment_core.hpp"

namespace nexg {

constexpr uint32_t kReasmLanes = kFragLanes;

// Rules 1-4 of include/nexg.h for one frame.
struct ReasmClass {
    uint32_t status, kind;  // kind: NEXG_REASM_NONE, NEXG_REASM_PASS, or NEXG_REASM_HELD for a fragment (the plan decides)
    uint32_t hl, fo, mf, d; // a fragment's header length, 13-bit offset, MF bit and data bytes
    uint32_t ff0;           // its flags / fragment offset word
    uint32_t id, proto, src, dst;
};

NEXG_HD bool reasm_is_frag(const ReasmClass& c) { return c.kind == NEXG_REASM_HELD; }

// `ext`: frame_extent accepted the frame, whose byte 0 is at address src.
NEXG_HD ReasmClass reasm_classify(bool ext, uint32_t len, uint64_t src) {
    const ReasmClass pass{NEXG_FRAME_OK, NEXG_REASM_PASS, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (!ext) return {NEXG_ERR_BAD_EXTENT, NEXG_REASM_NONE, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (len < 34u || encap_ethertype(src + 12u) != 0x0800u) return pass;
    const uint32_t w14 = encap_ethertype(src + 14u), hl = 4u * ((w14 >> 8) & 15u);
    if ((w14 >> 12) != 4u || hl < 20u || 14u + hl > len) return pass;
    const uint32_t TL = encap_ethertype(src + 16u);
    if (TL < hl || 14u + TL > len) return pass;
    const uint32_t ff0 = encap_ethertype(src + 20u);
    if ((ff0 & 0x3FFFu) == 0u) return pass;  // MF clear and offset 0: whole
    return {NEXG_FRAME_OK, NEXG_REASM_HELD, hl, ff0 & 0x1FFFu, (ff0 >> 13) & 1u, TL - hl, ff0, encap_ethertype(src + 18u),
            encap_ethertype(src + 22u) & 0xFFu, encap_ethertype(src + 26u) << 16 | encap_ethertype(src + 28u),
            encap_ethertype(src + 30u) << 16 | encap_ethertype(src + 32u)};
}

// The Toeplitz hash (nexg_flow_batch's, NEXG_FLOW_DEFAULT_KEY) of the 12 bytes
// source, destination, 0, protocol, 0, 0: key bits 0..127 are the first four
// key words.
NEXG_HD uint32_t reasm_hash(uint32_t src, uint32_t dst, uint32_t proto) {
    const uint32_t K[4] = {0x6d5a56dau, 0x255b0ec2u, 0x4167253du, 0x43a38fb0u};
    const uint32_t W[3] = {src, dst, proto << 16};
    uint32_t h = 0;
#pragma unroll
    for (uint32_t j = 0; j < 3; j++) {
        const uint64_t kk = (uint64_t)K[j] << 32 | K[j + 1];
        for (uint32_t k = 0; k < 32; k++)
            if ((W[j] >> (31u - k)) & 1u) h ^= (uint32_t)((kk << k) >> 32);
    }
    return h;
}

// What the plan keeps per frame. A frame that is no fragment sorts behind
// every fragment: both keys all ones (a fragment's idfo is below 2^29).
struct ReasmInfo {
    uint32_t hash, idfo;  // id << 13 | fo
    uint32_t shape;       // hl | mf << 8 | frag << 9 | status << 16 | kind << 24
    uint32_t d;
    uint32_t src, dst, proto;
    uint32_t len;         // the frame's length: a PASS frame's output length
};
static_assert(sizeof(ReasmInfo) == 32, "ReasmInfo is 32 bytes (workspace_layout.hpp ReasmPlanLayout)");

NEXG_HD ReasmInfo reasm_info(const ReasmClass& c, uint32_t len) {
    const bool f = reasm_is_frag(c);
    return {f ? reasm_hash(c.src, c.dst, c.proto) : 0xFFFFFFFFu, f ? c.id << 13 | c.fo : 0xFFFFFFFFu,
            c.hl | c.mf << 8 | (f ? 1u << 9 : 0u) | c.status << 16 | c.kind << 24, c.d, c.src, c.dst, c.proto, len};
}
NEXG_HD bool info_frag(const ReasmInfo& x) { return (x.shape >> 9) & 1u; }
NEXG_HD uint32_t info_hl(const ReasmInfo& x) { return x.shape & 0xFFu; }
NEXG_HD uint32_t info_mf(const ReasmInfo& x) { return (x.shape >> 8) & 1u; }
NEXG_HD uint32_t info_fo(const ReasmInfo& x) { return x.idfo & 0x1FFFu; }

// What a sorted position says: it starts a run (the position before is none,
// no fragment, or of another (hash, identification)); its exact key differs
// from the position before's in the same run; it breaks the datagram (a run's
// first with fo != 0; a later one that does not start where the one before
// ends, whose predecessor has fewer than 8 data bytes or MF clear). `prev`:
// there is a position before, whose frame's info is p.
struct ReasmMark {
    bool head, brk, bad;
};
NEXG_HD ReasmMark reasm_mark(const ReasmInfo& x, bool prev, const ReasmInfo& p) {
    if (!info_frag(x)) return {true, false, false};
    const bool same = prev && info_frag(p) && p.hash == x.hash && (p.idfo >> 13) == (x.idfo >> 13);
    if (!same) return {true, false, info_fo(x) != 0u};
    const bool brk = p.src != x.src || p.dst != x.dst || p.proto != x.proto;
    const bool bad = 8u * info_fo(x) != 8u * info_fo(p) + p.d || p.d < 8u || !info_mf(p);
    return {false, brk, bad};
}

// A run's verdict from its sums and its two ends: complete, and D
NEXG_HD bool reasm_complete(uint32_t brk, uint32_t bad, const ReasmInfo& head, const ReasmInfo& last, uint32_t& D) {
    D = 8u * info_fo(last) + last.d;
    return brk == 0u && bad == 0u && !info_mf(last) && last.d >= 1u && info_hl(head) + D <= 65535u;
}

// ---- fill ------------------------------------------------------------------------------

// Everything the fill reads for one frame before it looks at frame bytes.
struct ReasmJob {
    bool live, ext;            // the frame is in the table; frame_extent accepted its extent
    uint32_t len, index;       // its length (0 unless ext) and i
    uint64_t src;              // the address of frame byte 0: looked at only when ext
    uint32_t kind, data_len;   // rows[i].kind, rows[i].data_len
    uint32_t first, first_end; // out_first[i], out_first[i + 1]
    bool named;                // PASS / HEAD: always; PART: rows[i].head < count, and then
    uint32_t head_hl;          // rows[head].hdr_len (its own for a HEAD)
    uint64_t lo, next;         // out_bytes[h], out_bytes[h + 1] of the head h it names (h = i for PASS and HEAD)
};

// Phase 1, every lane: a HEAD's header template. Phase 2, lane 0: its word sum.
NEXG_HD bool reasm_heads(const ReasmJob& j, const ReasmClass& c) {
    return j.live && j.kind == NEXG_REASM_HEAD && reasm_is_frag(c) && c.fo == 0u;
}
NEXG_HD void reasm_stage(const ReasmJob& j, const ReasmClass& c, FragHdr& H, uint32_t lane) {
    if (!reasm_heads(j, c)) return;
    FragShape s{};
    s.kind = NEXG_FRAG_SPLIT;
    s.hl = c.hl;
    FragJob fj{};
    fj.src = j.src;
    frag_stage(fj, s, H, lane);
}
NEXG_HD void reasm_sum(const ReasmJob& j, const ReasmClass& c, FragHdr& H) {
    if (reasm_heads(j, c)) H.sum0 = frag_header_sum(H.h0, c.hl);
}

// Phase 3, every lane: the lane's chunks of the frame's bytes, and lane 0 the
// table entry. rows, out_first and out_bytes are caller memory: every store
// lies in [x.lo, x.hi), which lies in [j.lo, min(j.next, out.cap)); the copy
// runs over the frame's own H + m bytes (and at most 15 pad bytes); a table
// index stays below min(j.first_end, out.count).
NEXG_HD void reasm_fill(const ReasmJob& j, const ReasmClass& c, const FragHdr& H, const FragOut& out, uint32_t lane) {
    if (!j.live || !j.named) return;
    const uint64_t f_end = j.first_end < out.count ? j.first_end : out.count;
    EncapFrame x{};
    x.pos03 = 0xFFFFFFFFu;
    x.pos4 = 0xFFu;
    x.csum_at = kEncapPatches;
    if (j.kind == NEXG_REASM_PASS && c.kind == NEXG_REASM_PASS) {
        x.m = j.len;
        x.S = j.src;
        encap_range(j.lo, j.next, out.cap, EncapShape{NEXG_FRAME_OK, 0u, 0u, j.len}, x);
        (void)encap_copy(x, out.data, lane);  // no header chunk: every chunk leaves
        if (lane == 0u && j.first < f_end) {
            out.offsets[j.first] = j.lo;
            out.len[j.first] = j.len;
            out.src[j.first] = j.index;
        }
        return;
    }
    if (!reasm_is_frag(c)) return;
    if (j.kind == NEXG_REASM_HEAD) {
        if (c.fo != 0u) return;
        const uint32_t Hb = 14u + c.hl, tl = c.hl + j.data_len, ff = c.ff0 & 0xC000u;
        x.H = Hb;
        x.m = c.d;
        x.S = j.src + Hb;
        encap_range(j.lo, j.next, out.cap, EncapShape{NEXG_FRAME_OK, Hb, 0u, c.d}, x);
        if (x.hi > j.lo + Hb + c.d) x.hi = j.lo + Hb + c.d;  // no pad: the last member writes it
        x.pos03 = kFragPos;
        x.hdr = H.h0;
        x.val[0] = tl & 0xFFFFu;
        x.val[1] = ~fold16(H.sum0 + (tl & 0xFFFFu) + ff) & 0xFFFFu;
        x.val[2] = ff;
        const EncapLane L = encap_copy(x, out.data, lane);
        encap_finish(x, out.data, lane, L);
        if (lane == 0u && j.first < f_end) {
            out.offsets[j.first] = j.lo;
            out.len[j.first] = Hb + j.data_len;
            out.src[j.first] = j.index;
        }
        return;
    }
    if (j.kind != NEXG_REASM_PART) return;
    const uint64_t lo = j.lo + 14u + j.head_hl + 8u * c.fo;
    if (lo < j.lo || lo >= j.next) return;  // (below out.cap: encap_range)
    x.m = c.d;
    x.S = j.src + 14u + c.hl;
    encap_range(lo, j.next, out.cap, EncapShape{NEXG_FRAME_OK, 0u, 0u, c.d}, x);
    if (c.mf && x.hi > lo + c.d) x.hi = lo + c.d;  // the pad is the last member's
    (void)encap_copy(x, out.data, lane);
}

}  // namespace nexg
