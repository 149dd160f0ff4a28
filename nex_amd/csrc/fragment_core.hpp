// fragment_core.hpp — the per-frame core of nexg_fragment_plan /
// nexg_fragment_frames (k_fragment_*, nexg_fragment.hip): RFC 791 section 3.2
// as include/nexg.h states it, each piece the bytes the reference's
// Ipv4PacketBuilder gives for its fields. The kernels run it on gfx950; the
// test-only host driver (tests/native/fragment_fuzz.cpp) runs the very same
// code on the CPU, one call per lane and phase.
//
// A frame belongs to a group of kFragLanes lanes, as in encap_core.hpp, and a
// piece is to the copy what an encapsulated frame is there: a header of H =
// 14 + hl bytes in front of a run of source bytes. So a piece is an EncapFrame
// and leaves through encap_copy / encap_finish: aligned 16-B output chunks
// round robin over the lanes, the header's chunks built from a template with
// patches. The template is the frame's own Ethernet + IPv4 header, staged once
// per frame in the group's FragHdr (LDS on the device) with total length,
// flags / fragment offset and checksum zero: h0 for piece 0, h1 with the
// options that are not copied set to NOPs for the pieces behind it, and the
// folded word sum of each, so a piece's checksum is three additions. The three
// phases (frag_stage by every lane, frag_walk by lane 0, frag_fill by every
// lane) are separated by the workgroup's barriers.
#pragma once

#include "encap_core.hpp"

namespace nexg {

constexpr uint32_t kFragLanes = kEncapLanes;
constexpr uint32_t kFragHdrDwords = kEncapHdrDwords;  // 80 B >= 14 + 60
constexpr uint32_t kFragPos = 16u | 24u << 8 | 20u << 16 | 0xFFu << 24;  // patches 0..2: total length, checksum, flags / offset

// nullptr when nexg_frag_option_check would accept the option, else what is wrong with it
inline const char* check_frag_option(const nexg_frag_option* o) {
    if (!o) return "NULL option";
    if (o->mtu < 68u || o->mtu > 65535u) return "mtu must be 68..65535";
    if (o->flags & ~NEXG_FRAG_IGNORE_DF) return "unknown flag bits";
    if (o->align != 1u && o->align != 4u && o->align != 8u && o->align != 16u) return "align must be 1, 4, 8 or 16";
    if (o->reserved != 0u) return "reserved must be 0";
    return nullptr;
}

// Rules 1-6 of include/nexg.h for one frame.
struct FragShape {
    uint32_t status, kind;
    uint32_t n;        // output frames
    uint32_t hl, p, D; // a split frame's header length, data bytes per piece and data bytes in all
    uint32_t ff;       // its flags / fragment offset word without MF: reserved bit, DF as the pieces carry it, fo0
    uint32_t mf0;
};

// `ext`: frame_extent accepted the frame, whose byte 0 is at address src. The
// header words come through encap_ethertype (a big-endian u16 from the one or
// two aligned dwords that hold it), each behind the length check that places
// it inside the frame.
NEXG_HD FragShape frag_shape(bool ext, uint32_t len, uint64_t src, uint32_t mtu, uint32_t flags) {
    const FragShape pass{NEXG_FRAME_OK, NEXG_FRAG_PASS, 1u, 0u, 0u, 0u, 0u, 0u};
    const FragShape too_big{NEXG_FRAME_OK, NEXG_FRAG_TOO_BIG, 0u, 0u, 0u, 0u, 0u, 0u};
    if (!ext) return {NEXG_ERR_BAD_EXTENT, NEXG_FRAG_NONE, 0u, 0u, 0u, 0u, 0u, 0u};
    if (len < 14u) return pass;
    const uint32_t et = encap_ethertype(src + 12u);
    if (et == 0x86DDu && len >= 54u && (encap_ethertype(src + 14u) >> 12) == 6u) {
        const uint32_t ip = 40u + encap_ethertype(src + 18u);
        if (ip <= len - 14u) return ip > mtu ? too_big : pass;
    }
    if (et != 0x0800u || len < 34u) return pass;
    const uint32_t w14 = encap_ethertype(src + 14u), hl = 4u * ((w14 >> 8) & 15u);
    if ((w14 >> 12) != 4u || hl < 20u || 14u + hl > len) return pass;
    const uint32_t TL = encap_ethertype(src + 16u);
    if (TL < hl || 14u + TL > len || TL <= mtu) return pass;
    const uint32_t ff0 = encap_ethertype(src + 20u);
    const bool ignore_df = (flags & NEXG_FRAG_IGNORE_DF) != 0u;
    if ((ff0 & 0x4000u) && !ignore_df) return too_big;
    const uint32_t D = TL - hl, p = (mtu - hl) & ~7u, n = (D + p - 1u) / p, fo0 = ff0 & 0x1FFFu;
    if (fo0 + (n - 1u) * (p >> 3) > 8191u) return {NEXG_ERR_INVALID_LENGTH, NEXG_FRAG_NONE, 0u, 0u, 0u, 0u, 0u, 0u};
    return {NEXG_FRAME_OK, NEXG_FRAG_SPLIT, n, hl, p, D, (ff0 & (ignore_df ? 0x8000u : 0xC000u)) | fo0, (ff0 >> 13) & 1u};
}

NEXG_HD uint32_t frag_pad(uint32_t v, uint32_t align) { return (v + align - 1u) & ~(align - 1u); }

// data bytes and length of piece k of a split frame
NEXG_HD uint32_t frag_piece_data(const FragShape& s, uint32_t k) {
    const uint32_t left = s.D - k * s.p;
    return left < s.p ? left : s.p;
}
NEXG_HD uint32_t frag_piece_len(const FragShape& s, uint32_t k) { return 14u + s.hl + frag_piece_data(s, k); }
// from the start of one piece to the start of the next
NEXG_HD uint32_t frag_stride(const FragShape& s, uint32_t align) { return frag_pad(14u + s.hl + s.p, align); }

// the frame's output bytes, every output frame rounded up to `align` (a power of two): below 2^20
NEXG_HD uint32_t frag_out_bytes(const FragShape& s, uint32_t len, uint32_t align) {
    if (s.kind == NEXG_FRAG_PASS) return frag_pad(len, align);
    if (s.kind != NEXG_FRAG_SPLIT) return 0u;
    return (s.n - 1u) * frag_stride(s, align) + frag_pad(frag_piece_len(s, s.n - 1u), align);
}

NEXG_HD nexg_fragged frag_row(const FragShape& s, uint32_t first) {
    const bool split = s.kind == NEXG_FRAG_SPLIT;
    return {(uint8_t)s.status, (uint8_t)s.kind, (uint8_t)(split ? s.hl : 0u), 0, (uint16_t)s.n, (uint16_t)(split ? s.p : 0u), first, 0u};
}

// A split frame's header as its pieces' templates (little-endian dwords of
// frame bytes [0, 14 + hl), zero behind them and in the three patched fields),
// and the folded big-endian word sum of each template's IPv4 header.
struct FragHdr {
    uint32_t h0[kFragHdrDwords], h1[kFragHdrDwords];
    uint32_t sum0, sum1;
};

// Everything the fill reads for one frame before it looks at frame bytes.
struct FragJob {
    bool live, ext;            // the frame is in the table; frame_extent accepted its extent
    uint32_t len, index;       // its length (0 unless ext) and i
    uint64_t src;              // the address of frame byte 0: looked at only when ext
    uint32_t first, first_end; // out_first[i], out_first[i + 1]
    uint64_t lo, next;         // out_bytes[i], out_bytes[i + 1]
};

struct FragOut {
    uint64_t* offsets;
    uint32_t* len;
    uint32_t* src;
    uint8_t* data;
    uint64_t cap, count;
};

// Phase 1, every lane: dwords lane and lane + 16 of the templates. A dword is
// loaded as the one or two aligned dwords that hold its header bytes, so the
// loads stay inside the header's own 16-B blocks.
NEXG_HD void frag_stage(const FragJob& j, const FragShape& s, FragHdr& H, uint32_t lane) {
    if (s.kind != NEXG_FRAG_SPLIT) return;
    const uint32_t Hb = 14u + s.hl;
    for (uint32_t d = lane; d < kFragHdrDwords; d += kFragLanes) {
        uint32_t v = 0u;
        if (4u * d < Hb) {
            const uint64_t A = j.src + 4u * d;
            const uint32_t sh = (uint32_t)A & 3u;
            const auto* dw = NEXG_GLOBAL(uint32_t, reinterpret_cast<const void*>(A & ~3ull));
            const uint32_t d0 = dw[0], d1 = (sh && 4u * d + 4u - sh < Hb) ? dw[1] : 0u;
            v = align_bytes(d1, d0, sh) & bytes_in((int32_t)(4u * d), 0, (int32_t)Hb);
            if (d >= 4u && d <= 6u) v &= 0xFFFF0000u;  // bytes 16..17, 20..21, 24..25: the patches
        }
        H.h0[d] = H.h1[d] = v;
    }
}

// the folded big-endian word sum of template bytes [14, 14 + hl): byte 14 is a
// dword's upper half, so the little-endian halves of the dwords are the words
// byte-swapped, and the swap commutes with the end-around sum
NEXG_HD uint32_t frag_header_sum(const uint32_t* h, uint32_t hl) {
    const uint32_t q = 3u + (hl >> 2);  // the dword whose lower half ends the header
    uint32_t a = (h[3] >> 16) + (h[q] & 0xFFFFu);
    for (uint32_t k = 4; k < q; k++) a = halves_acc(h[k], a);
    a = fold16(a);
    return ((a & 0xFFu) << 8) | (a >> 8);
}

// Phase 2, lane 0 of the group: the options of the pieces behind the first
// (rule 6's walk) and the two sums.
NEXG_HD void frag_walk(const FragShape& s, FragHdr& H) {
    if (s.kind != NEXG_FRAG_SPLIT) return;
    const uint32_t end = 14u + s.hl;
    uint32_t i = 34u;
    while (i < end) {
        const uint32_t t = (H.h1[i >> 2] >> (8u * (i & 3u))) & 0xFFu;
        if (t == 0u) break;
        if (t == 1u) {
            i++;
            continue;
        }
        if (i + 1u >= end) break;
        const uint32_t L = (H.h1[(i + 1u) >> 2] >> (8u * ((i + 1u) & 3u))) & 0xFFu;
        if (L < 2u || L > end - i) break;
        if (!(t & 0x80u))
            for (uint32_t b = i; b < i + L; b++) {
                const uint32_t at = 8u * (b & 3u);
                H.h1[b >> 2] = (H.h1[b >> 2] & ~(0xFFu << at)) | 1u << at;
            }
        i += L;
    }
    H.sum0 = frag_header_sum(H.h0, s.hl);
    H.sum1 = frag_header_sum(H.h1, s.hl);
}

// Phase 3, every lane: the lane's chunks of every output frame, and its share
// of the table. out_first and out_bytes are caller memory: a piece's stores lie
// in [its start, min(the next piece's start, its end + 15, j.next, out.cap)) and
// its start in [j.lo, j.next); the loops run to the n of the frame's own shape;
// a table index stays below min(j.first_end, out.count).
NEXG_HD void frag_fill(const FragJob& j, const FragShape& s, const FragHdr& H, uint32_t align, const FragOut& out, uint32_t lane) {
    if (!j.live || s.n == 0u) return;
    const uint64_t f_end = j.first_end < out.count ? j.first_end : out.count;
    EncapFrame x{};
    x.pos03 = 0xFFFFFFFFu;
    x.pos4 = 0xFFu;
    x.csum_at = kEncapPatches;
    if (s.kind == NEXG_FRAG_PASS) {
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
    const uint32_t Hb = 14u + s.hl, stride = frag_stride(s, align);
    x.pos03 = kFragPos;
    x.H = Hb;
    for (uint32_t k = 0; k < s.n; k++) {
        const uint64_t lo = j.lo + (uint64_t)k * stride;
        if (lo < j.lo || lo >= j.next || lo >= out.cap) break;  // every later piece starts further on
        const bool last = k + 1u == s.n;
        const uint32_t d = frag_piece_data(s, k), tl = s.hl + d;
        const uint32_t ff = (s.ff + k * (s.p >> 3)) | ((!last || s.mf0) ? 0x2000u : 0u);
        uint64_t next = j.next;
        if (!last && lo + stride < next) next = lo + stride;
        x.m = d;
        x.S = j.src + Hb + k * s.p;
        encap_range(lo, next, out.cap, EncapShape{NEXG_FRAME_OK, Hb, 0u, d}, x);
        x.hdr = k ? H.h1 : H.h0;
        x.val[0] = tl;
        x.val[1] = ~fold16((k ? H.sum1 : H.sum0) + tl + ff) & 0xFFFFu;
        x.val[2] = ff;
        const EncapLane L = encap_copy(x, out.data, lane);
        encap_finish(x, out.data, lane, L);
    }
    for (uint32_t k = lane; k < s.n; k += kFragLanes) {
        const uint64_t f = (uint64_t)j.first + k;
        if (f >= f_end) break;
        out.offsets[f] = j.lo + (uint64_t)k * stride;
        out.len[f] = frag_piece_len(s, k);
        out.src[f] = j.index;
    }
}

}  // namespace nexg
