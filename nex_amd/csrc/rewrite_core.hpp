// rewrite_core.hpp — the per-frame core of nexg_rewrite_batch (k_rewrite,
// nexg_rewrite.hip): the reference's mutable setters (MutableEthernetPacket::
// set_destination / set_source, MutableIpv4Packet::set_source / set_destination
// / set_ttl / set_dscp / set_ecn, MutableIpv6Packet::set_source /
// set_destination / set_hop_limit / set_traffic_class, MutableTcpPacket /
// MutableUdpPacket::set_source / set_destination) under ChecksumMode::Automatic
// (checksum.rs:8-14), over the views checksum_core.hpp builds. include/nexg.h
// is the specification. The kernel runs it on gfx950; the test-only host
// driver (tests/native/rewrite_fuzz.cpp) runs the very same code on the CPU.
#pragma once

#include "checksum_core.hpp"

namespace nexg {

// nullptr when nexg_rewrite_batch would accept the set, else what is wrong with it
inline const char* check_actions(const nexg_actions* s) {
    if (!s) return "NULL action set";
    if (s->n_actions == 0 || s->n_actions > NEXG_REWRITE_MAX_ACTIONS) return "n_actions must be 1..16";
    if (s->flags & ~NEXG_REWRITE_INCREMENTAL) return "unknown flag bits";
    for (uint32_t i = 0; i < s->n_actions; i++) {
        const nexg_action& a = s->actions[i];
        if (a.sets & ~NEXG_SET_ALL) return "unknown sets bits";
        for (uint32_t k = 0; k < 8; k++)
            if (a.reserved[k]) return "reserved must be 0";
        if ((a.sets & NEXG_SET_TTL) && (a.sets & NEXG_DEC_TTL)) return "SET_TTL together with DEC_TTL";
        if ((a.sets & NEXG_DEC_TTL) && a.ttl == 0) return "DEC_TTL by 0";
        const bool addr = (a.sets & (NEXG_SET_IP_SRC | NEXG_SET_IP_DST)) != 0;
        if (addr && a.family != 4 && a.family != 6) return "an address set needs family 4 or 6";
        if (!addr && a.family != 0) return "a family without an address set";
        if ((a.sets & NEXG_SET_TOS) && (a.tos_mask == 0 || (a.tos & ~a.tos_mask))) return "SET_TOS with an empty mask or bits outside it";
    }
    return nullptr;
}

NEXG_HD uint32_t rd_be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }

// RFC 1624 eqn. 3 on a stored checksum: HC' = ~fold(~HC + sum(~m + m'))
NEXG_HD uint32_t csum_update(uint32_t hc, uint32_t delta) {
    uint32_t s = (~hc & 0xFFFFu) + delta;
    s = (s & 0xFFFFu) + (s >> 16);
    s = (s & 0xFFFFu) + (s >> 16);
    return ~s & 0xFFFFu;
}

// The INCREMENTAL instance's reader: the frame's first 16-B aligned blocks
// (kWindowBlocks of them, those that overlap the frame: the block rule of the
// frame batch layout) loaded once with 16-B loads and kept as dwords, dword j
// at col[j * stride]. The kernel keeps them in LDS, one column per lane
// (stride 256: lanes that read the same frame byte hit different banks); the
// host driver in an array (stride 1). Frame byte i < wlen is window byte
// o + i; a byte past the window (an L4 header behind a long IPv4 option list
// in a frame at a late phase) is read from memory. The window is a snapshot:
// rewrite_frame<true> reads every byte before it stores it, so it never needs
// a byte it has written.
constexpr uint32_t kWindowBlocks = 6;  // 96 B: Ethernet + IPv6 + 20 L4 bytes = 74, + 15 of phase
struct HeaderWindow {
    NEXG_NO_DEFER
    const uint32_t* col;
    uint32_t stride;
    const uint8_t* g;
    uint32_t o, wlen;
    NEXG_HD uint32_t u8(uint32_t i) const {
        if (i >= wlen) return g[i];
        const uint32_t b = o + i;
        return (col[(b >> 2) * stride] >> (8u * (b & 3u))) & 0xFFu;
    }
    NEXG_HD uint64_t le_sum(uint32_t a, uint32_t b) const {  // RECOMPUTE's sums; not used through a window
        const uint64_t base = reinterpret_cast<uint64_t>(g);
        return global_le_sum(base + a, base + b);
    }
};

NEXG_HD HeaderWindow load_header_window(const uint8_t* f, uint32_t len, uint32_t* col, uint32_t stride) {
    const uint64_t addr = reinterpret_cast<uint64_t>(f);
    const uint32_t o = (uint32_t)(addr & 15u);
    if (len) {
        // all six loads are issued before the first is used: a block past the frame's last one is that last one
        // again (an address inside the frame's own blocks), so no load hangs on a branch of its own
        const uint32_t last = (o + len - 1u) >> 4;
        uint4 w[kWindowBlocks];
#pragma unroll
        for (uint32_t k = 0; k < kWindowBlocks; k++)
            w[k] = load16(reinterpret_cast<const void*>(addr - o + 16u * (k < last ? k : last)));
#pragma unroll
        for (uint32_t k = 0; k < kWindowBlocks; k++) {
            col[(4u * k + 0u) * stride] = w[k].x;
            col[(4u * k + 1u) * stride] = w[k].y;
            col[(4u * k + 2u) * stride] = w[k].z;
            col[(4u * k + 3u) * stride] = w[k].w;
        }
    }
    const uint32_t room = 16u * kWindowBlocks - o;
    return HeaderWindow{col, stride, f, o, len < room ? len : room};
}

// Frame f[0, len) rewritten in place by action A (number a of the set), its
// bytes read through `rd` (GlobalFrame{f}, or a HeaderWindow of it in INCR
// mode); INCR = NEXG_REWRITE_INCREMENTAL. Only the bytes of the fields and
// checksum fields written are stored, as bytes; in INCR mode nothing past the
// first 20 L4 bytes is read.
template <bool INCR, class R>
NEXG_HD nexg_rewritten rewrite_frame(uint8_t* f, const R& rd, uint32_t len, uint32_t opt_flags, uint32_t ip_offset,
                                     const nexg_action& A, uint32_t a) {
    nexg_rewritten rw{0, 0, (uint8_t)a, 0, 0};
    const uint32_t sets = A.sets;
    const FrameOps<R> o{rd, (uint32_t)(reinterpret_cast<uint64_t>(f) & 1u)};
    const FrameViews v = frame_views(o, len, opt_flags, ip_offset);
    const uint32_t L = v.L, P = v.P;
    uint32_t applied = 0;
    uint32_t dip = 0, dl4 = 0;  // sum(~m + m') over the IPv4 header's words / the words the L4 checksum covers

    if (v.eth) {
        if (sets & NEXG_SET_ETH_DST) {
#pragma unroll
            for (uint32_t k = 0; k < 6; k++) f[k] = A.eth_dst[k];
            applied |= NEXG_SET_ETH_DST;
        }
        if (sets & NEXG_SET_ETH_SRC) {
#pragma unroll
            for (uint32_t k = 0; k < 6; k++) f[6 + k] = A.eth_src[k];
            applied |= NEXG_SET_ETH_SRC;
        }
    }

    // the L4 view, looked at only when the action has a field that needs it
    L4View q;
    if (v.l4 && (sets & (NEXG_SET_IP_SRC | NEXG_SET_IP_DST | NEXG_SET_SRC_PORT | NEXG_SET_DST_PORT))) {
        // a later IPv4 fragment holds no L4 header (INCR only: the reference's views know nothing of fragments)
        const bool later_fragment = INCR && v.family == 4u && (o.be16(L + 6) & 0x1FFFu) != 0u;
        if (!later_fragment) q = l4_view(o, v);
    }
    const bool pseudo = v.proto != 1u;  // ICMPv4 has no pseudo-header

    if (v.family && v.family == A.family) {
        const uint32_t words = v.family == 4u ? 2u : 8u;
        const uint32_t so = v.family == 4u ? L + 12u : L + 8u, dof = so + 2u * words;
        if (sets & NEXG_SET_IP_SRC) {
            for (uint32_t k = 0; k < words; k++) {
                const uint32_t nv = rd_be16(A.src + 2u * k);
                if (INCR) dip += (~o.be16(so + 2u * k) & 0xFFFFu) + nv;
                put_be16(f + so + 2u * k, nv);
            }
            applied |= NEXG_SET_IP_SRC;
        }
        if (sets & NEXG_SET_IP_DST) {
            for (uint32_t k = 0; k < words; k++) {
                const uint32_t nv = rd_be16(A.dst + 2u * k);
                if (INCR) dip += (~o.be16(dof + 2u * k) & 0xFFFFu) + nv;
                put_be16(f + dof + 2u * k, nv);
            }
            applied |= NEXG_SET_IP_DST;
        }
        if (INCR && pseudo) dl4 = dip;  // the same words sit in the pseudo-header
    }
    if (v.family && (sets & (NEXG_SET_TTL | NEXG_DEC_TTL))) {
        const uint32_t at = L + (v.family == 4u ? 8u : 7u);
        const uint32_t old = o.f.u8(at);
        const uint32_t nv = (sets & NEXG_SET_TTL) ? A.ttl : (old > A.ttl ? old - A.ttl : 0u);
        if (INCR && v.family == 4u) {
            const uint32_t proto = v.proto;  // the word's other byte
            dip += (~(old << 8 | proto) & 0xFFFFu) + (nv << 8 | proto);
        }
        f[at] = (uint8_t)nv;
        applied |= sets & (NEXG_SET_TTL | NEXG_DEC_TTL);
    }
    if (v.family && (sets & NEXG_SET_TOS)) {
        if (v.family == 4u) {
            const uint32_t b0 = o.f.u8(L), old = o.f.u8(L + 1);
            const uint32_t nv = (old & ~(uint32_t)A.tos_mask) | A.tos;
            if (INCR) dip += (~(b0 << 8 | old) & 0xFFFFu) + (b0 << 8 | nv);
            f[L + 1] = (uint8_t)nv;
        } else {
            const uint32_t b0 = o.f.u8(L), b1 = o.f.u8(L + 1);
            const uint32_t old = ((b0 & 15u) << 4) | (b1 >> 4);
            const uint32_t nv = (old & ~(uint32_t)A.tos_mask) | A.tos;
            f[L] = (uint8_t)((b0 & 0xF0u) | (nv >> 4));
            f[L + 1] = (uint8_t)((b1 & 0x0Fu) | ((nv & 15u) << 4));
        }
        applied |= NEXG_SET_TOS;
    }
    if (v.family != 4u) dip = 0;
    if (q.view && (v.proto == 17u || v.proto == 6u)) {
        if (sets & NEXG_SET_SRC_PORT) {
            if (INCR) dl4 += (~o.be16(P) & 0xFFFFu) + A.src_port;
            put_be16(f + P, A.src_port);
            applied |= NEXG_SET_SRC_PORT;
        }
        if (sets & NEXG_SET_DST_PORT) {
            if (INCR) dl4 += (~o.be16(P + 2) & 0xFFFFu) + A.dst_port;
            put_be16(f + P + 2, A.dst_port);
            applied |= NEXG_SET_DST_PORT;
        }
    }

    const bool ip_dirty = v.family == 4u && (applied & (NEXG_SET_IP_SRC | NEXG_SET_IP_DST | NEXG_SET_TTL | NEXG_DEC_TTL | NEXG_SET_TOS));
    const bool l4_dirty = q.view && ((applied & (NEXG_SET_SRC_PORT | NEXG_SET_DST_PORT)) ||
                                     ((applied & (NEXG_SET_IP_SRC | NEXG_SET_IP_DST)) && pseudo));
    if (ip_dirty) {
        const uint32_t c = INCR ? csum_update(o.be16(L + 10), dip) : ipv4_header_checksum(o, v);
        put_be16(f + L + 10, c);
        rw.fixed |= NEXG_FIX_IP;
        rw.ip_csum = (uint16_t)c;
    }
    if (l4_dirty) {
        uint8_t* cs = f + P + q.sk;
        if (INCR) {
            const uint32_t hc = o.be16(P + q.sk);
            if (!(v.proto == 17u && v.family == 4u && hc == 0u)) {  // UDP over IPv4 "no checksum" stays none
                const uint32_t c = csum_update(hc, dl4);
                put_be16(cs, c);
                rw.fixed |= NEXG_FIX_L4;
                rw.l4_csum = (uint16_t)c;
            }
        } else {
            const uint32_t c = l4_checksum(o, v, q.sk, pseudo ? pseudo_addresses(o, v) : 0ull);
            put_be16(cs, c);
            rw.fixed |= NEXG_FIX_L4;
            rw.l4_csum = (uint16_t)c;
        }
    }
    rw.applied = (uint16_t)applied;
    return rw;
}

}  // namespace nexg
