// checksum_core.hpp — the per-frame cores of nexg_recompute_checksums_batch
// (k_recompute, nexg_fixup.hip) and nexg_checksum_batch (k_checksum,
// nexg_parse.hip) over a frame read entirely from HBM. The kernels run them
// on gfx950 after their extent checks; the test-only host harness
// (tests/native/core_harness.hip) runs the very same code on the CPU.
#pragma once

#include "frame_core.hpp"

namespace nexg {

// Frame read entirely from HBM (checksum utility path).
struct GlobalFrame {
    NEXG_NO_DEFER
    const uint8_t* g;
    NEXG_HD uint32_t u8(uint32_t i) const { return g[i]; }
    NEXG_HD uint64_t le_sum(uint32_t a, uint32_t b) const {
        const uint64_t base = reinterpret_cast<uint64_t>(g);
        return global_le_sum(base + a, base + b);
    }
};

NEXG_HD void put_be16(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 8);
    p[1] = (uint8_t)v;
}

// The mutable views' constructor conditions over one frame of `len` bytes read
// through accessor o.f, stated
// once for recompute_frame below and rewrite_frame (rewrite_core.hpp). The IP
// part: the Ethernet view (ethernet.rs:355-361) or the raw IP packet at
// ip_offset, then MutableIpv4Packet::new (ipv4.rs:540-566) or
// MutableIpv6Packet::new (>= 40 B, payload = the rest; extension headers are
// not walked).
struct FrameViews {
    uint32_t L = 14;     // offset of the IP header
    uint32_t family = 0; // 4 / 6 when that IP view exists, else 0
    uint32_t hl = 0;     // IP header bytes (IPv6: 40)
    uint32_t P = 0, m = 0;  // the IP view's payload_mut: f[P, P + m)
    uint32_t proto = 0;  // protocol / next header byte
    bool eth = false;    // the Ethernet view exists
    bool l4 = false;     // the protocol has an L4 view kind (17, 6, 1 over IPv4 / 58 over IPv6)
};

template <class O>
NEXG_HD FrameViews frame_views(const O& o, uint32_t len, uint32_t opt_flags, uint32_t ip_offset) {
    FrameViews v;
    uint32_t family = 0;
    if (opt_flags & NEXG_PARSE_FROM_IP) {
        v.L = ip_offset;
        const uint32_t ver = v.L < len ? o.f.u8(v.L) >> 4 : 0u;
        family = ver == 4u ? 4u : (ver == 6u ? 6u : 0u);
    } else if (len >= 14u) {
        v.eth = true;
        const uint32_t et = o.be16(12);
        family = et == 0x0800u ? 4u : (et == 0x86DDu ? 6u : 0u);
    }
    const uint32_t L = v.L;
    const uint32_t n = family && L < len ? len - L : 0u;
    if (family == 4u && n >= 20u) {
        // MutableIpv4Packet::new (ipv4.rs:540-566)
        const uint32_t hl = (o.f.u8(L) & 15u) * 4u, total = o.be16(L + 2);
        if (hl >= 20u && hl <= n && (total == 0u || total >= hl)) {
            const uint32_t eff = total == 0u ? n : (total < n ? total : n);  // total_len, ipv4.rs:697-704
            v.family = 4u;
            v.hl = hl;
            v.P = L + hl;
            v.m = eff - hl;
            v.proto = o.f.u8(L + 9);
            v.l4 = v.proto == 17u || v.proto == 6u || v.proto == 1u;
        }
    } else if (family == 6u && n >= 40u) {  // MutableIpv6Packet::new: >= 40 B, payload = rest
        v.family = 6u;
        v.hl = 40u;
        v.P = L + 40u;
        v.m = n - 40u;
        v.proto = o.f.u8(L + 6);
        v.l4 = v.proto == 17u || v.proto == 6u || v.proto == 58u;
    }
    return v;
}

// The L4 view of a frame whose FrameViews has l4 set: whether its constructor
// accepts the IP payload, and the byte offset of the checksum word in it.
struct L4View {
    bool view = false;
    uint32_t sk = 0;  // skipword * 2
};

template <class O>
NEXG_HD L4View l4_view(const O& o, const FrameViews& v) {
    L4View q;
    const uint32_t P = v.P, m = v.m;
    if (v.proto == 17u) {  // MutableUdpPacket::new (udp.rs:101-121)
        const uint32_t ul = m >= 8u ? o.be16(P + 4) : 0u;
        q.view = m >= 8u && (ul == 0u || (ul >= 8u && ul <= m));
        q.sk = 6;
    } else if (v.proto == 6u) {  // MutableTcpPacket::new (tcp.rs:857-876)
        const uint32_t hl = m >= 20u ? (o.f.u8(P + 12) >> 4) * 4u : 0u;
        q.view = m >= 20u && hl >= 20u && hl <= m;
        q.sk = 16;
    } else {  // ICMP / ICMPv6: IcmpPacket::from_buf needs the 8-B header (icmp.rs:188-191)
        q.view = m >= 8u;
        q.sk = 2;
    }
    return q;
}

// util::checksum(raw[..header_len], 5) of the IPv4 view
template <class O>
NEXG_HD uint32_t ipv4_header_checksum(const O& o, const FrameViews& v) {
    return fold_complement(o.wsum(v.L, v.L + 10) + o.wsum(v.L + 12, v.L + v.hl));
}

// the pseudo-header's address words (util.rs:91-93 / 135-137)
template <class O>
NEXG_HD uint64_t pseudo_addresses(const O& o, const FrameViews& v) {
    const uint32_t L = v.L;
    if (v.family == 4u) return (uint64_t)o.be16(L + 12) + o.be16(L + 14) + o.be16(L + 16) + o.be16(L + 18);
    uint64_t pseudo = 0;
#pragma unroll
    for (uint32_t k = 0; k < 32; k += 2) pseudo += o.be16(L + 8 + k);
    return pseudo;
}

// the L4 view's recompute_checksum over the whole payload_mut slice
template <class O>
NEXG_HD uint32_t l4_checksum(const O& o, const FrameViews& v, uint32_t sk, uint64_t pseudo) {
    uint64_t t = o.wsum(v.P, v.P + sk) + o.wsum(v.P + sk + 2u, v.P + v.m);
    if (v.proto != 1u) t += pseudo + v.proto + v.m;  // util.rs:89-97 / 119-127 (len as one u32)
    return fold_complement(t);
}

// The mutable views' recompute_checksum chained over one frame f[0, len), in
// place (nexg_fixup.hip's header names the reference's lines); returns the
// frame's report row.
NEXG_HD nexg_fixup recompute_frame(uint8_t* f, uint32_t len, uint32_t opt_flags, uint32_t ip_offset,
                                   uint32_t which) {
    nexg_fixup fx{0, 0, 0, 0, 0};
    const GlobalFrame gf{f};
    const FrameOps<GlobalFrame> o{gf, (uint32_t)(reinterpret_cast<uint64_t>(f) & 1u)};
    const FrameViews v = frame_views(o, len, opt_flags, ip_offset);
    if (v.family == 4u && (which & NEXG_FIX_IP)) {
        const uint32_t c = ipv4_header_checksum(o, v);
        put_be16(f + v.L + 10, c);
        fx.done |= NEXG_FIX_IP;
        fx.ip_csum = (uint16_t)c;
    }
    if (v.l4 && (which & NEXG_FIX_L4)) {
        const L4View q = l4_view(o, v);
        if (q.view) {
            const uint32_t c = l4_checksum(o, v, q.sk, v.proto != 1u ? pseudo_addresses(o, v) : 0ull);
            put_be16(f + v.P + q.sk, c);
            fx.done |= NEXG_FIX_L4;
            fx.proto = (uint8_t)v.proto;
            fx.l4_csum = (uint16_t)c;
            fx.l4_off = (uint16_t)v.P;
        }
    }
    return fx;
}

// util.rs:65-71 checksum(buf, skipword) of g[0, len), 0 < len <= 65535: the
// skipped word contributes nothing, nor does the last byte of an odd-length
// buffer when the skipped word starts at it (util.rs:158).
NEXG_HD uint16_t checksum_buffer(const uint8_t* g, uint32_t len, uint32_t skipword) {
    GlobalFrame f{g};
    FrameOps<GlobalFrame> o{f, (uint32_t)((reinterpret_cast<uint64_t>(f.g)) & 1u)};
    const uint64_t sk = 2ull * skipword;
    uint64_t t;
    if (sk >= len) {
        t = o.wsum(0, len);
    } else {
        t = o.wsum(0, (uint32_t)sk);
        if (sk + 2 < len) t += o.wsum((uint32_t)sk + 2u, len);
    }
    return (uint16_t)fold_complement(t);
}

}  // namespace nexg
