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

// The mutable views' recompute_checksum chained over one frame f[0, len), in
// place (nexg_fixup.hip's header names the reference's lines); returns the
// frame's report row.
NEXG_HD nexg_fixup recompute_frame(uint8_t* f, uint32_t len, uint32_t opt_flags, uint32_t ip_offset,
                                   uint32_t which) {
    nexg_fixup fx{0, 0, 0, 0, 0};
    const GlobalFrame gf{f};
    const FrameOps<GlobalFrame> o{gf, (uint32_t)(reinterpret_cast<uint64_t>(f) & 1u)};
    // Ethernet view (ethernet.rs:355-361) or the raw IP packet at ip_offset
    uint32_t L = 14, family = 0;
    if (opt_flags & NEXG_PARSE_FROM_IP) {
        L = ip_offset;
        const uint32_t v = L < len ? (uint32_t)f[L] >> 4 : 0u;
        family = v == 4u ? 4u : (v == 6u ? 6u : 0u);
    } else if (len >= 14u) {
        const uint32_t et = o.be16(12);
        family = et == 0x0800u ? 4u : (et == 0x86DDu ? 6u : 0u);
    }
    const uint32_t n = family && L < len ? len - L : 0u;
    uint32_t P = 0, m = 0, proto = 0;
    uint64_t pseudo = 0;
    bool l4 = false;
    if (family == 4u && n >= 20u) {
        // MutableIpv4Packet::new (ipv4.rs:540-566)
        const uint32_t hl = ((uint32_t)f[L] & 15u) * 4u, total = o.be16(L + 2);
        if (hl >= 20u && hl <= n && (total == 0u || total >= hl)) {
            if (which & NEXG_FIX_IP) {  // util::checksum(raw[..header_len], 5)
                const uint32_t c = fold_complement(o.wsum(L, L + 10) + o.wsum(L + 12, L + hl));
                put_be16(f + L + 10, c);
                fx.done |= NEXG_FIX_IP;
                fx.ip_csum = (uint16_t)c;
            }
            const uint32_t eff = total == 0u ? n : (total < n ? total : n);  // total_len, ipv4.rs:697-704
            P = L + hl;
            m = eff - hl;
            proto = f[L + 9];
            pseudo = (uint64_t)o.be16(L + 12) + o.be16(L + 14) + o.be16(L + 16) + o.be16(L + 18);
            l4 = proto == 17u || proto == 6u || proto == 1u;
        }
    } else if (family == 6u && n >= 40u) {  // MutableIpv6Packet::new: >= 40 B, payload = rest
        P = L + 40;
        m = n - 40u;
        proto = f[L + 6];
#pragma unroll
        for (uint32_t k = 0; k < 32; k += 2) pseudo += o.be16(L + 8 + k);
        l4 = proto == 17u || proto == 6u || proto == 58u;
    }
    if (l4 && (which & NEXG_FIX_L4)) {
        uint32_t sk = 0;  // byte offset of the checksum word (skipword * 2)
        bool view = false;
        if (proto == 17u) {  // MutableUdpPacket::new (udp.rs:101-121)
            const uint32_t ul = m >= 8u ? o.be16(P + 4) : 0u;
            view = m >= 8u && (ul == 0u || (ul >= 8u && ul <= m));
            sk = 6;
        } else if (proto == 6u) {  // MutableTcpPacket::new (tcp.rs:857-876)
            const uint32_t hl = m >= 20u ? ((uint32_t)f[P + 12] >> 4) * 4u : 0u;
            view = m >= 20u && hl >= 20u && hl <= m;
            sk = 16;
        } else {  // ICMP / ICMPv6: IcmpPacket::from_buf needs the 8-B header (icmp.rs:188-191)
            view = m >= 8u;
            sk = 2;
        }
        if (view) {
            uint64_t t = o.wsum(P, P + sk) + o.wsum(P + sk + 2u, P + m);
            if (proto != 1u) t += pseudo + proto + m;  // util.rs:89-97 / 119-127 (len as one u32)
            const uint32_t c = fold_complement(t);
            put_be16(f + P + sk, c);
            fx.done |= NEXG_FIX_L4;
            fx.proto = (uint8_t)proto;
            fx.l4_csum = (uint16_t)c;
            fx.l4_off = (uint16_t)P;
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
