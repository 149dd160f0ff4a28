// encap_core.hpp — the per-frame core of nexg_encap_plan / nexg_encap_frames
// (k_encap_*, nexg_encap.hip): the outer Ethernet / IP / UDP + VXLAN or GRE
// header the reference's builders give (EthernetPacketBuilder(Ipv4PacketBuilder
// or Ipv6PacketBuilder(UdpPacketBuilder(VxlanPacket::to_bytes))), GrePacket::
// to_bytes for GRE) in front of a copy of the inner frame. include/nexg.h is
// the specification. The kernels run it on gfx950; the test-only host driver
// (tests/native/encap_fuzz.cpp) runs the very same code on the CPU, one call
// per lane.
//
// A frame belongs to a group of kEncapLanes lanes. Its output is cut into the
// aligned 16-B chunks of out_data that overlap [out_offsets[i], out_offsets[i
// + 1]); lane l owns chunks l, l + 16, ... of the frame. A chunk's 16 bytes
// are the OR of two parts, each built from aligned dwords funnel-shifted to
// the chunk's phase: the header part from the spec's template with the
// per-frame fields patched in, and the payload part from the inner frame.
// The chunks that hold header bytes (the frame's first three to six) are kept
// in their lanes' registers until the UDP checksum, summed from the very
// dwords that feed the copy, has been reduced across the group; every other
// chunk leaves as soon as it is assembled.
#pragma once

#include <string.h>

#include "frame_core.hpp"

namespace nexg {

constexpr uint32_t kEncapLanes = 16;       // lanes per frame: a quarter wave
constexpr uint32_t kEncapHdrDwords = 20;   // 80 B >= the longest header (VXLAN over IPv6: 70 B)
constexpr uint32_t kEncapPatches = 5;
constexpr uint32_t kEncapMaxPad = 15;      // zero bytes written behind a frame, at most

// EncapTpl.meta >> 8
constexpr uint32_t kEncVxlan = 1u, kEncCsum = 2u, kEncFlowPort = 4u, kEncL3 = 8u, kEncV4 = 16u;

// nullptr when nexg_tunnels_check would accept the set, else what is wrong with it
inline const char* check_tunnels(const nexg_tunnels* s) {
    if (!s) return "NULL tunnel set";
    if (s->n_tunnels == 0 || s->n_tunnels > NEXG_ENCAP_MAX_TUNNELS) return "n_tunnels must be 1..16";
    if (s->reserved != 0) return "reserved must be 0";
    const uint32_t vx = NEXG_ENCAP_UDP_CSUM | NEXG_ENCAP_FLOW_PORT;
    const uint32_t gre = NEXG_ENCAP_GRE_KEY | NEXG_ENCAP_GRE_SEQ | NEXG_ENCAP_GRE_L3;
    for (uint32_t i = 0; i < s->n_tunnels; i++) {
        const nexg_tunnel_spec& t = s->tunnels[i];
        if (t.kind != NEXG_ENCAP_VXLAN && t.kind != NEXG_ENCAP_GRE) return "kind must be VXLAN or GRE";
        if (t.family != 4 && t.family != 6) return "family must be 4 or 6";
        if (t.flags & ~(vx | gre)) return "unknown flag bits";
        if (t.kind == NEXG_ENCAP_VXLAN && (t.flags & gre)) return "a GRE flag on a VXLAN spec";
        if (t.kind == NEXG_ENCAP_GRE && (t.flags & vx)) return "a VXLAN flag on a GRE spec";
        if (t.kind == NEXG_ENCAP_VXLAN && t.id > 0xFFFFFFu) return "a VXLAN id above 24 bits";
        if (t.flow_label > 0xFFFFFu) return "flow_label above 20 bits";
        if (t.ip_flags > 7) return "ip_flags above 7";
        if (t.flags & NEXG_ENCAP_FLOW_PORT) {
            if (t.port_span == 0 || (uint32_t)t.src_port + t.port_span > 65536u) return "FLOW_PORT needs 1 <= port_span <= 65536 - src_port";
        } else if (t.port_span != 0) {
            return "port_span without FLOW_PORT";
        }
        for (uint32_t k = 0; k < sizeof(t.reserved); k++)
            if (t.reserved[k]) return "reserved must be 0";
    }
    return nullptr;
}

// A spec as the kernel takes it: the header's bytes as little-endian dwords
// with the per-frame fields zero, and where those fields go. Patch p is a
// big-endian u16 at the even byte position pos[p] (0xFF: none):
//   0  IPv4 total length / IPv6 payload length = len_base + m
//   1  IPv4 header checksum = ~fold(ip_sum + total length): RFC 1624's update
//      of the template's checksum for the one word that changes
//   2  VXLAN: UDP source port                GRE: protocol_type under GRE_L3
//   3  VXLAN: UDP length = 16 + m            GRE: sequence, high half
//   4  VXLAN: UDP checksum                   GRE: sequence, low half
struct EncapTpl {  // 32 dwords
    uint32_t hdr[kEncapHdrDwords];
    uint32_t meta;       // H | kEnc* << 8 | len_base << 16
    uint32_t pos03;      // pos[0..3], a byte each
    uint32_t pos4;       // pos[4]
    uint32_t ip_sum;     // folded sum of the IPv4 header's words with total length and checksum 0
    uint32_t udp_sum;    // folded sum of the pseudo-header's addresses, 17, dst_port and the VXLAN header
    uint32_t src_port, port_span, seq_base;
    uint32_t pad[4];
};
struct EncapSet {
    uint32_t n, pad[3];
    EncapTpl t[NEXG_ENCAP_MAX_TUNNELS];
};
static_assert(sizeof(EncapTpl) == 128 && sizeof(EncapSet) == 16 + 16 * 128, "EncapTpl is 32 dwords");

NEXG_HD uint32_t fold16(uint32_t s) {
    s = (s & 0xFFFFu) + (s >> 16);
    return (s & 0xFFFFu) + (s >> 16);
}

// `set` has passed check_tunnels
inline void prepare_tunnels(const nexg_tunnels& set, EncapSet& out) {
    memset(&out, 0, sizeof(out));
    out.n = set.n_tunnels;
    for (uint32_t i = 0; i < set.n_tunnels; i++) {
        const nexg_tunnel_spec& s = set.tunnels[i];
        EncapTpl& T = out.t[i];
        uint8_t h[4 * kEncapHdrDwords] = {0};
        uint8_t pos[kEncapPatches] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF};
        const bool v4 = s.family == 4, vx = s.kind == NEXG_ENCAP_VXLAN;
        const uint32_t proto = vx ? 17u : 47u;
        memcpy(h, s.eth_dst, 6);
        memcpy(h + 6, s.eth_src, 6);
        h[12] = v4 ? 0x08 : 0x86;
        h[13] = v4 ? 0x00 : 0xDD;
        uint32_t L4, addr_sum = 0;
        if (v4) {
            uint8_t* ip = h + 14;
            ip[0] = 0x45;
            ip[1] = s.tos;
            ip[4] = (uint8_t)(s.ip_id >> 8);
            ip[5] = (uint8_t)s.ip_id;
            ip[6] = (uint8_t)(s.ip_flags << 5);
            ip[8] = s.ttl;
            ip[9] = (uint8_t)proto;
            memcpy(ip + 12, s.src, 4);
            memcpy(ip + 16, s.dst, 4);
            uint32_t sum = 0;
            for (uint32_t k = 0; k < 20; k += 2) sum += (uint32_t)ip[k] << 8 | ip[k + 1];
            T.ip_sum = fold16(sum);
            for (uint32_t k = 12; k < 20; k += 2) addr_sum += (uint32_t)ip[k] << 8 | ip[k + 1];
            pos[0] = 16;
            pos[1] = 24;
            L4 = 34;
        } else {
            uint8_t* ip = h + 14;
            ip[0] = (uint8_t)(0x60 | s.tos >> 4);
            ip[1] = (uint8_t)((s.tos & 15u) << 4 | s.flow_label >> 16);
            ip[2] = (uint8_t)(s.flow_label >> 8);
            ip[3] = (uint8_t)s.flow_label;
            ip[6] = (uint8_t)proto;
            ip[7] = s.ttl;
            memcpy(ip + 8, s.src, 16);
            memcpy(ip + 24, s.dst, 16);
            for (uint32_t k = 8; k < 40; k += 2) addr_sum += (uint32_t)ip[k] << 8 | ip[k + 1];
            pos[0] = 18;
            L4 = 54;
        }
        uint32_t H, flags = v4 ? kEncV4 : 0u;
        if (vx) {
            const uint32_t dport = s.dst_port ? s.dst_port : 4789u;
            uint8_t* u = h + L4;
            u[2] = (uint8_t)(dport >> 8);
            u[3] = (uint8_t)dport;
            u[8] = 0x08;  // VxlanPacket: flags 0x08, reserved1 0, the vni, reserved2 0
            u[12] = (uint8_t)(s.id >> 16);
            u[13] = (uint8_t)(s.id >> 8);
            u[14] = (uint8_t)s.id;
            T.udp_sum = fold16(addr_sum + 17u + dport + 0x0800u + (s.id >> 8) + ((s.id & 0xFFu) << 8));
            pos[2] = (uint8_t)L4;
            pos[3] = (uint8_t)(L4 + 4);
            pos[4] = (uint8_t)(L4 + 6);
            H = L4 + 16;
            flags |= kEncVxlan;
            if (s.flags & NEXG_ENCAP_UDP_CSUM) flags |= kEncCsum;
            if (s.flags & NEXG_ENCAP_FLOW_PORT) flags |= kEncFlowPort;
        } else {
            const bool K = s.flags & NEXG_ENCAP_GRE_KEY, S = s.flags & NEXG_ENCAP_GRE_SEQ;
            uint8_t* g = h + L4;
            g[0] = (uint8_t)((K ? 0x20 : 0) | (S ? 0x10 : 0));
            if (s.flags & NEXG_ENCAP_GRE_L3) {
                flags |= kEncL3;
                pos[2] = (uint8_t)(L4 + 2);
            } else {
                g[2] = 0x65;
                g[3] = 0x58;
            }
            H = L4 + 4;
            if (K) {
                h[H] = (uint8_t)(s.id >> 24);
                h[H + 1] = (uint8_t)(s.id >> 16);
                h[H + 2] = (uint8_t)(s.id >> 8);
                h[H + 3] = (uint8_t)s.id;
                H += 4;
            }
            if (S) {
                pos[3] = (uint8_t)H;
                pos[4] = (uint8_t)(H + 2);
                H += 4;
            }
        }
        for (uint32_t k = 0; k < kEncapHdrDwords; k++)
            T.hdr[k] = (uint32_t)h[4 * k] | (uint32_t)h[4 * k + 1] << 8 | (uint32_t)h[4 * k + 2] << 16 | (uint32_t)h[4 * k + 3] << 24;
        T.meta = H | flags << 8 | (H - (v4 ? 14u : 54u)) << 16;
        T.pos03 = (uint32_t)pos[0] | (uint32_t)pos[1] << 8 | (uint32_t)pos[2] << 16 | (uint32_t)pos[3] << 24;
        T.pos4 = pos[4];
        T.src_port = s.src_port;
        T.port_span = s.port_span;
        T.seq_base = s.seq_base;
    }
}

// Rules 1-3 of include/nexg.h for one frame. `spec`: the frame has a spec
// (t < n_tunnels) whose EncapTpl.meta is `meta`; `ext`: frame_extent accepted
// the frame.
struct EncapShape {
    uint32_t status, H, skip, m;  // H header bytes, then inner bytes [skip, skip + m); both 0 on an error
};
NEXG_HD EncapShape encap_shape(bool spec, uint32_t meta, bool ext, uint32_t len) {
    if (!ext) return {NEXG_ERR_BAD_EXTENT, 0u, 0u, 0u};
    if (!spec) return {NEXG_FRAME_OK, 0u, 0u, len};
    const uint32_t H = meta & 0xFFu;
    const bool l3 = ((meta >> 8) & kEncL3) != 0u;
    if (l3 && len < 14u) return {NEXG_ERR_BUFFER_TOO_SHORT, 0u, 0u, 0u};
    const uint32_t skip = l3 ? 14u : 0u, m = len - skip;
    if (H + m > 65535u) return {NEXG_ERR_INVALID_LENGTH, 0u, 0u, 0u};
    return {NEXG_FRAME_OK, H, skip, m};
}

// v_alignbyte_b32: bytes sh .. sh + 3 of the eight bytes lo, hi
NEXG_HD uint32_t align_bytes(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * (sh & 3u)));
#endif
}

// which of the four bytes at positions p .. p + 3 lie in [lo, hi), a byte of ones each
NEXG_HD uint32_t bytes_in(int32_t p, int32_t lo, int32_t hi) {
    uint32_t m = 0;
#pragma unroll
    for (int32_t b = 0; b < 4; b++)
        if (p + b >= lo && p + b < hi) m |= 0xFFu << (8 * b);
    return m;
}

// One frame's values, the same in every lane of its group.
struct EncapFrame {
    uint32_t H, m;        // H header bytes, then m payload bytes
    uint64_t S;           // address of payload byte 0
    uint64_t lo, hi;      // the bytes of out_data this frame may store: [lo, hi)
    const uint32_t* hdr;  // the spec's template: dword k at hdr[k] (LDS on the device); unused when H == 0
    uint32_t pos03, pos4;
    uint32_t val[kEncapPatches];
    uint32_t csum_at;     // the patch the UDP checksum goes into after the reduction: 4, or kEncapPatches for none
};

// the frame's chunks: chunk c is the aligned 16 bytes of out_data at 16 * ((lo >> 4) + c)
NEXG_HD uint32_t encap_chunks(const EncapFrame& x) {
    return x.hi > x.lo ? (uint32_t)(((x.hi + 15u) >> 4) - (x.lo >> 4)) : 0u;
}
// chunks [0, encap_header_chunks) hold header bytes
NEXG_HD uint32_t encap_header_chunks(const EncapFrame& x) {
    return x.H ? (((uint32_t)x.lo & 15u) + x.H + 15u) >> 4 : 0u;
}
// frame byte (header first) at byte 0 of chunk c: -15 .. for chunk 0
NEXG_HD int32_t encap_chunk_q(const EncapFrame& x, uint32_t c) { return (int32_t)(16u * c) - (int32_t)((uint32_t)x.lo & 15u); }

// The payload part of the chunk whose byte 0 is frame byte q0: inner bytes as
// the covering aligned dwords, byte-aligned in registers, bytes outside the
// payload zero. Every dword loaded holds a payload byte, so the loads stay
// inside the inner frame's own 16-B blocks. A chunk whole inside the payload
// (encap_payload_whole, no branch) takes one 16-B load from a 4-B aligned
// address and one dword.
NEXG_HD void encap_payload_whole(const EncapFrame& x, int32_t q0, uint32_t (&w)[4]) {
    const uint64_t A = x.S + (uint32_t)(q0 - (int32_t)x.H);  // q0 >= H here
    const uint32_t sh = (uint32_t)A & 3u;
    const void* A4 = reinterpret_cast<const void*>(A & ~3ull);
    const u32x4a4 v = __builtin_nontemporal_load(NEXG_GLOBAL(u32x4a4, A4));
    // off phase the dword behind the four holds the chunk's last bytes; on phase it is not looked at: the fourth again
    const uint32_t d4 = NEXG_GLOBAL(uint32_t, A4)[sh ? 4 : 3];
    w[0] = align_bytes(v.y, v.x, sh);
    w[1] = align_bytes(v.z, v.y, sh);
    w[2] = align_bytes(v.w, v.z, sh);
    w[3] = align_bytes(d4, v.w, sh);
}

NEXG_HD void encap_payload(const EncapFrame& x, int32_t q0, uint32_t (&w)[4]) {
    const int32_t a = q0 - (int32_t)x.H, m = (int32_t)x.m;  // payload byte at chunk byte 0
    // no payload byte in the chunk. (m == 0 is said on its own: an empty range [S, S) still has a dword around
    // S, and S is nothing to load from when the frame has no payload: a bad extent, an error status)
    if (m <= 0 || a >= m || a + 16 <= 0) {
        w[0] = w[1] = w[2] = w[3] = 0u;
        return;
    }
    if (a >= 0 && a + 16 <= m) return encap_payload_whole(x, q0, w);
    const uint64_t A = x.S + (uint64_t)(int64_t)a;
    const uint32_t sh = (uint32_t)A & 3u;
    const uint64_t A4 = A & ~3ull;
    uint32_t d[5];
    const uint64_t E = x.S + x.m;
#pragma unroll
    for (uint32_t k = 0; k < 5; k++) {
        const uint64_t at = A4 + 4u * k;
        d[k] = at + 4u > x.S && at < E ? NEXG_GLOBAL(uint32_t, reinterpret_cast<const void*>(at))[0] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) w[j] = align_bytes(d[j + 1], d[j], sh) & bytes_in(a + 4 * (int32_t)j, 0, m);
}

// little-endian halfword sum of a chunk's payload part
NEXG_HD uint32_t encap_le_sum(const uint32_t (&w)[4], uint32_t acc) {
    return halves_acc(w[3], halves_acc(w[2], halves_acc(w[1], halves_acc(w[0], acc))));
}

// dword k of the frame's header: the template's with the patches in it; 0 outside the template
NEXG_HD uint32_t encap_header_dword(const EncapFrame& x, int32_t k) {
    if (k < 0 || k >= (int32_t)kEncapHdrDwords) return 0u;
    uint32_t v = x.hdr[k];
#pragma unroll
    for (uint32_t p = 0; p < kEncapPatches; p++) {
        const uint32_t pos = p < 4u ? (x.pos03 >> (8u * p)) & 0xFFu : x.pos4 & 0xFFu;
        const uint32_t be = ((x.val[p] >> 8) & 0xFFu) | ((x.val[p] & 0xFFu) << 8);
        if ((int32_t)(pos >> 2) == k) v |= be << (8u * (pos & 2u));
    }
    return v;
}

// The header part of the chunk whose byte 0 is frame byte q0 (template bytes
// past H are zero, as are the bytes in front of the frame).
NEXG_HD void encap_header(const EncapFrame& x, int32_t q0, uint32_t (&w)[4]) {
    const int32_t k0 = q0 >> 2;  // floor: q0 may be -15 .. -1 for chunk 0
    const uint32_t sh = (uint32_t)q0 & 3u;
    uint32_t d[5];
#pragma unroll
    for (int32_t k = 0; k < 5; k++) d[k] = encap_header_dword(x, k0 + k);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) w[j] = align_bytes(d[j + 1], d[j], sh);
}

// Chunk c leaves: one aligned non-temporal 16-B store when it lies whole
// inside [lo, hi), else byte stores of the frame's own bytes only.
NEXG_HD void encap_store(const EncapFrame& x, uint8_t* out_data, uint32_t c, const uint32_t (&w)[4]) {
    const uint64_t at = ((x.lo >> 4) + c) << 4;
    if (at >= x.lo && at + 16u <= x.hi) {
        __builtin_nontemporal_store(u32x4{w[0], w[1], w[2], w[3]}, reinterpret_cast<u32x4*>(out_data + at));
        return;
    }
#pragma unroll
    for (uint32_t b = 0; b < 16; b++)
        if (at + b >= x.lo && at + b < x.hi) out_data[at + b] = (uint8_t)(w[b >> 2] >> (8u * (b & 3u)));
}

// A lane's state between the copy and the header: the payload part of the
// header chunk it holds, and its share of the payload's sum.
struct EncapLane {
    uint32_t held[4];
    uint32_t sum;  // little-endian halfword sum of every payload byte this lane copied or holds
};

// Lane `lane` of the frame's group: its chunks' payload parts are loaded,
// summed and, but for a header chunk (the lane's first, c = lane, when lane <
// encap_header_chunks), stored. Four chunks' loads are in flight per step.
NEXG_HD EncapLane encap_copy(const EncapFrame& x, uint8_t* out_data, uint32_t lane) {
    EncapLane L{{0u, 0u, 0u, 0u}, 0u};
    const uint32_t n = encap_chunks(x), nh = encap_header_chunks(x);
    uint32_t c = lane;
    if (c < n && c < nh) {
        encap_payload(x, encap_chunk_q(x, c), L.held);
        L.sum = encap_le_sum(L.held, 0u);
        c += kEncapLanes;
    }
    for (; c + 3u * kEncapLanes < n; c += 4u * kEncapLanes) {
        uint32_t w[4][4];
        const int32_t q = encap_chunk_q(x, c);
        if (q >= (int32_t)x.H && q + (int32_t)(48u * kEncapLanes) + 16 <= (int32_t)(x.H + x.m)) {  // all four whole inside the payload
#pragma unroll
            for (uint32_t u = 0; u < 4; u++) encap_payload_whole(x, q + (int32_t)(16u * u * kEncapLanes), w[u]);
        } else {
#pragma unroll
            for (uint32_t u = 0; u < 4; u++) encap_payload(x, q + (int32_t)(16u * u * kEncapLanes), w[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            L.sum = encap_le_sum(w[u], L.sum);
            encap_store(x, out_data, c + u * kEncapLanes, w[u]);
        }
    }
    for (; c < n; c += kEncapLanes) {
        uint32_t w[4];
        encap_payload(x, encap_chunk_q(x, c), w);
        L.sum = encap_le_sum(w, L.sum);
        encap_store(x, out_data, c, w);
    }
    return L;
}

// udp::checksum from the group's payload sum (the lanes' EncapLane.sum added
// up): the words start at payload byte 0, which sits at output byte lo + H, so
// the chunks' little-endian halfwords are the checksum's words when that
// address is odd and the byte-swapped words (x 256 mod 0xFFFF) when it is even.
NEXG_HD uint32_t encap_udp_checksum(const EncapFrame& x, uint32_t udp_sum, uint32_t src_port, uint64_t group_sum) {
    uint32_t s = fold16((uint32_t)(group_sum & 0xFFFFFFFFull) + (uint32_t)(group_sum >> 32));
    s = fold16(s);
    if ((((uint32_t)x.lo + x.H) & 1u) == 0u) s = fold16(s << 8);
    const uint32_t udp_len = 16u + x.m;
    return ~fold16(fold16(udp_sum + src_port + s) + fold16(2u * udp_len)) & 0xFFFFu;
}

// The lane's header chunk leaves (lane < encap_header_chunks): header part OR
// the payload part held. x.val holds every patch by now.
NEXG_HD void encap_finish(const EncapFrame& x, uint8_t* out_data, uint32_t lane, const EncapLane& L) {
    if (lane >= encap_header_chunks(x) || lane >= encap_chunks(x)) return;
    uint32_t w[4];
    encap_header(x, encap_chunk_q(x, lane), w);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) w[j] |= L.held[j];
    encap_store(x, out_data, lane, w);
}

// The inner frame's bytes 12..13 as a big-endian u16 (A: the address of byte
// 12), from the one or two aligned dwords that hold them.
NEXG_HD uint32_t encap_ethertype(uint64_t A) {
    const uint32_t sh = (uint32_t)A & 3u;
    const auto* dw = NEXG_GLOBAL(uint32_t, reinterpret_cast<const void*>(A & ~3ull));
    const uint32_t d0 = dw[0], d1 = sh == 3u ? dw[1] : 0u;
    const uint32_t v = align_bytes(d1, d0, sh);
    return ((v & 0xFFu) << 8) | ((v >> 8) & 0xFFu);
}

// The output bytes a frame may store, [lo, hi): from its offset to the next
// frame's (both caller memory), no further than its own length and
// kEncapMaxPad pad bytes, and below out_cap.
NEXG_HD void encap_range(uint64_t lo, uint64_t next, uint64_t out_cap, const EncapShape& sh, EncapFrame& x) {
    x.lo = x.hi = lo;
    if (lo < out_cap && next > lo) {
        const uint64_t end = lo + sh.H + sh.m + kEncapMaxPad;
        x.hi = next < end ? next : end;
        if (x.hi > out_cap) x.hi = out_cap;
    }
}

// The frame's values from its spec and shape. flow_hash: flows[i].hash (read
// by the caller only under kEncFlowPort); et: the inner frame's bytes 12..13
// as a big-endian u16 (read only under kEncL3); index: i. The row's src_port
// is set; its l4_csum follows from encap_udp_checksum.
NEXG_HD void encap_frame_values(const EncapTpl& T, const uint32_t* hdr, const EncapShape& sh, uint32_t flow_hash,
                                uint32_t et, uint32_t index, EncapFrame& x, nexg_encapped& row) {
    const uint32_t flags = (T.meta >> 8) & 0xFFu, len_base = T.meta >> 16;
    x.hdr = hdr;
    x.pos03 = T.pos03;
    x.pos4 = T.pos4;
    const uint32_t ip_len = len_base + sh.m;
    x.val[0] = ip_len;
    x.val[1] = (flags & kEncV4) ? ~fold16(T.ip_sum + ip_len) & 0xFFFFu : 0u;
    x.csum_at = kEncapPatches;
    if (flags & kEncVxlan) {
        const uint32_t port = T.src_port + ((flags & kEncFlowPort) ? flow_hash % T.port_span : 0u);
        x.val[2] = port;
        x.val[3] = 16u + sh.m;
        x.val[4] = 0u;
        if (flags & kEncCsum) x.csum_at = 4u;
        row.src_port = (uint16_t)port;
    } else {
        const uint32_t seq = T.seq_base + index;
        x.val[2] = (flags & kEncL3) ? et : 0u;
        x.val[3] = seq >> 16;
        x.val[4] = seq & 0xFFFFu;
    }
}

// Everything the fill reads for one frame before it looks at frame bytes.
struct EncapJob {
    bool live, ext;        // the frame is in the table; frame_extent accepted its extent
    uint32_t t, len;       // its tunnel number (0 without an index) and length (0 unless ext)
    uint32_t index;        // i
    uint64_t src;          // the address of frame byte 0: looked at only when ext
    uint64_t lo, next;     // out_offsets[i], out_offsets[i + 1]
};

// One lane's whole part in frame i (k_encap_frames' body; the host driver calls
// it lane by lane): rules 1-3, the row, the output range, the spec's values,
// the lane's chunks, the checksum and the lane's header chunk. tpl: the set's
// n templates (LDS on the device). flow_hash() gives flows[i].hash and is
// called only for a spec with kEncFlowPort; reduce(v) gives the sum of v over
// the frame's lanes and is called by every lane once. Returns the frame's row
// (the same in every lane). Frame bytes are read only of a frame with ext set.
template <class Hash, class Reduce>
NEXG_HD nexg_encapped encap_group_lane(const EncapTpl* tpl, uint32_t n, const EncapJob& j, uint64_t out_cap,
                                       uint8_t* out_data, uint32_t lane, Hash flow_hash, Reduce reduce) {
    const bool spec = j.live && j.t < n;  // the index is caller memory: it never reaches past the set
    const EncapTpl& T = tpl[spec ? j.t : 0u];
    const EncapShape sh = encap_shape(spec, T.meta, j.live && j.ext, j.len);
    const uint32_t flags = (T.meta >> 8) & 0xFFu;
    nexg_encapped row{(uint8_t)sh.status, (uint8_t)(spec || !j.ext ? j.t : NEXG_TUNNEL_NONE), (uint8_t)sh.H, 0, 0, 0};
    EncapFrame x{};
    x.H = sh.H;
    x.m = sh.m;
    x.S = j.ext ? j.src + sh.skip : 0u;  // a rejected extent's offset is any number: no address is made of it
    if (j.live) encap_range(j.lo, j.next, out_cap, sh, x);
    x.pos03 = 0xFFFFFFFFu;
    x.pos4 = 0xFFu;
    x.csum_at = kEncapPatches;
    if (spec && sh.status == NEXG_FRAME_OK) {
        uint32_t hash = 0, et = 0;
        if (flags & kEncFlowPort) hash = flow_hash();
        if (flags & kEncL3) et = encap_ethertype(j.src + 12u);
        encap_frame_values(T, T.hdr, sh, hash, et, j.index, x, row);
    }
    const EncapLane L = encap_copy(x, out_data, lane);
    const uint32_t sum = reduce(L.sum);  // a lane's is below 2^28: the group's fits
    if (x.csum_at < kEncapPatches) {
        const uint32_t c = encap_udp_checksum(x, T.udp_sum, x.val[2], sum);
        x.val[4] = c;
        row.l4_csum = (uint16_t)c;
    }
    encap_finish(x, out_data, lane, L);
    return row;
}

}  // namespace nexg
