/*
 * nexg.hpp — C++17 host API above the C ABI (include/nexg.h), mirroring
 * nex-packet's frame API for code that called the reference from a compiled
 * language (the reference is Rust; cargo is absent here, so this is the host
 * side a C++ caller links against, INTEGRATION.md gives the Rust binding).
 *
 * Names, field meanings and error behaviour follow the reference:
 *   ParseMode / ParseOption / ParseError   parse.rs:34-97, frame.rs:47-50
 *   Frame, DatalinkLayer, IpLayer, TransportLayer   frame.rs:21-60
 *   EthernetHeader ethernet.rs:152-160, ArpHeader arp.rs:300-311,
 *   Ipv4Header ipv4.rs:187-202 (+ Ipv4OptionPacket ipv4.rs:39-182),
 *   Ipv6Header ipv6.rs:14-23, IcmpHeader icmp.rs:172-176,
 *   Icmpv6Header icmpv6.rs:229-234, TcpHeader tcp.rs:482-494
 *   (+ TcpOptionPacket tcp.rs:33-476), UdpHeader udp.rs:22-27
 *   Engine::try_from_bufs   Frame::try_from_buf_with_mode (frame.rs:309) on a
 *                           batch: one Result<Frame, ParseError> per frame
 *   Engine::frame_slices    FrameSlice::try_from_buf (frame.rs:86) on a batch
 *   Engine::build_udp_ping  UdpPacketBuilder -> Ipv4PacketBuilder ->
 *                           EthernetPacketBuilder (udp_ping.rs:68-109) per
 *                           tuple, Result<frames, BuildError>
 *   Engine::build_tcp_ping / build_icmp_ping   tcp_ping.rs:111-163 /
 *                           icmp_ping.rs:67-102 (IPv4 or IPv6 per batch)
 *   Engine::dns / dns_entries / dns_bufs   DnsPacket::try_from_buf
 *                           (dns.rs:1166-1259) on every UDP payload of a batch;
 *                           decode_dns_name   dns.rs:1303-1390 (on the host)
 *   Filter, Engine::select / gather_plan / gather / gather_rows / select_bufs
 *                           no reference counterpart (an extension): frames
 *                           picked by rules over the parsed fields, and the
 *                           gather of their bytes and rows (include/nexg.h)
 *   PatternSet, Engine::match / match_select / match_bufs
 *                           no reference counterpart (an extension): up to 32
 *                           byte strings looked for in every frame's payload,
 *                           and the frames picked by what was found
 *   Action, ActionSet, Engine::rewrite / rewrite_bufs
 *                           the mutable views' setters under
 *                           ChecksumMode::Automatic (MutableEthernetPacket,
 *                           MutableIpv4Packet, MutableIpv6Packet, MutableTcpPacket,
 *                           MutableUdpPacket; examples/mutable_chaining.rs) on
 *                           a batch in place, one action per filter rule
 *   Tunnel, TunnelSet, Engine::encap_plan / encap / encap_bufs
 *                           VxlanPacket::to_bytes (vxlan.rs:73-84) and
 *                           GrePacket::to_bytes (gre.rs:115-160) inside the
 *                           Ethernet / IP / UDP builders, around every frame
 *                           of a batch, one tunnel per filter rule
 *   FragOption, Engine::fragment_plan / fragment / fragment_bufs
 *                           RFC 791 fragmentation to an MTU: each piece the
 *                           bytes Ipv4PacketBuilder gives for its fields
 *                           (Ipv4Flags, fragment_offset, ipv4::checksum)
 *   Engine::reassemble_plan / reassemble / reassemble_held / reassemble_bufs
 *                           no reference counterpart: the way back, IPv4
 *                           fragments sorted into datagrams, every complete
 *                           one an output frame, the rest reported as held
 *   FlowOption, Engine::flow / flow_partition / flow_bufs
 *                           no reference counterpart (an extension): the
 *                           Toeplitz RSS hash of every frame's flow key and the
 *                           stable split of a batch into flow-affine buckets
 *   FlowGroup, Engine::flow_sort / flow_groups / flow_group_bufs
 *                           per-flow counters (an extension): the batch sorted
 *                           by flow hash and reduced to one row per flow
 *   FlowEntry, Engine::flow_table_merge / flow_table_bufs
 *                           the flow table across batches (an extension): a
 *                           batch's flow rows merged into a table sorted by hash
 * The device does the parse and the checksums (nexg_parse_batch,
 * NEXG_OUT_RECORD) and the option lists (nexg_decode_options); this header
 * only reads header fields out of the frame bytes at the offsets the device
 * reported. API misuse and HIP failures throw nexg::Error; per-frame parse
 * failures are data (Result), as in the reference. Header-only; link
 * libnexg.so and amdhip64.
 */
#ifndef NEXG_HPP
#define NEXG_HPP

#include <hip/hip_runtime.h>

#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "nexg.h"

namespace nexg {

/* ---- parse knobs and errors ------------------------------------------- */

enum class ParseMode { Lenient, Strict };  // parse.rs:34-46

struct ParseOption {  // frame.rs:47-50 (+ the NEXG_PARSE_VLAN extension, off by default)
    bool from_ip_packet = false;
    size_t offset = 0;
    bool unwrap_vlan = false;
    uint32_t flags(ParseMode mode) const {
        return (from_ip_packet ? NEXG_PARSE_FROM_IP : 0u) | (unwrap_vlan ? NEXG_PARSE_VLAN : 0u) |
               (mode == ParseMode::Strict ? NEXG_PARSE_STRICT : 0u);
    }
};

enum class ParseErrorKind : uint8_t {  // parse.rs:51-97
    BufferTooShort = NEXG_ERR_BUFFER_TOO_SHORT,
    InvalidLength = NEXG_ERR_INVALID_LENGTH,
    Malformed = NEXG_ERR_MALFORMED,
    Truncated = NEXG_ERR_TRUNCATED,
    BadExtent = NEXG_ERR_BAD_EXTENT,  // caller error: frame longer than 65535 bytes
};

// The reference's ParseError with its payload (parse.rs:53-81), carried in
// the failed frame's record (include/nexg.h NEXG_CTX_*): `context` is the
// reference's context string; minimum / actual (BufferTooShort), value
// (InvalidLength), expected / actual (Truncated).
struct ParseError {
    ParseErrorKind kind;
    const char* context = nullptr;
    size_t minimum = 0, actual = 0, value = 0, expected = 0;
    const char* name() const {
        switch (kind) {
            case ParseErrorKind::BufferTooShort: return "BufferTooShort";
            case ParseErrorKind::InvalidLength: return "InvalidLength";
            case ParseErrorKind::Malformed: return "Malformed";
            case ParseErrorKind::Truncated: return "Truncated";
            default: return "BadExtent";
        }
    }
    static const char* context_of(uint32_t ctx) {
        static const char* const k[] = {nullptr, "Ethernet packet", "Frame dummy Ethernet classification",
                                        "IPv4 packet", "IPv4 packet version", "IPv4 header length", "IPv4 header",
                                        "IPv4 total length", "IPv4 options", "IPv4 option length", "IPv6 packet",
                                        "IPv6 packet version", "IPv6 payload", "IPv6 extension header",
                                        "IPv6 routing header", "IPv6 fragment header"};
        return ctx < sizeof(k) / sizeof(k[0]) ? k[ctx] : nullptr;
    }
    // the error of a failed frame's NEXG_OUT_RECORD record
    static ParseError from_record(const nexg_record& r) {
        ParseError e{(ParseErrorKind)NEXG_STATUS(r.flags)};
        if (e.kind == ParseErrorKind::BadExtent) return e;
        e.context = context_of(r.l4_type);
        if (e.kind == ParseErrorKind::BufferTooShort) { e.minimum = r.ip_src; e.actual = r.ip_dst; }
        if (e.kind == ParseErrorKind::InvalidLength) e.value = r.ip_src;
        if (e.kind == ParseErrorKind::Truncated) { e.expected = r.ip_src; e.actual = r.ip_dst; }
        return e;
    }
};

enum class BuildError { LengthOverflow, AddressFamilyMismatch, InvalidFieldLength };  // builder/error.rs:6-53

// Result<T, E>, as the reference's parse (ParseError) and build (BuildError)
// functions return
template <class T, class E = ParseError>
class Result {
   public:
    Result(T v) : v_(std::move(v)) {}
    Result(E e) : v_(e) {}
    bool is_ok() const { return v_.index() == 0; }
    bool is_err() const { return v_.index() == 1; }
    const T& value() const { return std::get<0>(v_); }
    T& value() { return std::get<0>(v_); }
    const E& error() const { return std::get<1>(v_); }

   private:
    std::variant<T, E> v_;
};

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

/* ---- DNS names ---------------------------------------------------------- */

// A decoded DNS name and the bytes it took at `start`
struct DnsNameDecoded {
    std::string name;
    size_t consumed = 0;
};

// decode_dns_name (dns.rs:1303-1390) over buf[0, n) from `start`: labels
// joined with '.', compression pointers followed inside buf (a target seen
// before, or more than 16 jumps: CompressionLoop; a target at or past n:
// InvalidCompression), label types 0x40 / 0x80 InvalidCompression, labels
// checked as UTF-8. The error is the ParseError variant's name. Names are
// decoded on the host from the offsets the nexg_dns_entry rows carry
// (Engine::dns / dns_entries): a query's over its qname bytes alone.
inline Result<DnsNameDecoded, const char*> decode_dns_name(const uint8_t* buf, size_t n, size_t start = 0) {
    auto utf8 = [](const uint8_t* p, size_t len) {  // what str::from_utf8 accepts
        for (size_t i = 0; i < len;) {
            const uint8_t c = p[i];
            size_t k;
            uint32_t cp;
            if (c < 0x80) { i++; continue; }
            if (c >= 0xC2 && c <= 0xDF) k = 1, cp = c & 0x1Fu;
            else if (c >= 0xE0 && c <= 0xEF) k = 2, cp = c & 0x0Fu;
            else if (c >= 0xF0 && c <= 0xF4) k = 3, cp = c & 0x07u;
            else return false;
            if (i + k >= len) return false;
            for (size_t j = 1; j <= k; j++) {
                if ((p[i + j] & 0xC0) != 0x80) return false;
                cp = (cp << 6) | (p[i + j] & 0x3Fu);
            }
            if ((k == 2 && (cp < 0x800 || (cp >= 0xD800 && cp <= 0xDFFF))) || (k == 3 && (cp < 0x10000 || cp > 0x10FFFF)))
                return false;
            i += k + 1;
        }
        return true;
    };
    DnsNameDecoded out;
    std::vector<size_t> visited;
    size_t pos = start, depth = 0;
    bool jumped = false, first = true;
    for (;;) {
        if (pos >= n) return "Truncated";
        const uint8_t len = buf[pos];
        if (!jumped) out.consumed++;
        if (len == 0) break;
        if ((len & 0xC0) == 0xC0) {
            if (pos + 1 >= n) return "Truncated";
            const size_t pointer = ((size_t)(len & 0x3F) << 8) | buf[pos + 1];
            if (pointer >= n) return "InvalidCompression";
            for (size_t v : visited)
                if (v == pointer) return "CompressionLoop";
            visited.push_back(pointer);
            if (++depth > 16) return "CompressionLoop";
            if (!jumped) out.consumed++;
            pos = pointer;
            jumped = true;
            continue;
        }
        if (len & 0xC0) return "InvalidCompression";
        pos++;
        if (pos + len > n) return "Truncated";
        if (!utf8(buf + pos, len)) return "InvalidUtf8";
        if (!first) out.name += '.';
        first = false;
        out.name.append(reinterpret_cast<const char*>(buf + pos), len);
        if (!jumped) out.consumed += len;
        pos += len;
    }
    return out;
}

/* ---- addresses and headers -------------------------------------------- */

using MacAddr = std::array<uint8_t, 6>;

struct Ipv4Addr {
    std::array<uint8_t, 4> octets{};
    std::string to_string() const {
        char b[16];
        snprintf(b, sizeof(b), "%u.%u.%u.%u", octets[0], octets[1], octets[2], octets[3]);
        return b;
    }
    bool operator==(const Ipv4Addr& o) const { return octets == o.octets; }
};

struct Ipv6Addr {
    std::array<uint8_t, 16> octets{};
    bool operator==(const Ipv6Addr& o) const { return octets == o.octets; }
};

struct EthernetHeader {  // ethernet.rs:152-160
    MacAddr destination{}, source{};
    uint16_t ethertype = 0;  // EtherType::value()
};

struct ArpHeader {  // arp.rs:300-311
    uint16_t hardware_type = 0, protocol_type = 0;
    uint8_t hw_addr_len = 0, proto_addr_len = 0;
    uint16_t operation = 0;
    MacAddr sender_hw_addr{};
    Ipv4Addr sender_proto_addr;
    MacAddr target_hw_addr{};
    Ipv4Addr target_proto_addr;
};

struct Ipv4OptionHeader {  // ipv4.rs:39-182
    uint8_t copied = 0, class_ = 0, number = 0;  // number = Ipv4OptionType::value()
    std::optional<uint8_t> length;
};
struct Ipv4OptionPacket {
    Ipv4OptionHeader header;
    std::vector<uint8_t> data;
};

struct Ipv4Header {  // ipv4.rs:187-202
    uint8_t version = 4, header_length = 0, dscp = 0, ecn = 0;
    uint16_t total_length = 0, identification = 0;
    uint8_t flags = 0;
    uint16_t fragment_offset = 0;
    uint8_t ttl = 0;
    uint8_t next_level_protocol = 0;  // IpNextProtocol::value() (143..=252 -> 255, Q8)
    uint16_t checksum = 0;
    Ipv4Addr source, destination;
    std::vector<Ipv4OptionPacket> options;
};

struct Ipv6Header {  // ipv6.rs:14-23
    uint8_t version = 6, traffic_class = 0;
    uint32_t flow_label = 0;
    uint16_t payload_length = 0;
    uint8_t next_header = 0;  // raw byte 6 (Q10)
    uint8_t hop_limit = 0;
    Ipv6Addr source, destination;
};

struct IcmpHeader {  // icmp.rs:172-176
    uint8_t icmp_type = 0, icmp_code = 0;
    uint16_t checksum = 0;
};
struct Icmpv6Header {  // icmpv6.rs:229-234
    uint8_t icmpv6_type = 0, icmpv6_code = 0;
    uint16_t checksum = 0;
};

struct TcpOptionPacket {  // tcp.rs:33-476
    uint8_t kind = 0;
    std::optional<uint8_t> length;
    std::vector<uint8_t> data;
};

struct TcpHeader {  // tcp.rs:482-494
    uint16_t source = 0, destination = 0;
    uint32_t sequence = 0, acknowledgement = 0;
    uint8_t data_offset = 0, reserved = 0, flags = 0;
    uint16_t window = 0, checksum = 0, urgent_ptr = 0;
    std::vector<TcpOptionPacket> options;
};

struct UdpHeader {  // udp.rs:22-27
    uint16_t source = 0, destination = 0, length = 0, checksum = 0;
};

struct DatalinkLayer {
    std::optional<EthernetHeader> ethernet;
    std::optional<ArpHeader> arp;
};
struct IpLayer {
    std::optional<Ipv4Header> ipv4;
    std::optional<Ipv6Header> ipv6;
    std::optional<IcmpHeader> icmp;
    std::optional<Icmpv6Header> icmpv6;
};
struct TransportLayer {
    std::optional<TcpHeader> tcp;
    std::optional<UdpHeader> udp;
};

// What the engine adds to the Frame path: the packet-API verification
// checksums (DESIGN.md §1 "Verify semantics")
struct Checksums {
    bool ip_checked = false, ip_ok = false, ip_panic = false, l4_checked = false, l4_ok = false;
    uint16_t ip_computed = 0, l4_computed = 0;
};

struct Frame {  // frame.rs:54-60
    std::optional<DatalinkLayer> datalink;
    std::optional<IpLayer> ip;
    std::optional<TransportLayer> transport;
    std::vector<uint8_t> payload;
    size_t packet_len = 0;
    Checksums checksums;
};

// FrameSlice (frame.rs:62-83): layer boundaries borrowed from the input frame
struct Bytes {
    const uint8_t* data = nullptr;
    size_t len = 0;
    std::vector<uint8_t> to_vec() const { return std::vector<uint8_t>(data, data + len); }
};
struct FrameSlice {
    Bytes packet;
    std::optional<Bytes> datalink, network, transport;
    Bytes payload;
    std::optional<uint16_t> ethertype;
    std::optional<uint8_t> ip_protocol;
};

inline Result<FrameSlice> frame_slice_from(const nexg_slice& s, const uint8_t* b, size_t len) {
    if (NEXG_STATUS(s.flags)) return ParseError{(ParseErrorKind)NEXG_STATUS(s.flags)};
    FrameSlice fs;
    fs.packet = Bytes{b, len};
    if (s.flags & NEXG_S_DATALINK) fs.datalink = Bytes{b, 14};
    if (s.flags & NEXG_S_NETWORK) fs.network = Bytes{b + s.l3_off, s.l3_len};
    if (s.flags & NEXG_S_TRANSPORT) fs.transport = Bytes{b + s.l3_off + s.l3_len, s.l4_len};
    fs.payload = Bytes{b + s.payload_off, s.payload_len};
    if (s.flags & NEXG_S_ETHERTYPE) fs.ethertype = s.ethertype;
    if (s.flags & NEXG_S_IP_PROTOCOL) fs.ip_protocol = (uint8_t)(s.flags >> NEXG_S_PROTO_SHIFT);
    return fs;
}

// The udp_ping frame shape (examples/udp_ping.rs:68-109): UdpPacketBuilder ->
// Ipv4PacketBuilder -> EthernetPacketBuilder, one frame per tuple
struct UdpPingTuple {
    Ipv4Addr source, destination;
    uint16_t src_port = 0, dst_port = 0, ip_id = 0;
};
struct UdpPingShape {
    MacAddr src_mac{}, dst_mac{};
    uint8_t ttl = 64;       // Ipv4PacketBuilder default (builder/ipv4.rs:37)
    uint8_t ip_flags = 2;   // udp_ping sets DontFragment
    std::vector<uint8_t> payload;
};

// An IPv4 or IPv6 address for the builders (std::net::IpAddr)
struct IpAddr {
    uint8_t family = 4;                // 4 or 6
    std::array<uint8_t, 16> octets{};  // IPv4 in the first 4 bytes
    static IpAddr from(const Ipv4Addr& a) {
        IpAddr r;
        memcpy(r.octets.data(), a.octets.data(), 4);
        return r;
    }
    static IpAddr from(const Ipv6Addr& a) {
        IpAddr r;
        r.family = 6;
        r.octets = a.octets;
        return r;
    }
};

// tcp_ping's frame (examples/tcp_ping.rs:111-163): TcpPacketBuilder ->
// Ipv4/Ipv6PacketBuilder -> EthernetPacketBuilder
struct TcpPingTuple {
    IpAddr source, destination;
    uint16_t src_port = 0, dst_port = 0, ip_id = 0;
    uint32_t sequence = 0, acknowledgement = 0;
};
struct TcpPingShape {
    MacAddr src_mac{}, dst_mac{};
    uint8_t ttl = 64, ip_flags = 2, tos = 0;
    uint32_t flow_label = 0;
    uint8_t flags = 0x02;  // SYN
    uint16_t window = 0xffff, urgent_ptr = 0;
    std::vector<uint8_t> options;  // encoded TcpOptionPacket bytes (padded to 4 B on the wire)
    std::vector<uint8_t> payload;
};

// icmp_ping's frame (examples/icmp_ping.rs:67-102): an echo request
// (IcmpPacketBuilder / Icmpv6PacketBuilder with echo_fields)
struct IcmpPingTuple {
    IpAddr source, destination;
    uint16_t identifier = 0, sequence = 0, ip_id = 0;
};
struct IcmpPingShape {
    MacAddr src_mac{}, dst_mac{};
    uint8_t ttl = 64, ip_flags = 2, tos = 0;
    uint32_t flow_label = 0;
    std::vector<uint8_t> payload;
};

// arp.rs's request (examples/arp.rs:59-67): ArpPacketBuilder::new(sender_mac,
// sender_ip, target) behind a broadcast EthernetPacketBuilder
struct ArpProbeShape {
    MacAddr sender_mac{};
    Ipv4Addr sender_ip{};
    MacAddr eth_dst{{0xff, 0xff, 0xff, 0xff, 0xff, 0xff}};
    uint16_t operation = 1;  // ArpOperation::Request
    uint8_t hw_addr_len = 6, proto_addr_len = 4;  // build() accepts only 6 / 4
};
// ndp.rs's solicitation (examples/ndp.rs:82-108): NdpPacketBuilder::new(src_mac,
// src_ip, target) inside Ipv6PacketBuilder (hop limit 255) and Ethernet to
// 33:33 + the target's last four bytes
struct NdpProbeShape {
    MacAddr src_mac{};
    Ipv6Addr src_ip{};
    uint8_t hop_limit = 255;
};

/* ---- materialisation from a device record ------------------------------ */

namespace detail {
inline uint16_t be16(const uint8_t* p) { return (uint16_t)((p[0] << 8) | p[1]); }
inline Ipv4Addr v4(uint32_t be_value) {
    return Ipv4Addr{{(uint8_t)(be_value >> 24), (uint8_t)(be_value >> 16), (uint8_t)(be_value >> 8),
                     (uint8_t)be_value}};
}
inline MacAddr mac(const uint8_t* p) {
    MacAddr m;
    memcpy(m.data(), p, 6);
    return m;
}
inline Ipv4OptionPacket ipv4_option_at(const uint8_t* p) {
    Ipv4OptionPacket o;
    o.header.copied = (p[0] >> 7) & 1;
    o.header.class_ = (p[0] >> 5) & 3;
    o.header.number = p[0] & 0x1F;
    if (o.header.number > 1) {
        o.header.length = p[1];
        o.data.assign(p + 2, p + p[1]);
    }
    return o;
}
inline TcpOptionPacket tcp_option_at(const uint8_t* p) {
    TcpOptionPacket o;
    o.kind = p[0];
    if (o.kind > 1) {
        o.length = p[1];
        o.data.assign(p + 2, p + p[1]);
    }
    return o;
}
}  // namespace detail

// Frame from one NEXG_OUT_RECORD record, the frame bytes and (for the option
// lists) the frame's nexg_options. Mirrors nex_amd/frame.py::frame_from_record.
inline Result<Frame> frame_from_record(const nexg_record& r, const uint8_t* b, size_t len,
                                       const nexg_options& opts) {
    using namespace detail;
    const uint32_t f = r.flags;
    if (NEXG_STATUS(f)) return ParseError::from_record(r);
    if (r.payload_off + (size_t)r.payload_len > len || r.l3_off > len) throw Error("record does not fit its frame");
    Frame fr;
    const uint32_t l3 = r.l3_off;
    if (f & NEXG_L_ETHERNET) {
        DatalinkLayer dl;
        EthernetHeader eth;
        eth.ethertype = r.ethertype;
        // a real Ethernet header unless from_ip_packet fabricated one (frame.rs:396-400)
        if ((f & NEXG_L_VLAN) || (l3 == 14 && be16(b + 12) == r.ethertype)) {
            eth.destination = mac(b);
            eth.source = mac(b + 6);
        }
        dl.ethernet = eth;
        if (f & NEXG_L_ARP) {
            ArpHeader a;
            const uint8_t* p = b + l3;
            a.hardware_type = be16(p);
            a.protocol_type = be16(p + 2);
            a.hw_addr_len = p[4];
            a.proto_addr_len = p[5];
            a.operation = be16(p + 6);
            a.sender_hw_addr = mac(p + 8);
            memcpy(a.sender_proto_addr.octets.data(), p + 14, 4);
            a.target_hw_addr = mac(p + 18);
            memcpy(a.target_proto_addr.octets.data(), p + 24, 4);
            dl.arp = a;
        }
        fr.datalink = dl;
    }
    if (f & NEXG_L_IP) {
        IpLayer ip;
        if (f & NEXG_L_IPV4) {
            Ipv4Header h;
            h.header_length = r.ip_ver_ihl & 15;
            h.dscp = r.ip_tos >> 2;
            h.ecn = r.ip_tos & 3;
            h.total_length = r.ip_length;
            h.identification = (uint16_t)(r.ip_word >> 16);
            h.flags = (r.ip_word >> 13) & 7;
            h.fragment_offset = r.ip_word & 0x1FFF;
            h.ttl = r.ip_ttl;
            h.next_level_protocol = r.ip_proto;
            h.checksum = r.ip_csum;
            h.source = v4(r.ip_src);
            h.destination = v4(r.ip_dst);
            for (int k = 0; k < opts.n_ip; k++) h.options.push_back(ipv4_option_at(b + opts.ip_opt_off + opts.ip_pos[k]));
            ip.ipv4 = std::move(h);
        }
        if (f & NEXG_L_IPV6) {
            Ipv6Header h;
            h.traffic_class = r.ip_tos;
            h.flow_label = r.ip_word;
            h.payload_length = r.ip_length;
            h.next_header = r.ip_proto;
            h.hop_limit = r.ip_ttl;
            memcpy(h.source.octets.data(), b + l3 + 8, 16);
            memcpy(h.destination.octets.data(), b + l3 + 24, 16);
            ip.ipv6 = h;
        }
        if (f & NEXG_L_ICMP) ip.icmp = IcmpHeader{r.l4_type, r.l4_code, r.l4_csum};
        if (f & NEXG_L_ICMPV6) ip.icmpv6 = Icmpv6Header{r.l4_type, r.l4_code, r.l4_csum};
        fr.ip = std::move(ip);
    }
    if (f & NEXG_L_TRANSPORT) {
        TransportLayer tp;
        if (f & NEXG_L_TCP) {
            TcpHeader h;
            h.source = r.src_port;
            h.destination = r.dst_port;
            h.sequence = r.tcp_seq;
            h.acknowledgement = r.tcp_ack;
            h.data_offset = r.l4_code >> 4;
            h.reserved = r.l4_code & 15;
            h.flags = r.l4_type;
            h.window = r.tcp_window;
            h.checksum = r.l4_csum;
            h.urgent_ptr = r.tcp_urg;
            for (int k = 0; k < opts.n_tcp; k++) h.options.push_back(tcp_option_at(b + opts.tcp_opt_off + opts.tcp_pos[k]));
            tp.tcp = std::move(h);
        }
        if (f & NEXG_L_UDP) tp.udp = UdpHeader{r.src_port, r.dst_port, r.l4_length, r.l4_csum};
        fr.transport = std::move(tp);
    }
    fr.payload.assign(b + r.payload_off, b + r.payload_off + r.payload_len);
    fr.packet_len = r.packet_len;
    fr.checksums = Checksums{(f & NEXG_C_IP_CHECKED) != 0, (f & NEXG_C_IP_OK) != 0, (f & NEXG_C_IP_PANIC) != 0,
                             (f & NEXG_C_L4_CHECKED) != 0, (f & NEXG_C_L4_OK) != 0, r.ip_csum_calc,
                             r.l4_csum_calc};
    return fr;
}

/* ---- ICMP sub-message views (icmp.rs:434-700, icmpv6.rs echo) ---------------
 * What examples/dump.rs:226-350 downcasts an IcmpPacket / Icmpv6Packet to.
 * The packet comes from a Frame (Frame.ip.icmp + Frame.payload, which for
 * ICMP is every byte after the 4-B header, Q15); each conversion applies the
 * reference's type check and minimum payload and fails with its message. */
struct IcmpPacket {  // icmp.rs:178-183
    IcmpHeader header;
    std::vector<uint8_t> payload;
    size_t total_len() const { return 4 + payload.size(); }  // icmp.rs:241-243
};
struct Icmpv6Packet {  // icmpv6.rs:236-241
    Icmpv6Header header;
    std::vector<uint8_t> payload;
    size_t total_len() const { return 4 + payload.size(); }
};
inline std::optional<IcmpPacket> icmp_packet(const Frame& f) {
    if (!f.ip || !f.ip->icmp) return std::nullopt;
    return IcmpPacket{*f.ip->icmp, f.payload};
}
inline std::optional<Icmpv6Packet> icmpv6_packet(const Frame& f) {
    if (!f.ip || !f.ip->icmpv6) return std::nullopt;
    return Icmpv6Packet{*f.ip->icmpv6, f.payload};
}
namespace icmp {
template <uint8_t TYPE>
struct EchoPacket {  // echo_request (icmp.rs:478-504) / echo_reply (icmp.rs:547-573)
    IcmpHeader header;
    uint16_t identifier = 0, sequence_number = 0;
    std::vector<uint8_t> payload;
    static Result<EchoPacket, const char*> try_from(const IcmpPacket& p) {
        if (p.header.icmp_type != TYPE) return TYPE == 8 ? "Not an Echo Request" : "Not an Echo Reply";
        if (p.payload.size() < 4) return TYPE == 8 ? "Payload too short for Echo Request" : "Payload too short for Echo Reply";
        return EchoPacket{p.header, detail::be16(p.payload.data()), detail::be16(p.payload.data() + 2),
                          std::vector<uint8_t>(p.payload.begin() + 4, p.payload.end())};
    }
};
using EchoRequestPacket = EchoPacket<8>;
using EchoReplyPacket = EchoPacket<0>;
struct DestinationUnreachablePacket {  // icmp.rs:618-647
    IcmpHeader header;
    uint16_t unused = 0, next_hop_mtu = 0;
    std::vector<uint8_t> payload;
    static Result<DestinationUnreachablePacket, const char*> try_from(const IcmpPacket& p) {
        if (p.header.icmp_type != 3) return "Not a Destination Unreachable";
        if (p.payload.size() < 4) return "Payload too short for Destination Unreachable";
        return DestinationUnreachablePacket{p.header, detail::be16(p.payload.data()), detail::be16(p.payload.data() + 2),
                                            std::vector<uint8_t>(p.payload.begin() + 4, p.payload.end())};
    }
};
struct TimeExceededPacket {  // icmp.rs:664-699
    IcmpHeader header;
    uint32_t unused = 0;
    std::vector<uint8_t> payload;
    static Result<TimeExceededPacket, const char*> try_from(const IcmpPacket& p) {
        if (p.header.icmp_type != 11) return "Not a Time Exceeded";
        if (p.payload.size() < 4) return "Payload too short for Time Exceeded";
        const uint32_t u = ((uint32_t)detail::be16(p.payload.data()) << 16) | detail::be16(p.payload.data() + 2);
        return TimeExceededPacket{p.header, u, std::vector<uint8_t>(p.payload.begin() + 4, p.payload.end())};
    }
};
}  // namespace icmp
namespace icmpv6 {
template <uint8_t TYPE>
struct EchoPacket {  // echo_request (icmpv6.rs:2268-2294) / echo_reply (2427-2453): 8-B minimum
    Icmpv6Header header;
    uint16_t identifier = 0, sequence_number = 0;
    std::vector<uint8_t> payload;
    static Result<EchoPacket, const char*> try_from(const Icmpv6Packet& p) {
        if (p.header.icmpv6_type != TYPE)
            return TYPE == 128 ? "Not an Echo Request packet" : "Not an Echo Reply packet";
        if (p.payload.size() < 8) return TYPE == 128 ? "Payload too short for Echo Request" : "Payload too short for Echo Reply";
        return EchoPacket{p.header, detail::be16(p.payload.data()), detail::be16(p.payload.data() + 2),
                          std::vector<uint8_t>(p.payload.begin() + 4, p.payload.end())};
    }
    size_t total_len() const { return 8 + payload.size(); }
};
using EchoRequestPacket = EchoPacket<128>;
using EchoReplyPacket = EchoPacket<129>;

/* Neighbor Discovery messages (icmpv6.rs ndp, 640-1901), both ways the
 * reference builds them: try_from(Icmpv6Packet) is the TryFrom conversion
 * dump.rs uses (fixed part read from the packet payload, options in 8-B
 * chunks), from_bytes(message) is Packet::try_from_buf over the whole ICMPv6
 * message (type byte first; options walked by their length field, the rest
 * kept as payload) as the reference's ndp_tests call it. Quirks kept: RS / RA
 * from_bytes need 24 B and panic in the reference on a length-0 option (an
 * error here), NS / NA / Redirect stop there; TryFrom for NS asks a 24-B and
 * for Redirect a 40-B payload although their fixed parts are 20 / 36 B. */
namespace ndp {
struct NdpOptionPacket {  // icmpv6.rs:776-857
    uint8_t option_type = 0;
    uint8_t length = 0;  // unit: 8 bytes
    std::vector<uint8_t> payload;
    static Result<NdpOptionPacket, const char*> from_bytes(const uint8_t* b, size_t n) {  // icmpv6.rs:784-810
        if (n < 2) return "Malformed";
        const size_t total = (size_t)b[1] * 8;
        if (n < total) return "Malformed";
        if (total < 2) return "NDP option of length 0 (the reference underflows)";
        return NdpOptionPacket{b[0], b[1], std::vector<uint8_t>(b + 2, b + total)};
    }
    void append_to(std::vector<uint8_t>& out) const {  // icmpv6.rs:817-823
        out.push_back(option_type);
        out.push_back(length);
        out.insert(out.end(), payload.begin(), payload.end());
    }
};
namespace detail_ndp {
inline Result<std::vector<NdpOptionPacket>, const char*> chunks(const std::vector<uint8_t>& p, size_t from) {
    std::vector<NdpOptionPacket> out;  // TryFrom: 8-B chunks, type = chunk[0], length = chunk[1]
    for (size_t k = from; k < p.size(); k += 8) {
        const size_t e = k + 8 < p.size() ? k + 8 : p.size();
        if (e - k < 2) return "NDP option chunk of 1 byte (the reference panics)";
        out.push_back(NdpOptionPacket{p[k], p[k + 1], std::vector<uint8_t>(p.begin() + k + 2, p.begin() + e)});
    }
    return out;
}
// try_from_buf option walk from byte i; the rest becomes `rest`
inline const char* walk(const uint8_t* b, size_t n, size_t i, bool stop_short, std::vector<NdpOptionPacket>& out,
                        std::vector<uint8_t>& rest) {
    while (i + 2 <= n) {
        const size_t ol = (size_t)b[i + 1] * 8;
        if (stop_short && ol < 2) break;
        if (i + ol > n) break;
        if (ol < 2) return "NDP option of length 0 (the reference panics)";
        out.push_back(NdpOptionPacket{b[i], b[i + 1], std::vector<uint8_t>(b + i + 2, b + i + ol)});
        i += ol;
    }
    rest.assign(b + i, b + n);
    return nullptr;
}
inline uint32_t be32(const uint8_t* p) { return ((uint32_t)detail::be16(p) << 16) | detail::be16(p + 2); }
inline Ipv6Addr v6(const uint8_t* p) {
    Ipv6Addr a;
    memcpy(a.octets.data(), p, 16);
    return a;
}
inline void head(std::vector<uint8_t>& o, const Icmpv6Header& h) {
    o.push_back(h.icmpv6_type);
    o.push_back(h.icmpv6_code);
    o.push_back((uint8_t)(h.checksum >> 8));
    o.push_back((uint8_t)h.checksum);
}
inline void put32(std::vector<uint8_t>& o, uint32_t v) {
    for (int k = 3; k >= 0; k--) o.push_back((uint8_t)(v >> (8 * k)));
}
inline Icmpv6Header hdr(const uint8_t* b) { return Icmpv6Header{b[0], b[1], detail::be16(b + 2)}; }
}  // namespace detail_ndp

struct RouterSolicitPacket {  // icmpv6.rs:872-1023
    Icmpv6Header header;
    uint32_t reserved = 0;
    std::vector<NdpOptionPacket> options;
    std::vector<uint8_t> payload;
    static Result<RouterSolicitPacket, const char*> try_from(const Icmpv6Packet& p) {
        if (p.header.icmpv6_type != 133) return "Not a Router Solicitation packet";
        if (p.payload.size() < 8) return "Payload too short for Router Solicitation";
        auto o = detail_ndp::chunks(p.payload, 4);
        if (o.is_err()) return o.error();
        return RouterSolicitPacket{p.header, detail_ndp::be32(p.payload.data()), o.value(), {}};
    }
    static Result<RouterSolicitPacket, const char*> from_bytes(const uint8_t* b, size_t n) {
        if (n < 24) return "Malformed";  // NDP_SOL_PACKET_LEN
        RouterSolicitPacket m{detail_ndp::hdr(b), detail_ndp::be32(b + 4), {}, {}};
        if (const char* e = detail_ndp::walk(b, n, 8, false, m.options, m.payload)) return e;
        return m;
    }
    std::vector<uint8_t> to_bytes() const {
        std::vector<uint8_t> o;
        detail_ndp::head(o, header);
        detail_ndp::put32(o, reserved);
        for (const auto& x : options) x.append_to(o);
        return o;
    }
    size_t total_len() const { return 8 + 4 + payload.size(); }
};

struct RouterAdvertPacket {  // icmpv6.rs:1055-1234
    Icmpv6Header header;
    uint8_t hop_limit = 0, flags = 0;
    uint16_t lifetime = 0;
    uint32_t reachable_time = 0, retrans_time = 0;
    std::vector<NdpOptionPacket> options;
    std::vector<uint8_t> payload;
    static Result<RouterAdvertPacket, const char*> try_from(const Icmpv6Packet& p) {
        if (p.header.icmpv6_type != 134) return "Not a Router Advertisement packet";
        if (p.payload.size() < 16) return "Payload too short for Router Advertisement";
        auto o = detail_ndp::chunks(p.payload, 12);
        if (o.is_err()) return o.error();
        const uint8_t* q = p.payload.data();
        return RouterAdvertPacket{p.header, q[0], q[1], detail::be16(q + 2), detail_ndp::be32(q + 4),
                                  detail_ndp::be32(q + 8), o.value(), {}};
    }
    static Result<RouterAdvertPacket, const char*> from_bytes(const uint8_t* b, size_t n) {
        if (n < 24) return "Malformed";  // NDP_ADV_PACKET_LEN
        RouterAdvertPacket m{detail_ndp::hdr(b), b[4], b[5], detail::be16(b + 6), detail_ndp::be32(b + 8),
                             detail_ndp::be32(b + 12), {}, {}};
        if (const char* e = detail_ndp::walk(b, n, 16, false, m.options, m.payload)) return e;
        return m;
    }
    std::vector<uint8_t> to_bytes() const {
        std::vector<uint8_t> o;
        detail_ndp::head(o, header);
        o.push_back(hop_limit);
        o.push_back(flags);
        o.push_back((uint8_t)(lifetime >> 8));
        o.push_back((uint8_t)lifetime);
        detail_ndp::put32(o, reachable_time);
        detail_ndp::put32(o, retrans_time);
        for (const auto& x : options) x.append_to(o);
        return o;
    }
    size_t total_len() const { return 8 + 16 + payload.size(); }
};

struct NeighborSolicitPacket {  // icmpv6.rs:1258-1434
    Icmpv6Header header;
    uint32_t reserved = 0;
    Ipv6Addr target_addr;
    std::vector<NdpOptionPacket> options;
    std::vector<uint8_t> payload;
    static Result<NeighborSolicitPacket, const char*> try_from(const Icmpv6Packet& p) {
        if (p.header.icmpv6_type != 135) return "Not a Neighbor Solicitation packet";
        if (p.payload.size() < 24) return "Payload too short for Neighbor Solicitation";
        auto o = detail_ndp::chunks(p.payload, 20);
        if (o.is_err()) return o.error();
        return NeighborSolicitPacket{p.header, detail_ndp::be32(p.payload.data()), detail_ndp::v6(p.payload.data() + 4),
                                     o.value(), {}};
    }
    static Result<NeighborSolicitPacket, const char*> from_bytes(const uint8_t* b, size_t n) {
        if (n < 24) return "Malformed";
        NeighborSolicitPacket m{detail_ndp::hdr(b), detail_ndp::be32(b + 4), detail_ndp::v6(b + 8), {}, {}};
        if (const char* e = detail_ndp::walk(b, n, 24, true, m.options, m.payload)) return e;
        return m;
    }
    std::vector<uint8_t> to_bytes() const {
        std::vector<uint8_t> o;
        detail_ndp::head(o, header);
        detail_ndp::put32(o, reserved);
        o.insert(o.end(), target_addr.octets.begin(), target_addr.octets.end());
        for (const auto& x : options) x.append_to(o);
        return o;
    }
    size_t total_len() const { return 8 + 24 + payload.size(); }
};

struct NeighborAdvertPacket {  // icmpv6.rs:1472-1664
    Icmpv6Header header;
    uint8_t flags = 0;
    uint32_t reserved = 0;  // u24be
    Ipv6Addr target_addr;
    std::vector<NdpOptionPacket> options;
    std::vector<uint8_t> payload;
    static Result<NeighborAdvertPacket, const char*> try_from(const Icmpv6Packet& p) {
        if (p.header.icmpv6_type != 136) return "Not a Neighbor Advert packet";
        if (p.payload.size() < 20) return "Payload too short for Neighbor Advert";
        auto o = detail_ndp::chunks(p.payload, 20);
        if (o.is_err()) return o.error();
        const uint8_t* q = p.payload.data();
        return NeighborAdvertPacket{p.header, q[0], detail_ndp::be32(q) & 0xFFFFFFu, detail_ndp::v6(q + 4), o.value(), {}};
    }
    static Result<NeighborAdvertPacket, const char*> from_bytes(const uint8_t* b, size_t n) {
        if (n < 24) return "Malformed";
        NeighborAdvertPacket m{detail_ndp::hdr(b), b[4], detail_ndp::be32(b + 4) & 0xFFFFFFu, detail_ndp::v6(b + 8), {}, {}};
        if (const char* e = detail_ndp::walk(b, n, 24, true, m.options, m.payload)) return e;
        return m;
    }
    std::vector<uint8_t> to_bytes() const {
        std::vector<uint8_t> o;
        detail_ndp::head(o, header);
        detail_ndp::put32(o, (uint32_t)flags << 24 | (reserved & 0xFFFFFFu));
        o.insert(o.end(), target_addr.octets.begin(), target_addr.octets.end());
        for (const auto& x : options) x.append_to(o);
        return o;
    }
    size_t total_len() const { return 8 + 24 + payload.size(); }
};

struct RedirectPacket {  // icmpv6.rs:1696-1901
    Icmpv6Header header;
    uint32_t reserved = 0;
    Ipv6Addr target_addr, dest_addr;
    std::vector<NdpOptionPacket> options;
    std::vector<uint8_t> payload;
    static Result<RedirectPacket, const char*> try_from(const Icmpv6Packet& p) {
        if (p.header.icmpv6_type != 137) return "Not a Redirect packet";
        if (p.payload.size() < 40) return "Payload too short for Redirect";
        auto o = detail_ndp::chunks(p.payload, 36);
        if (o.is_err()) return o.error();
        const uint8_t* q = p.payload.data();
        return RedirectPacket{p.header, detail_ndp::be32(q), detail_ndp::v6(q + 4), detail_ndp::v6(q + 20), o.value(), {}};
    }
    static Result<RedirectPacket, const char*> from_bytes(const uint8_t* b, size_t n) {
        if (n < 40) return "Malformed";
        RedirectPacket m{detail_ndp::hdr(b), detail_ndp::be32(b + 4), detail_ndp::v6(b + 8), detail_ndp::v6(b + 24), {}, {}};
        if (const char* e = detail_ndp::walk(b, n, 40, true, m.options, m.payload)) return e;
        return m;
    }
    std::vector<uint8_t> to_bytes() const {
        std::vector<uint8_t> o;
        detail_ndp::head(o, header);
        detail_ndp::put32(o, reserved);
        o.insert(o.end(), target_addr.octets.begin(), target_addr.octets.end());
        o.insert(o.end(), dest_addr.octets.begin(), dest_addr.octets.end());
        for (const auto& x : options) x.append_to(o);
        return o;
    }
    size_t total_len() const { return 8 + 40 + payload.size(); }
};

// The whole ICMPv6 message of a Frame's Icmpv6Packet (header + payload),
// what from_bytes takes
inline std::vector<uint8_t> message_bytes(const Icmpv6Packet& p) {
    std::vector<uint8_t> o;
    detail_ndp::head(o, p.header);
    o.insert(o.end(), p.payload.begin(), p.payload.end());
    return o;
}
}  // namespace ndp
}  // namespace icmpv6

/* ---- flow keys (extension: the reference has no flow notion) --------------- */

using FlowGroup = nexg_flow_group;  // one row of Engine::flow_groups (include/nexg.h)
using FlowEntry = nexg_flow_entry;  // one row of a flow table, Engine::flow_table_merge (include/nexg.h)

// nexg_flow_option (include/nexg.h): which key a frame's flow row hashes.
//   FlowOption().symmetric()        both directions of a conversation get one key
//   FlowOption().no_ports()         addresses only
//   FlowOption().key(bytes40)       a Toeplitz key other than the default RSS one
struct FlowOption {
    nexg_flow_option o{};
    FlowOption& symmetric(bool on = true) { return set(NEXG_FLOW_SYMMETRIC, on); }
    FlowOption& no_ports(bool on = true) { return set(NEXG_FLOW_NO_PORTS, on); }
    FlowOption& key(const std::array<uint8_t, 40>& k) {
        std::memcpy(o.key, k.data(), 40);
        return set(NEXG_FLOW_KEY, true);
    }
    const nexg_flow_option& get() const { return o; }

private:
    FlowOption& set(uint32_t bit, bool on) {
        o.flags = on ? o.flags | bit : o.flags & ~bit;
        return *this;
    }
};

/* ---- frame selection (extension: the reference has no filter) ------------- */

// Builder of a nexg_filter (include/nexg.h): any / flags / udp / tcp / status /
// bad_checksum_* append a rule; proto / *_port / length / *_net4 / *_net6 add a
// further test to the last rule. get() throws nexg::Error where
// nexg_select_batch would return NEXG_EINVAL.
//   Filter().tcp(0x12, 0x02).dst_net4({10, 0, 0, 0}, 8)      TCP SYNs to 10/8
//           .udp().any_port(53)                              or UDP port 53
//           .bad_checksum_l4()                               or a failed L4 checksum
class Filter {
   public:
    nexg_filter f{};

    Filter& rule(const nexg_rule& r) {
        if (f.n_rules >= NEXG_FILTER_MAX_RULES) throw Error("Filter: more than 16 rules");
        f.rules[f.n_rules++] = r;
        return *this;
    }
    Filter& any() { return rule(nexg_rule{}); }
    Filter& flags(uint32_t mask, uint32_t value) {
        nexg_rule r{};
        r.flags_mask = mask;
        r.flags_value = value;
        return rule(r);
    }
    Filter& udp() { return flags(NEXG_L_UDP, NEXG_L_UDP); }
    // TCP frames; tcp_mask != 0 adds (flags & tcp_mask) == tcp_value on the TCP flags byte
    Filter& tcp(uint8_t tcp_mask = 0, uint8_t tcp_value = 0) {
        flags(NEXG_L_TCP, NEXG_L_TCP);
        if (tcp_mask) {
            last().tests |= NEXG_RULE_TCP_FLAGS;
            last().tcp_mask = tcp_mask;
            last().tcp_value = tcp_value;
        }
        return *this;
    }
    Filter& status(uint32_t code) { return flags(7u << NEXG_STATUS_SHIFT, code << NEXG_STATUS_SHIFT); }
    Filter& bad_checksum_l4() { return flags(NEXG_C_L4_CHECKED | NEXG_C_L4_OK, NEXG_C_L4_CHECKED); }
    Filter& bad_checksum_ip() { return flags(NEXG_C_IP_CHECKED | NEXG_C_IP_OK, NEXG_C_IP_CHECKED); }
    Filter& invert(bool on = true) {
        f.flags = on ? NEXG_FILTER_INVERT : 0u;
        return *this;
    }
    // further tests on the last rule (a new match-all rule when there is none)
    Filter& proto(uint8_t p) {
        last().tests |= NEXG_RULE_PROTO;
        last().ip_proto = p;
        return *this;
    }
    Filter& any_port(uint16_t lo, uint16_t hi) {
        last().tests |= NEXG_RULE_ANY_PORT;
        last().sport_lo = lo;
        last().sport_hi = hi;
        return *this;
    }
    Filter& any_port(uint16_t p) { return any_port(p, p); }
    Filter& src_port(uint16_t lo, uint16_t hi) {
        last().tests |= NEXG_RULE_SRC_PORT;
        last().sport_lo = lo;
        last().sport_hi = hi;
        return *this;
    }
    Filter& dst_port(uint16_t lo, uint16_t hi) {
        last().tests |= NEXG_RULE_DST_PORT;
        last().dport_lo = lo;
        last().dport_hi = hi;
        return *this;
    }
    Filter& length(uint16_t lo, uint16_t hi) {
        last().tests |= NEXG_RULE_LENGTH;
        last().len_lo = lo;
        last().len_hi = hi;
        return *this;
    }
    Filter& src_net4(const std::array<uint8_t, 4>& a, uint8_t bits) { return addr(NEXG_RULE_SRC_ADDR, 4, a.data(), 4, bits); }
    Filter& dst_net4(const std::array<uint8_t, 4>& a, uint8_t bits) { return addr(NEXG_RULE_DST_ADDR, 4, a.data(), 4, bits); }
    Filter& any_net4(const std::array<uint8_t, 4>& a, uint8_t bits) { return addr(NEXG_RULE_ANY_ADDR, 4, a.data(), 4, bits); }
    Filter& src_net6(const std::array<uint8_t, 16>& a, uint8_t bits) { return addr(NEXG_RULE_SRC_ADDR, 6, a.data(), 16, bits); }
    Filter& dst_net6(const std::array<uint8_t, 16>& a, uint8_t bits) { return addr(NEXG_RULE_DST_ADDR, 6, a.data(), 16, bits); }
    Filter& any_net6(const std::array<uint8_t, 16>& a, uint8_t bits) { return addr(NEXG_RULE_ANY_ADDR, 6, a.data(), 16, bits); }

    // the filter, checked as nexg_select_batch checks it
    const nexg_filter& get() const {
        if (nexg_filter_check(&f) != NEXG_OK) throw Error("Filter: not a valid nexg_filter (include/nexg.h)");
        return f;
    }

   private:
    nexg_rule& last() {
        if (f.n_rules == 0) any();
        return f.rules[f.n_rules - 1];
    }
    Filter& addr(uint32_t test, uint8_t family, const uint8_t* a, size_t n, uint8_t bits) {
        nexg_rule& r = last();
        if ((r.tests & (NEXG_RULE_SRC_ADDR | NEXG_RULE_DST_ADDR | NEXG_RULE_ANY_ADDR)) && r.family != family)
            throw Error("Filter: address tests of two families in one rule");
        r.tests |= test;
        r.family = family;
        if (test == NEXG_RULE_DST_ADDR) {
            memcpy(r.dst, a, n);
            r.dst_bits = bits;
        } else {
            memcpy(r.src, a, n);
            r.src_bits = bits;
        }
        return *this;
    }
};

/* ---- fixed-string match on frame bytes (extension: the reference has no payload search) --- */

// Builder of a nexg_patterns (include/nexg.h): add / prefix / nocase append a
// pattern of 1..16 bytes; frame() searches the whole frame instead of
// Frame.payload. add throws nexg::Error for what cannot be stored, get()
// where nexg_match_batch would return NEXG_EINVAL.
//   PatternSet().prefix("\x16\x03", 2)                     payload starts with a TLS record
//               .nocase("Host: ", 6)                         "host: " anywhere, in any case
//               .add("\r\n\r\n", 4, 0, 16, 512)              starting at payload bytes 16..512
class PatternSet {
   public:
    nexg_patterns s{};

    PatternSet& add(const void* bytes, size_t len, uint8_t flags = 0, uint16_t off_lo = 0, uint16_t off_hi = 65535) {
        if (s.n_patterns >= NEXG_MATCH_MAX_PATTERNS) throw Error("PatternSet: more than 32 patterns");
        if (len == 0 || len > NEXG_MATCH_MAX_LEN) throw Error("PatternSet: a pattern is 1..16 bytes");
        nexg_pattern& p = s.pat[s.n_patterns++];
        memcpy(p.bytes, bytes, len);
        p.len = (uint8_t)len;
        p.flags = flags;
        p.off_lo = off_lo;
        p.off_hi = off_hi;
        return *this;
    }
    PatternSet& add(const std::string& bytes, uint8_t flags = 0, uint16_t off_lo = 0, uint16_t off_hi = 65535) {
        return add(bytes.data(), bytes.size(), flags, off_lo, off_hi);
    }
    PatternSet& prefix(const void* bytes, size_t len, uint8_t flags = 0) { return add(bytes, len, flags, 0, 0); }
    PatternSet& nocase(const void* bytes, size_t len, uint16_t off_lo = 0, uint16_t off_hi = 65535) {
        return add(bytes, len, NEXG_PAT_NOCASE, off_lo, off_hi);
    }
    PatternSet& frame(bool on = true) {
        s.flags = on ? NEXG_MATCH_FRAME : 0u;
        return *this;
    }

    // the set, checked as nexg_match_batch checks it
    const nexg_patterns& get() const {
        if (nexg_patterns_check(&s) != NEXG_OK) throw Error("PatternSet: not a valid nexg_patterns (include/nexg.h)");
        return s;
    }
};

/* ---- header rewrite (the mutable setters under ChecksumMode::Automatic) ---------- */

// Builder of one nexg_action (include/nexg.h): each call names a field and its
// value, as the reference's setters do one by one.
//   Action().nat4(src, dst).ports(40000, 443).dec_ttl(1)   NAT44 with ports, one hop
//   Action().mac(next_hop, mine).dec_ttl(1)                the router
//   Action()                                                leave it
class Action {
   public:
    nexg_action a{};

    Action& eth_dst(const uint8_t mac[6]) { return bytes(NEXG_SET_ETH_DST, a.eth_dst, mac, 6); }
    Action& eth_src(const uint8_t mac[6]) { return bytes(NEXG_SET_ETH_SRC, a.eth_src, mac, 6); }
    Action& mac(const uint8_t dst[6], const uint8_t src[6]) { return eth_dst(dst).eth_src(src); }
    // addresses in network order: 4 bytes (family 4) or 16 (family 6)
    Action& ip_src(uint8_t family, const uint8_t* addr) { return address(NEXG_SET_IP_SRC, a.src, family, addr); }
    Action& ip_dst(uint8_t family, const uint8_t* addr) { return address(NEXG_SET_IP_DST, a.dst, family, addr); }
    Action& nat4(const uint8_t src[4], const uint8_t dst[4]) { return ip_src(4, src).ip_dst(4, dst); }
    Action& nat6(const uint8_t src[16], const uint8_t dst[16]) { return ip_src(6, src).ip_dst(6, dst); }
    Action& src_port(uint16_t p) {
        a.sets |= NEXG_SET_SRC_PORT;
        a.src_port = p;
        return *this;
    }
    Action& dst_port(uint16_t p) {
        a.sets |= NEXG_SET_DST_PORT;
        a.dst_port = p;
        return *this;
    }
    Action& ports(uint16_t src, uint16_t dst) { return src_port(src).dst_port(dst); }
    Action& set_ttl(uint8_t ttl) {
        a.sets |= NEXG_SET_TTL;
        a.ttl = ttl;
        return *this;
    }
    Action& dec_ttl(uint8_t by = 1) {
        a.sets |= NEXG_DEC_TTL;
        a.ttl = by;
        return *this;
    }
    // (old & ~mask) | tos: mask 0xFC is set_dscp (tos = dscp << 2), mask 0x03 set_ecn
    Action& set_tos(uint8_t tos, uint8_t mask = 0xFF) {
        a.sets |= NEXG_SET_TOS;
        a.tos = tos;
        a.tos_mask = mask;
        return *this;
    }

   private:
    Action& bytes(uint32_t bit, uint8_t* to, const uint8_t* from, size_t n) {
        a.sets |= bit;
        memcpy(to, from, n);
        return *this;
    }
    Action& address(uint32_t bit, uint8_t* to, uint8_t family, const uint8_t* addr) {
        if (family != 4 && family != 6) throw Error("Action: an address family is 4 or 6");
        if (a.family && a.family != family) throw Error("Action: addresses of two families");
        a.family = family;
        memset(to, 0, 16);
        return bytes(bit, to, addr, family == 4 ? 4 : 16);
    }
};

// Builder of a nexg_actions: up to 16 actions; incremental() updates the stored
// checksums by RFC 1624 instead of recomputing them. add throws nexg::Error
// for the 17th action, get() where nexg_rewrite_batch would return NEXG_EINVAL.
class ActionSet {
   public:
    nexg_actions s{};

    ActionSet& add(const Action& action) {
        if (s.n_actions >= NEXG_REWRITE_MAX_ACTIONS) throw Error("ActionSet: more than 16 actions");
        s.actions[s.n_actions++] = action.a;
        return *this;
    }
    ActionSet& incremental(bool on = true) {
        s.flags = on ? NEXG_REWRITE_INCREMENTAL : 0u;
        return *this;
    }
    // the set, checked as nexg_rewrite_batch checks it
    const nexg_actions& get() const {
        if (nexg_actions_check(&s) != NEXG_OK) throw Error("ActionSet: not a valid nexg_actions (include/nexg.h)");
        return s;
    }
};

/* ---- tunnel encapsulation (VXLAN, GRE) ------------------------------------------- */

// Builder of one nexg_tunnel_spec (include/nexg.h). Addresses in network
// order: 4 bytes (family 4) or 16 (family 6).
//   Tunnel::vxlan(4, src, dst, 5001).macs(next_hop, mine).ports(49152, 0, 16384).udp_csum()
//   Tunnel::gre(6, src, dst).key(7).l3()
class Tunnel {
   public:
    nexg_tunnel_spec t{};

    static Tunnel vxlan(uint8_t family, const uint8_t* src, const uint8_t* dst, uint32_t vni) {
        Tunnel x(NEXG_ENCAP_VXLAN, family, src, dst);
        x.t.id = vni;
        return x;
    }
    static Tunnel gre(uint8_t family, const uint8_t* src, const uint8_t* dst) { return Tunnel(NEXG_ENCAP_GRE, family, src, dst); }
    Tunnel& macs(const uint8_t dst[6], const uint8_t src[6]) {
        memcpy(t.eth_dst, dst, 6);
        memcpy(t.eth_src, src, 6);
        return *this;
    }
    // VXLAN: the UDP ports (dst 0: 4789); span > 0: source port = src + flow hash % span (NEXG_ENCAP_FLOW_PORT)
    Tunnel& ports(uint16_t src, uint16_t dst = 0, uint16_t span = 0) {
        t.src_port = src;
        t.dst_port = dst;
        t.port_span = span;
        t.flags = span ? t.flags | NEXG_ENCAP_FLOW_PORT : t.flags & ~NEXG_ENCAP_FLOW_PORT;
        return *this;
    }
    Tunnel& udp_csum(bool on = true) { return flag(NEXG_ENCAP_UDP_CSUM, on); }
    Tunnel& key(uint32_t k) {
        t.id = k;
        return flag(NEXG_ENCAP_GRE_KEY, true);
    }
    Tunnel& sequence(uint32_t base) {
        t.seq_base = base;
        return flag(NEXG_ENCAP_GRE_SEQ, true);
    }
    Tunnel& l3(bool on = true) { return flag(NEXG_ENCAP_GRE_L3, on); }
    Tunnel& ip(uint8_t ttl, uint8_t tos = 0, uint16_t ip_id = 0, uint8_t ip_flags = 0, uint32_t flow_label = 0) {
        t.ttl = ttl;
        t.tos = tos;
        t.ip_id = ip_id;
        t.ip_flags = ip_flags;
        t.flow_label = flow_label;
        return *this;
    }

   private:
    Tunnel(uint8_t kind, uint8_t family, const uint8_t* src, const uint8_t* dst) {
        if (family != 4 && family != 6) throw Error("Tunnel: an address family is 4 or 6");
        t.kind = kind;
        t.family = family;
        t.ttl = 64;
        memcpy(t.src, src, family == 4 ? 4 : 16);
        memcpy(t.dst, dst, family == 4 ? 4 : 16);
    }
    Tunnel& flag(uint32_t bit, bool on) {
        t.flags = on ? t.flags | bit : t.flags & ~bit;
        return *this;
    }
};

// Builder of a nexg_tunnels: up to 16 specs. add throws nexg::Error for the
// 17th, get() where nexg_encap_plan would return NEXG_EINVAL.
class TunnelSet {
   public:
    nexg_tunnels s{};

    TunnelSet& add(const Tunnel& tunnel) {
        if (s.n_tunnels >= NEXG_ENCAP_MAX_TUNNELS) throw Error("TunnelSet: more than 16 tunnels");
        s.tunnels[s.n_tunnels++] = tunnel.t;
        return *this;
    }
    bool needs_flows() const {
        for (uint32_t i = 0; i < s.n_tunnels && i < NEXG_ENCAP_MAX_TUNNELS; i++)
            if (s.tunnels[i].flags & NEXG_ENCAP_FLOW_PORT) return true;
        return false;
    }
    // the set, checked as nexg_encap_plan checks it
    const nexg_tunnels& get() const {
        if (nexg_tunnels_check(&s) != NEXG_OK) throw Error("TunnelSet: not a valid nexg_tunnels (include/nexg.h)");
        return s;
    }
};

/* ---- IPv4 fragmentation to an MTU ------------------------------------------------ */

// Builder of a nexg_frag_option. get() throws nexg::Error where
// nexg_fragment_plan would return NEXG_EINVAL.
//   FragOption(1500).ignore_df().align(16)
class FragOption {
   public:
    nexg_frag_option o{};

    explicit FragOption(uint32_t mtu) {
        o.mtu = mtu;
        o.align = 1;
    }
    FragOption& ignore_df(bool on = true) {
        o.flags = on ? (o.flags | NEXG_FRAG_IGNORE_DF) : (o.flags & ~NEXG_FRAG_IGNORE_DF);
        return *this;
    }
    FragOption& align(uint32_t a) {
        o.align = a;
        return *this;
    }
    // the option, checked as nexg_fragment_plan checks it
    const nexg_frag_option& get() const {
        if (nexg_frag_option_check(&o) != NEXG_OK) throw Error("FragOption: not a valid nexg_frag_option (include/nexg.h)");
        return o;
    }
};

/* ---- the engine --------------------------------------------------------- */

// The calling thread's current device switched for a scope and restored after
// (Engine methods: scratch hipMalloc, copies and launches on the engine's device
// whatever device the caller has current).
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != d) {
            const hipError_t e = hipSetDevice(d);
            if (e != hipSuccess) throw Error(std::string("hipSetDevice: ") + hipGetErrorString(e));
        }
    }
    ~DeviceScope() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

class Engine {  // one nexg context on one gfx950 device, one stream
   public:
    explicit Engine(int device = 0) : device_(device) {
        DeviceScope ds(device);
        check(nexg_ctx_create(device, &ctx_), "nexg_ctx_create");
        check_hip(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    }
    ~Engine() {
        DeviceScope ds(device_);
        for (auto& b : scratch_) (void)hipFree(b.p);
        if (stream_) (void)hipStreamDestroy(stream_);
        if (ctx_) nexg_ctx_destroy(ctx_);
    }
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;

    nexg_ctx* ctx() const { return ctx_; }
    int device() const { return device_; }
    hipStream_t stream() const { return stream_; }

    // Device-resident batch (frames / out are device pointers), stream-ordered
    void parse(const nexg_frames& frames, ParseOption option, ParseMode mode, int out_kind, void* out) {
        DeviceScope ds(device_);
        const nexg_parse_option o{option.flags(mode), (uint32_t)option.offset};
        check(nexg_parse_batch(ctx_, &frames, &o, out_kind, out, stream_), "nexg_parse_batch");
    }

    // Tunnel decapsulation of a device-resident batch already parsed with
    // NEXG_OUT_RECORD (VxlanPacket::try_from_buf vxlan.rs:28-65,
    // GrePacket::try_from_buf gre.rs:32-107 on Frame.payload): tunnels /
    // inner_off / inner_len are device arrays of frames.count entries;
    // {frames.data, frames.data_bytes, inner_off, inner_len} is the inner batch
    void decap(const nexg_frames& frames, const nexg_record* records, nexg_tunnel* tunnels, uint64_t* inner_off,
               uint32_t* inner_len, uint32_t which = NEXG_DECAP_VXLAN | NEXG_DECAP_GRE, uint16_t vxlan_port = 4789) {
        DeviceScope ds(device_);
        const nexg_decap_option o{which, vxlan_port, 0};
        check(nexg_decap_batch(ctx_, &frames, records, &o, tunnels, inner_off, inner_len, stream_), "nexg_decap_batch");
    }

    // Order-preserving compaction of a decap result by inner class
    // (inner_mask: bits 1u << NEXG_INNER_*): device arrays of capacity `count`;
    // returns the number selected (one stream synchronisation). Parse the
    // selected table with the default option for NEXG_INNER_ETHERNET, with
    // ParseOption{from_ip_packet = true, offset = 0} for the IP classes.
    uint64_t decap_select(const nexg_tunnel* tunnels, const uint64_t* inner_off, const uint32_t* inner_len,
                          uint64_t count, uint32_t inner_mask, uint32_t* out_index, uint64_t* out_off,
                          uint32_t* out_len) {
        DeviceScope ds(device_);
        const uint64_t wsb = nexg_decap_select_workspace(count);
        void* ws = scratch(16, wsb);
        uint64_t* d_count = static_cast<uint64_t*>(scratch(17, 8));
        check(nexg_decap_select(ctx_, tunnels, inner_off, inner_len, count, inner_mask, out_index, out_off, out_len,
                                d_count, ws, wsb, stream_),
              "nexg_decap_select");
        return read_u64(d_count);
    }

    // The tunnel of every host frame: parse (NEXG_OUT_RECORD) + decap on the
    // device; inner_off is relative to the frame's first byte
    struct Decap {
        nexg_tunnel tunnel;
        uint32_t inner_off, inner_len;
    };
    std::vector<Decap> decap_bufs(const std::vector<std::vector<uint8_t>>& frames, ParseOption option = {},
                                  uint32_t which = NEXG_DECAP_VXLAN | NEXG_DECAP_GRE, uint16_t vxlan_port = 4789) {
        DeviceScope ds(device_);
        const uint64_t n = frames.size();
        std::vector<Decap> out(n);
        if (n == 0) return out;
        HostBatch hb(*this, frames);
        void* d_recs = scratch(3, n * 64);
        nexg_tunnel* d_tun = static_cast<nexg_tunnel*>(scratch(4, n * sizeof(nexg_tunnel)));
        uint64_t* d_off = static_cast<uint64_t*>(scratch(5, n * 8));
        uint32_t* d_len = static_cast<uint32_t*>(scratch(6, n * 4));
        parse(hb.fb, option, ParseMode::Lenient, NEXG_OUT_RECORD, d_recs);
        decap(hb.fb, static_cast<const nexg_record*>(d_recs), d_tun, d_off, d_len, which, vxlan_port);
        std::vector<nexg_tunnel> tun(n);
        std::vector<uint64_t> off(n);
        std::vector<uint32_t> len(n);
        check_hip(hipMemcpyAsync(tun.data(), d_tun, n * sizeof(nexg_tunnel), hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipMemcpyAsync(off.data(), d_off, n * 8, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipMemcpyAsync(len.data(), d_len, n * 4, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        for (uint64_t i = 0; i < n; i++) out[i] = Decap{tun[i], (uint32_t)(off[i] - hb.offs[i]), len[i]};
        return out;
    }

    // The DNS message pass over a device-resident batch already parsed with
    // NEXG_OUT_RECORD (DnsPacket::try_from_buf dns.rs:1166-1259 on
    // Frame.payload): `out` holds frames.count summaries, tile_first
    // nexg_dns_tile_first_bytes(frames.count) bytes; its last element is the
    // number of entries. any_udp: every UDP frame with a non-empty payload is
    // tried (dns_dump.rs:98-100), else those from or to `port`.
    void dns(const nexg_frames& frames, const nexg_record* records, nexg_dns* out, uint64_t* tile_first,
             uint16_t port = 53, bool any_udp = false) {
        DeviceScope ds(device_);
        const nexg_dns_option o{any_udp ? NEXG_DNS_ANY_UDP : 0u, port, 0};
        check(nexg_dns_batch(ctx_, &frames, records, &o, out, tile_first, stream_), "nexg_dns_batch");
    }

    // One nexg_dns_entry per query / resource record: the k-th entry of frame
    // i at tile_first[i >> 8] + dns[i].first + k; nothing at or past entries_cap
    void dns_entries(const nexg_frames& frames, const nexg_dns* dns, const uint64_t* tile_first,
                     nexg_dns_entry* entries, uint64_t entries_cap) {
        DeviceScope ds(device_);
        check(nexg_dns_entries(ctx_, &frames, dns, tile_first, entries, entries_cap, stream_), "nexg_dns_entries");
    }

    // The DNS message of every host frame: parse (NEXG_OUT_RECORD) + dns +
    // dns_entries on the device, sized exactly (one stream synchronisation
    // for the total); frame i's rows are entries[row[i], row[i + 1])
    struct DnsBatch {
        std::vector<nexg_dns> dns;
        std::vector<uint64_t> row;  // frames + 1
        std::vector<nexg_dns_entry> entries;
    };
    DnsBatch dns_bufs(const std::vector<std::vector<uint8_t>>& frames, ParseOption option = {}, uint16_t port = 53,
                      bool any_udp = false) {
        DeviceScope ds(device_);
        const uint64_t n = frames.size();
        DnsBatch out;
        out.row.assign(n + 1, 0);
        if (n == 0) return out;
        HostBatch hb(*this, frames);
        void* d_recs = scratch(3, n * 64);
        nexg_dns* d_dns = static_cast<nexg_dns*>(scratch(18, n * sizeof(nexg_dns)));
        const uint64_t tiles = (n + 255) / 256;
        uint64_t* d_tf = static_cast<uint64_t*>(scratch(19, nexg_dns_tile_first_bytes(n)));
        parse(hb.fb, option, ParseMode::Lenient, NEXG_OUT_RECORD, d_recs);
        dns(hb.fb, static_cast<const nexg_record*>(d_recs), d_dns, d_tf, port, any_udp);
        std::vector<uint64_t> tf(tiles + 1);
        out.dns.resize(n);
        check_hip(hipMemcpyAsync(tf.data(), d_tf, (tiles + 1) * 8, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipMemcpyAsync(out.dns.data(), d_dns, n * sizeof(nexg_dns), hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        const uint64_t total = tf[tiles];
        out.entries.resize(total);
        if (total) {
            nexg_dns_entry* d_ent = static_cast<nexg_dns_entry*>(scratch(20, total * sizeof(nexg_dns_entry)));
            dns_entries(hb.fb, d_dns, d_tf, d_ent, total);
            check_hip(hipMemcpyAsync(out.entries.data(), d_ent, total * sizeof(nexg_dns_entry), hipMemcpyDeviceToHost,
                                     stream_),
                      "D2H");
            check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        }
        for (uint64_t i = 0; i < n; i++) {
            const nexg_dns& s = out.dns[i];
            out.row[i] = tf[i >> 8] + s.first;
            out.row[i + 1] = out.row[i] + s.n_q + s.n_an + s.n_ns + s.n_ar;
        }
        return out;
    }

    // Order-preserving selection of the frames of a device-resident batch
    // already parsed with NEXG_OUT_RECORD that match `filter` (an extension,
    // include/nexg.h nexg_select_batch): device arrays of capacity
    // frames.count (out_rule may be null); returns the number selected (one
    // stream synchronisation). {frames.data, frames.data_bytes, out_off,
    // out_len, returned count} is the selected batch: parse, decap and dns
    // take it as it stands, with gather_rows(records, 64, ...) for its records.
    uint64_t select(const nexg_frames& frames, const nexg_record* records, const Filter& filter, uint32_t* out_index,
                    uint64_t* out_off, uint32_t* out_len, uint8_t* out_rule = nullptr) {
        DeviceScope ds(device_);
        const uint64_t wsb = nexg_select_workspace(frames.count);
        void* ws = scratch(21, wsb);
        uint64_t* d_count = static_cast<uint64_t*>(scratch(22, 8));
        check(nexg_select_batch(ctx_, &frames, records, &filter.get(), out_index, out_off, out_len, out_rule, d_count,
                                ws, wsb, stream_),
              "nexg_select_batch");
        return read_u64(d_count);
    }

    // Where gather puts each frame of `sel` (nexg_gather_plan): out_offsets
    // holds sel.count + 1 entries, out_len (may be null) sel.count; returns
    // the total bytes (one stream synchronisation) to allocate for gather
    uint64_t gather_plan(const nexg_frames& sel, uint32_t align, uint64_t* out_offsets, uint32_t* out_len) {
        DeviceScope ds(device_);
        const uint64_t wsb = nexg_gather_plan_workspace(sel.count);
        void* ws = scratch(23, wsb);
        check(nexg_gather_plan(ctx_, &sel, align, out_offsets, out_len, ws, wsb, stream_), "nexg_gather_plan");
        return read_u64(out_offsets + sel.count);
    }

    // The frames of `sel` copied to out_data at the planned offsets, pads
    // zero, nothing at or past out_cap (nexg_gather_frames)
    void gather(const nexg_frames& sel, const uint64_t* out_offsets, uint8_t* out_data, uint64_t out_cap) {
        DeviceScope ds(device_);
        check(nexg_gather_frames(ctx_, &sel, out_offsets, out_data, out_cap, stream_), "nexg_gather_frames");
    }

    // out row k = rows[index[k]] (zeros when index[k] >= rows_count): records,
    // tunnels, DNS summaries, descriptors or flags words of the selected frames
    void gather_rows(const void* rows, uint32_t row_bytes, uint64_t rows_count, const uint32_t* index, uint64_t n,
                     void* out) {
        DeviceScope ds(device_);
        check(nexg_gather_rows(ctx_, rows, row_bytes, rows_count, index, n, out, stream_), "nexg_gather_rows");
    }

    // parse (NEXG_OUT_RECORD) + select + gather of host frames: the selected
    // frames' numbers, first matching rules, records, and their bytes as one
    // dense buffer with count + 1 offsets (each start rounded up to `align`)
    struct Selected {
        std::vector<uint32_t> index;
        std::vector<uint8_t> rule;
        std::vector<nexg_record> records;
        std::vector<uint64_t> offsets;  // index.size() + 1
        std::vector<uint32_t> lengths;
        std::vector<uint8_t> data;
    };
    Selected select_bufs(const std::vector<std::vector<uint8_t>>& frames, const Filter& filter, ParseOption option = {},
                         ParseMode mode = ParseMode::Lenient, uint32_t align = 1) {
        DeviceScope ds(device_);
        const uint64_t n = frames.size();
        Selected out;
        out.offsets.assign(1, 0);
        if (n == 0) return out;
        HostBatch hb(*this, frames);
        nexg_record* d_recs = static_cast<nexg_record*>(scratch(3, n * 64));
        uint32_t* d_idx = static_cast<uint32_t*>(scratch(24, n * 4));
        uint64_t* d_off = static_cast<uint64_t*>(scratch(25, n * 8));
        uint32_t* d_len = static_cast<uint32_t*>(scratch(26, n * 4));
        uint8_t* d_rule = static_cast<uint8_t*>(scratch(27, n));
        parse(hb.fb, option, mode, NEXG_OUT_RECORD, d_recs);
        const uint64_t k = select(hb.fb, d_recs, filter, d_idx, d_off, d_len, d_rule);
        nexg_frames sel = hb.fb;
        sel.offsets = d_off;
        sel.lengths = d_len;
        sel.count = k;
        sel.hints = NEXG_FRAMES_MONOTONE;
        uint64_t* d_go = static_cast<uint64_t*>(scratch(28, (k + 1) * 8));
        uint32_t* d_gl = static_cast<uint32_t*>(scratch(29, k * 4));
        const uint64_t total = gather_plan(sel, align, d_go, d_gl);
        uint8_t* d_data = static_cast<uint8_t*>(scratch(30, total));
        gather(sel, d_go, d_data, total);
        nexg_record* d_rsel = static_cast<nexg_record*>(scratch(31, k * 64));
        gather_rows(d_recs, 64, n, d_idx, k, d_rsel);
        out.index.resize(k);
        out.rule.resize(k);
        out.records.resize(k);
        out.offsets.resize(k + 1);
        out.lengths.resize(k);
        out.data.resize(total);
        check_hip(hipMemcpyAsync(out.offsets.data(), d_go, (k + 1) * 8, hipMemcpyDeviceToHost, stream_), "D2H");
        if (k) {
            check_hip(hipMemcpyAsync(out.index.data(), d_idx, k * 4, hipMemcpyDeviceToHost, stream_), "D2H");
            check_hip(hipMemcpyAsync(out.rule.data(), d_rule, k, hipMemcpyDeviceToHost, stream_), "D2H");
            check_hip(hipMemcpyAsync(out.records.data(), d_rsel, k * 64, hipMemcpyDeviceToHost, stream_), "D2H");
            check_hip(hipMemcpyAsync(out.lengths.data(), d_gl, k * 4, hipMemcpyDeviceToHost, stream_), "D2H");
        }
        if (total) check_hip(hipMemcpyAsync(out.data.data(), d_data, total, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        return out;
    }

    // A row per frame of a device-resident batch (an extension, include/nexg.h
    // nexg_match_batch): which patterns of `set` occur in the frame's payload
    // (records: the batch's NEXG_OUT_RECORD parse) or, with PatternSet::frame,
    // anywhere in the frame (records may be null), and where the first one
    // starts. `out` is a device array of frames.count rows (8-B aligned).
    void match(const nexg_frames& frames, const nexg_record* records, const PatternSet& set, nexg_match* out) {
        DeviceScope ds(device_);
        check(nexg_match_batch(ctx_, &frames, records, &set.get(), out, stream_), "nexg_match_batch");
    }

    // Order-preserving selection by match's rows (nexg_match_select): frame i
    // is kept when some bit of any_mask is in its mask (0: no such condition),
    // every bit of all_mask is, and no bit of none_mask is. Device arrays of
    // capacity frames.count; returns the number selected (one stream
    // synchronisation). {frames.data, frames.data_bytes, out_off, out_len,
    // returned count} is the selected batch, as after select.
    uint64_t match_select(const nexg_frames& frames, const nexg_match* matches, uint32_t any_mask, uint32_t all_mask,
                          uint32_t none_mask, uint32_t* out_index, uint64_t* out_off, uint32_t* out_len) {
        DeviceScope ds(device_);
        const uint64_t wsb = nexg_match_select_workspace(frames.count);
        void* ws = scratch(44, wsb);
        uint64_t* d_count = static_cast<uint64_t*>(scratch(45, 8));
        check(nexg_match_select(ctx_, &frames, matches, any_mask, all_mask, none_mask, out_index, out_off, out_len, d_count,
                                ws, wsb, stream_),
              "nexg_match_select");
        return read_u64(d_count);
    }

    // parse (NEXG_OUT_RECORD) + match + match_select of host frames: every
    // frame's row, and the numbers of the frames the masks select
    struct Matched {
        std::vector<nexg_match> rows;
        std::vector<uint32_t> index;
        std::vector<uint64_t> offsets;  // of the selected frames in the packed upload (4-B aligned starts)
        std::vector<uint32_t> lengths;
    };
    Matched match_bufs(const std::vector<std::vector<uint8_t>>& frames, const PatternSet& set, uint32_t any_mask = 0,
                       uint32_t all_mask = 0, uint32_t none_mask = 0, ParseOption option = {},
                       ParseMode mode = ParseMode::Lenient) {
        DeviceScope ds(device_);
        const uint64_t n = frames.size();
        Matched out;
        if (n == 0) return out;
        HostBatch hb(*this, frames);
        nexg_record* d_recs = static_cast<nexg_record*>(scratch(3, n * 64));
        nexg_match* d_rows = static_cast<nexg_match*>(scratch(46, n * 8));
        uint32_t* d_idx = static_cast<uint32_t*>(scratch(24, n * 4));
        uint64_t* d_off = static_cast<uint64_t*>(scratch(25, n * 8));
        uint32_t* d_len = static_cast<uint32_t*>(scratch(26, n * 4));
        parse(hb.fb, option, mode, NEXG_OUT_RECORD, d_recs);
        match(hb.fb, d_recs, set, d_rows);
        const uint64_t k = match_select(hb.fb, d_rows, any_mask, all_mask, none_mask, d_idx, d_off, d_len);
        out.rows.resize(n);
        out.index.resize(k);
        out.offsets.resize(k);
        out.lengths.resize(k);
        check_hip(hipMemcpyAsync(out.rows.data(), d_rows, n * 8, hipMemcpyDeviceToHost, stream_), "D2H");
        if (k) {
            check_hip(hipMemcpyAsync(out.index.data(), d_idx, k * 4, hipMemcpyDeviceToHost, stream_), "D2H");
            check_hip(hipMemcpyAsync(out.offsets.data(), d_off, k * 8, hipMemcpyDeviceToHost, stream_), "D2H");
            check_hip(hipMemcpyAsync(out.lengths.data(), d_len, k * 4, hipMemcpyDeviceToHost, stream_), "D2H");
        }
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        return out;
    }

    // A flow row per frame of a device-resident batch already parsed with
    // NEXG_OUT_RECORD (an extension, include/nexg.h nexg_flow_batch): the
    // Toeplitz RSS hash of the addresses and ports, the kind of key, the IP
    // protocol. `out` is a device array of frames.count rows (8-B aligned).
    void flow(const nexg_frames& frames, const nexg_record* records, nexg_flow* out, const FlowOption& option = {}) {
        DeviceScope ds(device_);
        check(nexg_flow_batch(ctx_, &frames, records, &option.get(), out, stream_), "nexg_flow_batch");
    }

    // Stable split of the batch into `buckets` (1..256) buckets by
    // flows[i].hash % buckets (nexg_flow_partition): device arrays of capacity
    // frames.count (out_off and out_len may both be null); returns
    // bucket_first (buckets + 1 entries, one stream synchronisation). Bucket b
    // is {frames.data, frames.data_bytes, out_off + first[b], out_len +
    // first[b], first[b + 1] - first[b]}: parse, decap, dns, select and gather
    // take it as it stands, with gather_rows(records, 64, ..., out_index, ...)
    // for the records in the same order.
    std::vector<uint64_t> flow_partition(const nexg_frames& frames, const nexg_flow* flows, uint32_t buckets,
                                         uint32_t* out_index, uint64_t* out_off, uint32_t* out_len) {
        DeviceScope ds(device_);
        if (buckets < 1 || buckets > 256) throw Error("flow_partition: buckets must be 1..256");
        const uint64_t wsb = nexg_flow_partition_workspace(frames.count, buckets);
        void* ws = scratch(32, wsb);
        uint64_t* d_first = static_cast<uint64_t*>(scratch(33, 8 * (buckets + 1)));
        check(nexg_flow_partition(ctx_, &frames, flows, buckets, out_index, out_off, out_len, d_first, ws, wsb, stream_),
              "nexg_flow_partition");
        std::vector<uint64_t> first(buckets + 1);
        check_hip(hipMemcpyAsync(first.data(), d_first, 8 * (buckets + 1), hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        return first;
    }

    // parse (NEXG_OUT_RECORD) + flow + flow_partition of host frames: every
    // frame's flow row and bucket, and the frame numbers in bucket order
    struct Flows {
        std::vector<nexg_flow> flows;       // per frame
        std::vector<uint32_t> bucket;       // per frame
        std::vector<uint32_t> index;        // frame numbers ordered by bucket, then by frame
        std::vector<uint64_t> bucket_first; // buckets + 1
    };
    Flows flow_bufs(const std::vector<std::vector<uint8_t>>& frames, uint32_t buckets, const FlowOption& fopt = {},
                    ParseOption option = {}, ParseMode mode = ParseMode::Lenient) {
        DeviceScope ds(device_);
        const uint64_t n = frames.size();
        Flows out;
        out.bucket_first.assign(buckets + 1, 0);
        if (n == 0) return out;
        HostBatch hb(*this, frames);
        nexg_record* d_recs = static_cast<nexg_record*>(scratch(3, n * 64));
        nexg_flow* d_flows = static_cast<nexg_flow*>(scratch(34, n * 8));
        uint32_t* d_idx = static_cast<uint32_t*>(scratch(24, n * 4));
        parse(hb.fb, option, mode, NEXG_OUT_RECORD, d_recs);
        flow(hb.fb, d_recs, d_flows, fopt);
        out.bucket_first = flow_partition(hb.fb, d_flows, buckets, d_idx, nullptr, nullptr);
        out.flows.resize(n);
        out.index.resize(n);
        out.bucket.resize(n);
        check_hip(hipMemcpyAsync(out.flows.data(), d_flows, n * 8, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipMemcpyAsync(out.index.data(), d_idx, n * 4, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        for (uint32_t b = 0; b < buckets; b++)
            for (uint64_t k = out.bucket_first[b]; k < out.bucket_first[b + 1]; k++) out.bucket[out.index[k]] = b;
        return out;
    }

    // The frame numbers ordered by (flows[i].hash, i) (nexg_flow_sort): a
    // stable radix sort on the device. out_index: a device array of `count`
    // entries. Nothing is waited for.
    void flow_sort(const nexg_flow* flows, uint64_t count, uint32_t* out_index) {
        DeviceScope ds(device_);
        const uint64_t wsb = nexg_flow_sort_workspace(count);
        check(nexg_flow_sort(ctx_, flows, count, out_index, scratch(35, wsb), wsb, stream_), "nexg_flow_sort");
    }

    // One row per run of equal hashes in `order` (flow_sort's output):
    // packets, bytes, the first frame, and `mixed`, nonzero where flows with
    // different keys share the hash (nexg_flow_groups). `out` is a device
    // array of `cap` rows (16-B aligned), out_group (may be null) a device
    // array of frames.count group numbers by frame. Returns the number of
    // groups, which may exceed `cap` (one stream synchronisation).
    uint64_t flow_groups(const nexg_frames& frames, const nexg_record* records, const nexg_flow* flows,
                         const uint32_t* order, FlowGroup* out, uint64_t cap, uint32_t* out_group,
                         const FlowOption& option = {}) {
        DeviceScope ds(device_);
        const uint64_t wsb = nexg_flow_groups_workspace(frames.count);
        void* ws = scratch(36, wsb);
        uint64_t* d_count = static_cast<uint64_t*>(scratch(37, 8));
        check(nexg_flow_groups(ctx_, &frames, records, flows, &option.get(), order, out, cap, out_group, d_count, ws, wsb,
                               stream_),
              "nexg_flow_groups");
        return read_u64(d_count);
    }

    // parse (NEXG_OUT_RECORD) + flow + flow_sort + flow_groups of host frames
    struct FlowGroups {
        std::vector<FlowGroup> groups;   // ascending by hash
        std::vector<uint32_t> order;     // frame numbers by (hash, frame number)
        std::vector<uint32_t> group_of;  // per frame
    };
    FlowGroups flow_group_bufs(const std::vector<std::vector<uint8_t>>& frames, const FlowOption& fopt = {},
                               ParseOption option = {}, ParseMode mode = ParseMode::Lenient) {
        DeviceScope ds(device_);
        const uint64_t n = frames.size();
        FlowGroups out;
        if (n == 0) return out;
        HostBatch hb(*this, frames);
        nexg_record* d_recs = static_cast<nexg_record*>(scratch(3, n * 64));
        nexg_flow* d_flows = static_cast<nexg_flow*>(scratch(34, n * 8));
        uint32_t* d_order = static_cast<uint32_t*>(scratch(24, n * 4));
        uint32_t* d_group = static_cast<uint32_t*>(scratch(38, n * 4));
        FlowGroup* d_rows = static_cast<FlowGroup*>(scratch(39, n * 32));
        parse(hb.fb, option, mode, NEXG_OUT_RECORD, d_recs);
        flow(hb.fb, d_recs, d_flows, fopt);
        flow_sort(d_flows, n, d_order);
        const uint64_t g = flow_groups(hb.fb, d_recs, d_flows, d_order, d_rows, n, d_group, fopt);
        out.groups.resize(g);
        out.order.resize(n);
        out.group_of.resize(n);
        check_hip(hipMemcpyAsync(out.groups.data(), d_rows, g * 32, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipMemcpyAsync(out.order.data(), d_order, n * 4, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipMemcpyAsync(out.group_of.data(), d_group, n * 4, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        return out;
    }

    // The flow table across batches (nexg_flow_table_merge): table_out = the
    // union by hash of table_in[0, n_in) and one batch's groups
    // (flow_groups' rows), ascending. A hash in both adds the group's packets
    // and bytes and sets last_epoch = epoch; a new hash makes an entry; an
    // entry no group matches is dropped when last_epoch < min_epoch. All
    // arrays are device memory (table_in, table_out and groups 16-B aligned,
    // table_out apart from table_in); out_slot (may be null) receives the
    // position of every group's entry. Returns the size of the union, which
    // may exceed `cap` (one stream synchronisation).
    uint64_t flow_table_merge(const nexg_frames& frames, const nexg_record* records, const FlowGroup* groups,
                              uint64_t n_groups, const FlowEntry* table_in, uint64_t n_in, uint32_t epoch,
                              uint32_t min_epoch, FlowEntry* table_out, uint64_t cap, uint32_t* out_slot,
                              const FlowOption& option = {}) {
        DeviceScope ds(device_);
        const uint64_t wsb = nexg_flow_table_workspace(n_in, n_groups);
        void* ws = scratch(40, wsb);
        uint64_t* d_count = static_cast<uint64_t*>(scratch(37, 8));
        check(nexg_flow_table_merge(ctx_, &frames, records, &option.get(), groups, n_groups, table_in, n_in, epoch,
                                    min_epoch, table_out, cap, out_slot, d_count, ws, wsb, stream_),
              "nexg_flow_table_merge");
        return read_u64(d_count);
    }

    // parse (NEXG_OUT_RECORD) + flow + flow_sort + flow_groups of host frames,
    // merged into a host copy of a flow table
    struct FlowTableUpdate {
        std::vector<FlowEntry> table;    // the new table, ascending by hash
        std::vector<uint32_t> slot;      // per group of the batch: its entry's position
        std::vector<uint32_t> group_of;  // per frame
    };
    FlowTableUpdate flow_table_bufs(const std::vector<FlowEntry>& table, const std::vector<std::vector<uint8_t>>& frames,
                                    uint32_t epoch, uint32_t min_epoch = 0, const FlowOption& fopt = {},
                                    ParseOption option = {}, ParseMode mode = ParseMode::Lenient) {
        DeviceScope ds(device_);
        const uint64_t n = frames.size(), n_in = table.size();
        FlowTableUpdate out;
        HostBatch hb(*this, frames);
        nexg_record* d_recs = static_cast<nexg_record*>(scratch(3, n * 64));
        nexg_flow* d_flows = static_cast<nexg_flow*>(scratch(34, n * 8));
        uint32_t* d_order = static_cast<uint32_t*>(scratch(24, n * 4));
        uint32_t* d_group = static_cast<uint32_t*>(scratch(38, n * 4));
        FlowGroup* d_rows = static_cast<FlowGroup*>(scratch(39, n * 32));
        FlowEntry* d_in = static_cast<FlowEntry*>(scratch(41, n_in * 64));
        FlowEntry* d_out = static_cast<FlowEntry*>(scratch(42, (n_in + n) * 64));
        uint32_t* d_slot = static_cast<uint32_t*>(scratch(43, n * 4));
        uint64_t g = 0;
        if (n) {
            parse(hb.fb, option, mode, NEXG_OUT_RECORD, d_recs);
            flow(hb.fb, d_recs, d_flows, fopt);
            flow_sort(d_flows, n, d_order);
            g = flow_groups(hb.fb, d_recs, d_flows, d_order, d_rows, n, d_group, fopt);
        }
        if (n_in) check_hip(hipMemcpyAsync(d_in, table.data(), n_in * 64, hipMemcpyHostToDevice, stream_), "H2D");
        const uint64_t n_out = flow_table_merge(hb.fb, d_recs, d_rows, g, d_in, n_in, epoch, min_epoch, d_out, n_in + n,
                                                d_slot, fopt);
        out.table.resize(n_out);
        out.slot.resize(g);
        out.group_of.resize(n);
        if (n_out) check_hip(hipMemcpyAsync(out.table.data(), d_out, n_out * 64, hipMemcpyDeviceToHost, stream_), "D2H");
        if (g) check_hip(hipMemcpyAsync(out.slot.data(), d_slot, g * 4, hipMemcpyDeviceToHost, stream_), "D2H");
        if (n) check_hip(hipMemcpyAsync(out.group_of.data(), d_group, n * 4, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        return out;
    }

    // Frame::try_from_buf_with_mode (frame.rs:309) on every host frame: the
    // batch is packed, copied to the device, parsed (NEXG_OUT_RECORD), its
    // option lists decoded, and each Frame materialised from its record.
    std::vector<Result<Frame>> try_from_bufs(const std::vector<std::vector<uint8_t>>& frames,
                                             ParseOption option = {}, ParseMode mode = ParseMode::Lenient) {
        DeviceScope ds(device_);
        const uint64_t n = frames.size();
        std::vector<Result<Frame>> out;
        if (n == 0) return out;
        HostBatch hb(*this, frames);
        void* d_recs = scratch(3, n * 64);
        void* d_opts = scratch(4, n * 96);
        parse(hb.fb, option, mode, NEXG_OUT_RECORD, d_recs);
        check(nexg_decode_options(ctx_, &hb.fb, static_cast<const nexg_record*>(d_recs),
                                  static_cast<nexg_options*>(d_opts), stream_),
              "nexg_decode_options");
        std::vector<nexg_record> recs(n);
        std::vector<nexg_options> opts(n);
        check_hip(hipMemcpyAsync(recs.data(), d_recs, n * 64, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipMemcpyAsync(opts.data(), d_opts, n * 96, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        out.reserve(n);
        for (uint64_t i = 0; i < n; i++)
            out.push_back(frame_from_record(recs[i], frames[i].data(), frames[i].size(), opts[i]));
        return out;
    }

    // FrameSlice::try_from_buf (frame.rs:86) on every host frame; the slices
    // borrow `frames`, which must outlive them
    std::vector<Result<FrameSlice>> frame_slices(const std::vector<std::vector<uint8_t>>& frames,
                                                 ParseOption option = {}) {
        DeviceScope ds(device_);
        const uint64_t n = frames.size();
        std::vector<Result<FrameSlice>> out;
        if (n == 0) return out;
        HostBatch hb(*this, frames);
        void* d_sl = scratch(3, n * 16);
        parse(hb.fb, option, ParseMode::Lenient, NEXG_OUT_SLICE, d_sl);
        std::vector<nexg_slice> sl(n);
        check_hip(hipMemcpyAsync(sl.data(), d_sl, n * 16, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        out.reserve(n);
        for (uint64_t i = 0; i < n; i++) out.push_back(frame_slice_from(sl[i], frames[i].data(), frames[i].size()));
        return out;
    }

    // The parse result of every host frame as nexg_desc (layers, checksum
    // verdicts, payload location: what Frame::try_from_buf reports, without
    // the header fields), through the grouped output the bench times
    // (NEXG_OUT_GROUPED: 17 B per 64 single-shape frames) decoded on the host
    std::vector<nexg_desc> descriptors(const std::vector<std::vector<uint8_t>>& frames, ParseOption option = {},
                                       ParseMode mode = ParseMode::Lenient) {
        DeviceScope ds(device_);
        const uint64_t n = frames.size();
        std::vector<nexg_desc> out(n);
        if (n == 0) return out;
        HostBatch hb(*this, frames);
        const uint64_t bytes = NEXG_GROUPED_BYTES(n);
        void* d_g = scratch(3, bytes);
        parse(hb.fb, option, mode, NEXG_OUT_GROUPED, d_g);
        std::vector<uint8_t> g(bytes);
        check_hip(hipMemcpyAsync(g.data(), d_g, bytes, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        const nexg_desc* exc = reinterpret_cast<const nexg_desc*>(g.data() + NEXG_GROUPED_EXC_OFFSET(n));
        const uint32_t fl = option.flags(mode);
        uint64_t kg = 0, kt = 0;  // exceptions so far in the frame's group / tile
        for (uint64_t i = 0; i < n; i++) {
            if ((i & 63u) == 0) kg = 0;
            if ((i & 255u) == 0) kt = 0;
            if (!nexg_sparse_decode(nexg_grouped_code(g.data(), n, i), (uint32_t)frames[i].size(), fl,
                                    (uint32_t)option.offset, &out[i])) {
                // (nexg_grouped_exc_slot, without its rescan of the run)
                const bool run = g[i >> 6] == NEXG_GROUPED_TILE_RUN;
                out[i] = exc[run ? (i & ~(uint64_t)255u) + kt : (i & ~(uint64_t)63u) + kg];
                kg++;
                kt++;
            }
        }
        return out;
    }

    // udp_ping's probe batch: one source address and port pair (udp_ping.rs:30-31,
    // 54-66) and a destination per target, identification 0 (the
    // Ipv4PacketBuilder default): the builder reads 4 B per frame
    Result<std::vector<std::vector<uint8_t>>, BuildError> build_udp_probes(const Ipv4Addr& source,
                                                                           const std::vector<Ipv4Addr>& targets,
                                                                           uint16_t src_port, uint16_t dst_port,
                                                                           const UdpPingShape& shape) {
        DeviceScope ds(device_);
        if (28ull + shape.payload.size() > 65535ull) return BuildError::LengthOverflow;
        const uint64_t n = targets.size();
        const uint32_t L = 42u + (uint32_t)shape.payload.size();
        if (n == 0) return std::vector<std::vector<uint8_t>>{};
        std::vector<uint32_t> dst(n);
        for (uint64_t i = 0; i < n; i++) {
            const auto& b = targets[i].octets;
            dst[i] = (uint32_t)b[0] << 24 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 8 | b[3];
        }
        void* d_dst = upload(6, dst.data(), n * 4);
        void* d_pl = shape.payload.empty() ? nullptr : upload(10, shape.payload.data(), shape.payload.size());
        void* d_out = scratch(11, (uint64_t)n * L);
        nexg_udp4_build p{};
        p.dst_ip = static_cast<const uint32_t*>(d_dst);
        p.def_src_ip = (uint32_t)source.octets[0] << 24 | (uint32_t)source.octets[1] << 16 |
                       (uint32_t)source.octets[2] << 8 | source.octets[3];
        p.def_src_port = src_port;
        p.def_dst_port = dst_port;
        p.payload = static_cast<const uint8_t*>(d_pl);
        p.payload_len = (uint32_t)shape.payload.size();
        memcpy(p.def_src_mac, shape.src_mac.data(), 6);
        memcpy(p.def_dst_mac, shape.dst_mac.data(), 6);
        p.ttl = shape.ttl;
        p.ip_flags = shape.ip_flags;
        p.count = n;
        check(nexg_build_udp4_batch(ctx_, &p, static_cast<uint8_t*>(d_out), L, stream_), "nexg_build_udp4_batch");
        return download_frames(d_out, n, L);
    }

    // udp_ping's build (udp_ping.rs:68-109) for every tuple: 42 + payload bytes
    // each; BuildError::LengthOverflow when the UDP / IPv4 length would pass
    // 65535 (builder/udp.rs:83, builder/ipv4.rs:153)
    Result<std::vector<std::vector<uint8_t>>, BuildError> build_udp_ping(const std::vector<UdpPingTuple>& t,
                                                                         const UdpPingShape& shape) {
        DeviceScope ds(device_);
        if (28ull + shape.payload.size() > 65535ull) return BuildError::LengthOverflow;
        const uint64_t n = t.size();
        const uint32_t L = 42u + (uint32_t)shape.payload.size();
        std::vector<std::vector<uint8_t>> frames;
        if (n == 0) return frames;
        // one 16-B record per tuple: a single H2D copy and one load per frame
        // on the device (nexg_build_udp4_tuples)
        std::vector<nexg_udp4_tuple> tup(n);
        for (uint64_t i = 0; i < n; i++) {
            const auto& a = t[i].source.octets;
            const auto& b = t[i].destination.octets;
            tup[i].src_ip = (uint32_t)a[0] << 24 | (uint32_t)a[1] << 16 | (uint32_t)a[2] << 8 | a[3];
            tup[i].dst_ip = (uint32_t)b[0] << 24 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 8 | b[3];
            tup[i].src_port = t[i].src_port;
            tup[i].dst_port = t[i].dst_port;
            tup[i].ip_id = t[i].ip_id;
            tup[i].reserved = 0;
        }
        void* d_tup = scratch(5, n * sizeof(nexg_udp4_tuple));
        void* d_pl = scratch(10, shape.payload.size());
        void* d_out = scratch(11, (uint64_t)n * L);
        check_hip(hipMemcpyAsync(d_tup, tup.data(), n * sizeof(nexg_udp4_tuple), hipMemcpyHostToDevice, stream_),
                  "H2D");
        if (!shape.payload.empty())
            check_hip(hipMemcpyAsync(d_pl, shape.payload.data(), shape.payload.size(), hipMemcpyHostToDevice,
                                     stream_), "H2D");
        nexg_udp4_build p{};
        p.payload = shape.payload.empty() ? nullptr : static_cast<const uint8_t*>(d_pl);
        p.payload_len = (uint32_t)shape.payload.size();
        memcpy(p.def_src_mac, shape.src_mac.data(), 6);
        memcpy(p.def_dst_mac, shape.dst_mac.data(), 6);
        p.ttl = shape.ttl;
        p.ip_flags = shape.ip_flags;
        p.count = n;
        check(nexg_build_udp4_tuples(ctx_, &p, static_cast<const nexg_udp4_tuple*>(d_tup),
                                     static_cast<uint8_t*>(d_out), L, stream_), "nexg_build_udp4_tuples");
        std::vector<uint8_t> host((uint64_t)n * L);
        check_hip(hipMemcpyAsync(host.data(), d_out, host.size(), hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        frames.reserve(n);
        for (uint64_t i = 0; i < n; i++) frames.emplace_back(host.begin() + i * L, host.begin() + (i + 1) * L);
        return frames;
    }

    // tcp_ping's build for every tuple (one address family per batch:
    // BuildError::AddressFamilyMismatch otherwise, builder/error.rs)
    Result<std::vector<std::vector<uint8_t>>, BuildError> build_tcp_ping(const std::vector<TcpPingTuple>& t,
                                                                         const TcpPingShape& shape) {
        DeviceScope ds(device_);
        std::vector<std::vector<uint8_t>> frames;
        if (t.empty()) return frames;
        if (shape.options.size() > 40) return BuildError::LengthOverflow;
        const uint8_t fam = t[0].source.family;
        for (const auto& x : t)
            if (x.source.family != fam || x.destination.family != fam) return BuildError::AddressFamilyMismatch;
        const uint64_t n = t.size();
        const uint32_t L = 14u + (fam == 4 ? 20u : 40u) + 20u + (((uint32_t)shape.options.size() + 3u) & ~3u) +
                           (uint32_t)shape.payload.size();
        nexg_tcp_build p{};
        fill_ip(p.ip, t, shape.src_mac, shape.dst_mac, fam, shape.ttl, shape.ip_flags, shape.tos, shape.flow_label, 5);
        std::vector<uint16_t> sp(n), dp(n);
        std::vector<uint32_t> seq(n), ack(n);
        for (uint64_t i = 0; i < n; i++) {
            sp[i] = t[i].src_port;
            dp[i] = t[i].dst_port;
            seq[i] = t[i].sequence;
            ack[i] = t[i].acknowledgement;
        }
        p.src_port = static_cast<const uint16_t*>(upload(10, sp.data(), n * 2));
        p.dst_port = static_cast<const uint16_t*>(upload(11, dp.data(), n * 2));
        p.seq = static_cast<const uint32_t*>(upload(12, seq.data(), n * 4));
        p.ack = static_cast<const uint32_t*>(upload(13, ack.data(), n * 4));
        p.payload = shape.payload.empty() ? nullptr
                                          : static_cast<const uint8_t*>(upload(14, shape.payload.data(), shape.payload.size()));
        p.payload_len = (uint32_t)shape.payload.size();
        p.window = shape.window;
        p.urgent_ptr = shape.urgent_ptr;
        p.flags = shape.flags;
        p.options_len = (uint8_t)shape.options.size();
        if (!shape.options.empty()) memcpy(p.options, shape.options.data(), shape.options.size());
        p.count = n;
        void* d_out = scratch(15, n * L);
        const int rc = nexg_build_tcp_batch(ctx_, &p, static_cast<uint8_t*>(d_out), L, stream_);
        if (rc == NEXG_ERANGE) return BuildError::LengthOverflow;
        check(rc, "nexg_build_tcp_batch");
        return download_frames(d_out, n, L);
    }

    // icmp_ping's echo request for every tuple (EchoRequest 8 / ICMPv6 128, code 0)
    Result<std::vector<std::vector<uint8_t>>, BuildError> build_icmp_ping(const std::vector<IcmpPingTuple>& t,
                                                                          const IcmpPingShape& shape) {
        DeviceScope ds(device_);
        std::vector<std::vector<uint8_t>> frames;
        if (t.empty()) return frames;
        const uint8_t fam = t[0].source.family;
        for (const auto& x : t)
            if (x.source.family != fam || x.destination.family != fam) return BuildError::AddressFamilyMismatch;
        const uint64_t n = t.size();
        const uint32_t L = 14u + (fam == 4 ? 20u : 40u) + 8u + (uint32_t)shape.payload.size();
        nexg_icmp_echo_build p{};
        fill_ip(p.ip, t, shape.src_mac, shape.dst_mac, fam, shape.ttl, shape.ip_flags, shape.tos, shape.flow_label, 5);
        std::vector<uint16_t> id(n), sq(n);
        for (uint64_t i = 0; i < n; i++) {
            id[i] = t[i].identifier;
            sq[i] = t[i].sequence;
        }
        p.identifier = static_cast<const uint16_t*>(upload(10, id.data(), n * 2));
        p.sequence = static_cast<const uint16_t*>(upload(11, sq.data(), n * 2));
        p.payload = shape.payload.empty() ? nullptr
                                          : static_cast<const uint8_t*>(upload(14, shape.payload.data(), shape.payload.size()));
        p.payload_len = (uint32_t)shape.payload.size();
        p.icmp_type = fam == 4 ? 8 : 128;
        p.icmp_code = 0;
        p.count = n;
        void* d_out = scratch(15, n * L);
        const int rc = nexg_build_icmp_echo_batch(ctx_, &p, static_cast<uint8_t*>(d_out), L, stream_);
        if (rc == NEXG_ERANGE) return BuildError::LengthOverflow;
        check(rc, "nexg_build_icmp_echo_batch");
        return download_frames(d_out, n, L);
    }

    // an ARP request for every target (nexg_build_arp_batch)
    Result<std::vector<std::vector<uint8_t>>, BuildError> build_arp_requests(const std::vector<Ipv4Addr>& targets,
                                                                             const ArpProbeShape& shape) {
        DeviceScope ds(device_);
        std::vector<std::vector<uint8_t>> frames;
        if (shape.hw_addr_len != 6 || shape.proto_addr_len != 4) return BuildError::InvalidFieldLength;
        if (targets.empty()) return frames;
        const uint64_t n = targets.size();
        std::vector<uint8_t> tip(n * 4);
        for (uint64_t i = 0; i < n; i++) memcpy(tip.data() + 4 * i, targets[i].octets.data(), 4);
        nexg_arp_build p{};
        p.target_ip = static_cast<const uint8_t*>(upload(16, tip.data(), tip.size()));
        memcpy(p.def_sender_ip, shape.sender_ip.octets.data(), 4);
        memcpy(p.def_sender_mac, shape.sender_mac.data(), 6);
        memcpy(p.def_eth_dst, shape.eth_dst.data(), 6);
        p.hardware_type = 1;
        p.protocol_type = 0x0800;
        p.operation = shape.operation;
        p.hw_addr_len = shape.hw_addr_len;
        p.proto_addr_len = shape.proto_addr_len;
        p.count = n;
        void* d_out = scratch(15, n * 42);
        check(nexg_build_arp_batch(ctx_, &p, static_cast<uint8_t*>(d_out), 42, stream_), "nexg_build_arp_batch");
        return download_frames(d_out, n, 42);
    }

    // an NDP neighbor solicitation for every target (nexg_build_ndp_ns_batch)
    std::vector<std::vector<uint8_t>> build_ndp_solicits(const std::vector<Ipv6Addr>& targets,
                                                         const NdpProbeShape& shape) {
        DeviceScope ds(device_);
        if (targets.empty()) return {};
        const uint64_t n = targets.size();
        std::vector<uint8_t> src(n * 16), dst(n * 16);
        for (uint64_t i = 0; i < n; i++) {
            memcpy(src.data() + 16 * i, shape.src_ip.octets.data(), 16);
            memcpy(dst.data() + 16 * i, targets[i].octets.data(), 16);
        }
        nexg_ndp_ns_build p{};
        p.ip.src_ip = static_cast<const uint8_t*>(upload(16, src.data(), src.size()));
        p.ip.dst_ip = static_cast<const uint8_t*>(upload(17, dst.data(), dst.size()));
        p.ip.family = 6;
        memcpy(p.ip.def_src_mac, shape.src_mac.data(), 6);
        p.ip.ttl = shape.hop_limit;
        p.eth_dst_multicast = 1;
        p.count = n;
        void* d_out = scratch(15, n * 86);
        check(nexg_build_ndp_ns_batch(ctx_, &p, static_cast<uint8_t*>(d_out), 86, stream_), "nexg_build_ndp_ns_batch");
        return download_frames(d_out, n, 86);
    }

    // Mutable{Ipv4,Udp,Tcp,Icmp,Icmpv6}Packet::recompute_checksum over every
    // frame's raw buffer (ipv4.rs:669-679, udp.rs:338-369, tcp.rs:1009-1040,
    // icmp.rs:372-377, icmpv6.rs:450-470), chained as mutable_chaining.rs:
    // the frames are rewritten in place; one nexg_fixup per frame says which
    // fields were written (which = NEXG_FIX_IP | NEXG_FIX_L4)
    std::vector<nexg_fixup> recompute_checksums(std::vector<std::vector<uint8_t>>& frames, ParseOption option = {},
                                                uint32_t which = NEXG_FIX_IP | NEXG_FIX_L4) {
        DeviceScope ds(device_);
        const uint64_t n = frames.size();
        std::vector<nexg_fixup> fx(n);
        if (n == 0) return fx;
        HostBatch hb(*this, frames);
        void* d_fx = scratch(3, n * sizeof(nexg_fixup));
        const nexg_parse_option o{option.flags(ParseMode::Lenient), (uint32_t)option.offset};
        check(nexg_recompute_checksums_batch(ctx_, &hb.fb, &o, which, static_cast<nexg_fixup*>(d_fx), stream_),
              "nexg_recompute_checksums_batch");
        std::vector<uint8_t> data(hb.data.size());
        check_hip(hipMemcpyAsync(data.data(), const_cast<uint8_t*>(hb.fb.data), data.size(), hipMemcpyDeviceToHost,
                                 stream_), "D2H");
        check_hip(hipMemcpyAsync(fx.data(), d_fx, n * sizeof(nexg_fixup), hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        for (uint64_t i = 0; i < n; i++)
            std::copy(data.begin() + hb.offs[i], data.begin() + hb.offs[i] + hb.lens[i], frames[i].begin());
        return fx;
    }

    // Header fields of a device-resident batch rewritten in place
    // (nexg_rewrite_batch; MutableEthernetPacket::set_destination / set_source,
    // MutableIpv4Packet / MutableIpv6Packet::set_source / set_destination /
    // set_ttl / set_hop_limit / set_dscp / set_ecn / set_traffic_class,
    // MutableTcpPacket / MutableUdpPacket::set_source / set_destination under
    // ChecksumMode::Automatic). action_index: a device array with one action
    // number per frame (the out_rule of select: rule j gets action j;
    // NEXG_ACTION_NONE leaves a frame alone) or null (action 0 for all); out:
    // a device array of frames.count rows (8-B aligned) or null.
    void rewrite(const nexg_frames& frames, const ActionSet& actions, const uint8_t* action_index = nullptr,
                 nexg_rewritten* out = nullptr, ParseOption option = {}) {
        DeviceScope ds(device_);
        const nexg_parse_option o{option.flags(ParseMode::Lenient), (uint32_t)option.offset};
        check(nexg_rewrite_batch(ctx_, &frames, &o, &actions.get(), action_index, out, stream_), "nexg_rewrite_batch");
    }

    // rewrite of host frames, in place; index: one action number per frame, or
    // empty (action 0 for all). One nexg_rewritten per frame says what was written.
    std::vector<nexg_rewritten> rewrite_bufs(std::vector<std::vector<uint8_t>>& frames, const ActionSet& actions,
                                             const std::vector<uint8_t>& index = {}, ParseOption option = {}) {
        DeviceScope ds(device_);
        const uint64_t n = frames.size();
        std::vector<nexg_rewritten> rows(n);
        if (!index.empty() && index.size() != n) throw Error("rewrite_bufs: one action number per frame");
        if (n == 0) return rows;
        HostBatch hb(*this, frames);
        nexg_rewritten* d_rows = static_cast<nexg_rewritten*>(scratch(3, n * sizeof(nexg_rewritten)));
        const uint8_t* d_index = index.empty() ? nullptr : static_cast<const uint8_t*>(upload(47, index.data(), n));
        rewrite(hb.fb, actions, d_index, d_rows, option);
        std::vector<uint8_t> data(hb.data.size());
        check_hip(hipMemcpyAsync(data.data(), const_cast<uint8_t*>(hb.fb.data), data.size(), hipMemcpyDeviceToHost,
                                 stream_), "D2H");
        check_hip(hipMemcpyAsync(rows.data(), d_rows, n * sizeof(nexg_rewritten), hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        for (uint64_t i = 0; i < n; i++)
            std::copy(data.begin() + hb.offs[i], data.begin() + hb.offs[i] + hb.lens[i], frames[i].begin());
        return rows;
    }

    // Where encap puts each frame's outer frame (nexg_encap_plan): out_offsets
    // holds frames.count + 1 entries, out_len (may be null) frames.count;
    // tunnel_index: a device array with one tunnel number per frame (the
    // out_rule of select: rule j gets tunnel j; NEXG_TUNNEL_NONE copies a frame
    // unchanged) or null (tunnel 0 for all). Returns the total bytes (one
    // stream synchronisation) to allocate for encap.
    uint64_t encap_plan(const nexg_frames& frames, const TunnelSet& tunnels, const uint8_t* tunnel_index, uint32_t align,
                        uint64_t* out_offsets, uint32_t* out_len) {
        DeviceScope ds(device_);
        const uint64_t wsb = nexg_encap_plan_workspace(frames.count);
        void* ws = scratch(48, wsb);
        check(nexg_encap_plan(ctx_, &frames, &tunnels.get(), tunnel_index, align, out_offsets, out_len, ws, wsb, stream_),
              "nexg_encap_plan");
        return read_u64(out_offsets + frames.count);
    }

    // Every frame behind its tunnel's outer Ethernet / IP / UDP + VXLAN or GRE
    // header at out_data + out_offsets[i], pads zero, nothing at or past
    // out_cap (nexg_encap_frames; VxlanPacket::to_bytes vxlan.rs:73-84,
    // GrePacket::to_bytes gre.rs:115-160 inside the reference's builders).
    // flows: the rows of flow() over the same table, needed when a tunnel
    // takes its source port from the flow hash; rows: a device array of
    // frames.count nexg_encapped (8-B aligned) or null.
    void encap(const nexg_frames& frames, const TunnelSet& tunnels, const uint8_t* tunnel_index, const nexg_flow* flows,
               const uint64_t* out_offsets, uint8_t* out_data, uint64_t out_cap, nexg_encapped* rows = nullptr) {
        DeviceScope ds(device_);
        check(nexg_encap_frames(ctx_, &frames, &tunnels.get(), tunnel_index, flows, out_offsets, out_data, out_cap, rows,
                                stream_),
              "nexg_encap_frames");
    }

    // encap of host frames: index: one tunnel number per frame, or empty
    // (tunnel 0 for all). With a tunnel that takes its source port from the
    // flow hash the frames are parsed (NEXG_OUT_RECORD) and hashed first. The
    // outer frames lie in `data` at offsets[i], lengths[i] bytes each (each
    // start rounded up to `align`).
    struct Encapped {
        std::vector<nexg_encapped> rows;
        std::vector<uint64_t> offsets;  // rows.size() + 1
        std::vector<uint32_t> lengths;
        std::vector<uint8_t> data;
    };
    Encapped encap_bufs(const std::vector<std::vector<uint8_t>>& frames, const TunnelSet& tunnels,
                        const std::vector<uint8_t>& index = {}, uint32_t align = 1, ParseOption option = {}) {
        DeviceScope ds(device_);
        const uint64_t n = frames.size();
        Encapped out;
        out.offsets.assign(1, 0);
        if (!index.empty() && index.size() != n) throw Error("encap_bufs: one tunnel number per frame");
        (void)tunnels.get();
        if (n == 0) return out;
        HostBatch hb(*this, frames);
        const uint8_t* d_index = index.empty() ? nullptr : static_cast<const uint8_t*>(upload(47, index.data(), n));
        nexg_flow* d_flows = nullptr;
        if (tunnels.needs_flows()) {
            nexg_record* d_recs = static_cast<nexg_record*>(scratch(3, n * 64));
            d_flows = static_cast<nexg_flow*>(scratch(49, n * sizeof(nexg_flow)));
            parse(hb.fb, option, ParseMode::Lenient, NEXG_OUT_RECORD, d_recs);
            check(nexg_flow_batch(ctx_, &hb.fb, d_recs, nullptr, d_flows, stream_), "nexg_flow_batch");
        }
        uint64_t* d_off = static_cast<uint64_t*>(scratch(50, (n + 1) * 8));
        uint32_t* d_len = static_cast<uint32_t*>(scratch(51, n * 4));
        nexg_encapped* d_rows = static_cast<nexg_encapped*>(scratch(52, n * sizeof(nexg_encapped)));
        const uint64_t total = encap_plan(hb.fb, tunnels, d_index, align, d_off, d_len);
        uint8_t* d_data = static_cast<uint8_t*>(scratch(53, total));
        encap(hb.fb, tunnels, d_index, d_flows, d_off, d_data, total, d_rows);
        out.rows.resize(n);
        out.offsets.resize(n + 1);
        out.lengths.resize(n);
        out.data.resize(total);
        check_hip(hipMemcpyAsync(out.rows.data(), d_rows, n * sizeof(nexg_encapped), hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipMemcpyAsync(out.offsets.data(), d_off, (n + 1) * 8, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipMemcpyAsync(out.lengths.data(), d_len, n * 4, hipMemcpyDeviceToHost, stream_), "D2H");
        if (total) check_hip(hipMemcpyAsync(out.data.data(), d_data, total, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        return out;
    }

    // What fragment will write (nexg_fragment_plan): out_first and out_bytes
    // hold frames.count + 1 entries, rows (may be null) frames.count. Returns
    // the number of output frames and their bytes (one stream
    // synchronisation) to allocate for fragment; throws when the output
    // frames do not fit their 32-bit numbers.
    struct FragmentTotals {
        uint64_t frames, bytes;
    };
    FragmentTotals fragment_plan(const nexg_frames& frames, const FragOption& option, uint32_t* out_first,
                                 uint64_t* out_bytes, nexg_fragged* rows = nullptr) {
        DeviceScope ds(device_);
        const uint64_t wsb = nexg_fragment_plan_workspace(frames.count);
        void* ws = scratch(54, wsb);
        check(nexg_fragment_plan(ctx_, &frames, &option.get(), out_first, out_bytes, rows, ws, wsb, stream_),
              "nexg_fragment_plan");
        uint32_t n = 0;
        FragmentTotals t{0, 0};
        check_hip(hipMemcpyAsync(&n, out_first + frames.count, 4, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipMemcpyAsync(&t.bytes, out_bytes + frames.count, 8, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        if (n == 0xFFFFFFFFu) throw Error("fragment_plan: 2^32 - 1 output frames or more (include/nexg.h)");
        t.frames = n;
        return t;
    }

    // Every IPv4 frame over the MTU as its RFC 791 fragments, every other
    // frame unchanged, at out_data + out_bytes[i] on, pads zero, nothing at or
    // past out_cap (nexg_fragment_frames); out_offsets (out_count + 1
    // entries), out_len and out_src (out_count each) are the output frames'
    // table and the input frame of each.
    void fragment(const nexg_frames& frames, const FragOption& option, const uint32_t* out_first, const uint64_t* out_bytes,
                  uint64_t out_count, uint64_t* out_offsets, uint32_t* out_len, uint32_t* out_src, uint8_t* out_data,
                  uint64_t out_cap) {
        DeviceScope ds(device_);
        check(nexg_fragment_frames(ctx_, &frames, &option.get(), out_first, out_bytes, out_count, out_offsets, out_len,
                                   out_src, out_data, out_cap, stream_),
              "nexg_fragment_frames");
    }

    // fragment of host frames: output frame f lies in `data` at offsets[f],
    // lengths[f] bytes, and came from input frame src[f]; rows has one entry
    // per input frame.
    struct Fragged {
        std::vector<nexg_fragged> rows;
        std::vector<uint64_t> offsets;  // lengths.size() + 1
        std::vector<uint32_t> lengths, src;
        std::vector<uint8_t> data;
    };
    Fragged fragment_bufs(const std::vector<std::vector<uint8_t>>& frames, const FragOption& option) {
        DeviceScope ds(device_);
        const uint64_t n = frames.size();
        Fragged out;
        out.offsets.assign(1, 0);
        (void)option.get();
        if (n == 0) return out;
        HostBatch hb(*this, frames);
        uint32_t* d_first = static_cast<uint32_t*>(scratch(55, (n + 1) * 4));
        uint64_t* d_bytes = static_cast<uint64_t*>(scratch(56, (n + 1) * 8));
        nexg_fragged* d_rows = static_cast<nexg_fragged*>(scratch(57, n * sizeof(nexg_fragged)));
        const FragmentTotals t = fragment_plan(hb.fb, option, d_first, d_bytes, d_rows);
        uint64_t* d_off = static_cast<uint64_t*>(scratch(58, (t.frames + 1) * 8));
        uint32_t* d_len = static_cast<uint32_t*>(scratch(59, t.frames * 4));
        uint32_t* d_src = static_cast<uint32_t*>(scratch(60, t.frames * 4));
        uint8_t* d_data = static_cast<uint8_t*>(scratch(61, t.bytes));
        fragment(hb.fb, option, d_first, d_bytes, t.frames, d_off, d_len, d_src, d_data, t.bytes);
        out.rows.resize(n);
        out.offsets.resize(t.frames + 1);
        out.lengths.resize(t.frames);
        out.src.resize(t.frames);
        out.data.resize(t.bytes);
        check_hip(hipMemcpyAsync(out.rows.data(), d_rows, n * sizeof(nexg_fragged), hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipMemcpyAsync(out.offsets.data(), d_off, (t.frames + 1) * 8, hipMemcpyDeviceToHost, stream_), "D2H");
        if (t.frames) {
            check_hip(hipMemcpyAsync(out.lengths.data(), d_len, t.frames * 4, hipMemcpyDeviceToHost, stream_), "D2H");
            check_hip(hipMemcpyAsync(out.src.data(), d_src, t.frames * 4, hipMemcpyDeviceToHost, stream_), "D2H");
        }
        if (t.bytes) check_hip(hipMemcpyAsync(out.data.data(), d_data, t.bytes, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        return out;
    }

    // What reassemble will write (nexg_reasm_plan): out_first and out_bytes
    // hold frames.count + 1 entries, rows frames.count. Returns the number
    // of output frames and their bytes (one stream synchronisation) to
    // allocate for reassemble. align: 1, 4, 8 or 16.
    FragmentTotals reassemble_plan(const nexg_frames& frames, uint32_t align, uint32_t* out_first, uint64_t* out_bytes,
                                   nexg_reasm* rows) {
        DeviceScope ds(device_);
        const uint64_t wsb = nexg_reasm_plan_workspace(frames.count);
        void* ws = scratch(62, wsb);
        check(nexg_reasm_plan(ctx_, &frames, align, out_first, out_bytes, rows, ws, wsb, stream_), "nexg_reasm_plan");
        uint32_t n = 0;
        FragmentTotals t{0, 0};
        check_hip(hipMemcpyAsync(&n, out_first + frames.count, 4, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipMemcpyAsync(&t.bytes, out_bytes + frames.count, 8, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        t.frames = n;
        return t;
    }

    // Every complete IPv4 datagram of the table as one frame at its head's
    // place, every frame that is no fragment unchanged, at out_data +
    // out_bytes[i] on, pads zero, nothing at or past out_cap
    // (nexg_reasm_frames); out_offsets (out_count + 1 entries), out_len and
    // out_src (out_count each) are the output frames' table and the head or
    // pass-through input frame of each.
    void reassemble(const nexg_frames& frames, uint32_t align, const nexg_reasm* rows, const uint32_t* out_first,
                    const uint64_t* out_bytes, uint64_t out_count, uint64_t* out_offsets, uint32_t* out_len, uint32_t* out_src,
                    uint8_t* out_data, uint64_t out_cap) {
        DeviceScope ds(device_);
        check(nexg_reasm_frames(ctx_, &frames, align, rows, out_first, out_bytes, out_count, out_offsets, out_len, out_src,
                                out_data, out_cap, stream_),
              "nexg_reasm_frames");
    }

    // The NEXG_REASM_HELD frames as a frame table over frames.data, in order
    // (nexg_reasm_held); the outputs hold frames.count entries. Returns the
    // number held (one stream synchronisation).
    uint64_t reassemble_held(const nexg_frames& frames, const nexg_reasm* rows, uint32_t* out_index, uint64_t* out_off,
                             uint32_t* out_len) {
        DeviceScope ds(device_);
        const uint64_t wsb = nexg_reasm_held_workspace(frames.count);
        void* ws = scratch(63, wsb);
        uint64_t* d_count = static_cast<uint64_t*>(scratch(64, 8));
        check(nexg_reasm_held(ctx_, &frames, rows, frames.count, out_index, out_off, out_len, d_count, ws, wsb, stream_),
              "nexg_reasm_held");
        return read_u64(d_count);
    }

    // reassemble of host frames: output frame f lies in `data` at offsets[f],
    // lengths[f] bytes, and its head or pass-through was input frame src[f];
    // rows has one entry per input frame; held lists the input frames that
    // wait for the rest of their datagram.
    struct Reassembled {
        std::vector<nexg_reasm> rows;
        std::vector<uint64_t> offsets;  // lengths.size() + 1
        std::vector<uint32_t> lengths, src, held;
        std::vector<uint8_t> data;
    };
    Reassembled reassemble_bufs(const std::vector<std::vector<uint8_t>>& frames, uint32_t align = 1) {
        DeviceScope ds(device_);
        const uint64_t n = frames.size();
        Reassembled out;
        out.offsets.assign(1, 0);
        if (align != 1 && align != 4 && align != 8 && align != 16) throw Error("reassemble: align must be 1, 4, 8 or 16");
        if (n == 0) return out;
        HostBatch hb(*this, frames);
        uint32_t* d_first = static_cast<uint32_t*>(scratch(65, (n + 1) * 4));
        uint64_t* d_bytes = static_cast<uint64_t*>(scratch(66, (n + 1) * 8));
        nexg_reasm* d_rows = static_cast<nexg_reasm*>(scratch(67, n * sizeof(nexg_reasm)));
        const FragmentTotals t = reassemble_plan(hb.fb, align, d_first, d_bytes, d_rows);
        uint64_t* d_off = static_cast<uint64_t*>(scratch(68, (t.frames + 1) * 8));
        uint32_t* d_len = static_cast<uint32_t*>(scratch(69, t.frames * 4));
        uint32_t* d_src = static_cast<uint32_t*>(scratch(70, t.frames * 4));
        uint8_t* d_data = static_cast<uint8_t*>(scratch(71, t.bytes));
        reassemble(hb.fb, align, d_rows, d_first, d_bytes, t.frames, d_off, d_len, d_src, d_data, t.bytes);
        uint32_t* h_index = static_cast<uint32_t*>(scratch(72, n * 4));
        uint64_t* h_off = static_cast<uint64_t*>(scratch(73, n * 8));
        uint32_t* h_len = static_cast<uint32_t*>(scratch(74, n * 4));
        const uint64_t held = reassemble_held(hb.fb, d_rows, h_index, h_off, h_len);
        out.rows.resize(n);
        out.offsets.resize(t.frames + 1);
        out.lengths.resize(t.frames);
        out.src.resize(t.frames);
        out.held.resize(held);
        out.data.resize(t.bytes);
        check_hip(hipMemcpyAsync(out.rows.data(), d_rows, n * sizeof(nexg_reasm), hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipMemcpyAsync(out.offsets.data(), d_off, (t.frames + 1) * 8, hipMemcpyDeviceToHost, stream_), "D2H");
        if (t.frames) {
            check_hip(hipMemcpyAsync(out.lengths.data(), d_len, t.frames * 4, hipMemcpyDeviceToHost, stream_), "D2H");
            check_hip(hipMemcpyAsync(out.src.data(), d_src, t.frames * 4, hipMemcpyDeviceToHost, stream_), "D2H");
        }
        if (held) check_hip(hipMemcpyAsync(out.held.data(), h_index, held * 4, hipMemcpyDeviceToHost, stream_), "D2H");
        if (t.bytes) check_hip(hipMemcpyAsync(out.data.data(), d_data, t.bytes, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        return out;
    }

   private:
    void* upload(size_t slot, const void* src, size_t n) {
        void* d = scratch(slot, n);
        if (n) check_hip(hipMemcpyAsync(d, src, n, hipMemcpyHostToDevice, stream_), "H2D");
        return d;
    }
    std::vector<std::vector<uint8_t>> download_frames(const void* d_out, uint64_t n, uint32_t L) {
        std::vector<uint8_t> host(n * L);
        check_hip(hipMemcpyAsync(host.data(), d_out, host.size(), hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        std::vector<std::vector<uint8_t>> frames;
        frames.reserve(n);
        for (uint64_t i = 0; i < n; i++) frames.emplace_back(host.begin() + i * L, host.begin() + (i + 1) * L);
        return frames;
    }
    // per-tuple addresses / ids into nexg_ip_build (scratch slots first .. first+2)
    template <class Tuple>
    void fill_ip(nexg_ip_build& ip, const std::vector<Tuple>& t, const MacAddr& smac, const MacAddr& dmac,
                 uint8_t fam, uint8_t ttl, uint8_t ip_flags, uint8_t tos, uint32_t flow_label, size_t first) {
        const size_t w = fam == 4 ? 4 : 16;
        std::vector<uint8_t> src(t.size() * w), dst(t.size() * w);
        std::vector<uint16_t> id(t.size());
        for (size_t i = 0; i < t.size(); i++) {
            memcpy(src.data() + i * w, t[i].source.octets.data(), w);
            memcpy(dst.data() + i * w, t[i].destination.octets.data(), w);
            id[i] = t[i].ip_id;
        }
        ip.src_ip = static_cast<const uint8_t*>(upload(first, src.data(), src.size()));
        ip.dst_ip = static_cast<const uint8_t*>(upload(first + 1, dst.data(), dst.size()));
        ip.ip_id = fam == 4 ? static_cast<const uint16_t*>(upload(first + 2, id.data(), id.size() * 2)) : nullptr;
        ip.family = fam;
        ip.flow_label = flow_label;
        memcpy(ip.def_src_mac, smac.data(), 6);
        memcpy(ip.def_dst_mac, dmac.data(), 6);
        ip.ttl = ttl;
        ip.ip_flags = ip_flags;
        ip.tos = tos;
    }
    // grow-only device scratch, one buffer per slot: every call ends with a
    // stream sync, so the next call may reuse them (no hipMalloc per batch)
    struct Scratch {
        void* p = nullptr;
        size_t size = 0;
    };
    std::vector<Scratch> scratch_;
    int device_ = 0;
    void* scratch(size_t slot, size_t n) {
        if (slot >= scratch_.size()) scratch_.resize(slot + 1);
        Scratch& b = scratch_[slot];
        if (b.size < n || !b.p) {
            if (b.p) (void)hipFree(b.p);
            b.p = nullptr;
            b.size = 0;
            check_hip(hipMalloc(&b.p, n ? n : 16), "hipMalloc");
            b.size = n ? n : 16;
        }
        return b.p;
    }
    // one count or total a call left in device memory; waits for the stream
    uint64_t read_u64(const uint64_t* device) {
        uint64_t v = 0;
        check_hip(hipMemcpyAsync(&v, device, 8, hipMemcpyDeviceToHost, stream_), "D2H");
        check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        return v;
    }
    // host frames packed (4-B aligned starts) with offsets + lengths, on the device
    struct HostBatch {
        std::vector<uint8_t> data;
        std::vector<uint64_t> offs;
        std::vector<uint32_t> lens;
        nexg_frames fb{};
        HostBatch(Engine& e, const std::vector<std::vector<uint8_t>>& frames)
            : offs(frames.size()), lens(frames.size()) {
            uint64_t pos = 0;
            for (size_t i = 0; i < frames.size(); i++) {
                offs[i] = pos;
                lens[i] = (uint32_t)frames[i].size();
                pos += (frames[i].size() + 3) & ~(uint64_t)3;
            }
            data.assign(pos ? pos : 16, 0);
            for (size_t i = 0; i < frames.size(); i++)
                if (!frames[i].empty()) memcpy(data.data() + offs[i], frames[i].data(), frames[i].size());
            void* d_data = e.scratch(0, data.size());
            void* d_offs = e.scratch(1, offs.size() * 8);
            void* d_lens = e.scratch(2, lens.size() * 4);
            check_hip(hipMemcpyAsync(d_data, data.data(), data.size(), hipMemcpyHostToDevice, e.stream_), "H2D");
            check_hip(hipMemcpyAsync(d_offs, offs.data(), offs.size() * 8, hipMemcpyHostToDevice, e.stream_), "H2D");
            check_hip(hipMemcpyAsync(d_lens, lens.data(), lens.size() * 4, hipMemcpyHostToDevice, e.stream_), "H2D");
            fb.data = static_cast<const uint8_t*>(d_data);
            fb.data_bytes = data.size();
            fb.offsets = static_cast<const uint64_t*>(d_offs);
            fb.lengths = static_cast<const uint32_t*>(d_lens);
            fb.count = frames.size();
        }
    };

   public:
    Result<Frame> try_from_buf(const std::vector<uint8_t>& frame, ParseOption option = {},
                               ParseMode mode = ParseMode::Lenient) {
        return std::move(try_from_bufs({frame}, option, mode)[0]);
    }

   private:
    void check(int rc, const char* what) {
        if (rc != NEXG_OK)
            throw Error(std::string(what) + " failed: " + (ctx_ ? nexg_ctx_last_error(ctx_) : "no context"));
    }
    static void check_hip(hipError_t e, const char* what) {
        if (e != hipSuccess) throw Error(std::string(what) + ": " + hipGetErrorString(e));
    }
    nexg_ctx* ctx_ = nullptr;
    hipStream_t stream_ = nullptr;
};

/* ---- capture-file source (nexg_pcap_*; pcap::from_file, pcap.rs:95-109) -- */

class PcapReader {  // classic pcap / pcapng, a batch of records per call
   public:
    explicit PcapReader(const std::string& path) {
        if (nexg_pcap_open(path.c_str(), &p_) != NEXG_OK) throw Error("cannot open " + path + " as pcap/pcapng");
    }
    ~PcapReader() {
        if (p_) nexg_pcap_close(p_);
    }
    PcapReader(const PcapReader&) = delete;
    PcapReader& operator=(const PcapReader&) = delete;

    int linktype() const { return nexg_pcap_linktype(p_); }  // 1 Ethernet, 101 raw IP
    // ParseOption a capture of this link type needs (raw IP: from_ip_packet, offset 0)
    ParseOption parse_option() const {
        ParseOption o;
        o.from_ip_packet = linktype() == 101;
        return o;
    }
    // up to max_frames records (fewer at the end of the file, none after it);
    // throws on a malformed file after the complete records before the damage
    std::vector<std::vector<uint8_t>> next_batch(uint64_t max_frames, uint64_t data_cap = 64u << 20) {
        buf_.resize(data_cap);
        offs_.resize(max_frames + 1);
        uint64_t n = 0;
        if (nexg_pcap_read_batch(p_, buf_.data(), buf_.size(), offs_.data(), max_frames, nullptr, &n) != NEXG_OK)
            throw Error(std::string("capture read failed: ") + nexg_pcap_last_error(p_));
        std::vector<std::vector<uint8_t>> frames(n);
        for (uint64_t i = 0; i < n; i++) frames[i].assign(buf_.begin() + offs_[i], buf_.begin() + offs_[i + 1]);
        return frames;
    }

    // Zero-copy shape (nexg_pcap_map / nexg_pcap_walk_mapped): the file's
    // page-cache mapping (valid while the reader lives) and the records of
    // one window of it, described in place; register the mapping for DMA
    // (hipHostRegister) and copy [from, next) to the device as is.
    struct MappedWindow {
        uint64_t from = 0, next = 0;     // file range of the complete records
        std::vector<uint64_t> offsets;  // relative to from
        std::vector<uint32_t> lengths;
    };
    const uint8_t* map(uint64_t* size, uint64_t* first) {
        const uint8_t* d = nullptr;
        if (nexg_pcap_map(p_, &d, size, first) != NEXG_OK)
            throw Error(std::string("capture map failed: ") + nexg_pcap_last_error(p_));
        return d;
    }
    // records of [pos, pos + max_bytes); pos advances past them (end of file: pos == size)
    MappedWindow walk_mapped(uint64_t& pos, uint64_t max_bytes, uint64_t max_frames) {
        MappedWindow w;
        w.from = pos;
        w.offsets.resize(max_frames);
        w.lengths.resize(max_frames);
        uint64_t n = 0;
        if (nexg_pcap_walk_mapped(p_, pos, max_bytes, w.offsets.data(), w.lengths.data(), max_frames, nullptr, &n,
                                  &w.next) != NEXG_OK)
            throw Error(std::string("capture walk failed: ") + nexg_pcap_last_error(p_));
        w.offsets.resize(n);
        w.lengths.resize(n);
        pos = w.next;
        return w;
    }

   private:
    nexg_pcap* p_ = nullptr;
    std::vector<uint8_t> buf_;
    std::vector<uint64_t> offs_;
};

/* ---- live datalink (nexg_rx_* / nexg_tx_*; nex-datalink's Linux channel) -- */

namespace datalink {

enum class FanoutType : uint32_t {  // lib.rs:70-90
    HASH = NEXG_FANOUT_HASH, LB = NEXG_FANOUT_LB, CPU = NEXG_FANOUT_CPU,
    ROLLOVER = NEXG_FANOUT_ROLLOVER, RND = NEXG_FANOUT_RND, QM = NEXG_FANOUT_QM
};
struct FanoutOption {  // lib.rs:92-131
    uint16_t group_id = 0;
    FanoutType fanout_type = FanoutType::HASH;
    bool defrag = false, rollover = false;
};
struct Config {  // lib.rs:229-240 (the Linux knobs) + the batch ring
    uint32_t read_buffer_size = 4096;
    int32_t read_timeout_ms = -1;  // read_timeout: None
    bool promiscuous = true;
    bool has_fanout = false;
    FanoutOption linux_fanout{};
    uint32_t mode = NEXG_RX_RING;  // or NEXG_RX_MMSG
    uint32_t ring_block_size = 1u << 20, ring_blocks = 64, ring_block_tov_ms = 2;
    bool skip_outgoing = false;
};

// RawReceiver::next (linux.rs:356-397), a batch of frames per call
class RawReceiver {
   public:
    RawReceiver(const std::string& ifname, const Config& c = {}) {
        nexg_rx_config k;
        nexg_rx_config_default(&k);
        k.read_buffer_size = c.read_buffer_size;
        k.read_timeout_ms = c.read_timeout_ms;
        k.promiscuous = c.promiscuous;
        k.fanout = c.has_fanout;
        k.fanout_type = (uint32_t)c.linux_fanout.fanout_type | (c.linux_fanout.defrag ? NEXG_FANOUT_FLAG_DEFRAG : 0u) |
                        (c.linux_fanout.rollover ? NEXG_FANOUT_FLAG_ROLLOVER : 0u);
        k.fanout_group = c.linux_fanout.group_id;
        k.mode = c.mode;
        k.ring_block_size = c.ring_block_size;
        k.ring_blocks = c.ring_blocks;
        k.ring_block_tov_ms = c.ring_block_tov_ms;
        k.flags = c.skip_outgoing ? NEXG_RX_SKIP_OUTGOING : 0u;
        const int rc = nexg_rx_open(ifname.c_str(), &k, &rx_);
        if (rc != NEXG_OK) throw Error("nexg_rx_open(" + ifname + "): " + nexg_strerror(rc));
    }
    ~RawReceiver() {
        if (rx_) nexg_rx_close(rx_);
    }
    RawReceiver(const RawReceiver&) = delete;
    RawReceiver& operator=(const RawReceiver&) = delete;
    // frames already received (waits up to the read timeout for the first)
    std::vector<std::vector<uint8_t>> next_batch(uint64_t max_frames = 4096, uint64_t data_cap = 16u << 20) {
        buf_.resize(data_cap);
        offs_.resize(max_frames + 1);
        uint64_t n = 0;
        const int rc = nexg_rx_next_batch(rx_, buf_.data(), buf_.size(), offs_.data(), max_frames, nullptr, &n);
        if (rc != NEXG_OK) throw Error(std::string("nexg_rx_next_batch: ") + nexg_strerror(rc));
        std::vector<std::vector<uint8_t>> frames(n);
        for (uint64_t i = 0; i < n; i++) frames[i].assign(buf_.begin() + offs_[i], buf_.begin() + offs_[i + 1]);
        return frames;
    }
    nexg_rx* handle() const { return rx_; }

   private:
    nexg_rx* rx_ = nullptr;
    std::vector<uint8_t> buf_;
    std::vector<uint64_t> offs_;
};

// RawSender::send (linux.rs:302-346), a batch per call (sendmmsg)
class RawSender {
   public:
    explicit RawSender(const std::string& ifname) {
        const int rc = nexg_tx_open(ifname.c_str(), &tx_);
        if (rc != NEXG_OK) throw Error("nexg_tx_open(" + ifname + "): " + nexg_strerror(rc));
    }
    ~RawSender() {
        if (tx_) nexg_tx_close(tx_);
    }
    RawSender(const RawSender&) = delete;
    RawSender& operator=(const RawSender&) = delete;
    // frames the kernel accepted
    uint64_t send_batch(const std::vector<std::vector<uint8_t>>& frames) {
        std::vector<uint8_t> data;
        std::vector<uint64_t> offs(frames.size() + 1, 0);
        for (size_t i = 0; i < frames.size(); i++) {
            data.insert(data.end(), frames[i].begin(), frames[i].end());
            offs[i + 1] = data.size();
        }
        uint64_t sent = 0;
        const int rc = nexg_tx_send_batch(tx_, data.data(), offs.data(), nullptr, 0, frames.size(), &sent);
        if (rc != NEXG_OK) throw Error(std::string("nexg_tx_send_batch: ") + nexg_strerror(rc));
        return sent;
    }

   private:
    nexg_tx* tx_ = nullptr;
};

}  // namespace datalink

}  // namespace nexg

#endif  // NEXG_HPP
