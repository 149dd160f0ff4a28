/*
 * nexg.h — C ABI of the MI355X-native batched packet-dissect + checksum engine.
 *
 * This is the drop-in boundary for nex-packet's per-frame hot path
 * (shellrow/nex, reference mounted at /root/reference). The reference exposes
 * only a Rust API; each entry point below replaces a family of Rust calls that
 * the callers (examples/parse_frame.rs, examples/dump.rs, examples/udp_ping.rs)
 * make one frame at a time:
 *
 *   nexg_parse_batch      <- frame::Frame::try_from_buf / try_from_buf_with_mode
 *                            (nex-packet/src/frame.rs:299, :309) evaluated on N
 *                            frames, fused with the verification checksums
 *                            ipv4::checksum (ipv4.rs:932), udp::checksum
 *                            (udp.rs:443), tcp::checksum (tcp.rs:1207),
 *                            icmp::checksum (icmp.rs:429), icmpv6::checksum
 *                            (icmpv6.rs:589).
 *   nexg_checksum_batch   <- util::checksum (nex-packet/src/util.rs:65) on N
 *                            independent buffers.
 *   nexg_build_udp4_batch <- UdpPacketBuilder::build (builder/udp.rs:67) +
 *                            Ipv4PacketBuilder::to_bytes (builder/ipv4.rs:94,168)
 *                            + EthernetPacketBuilder::to_bytes
 *                            (builder/ethernet.rs:68), the udp_ping.rs:68-109
 *                            composition, on N parameter tuples.
 *   nexg_gen_frames       <- synthetic workload synthesis;
 *                            no reference counterpart (bench/test inputs).
 *
 * Conventions:
 *   - Plain C: no exceptions cross the ABI; every call returns an int status
 *     (NEXG_OK = 0, negative on error) and never aborts.
 *   - All frame / output buffers are DEVICE pointers owned by the caller;
 *     work is enqueued on `stream` (a hipStream_t, NULL = default stream) and
 *     is stream-ordered: the call returns before the kernels finish. Calls
 *     on one context may use different streams: the context's one device
 *     scratch (TwoPass tail sums) is handed between streams with an event.
 *   - One context per device; a context is not thread-safe (the reference's
 *     RawReceiver is likewise single-consumer, nex-datalink/src/lib.rs:363).
 *   - Frame-level parse failures are data, not call errors: they are reported
 *     per frame in the status field (ParseError kinds, parse.rs:51-97).
 */
#ifndef NEXG_H
#define NEXG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NEXG_ABI_VERSION 1

/* ---- call status ------------------------------------------------------ */
enum {
    NEXG_OK = 0,
    NEXG_EINVAL = -1,  /* bad argument (NULL pointer, unsupported layout) */
    NEXG_ENOMEM = -2,  /* host allocation failed                          */
    NEXG_EDEVICE = -3, /* HIP device error / not a gfx950 device          */
    NEXG_ELAUNCH = -4, /* kernel launch failed                            */
    NEXG_ERANGE = -5,  /* BuildError::LengthOverflow (builder/error.rs:8)  */
    NEXG_EPERM = -6,   /* datalink socket: no CAP_NET_RAW                 */
    NEXG_EIO = -7      /* datalink socket / ring system call failed       */
};

/* ---- per-frame status: ParseError kind (parse.rs:51-97) --------------- */
enum {
    NEXG_FRAME_OK = 0,
    NEXG_ERR_BUFFER_TOO_SHORT = 1, /* ParseError::BufferTooShort */
    NEXG_ERR_INVALID_LENGTH = 2,   /* ParseError::InvalidLength  */
    NEXG_ERR_MALFORMED = 3,        /* ParseError::Malformed      */
    NEXG_ERR_TRUNCATED = 4,        /* ParseError::Truncated      */
    NEXG_ERR_BAD_EXTENT = 7        /* caller error: frame extent past data_bytes
                                      or longer than 65535 bytes (no Frame)   */
};

/* ---- ParseOption / ParseMode (frame.rs:47-50, parse.rs:34-46) ---------- */
#define NEXG_PARSE_STRICT 0x1u  /* ParseMode::Strict (default Lenient)        */
#define NEXG_PARSE_FROM_IP 0x2u /* ParseOption.from_ip_packet (ip_offset used) */
/* Extension (Frame itself never unwraps VLAN, Q3): before
 * dispatching on the EtherType, unwrap up to two 802.1Q / 802.1ad / QinQ tags
 * (EtherType 0x8100 / 0x88A8 / 0x9100) as VlanPacket::try_from_buf reads one
 * (vlan.rs:102-127: 2-B TCI, inner EtherType), when all 4 bytes are present.
 * The record's ethertype is the inner one, l3_off moves by 4 per tag, the
 * tags stay readable at frame bytes [12, l3_off - 2); NEXG_L_VLAN is set. */
#define NEXG_PARSE_VLAN 0x4u

typedef struct nexg_parse_option {
    uint32_t flags;     /* NEXG_PARSE_* */
    uint32_t ip_offset; /* ParseOption.offset, used with NEXG_PARSE_FROM_IP */
} nexg_parse_option;

/* ---- per-frame flags word (shared by nexg_desc and nexg_record) --------
 * Layer bits mirror the Option<> structure of frame::Frame (frame.rs:21-60).
 * Checksum bits record the verify semantics DESIGN.md §3 states:
 *   ip ok  := ipv4::checksum(&Ipv4Packet) == header.checksum
 *   l4 ok  := {tcp,udp}::checksum(&pkt,&src,&dst) == header.checksum,
 *             icmp::checksum(&pkt) / icmpv6::checksum(&pkt,&src,&dst) likewise.
 * Bits 24..26 hold the frame status (NEXG_FRAME_OK / NEXG_ERR_*). */
#define NEXG_L_ETHERNET (1u << 0)  /* datalink.ethernet is Some            */
#define NEXG_L_ARP (1u << 1)       /* datalink.arp is Some                 */
#define NEXG_L_IP (1u << 2)        /* frame.ip is Some (maybe all-None)    */
#define NEXG_L_IPV4 (1u << 3)      /* ip.ipv4 is Some                      */
#define NEXG_L_IPV6 (1u << 4)      /* ip.ipv6 is Some                      */
#define NEXG_L_ICMP (1u << 5)      /* ip.icmp is Some                      */
#define NEXG_L_ICMPV6 (1u << 6)    /* ip.icmpv6 is Some                    */
#define NEXG_L_TRANSPORT (1u << 7) /* frame.transport is Some              */
#define NEXG_L_TCP (1u << 8)       /* transport.tcp is Some                */
#define NEXG_L_UDP (1u << 9)       /* transport.udp is Some                */
#define NEXG_C_IP_CHECKED (1u << 10) /* IPv4 header checksum evaluated     */
#define NEXG_C_IP_OK (1u << 11)      /* ... and equals the stored field    */
#define NEXG_C_IP_PANIC (1u << 12)   /* ipv4::checksum would panic (Q17)   */
#define NEXG_C_L4_CHECKED (1u << 13) /* L4 checksum evaluated              */
#define NEXG_C_L4_OK (1u << 14)      /* ... and equals the stored field    */
#define NEXG_L_VLAN (1u << 15)       /* NEXG_PARSE_VLAN unwrapped >= 1 tag  */
#define NEXG_STATUS_SHIFT 24
#define NEXG_STATUS(flags) (((flags) >> NEXG_STATUS_SHIFT) & 0x7u)

/* Compact 8-byte result per frame (out_kind NEXG_OUT_DESC). Together with the
 * frame bytes it determines the whole frame::Frame (nex_amd/frame.py
 * materialises it): header fields sit at fixed offsets of their layer.
 * payload_off/len locate Frame.payload inside the frame; an empty payload is
 * reported as (0, 0). */
typedef struct nexg_desc {
    uint32_t flags;
    uint16_t payload_off;
    uint16_t payload_len;
} nexg_desc;

/* Full decoded record per frame (out_kind NEXG_OUT_RECORD), 64 bytes.
 * Field values are the reference's parsed values (ipv4.rs:510-528,
 * ipv6.rs:259-268, tcp.rs:820-835, udp.rs:227-235, icmp.rs:188-204,
 * arp.rs:340-371). Fields of absent layers are 0.
 *
 * A frame whose status is a ParseError kind carries the error's payload
 * (parse.rs:53-81) and nothing else:
 *   l4_type = NEXG_CTX_* (which reference check failed: its context string)
 *   ip_src  = BufferTooShort.minimum | InvalidLength.value | Truncated.expected
 *   ip_dst  = BufferTooShort.actual  | Truncated.actual       (else 0) */
enum {
    NEXG_CTX_NONE = 0,
    NEXG_CTX_ETHERNET_PACKET = 1,     /* "Ethernet packet"  ethernet.rs:310-316           */
    NEXG_CTX_DUMMY_ETHERNET = 2,      /* "Frame dummy Ethernet classification" frame.rs:585 */
    NEXG_CTX_IPV4_PACKET = 3,         /* "IPv4 packet"  BufferTooShort ipv4.rs:380-386,
                                         Truncated (strict) ipv4.rs:429-435                */
    NEXG_CTX_IPV4_VERSION = 4,        /* "IPv4 packet version"  ipv4.rs:388-393           */
    NEXG_CTX_IPV4_HEADER_LENGTH = 5,  /* "IPv4 header length"  ipv4.rs:395-401            */
    NEXG_CTX_IPV4_HEADER = 6,         /* "IPv4 header"  ipv4.rs:403-410                   */
    NEXG_CTX_IPV4_TOTAL_LENGTH = 7,   /* "IPv4 total length" (value = declared) 421-427   */
    NEXG_CTX_IPV4_OPTIONS = 8,        /* "IPv4 options" (strict)  ipv4.rs:476-481          */
    NEXG_CTX_IPV4_OPTION_LENGTH = 9,  /* "IPv4 option length" (strict)  ipv4.rs:485-491    */
    NEXG_CTX_IPV6_PACKET = 10,        /* "IPv6 packet"  ipv6.rs:225-231                   */
    NEXG_CTX_IPV6_VERSION = 11,       /* "IPv6 packet version"  ipv6.rs:235-239           */
    NEXG_CTX_IPV6_PAYLOAD = 12,       /* "IPv6 payload" (strict)  ipv6.rs:271-277          */
    NEXG_CTX_IPV6_EXTENSION = 13,     /* "IPv6 extension header"  ipv6.rs:288-308         */
    NEXG_CTX_IPV6_ROUTING = 14,       /* "IPv6 routing header"  ipv6.rs:319-335           */
    NEXG_CTX_IPV6_FRAGMENT = 15       /* "IPv6 fragment header"  ipv6.rs:346-352          */
};
typedef struct nexg_record {
    uint32_t flags;          /* as nexg_desc.flags                              */
    uint16_t payload_off;    /* Frame.payload offset in the frame               */
    uint16_t payload_len;    /* Frame.payload length                            */
    uint16_t packet_len;     /* Frame.packet_len (frame.rs:575)                 */
    uint16_t ethertype;      /* EtherType value (dummy value when FROM_IP)      */
    uint16_t l3_off;         /* offset of the IP / ARP header                   */
    uint16_t l4_off;         /* offset of the TCP/UDP/ICMP header (0 if none)   */
    uint8_t ip_ver_ihl;      /* v4: version<<4|ihl  v6: version<<4  arp: hlen    */
    uint8_t ip_tos;          /* v4: dscp<<2|ecn     v6: traffic_class arp: plen  */
    uint16_t ip_length;      /* v4: total_length (effective, Q5) v6: payload_length */
    uint32_t ip_word;        /* v4: identification<<16 | flags<<13 | frag_off    */
                             /* v6: flow_label                                   */
    uint8_t ip_ttl;          /* v4: ttl   v6: hop_limit                          */
    uint8_t ip_proto;        /* IpNextProtocol::value() of v4 proto / v6 nh (Q8) */
    uint8_t ip_nopt;         /* v4: options.len()  v6: extensions.len()          */
    uint8_t l4_nopt;         /* tcp: options.len()                               */
    uint32_t ip_src;         /* v4 / arp sender proto addr, as a BE u32 value   */
    uint32_t ip_dst;         /* v4 / arp target proto addr                       */
    uint16_t ip_csum;        /* v4 header checksum field                         */
    uint16_t ip_csum_calc;   /* ipv4::checksum(&pkt) (0 if not evaluated)        */
    uint16_t l4_csum;        /* tcp/udp/icmp/icmpv6 checksum field               */
    uint16_t l4_csum_calc;   /* reference checksum of the L4 packet              */
    uint16_t src_port;       /* tcp/udp source      arp: hardware_type           */
    uint16_t dst_port;       /* tcp/udp destination arp: protocol_type           */
    uint16_t l4_length;      /* udp: length  tcp: data_offset*4  arp: operation  */
    uint8_t l4_type;         /* icmp(v6) type   tcp: flags                       */
    uint8_t l4_code;         /* icmp(v6) code   tcp: data_offset<<4|reserved     */
    uint32_t tcp_seq;
    uint32_t tcp_ack;
    uint16_t tcp_window;
    uint16_t tcp_urg;
} nexg_record;

#define NEXG_OUT_DESC 1
#define NEXG_OUT_RECORD 2
#define NEXG_OUT_SLICE 3
/* Flags-only result per frame (out_kind NEXG_OUT_FLAGS), 4 bytes: exactly
 * nexg_desc.flags (layer presence, checksum verdicts, status) without the
 * payload location — for consumers that only classify and verify. On HBM the
 * 8-B descriptor stream costs ~18 % of the read rate at 64-B frames; 4 B
 * halves that. */
#define NEXG_OUT_FLAGS 4
/* Verdict per frame (out_kind NEXG_OUT_VERDICT), 2 bytes, lossless for the
 * flags word: a parsed frame stores flags & 0xFFFF (layer and checksum bits;
 * bits 16..23 are never set), a frame with a nonzero status (no layers) stores
 * NEXG_VERDICT_ERR | status << 3. NEXG_L_ARP together with NEXG_L_IP marks it:
 * a Frame never holds both datalink.arp and ip (frame.rs:596-607). Output
 * alignment 2 B. Explicit-length batches (TwoPass layout) run the lane-window
 * kernel for this output. */
#define NEXG_OUT_VERDICT 5
#define NEXG_VERDICT_ERR (NEXG_L_ARP | NEXG_L_IP)
#define NEXG_VERDICT_FLAGS(v)                                                        \
    ((((v) & NEXG_VERDICT_ERR) == NEXG_VERDICT_ERR) ? ((((uint32_t)(v) >> 3) & 0x7u) \
                                                       << NEXG_STATUS_SHIFT)         \
                                                    : (uint32_t)(v))

/* Sparse descriptors (out_kind NEXG_OUT_SPARSE): lossless for nexg_desc at
 * 1 B per frame whenever the frame has one of the canonical shapes below
 * (every frame of the synthetic 64-B and IMIX workloads does), plus the full
 * 8-B descriptor for every other frame. `out` (16-B aligned) holds
 *   codes : uint8_t[count]                 at out
 *   exc   : nexg_desc[count] (capacity)    at out + NEXG_SPARSE_EXC_OFFSET(count)
 * The k-th exception (code 0) of the 64-frame group g = i / 64, counted in
 * frame order, is stored at exc[64 * g + k]; nothing else of exc is written.
 * Code byte: bits 0..3 shape, bit 4 NEXG_C_IP_OK, bit 5 NEXG_C_L4_OK, bits
 * 6..7 number of VLAN tags unwrapped (NEXG_PARSE_VLAN). With L = l3 offset
 * = (FROM_IP ? ip_offset : 14) + 4 * tags, h = L + NEXG_SHAPE_HDR(shape):
 *   flags       = NEXG_SHAPE_FLAGS(shape) | ok bits | (tags ? NEXG_L_VLAN : 0)
 *   payload_len = len - h, payload_off = payload_len ? h : 0
 * for shapes 1..9; shape 10 (IP layer present but all None, Q4/Q12) has an
 * empty payload; shapes 11..15 are error statuses 1..4, 7 (no layers, empty
 * payload). The device encoder stores a code only when this decodes to the
 * frame's exact descriptor, so the output is lossless by construction;
 * nexg_sparse_expand (below) or nexg_sparse_decode restores nexg_desc. */
#define NEXG_OUT_SPARSE 6
#define NEXG_SPARSE_EXC_OFFSET(count) ((((uint64_t)(count)) + 15u) & ~(uint64_t)15u)
#define NEXG_SPARSE_BYTES(count) (NEXG_SPARSE_EXC_OFFSET(count) + 8u * (uint64_t)(count))
#define NEXG_SPARSE_IP_OK 0x10u
#define NEXG_SPARSE_L4_OK 0x20u
#define NEXG_SPARSE_TAG_SHIFT 6
enum {
    NEXG_SHAPE_EXCEPTION = 0,
    NEXG_SHAPE_V4_UDP = 1,   /* IPv4 IHL 5 + UDP, datagram to the frame end   */
    NEXG_SHAPE_V4_TCP = 2,   /* IPv4 IHL 5 + TCP data offset 5                */
    NEXG_SHAPE_V4_ICMP = 3,  /* IPv4 IHL 5 + ICMP                             */
    NEXG_SHAPE_V6_UDP = 4,   /* IPv6 without extensions + UDP                 */
    NEXG_SHAPE_V6_TCP = 5,   /* IPv6 + TCP data offset 5                      */
    NEXG_SHAPE_V6_ICMP = 6,  /* IPv6 + ICMPv6                                 */
    NEXG_SHAPE_ETH_ONLY = 7, /* EtherType not IPv4/IPv6/ARP (Q3)              */
    NEXG_SHAPE_V4_OTHER = 8, /* IPv4 IHL 5, no L4 layer (Q9, Q15)             */
    NEXG_SHAPE_V6_OTHER = 9, /* IPv6 without extensions, no L4 layer          */
    NEXG_SHAPE_IP_NONE = 10, /* ip = Some(all None), payload empty (Q4, Q12)  */
    NEXG_SHAPE_ERR_FIRST = 11 /* 11..14 = status 1..4, 15 = NEXG_ERR_BAD_EXTENT */
};
#define NEXG_SHAPE_V4_ (NEXG_L_ETHERNET | NEXG_L_IP | NEXG_L_IPV4 | NEXG_C_IP_CHECKED)
#define NEXG_SHAPE_V6_ (NEXG_L_ETHERNET | NEXG_L_IP | NEXG_L_IPV6)
#define NEXG_SHAPE_FLAGS(s)                                                                     \
    ((s) == 1 ? NEXG_SHAPE_V4_ | NEXG_L_TRANSPORT | NEXG_L_UDP | NEXG_C_L4_CHECKED            \
   : (s) == 2 ? NEXG_SHAPE_V4_ | NEXG_L_TRANSPORT | NEXG_L_TCP | NEXG_C_L4_CHECKED            \
   : (s) == 3 ? NEXG_SHAPE_V4_ | NEXG_L_ICMP | NEXG_C_L4_CHECKED                              \
   : (s) == 4 ? NEXG_SHAPE_V6_ | NEXG_L_TRANSPORT | NEXG_L_UDP | NEXG_C_L4_CHECKED            \
   : (s) == 5 ? NEXG_SHAPE_V6_ | NEXG_L_TRANSPORT | NEXG_L_TCP | NEXG_C_L4_CHECKED            \
   : (s) == 6 ? NEXG_SHAPE_V6_ | NEXG_L_ICMPV6 | NEXG_C_L4_CHECKED                            \
   : (s) == 7 ? NEXG_L_ETHERNET                                                               \
   : (s) == 8 ? NEXG_SHAPE_V4_                                                                \
   : (s) == 9 ? NEXG_SHAPE_V6_                                                                \
   : (s) == 10 ? NEXG_L_ETHERNET | NEXG_L_IP                                                  \
   : (s) >= 11 && (s) <= 14 ? (uint32_t)((s) - 10) << NEXG_STATUS_SHIFT                       \
   : (s) == 15 ? (uint32_t)NEXG_ERR_BAD_EXTENT << NEXG_STATUS_SHIFT : 0u)
/* bytes from the l3 offset to the payload: IP header + L4 header */
#define NEXG_SHAPE_HDR(s)                                                                       \
    ((s) == 1 ? 28u : (s) == 2 ? 40u : (s) == 3 ? 24u : (s) == 4 ? 48u : (s) == 5 ? 60u       \
   : (s) == 6 ? 44u : (s) == 8 ? 20u : (s) == 9 ? 40u : 0u)

/* nexg_desc of a frame from its sparse code (host side; the device encoder
 * uses the same table). len = the frame's length, flags/ip_offset = the
 * batch's parse option. Returns 0 for an exception code (look the descriptor
 * up in exc), 1 otherwise. */
static inline int nexg_sparse_decode(uint8_t code, uint32_t len, uint32_t parse_flags,
                                     uint32_t ip_offset, nexg_desc* d) {
    const uint32_t shape = code & 0xFu, tags = (uint32_t)code >> NEXG_SPARSE_TAG_SHIFT;
    if (shape == NEXG_SHAPE_EXCEPTION) return 0;
    d->flags = NEXG_SHAPE_FLAGS(shape);
    d->payload_off = 0;
    d->payload_len = 0;
    if (shape >= NEXG_SHAPE_IP_NONE) {
        if (shape == NEXG_SHAPE_IP_NONE && tags) d->flags |= NEXG_L_VLAN;
        return 1;
    }
    d->flags |= ((code & NEXG_SPARSE_IP_OK) ? NEXG_C_IP_OK : 0u) | ((code & NEXG_SPARSE_L4_OK) ? NEXG_C_L4_OK : 0u) |
                (tags ? NEXG_L_VLAN : 0u);
    const uint32_t h = ((parse_flags & NEXG_PARSE_FROM_IP) ? ip_offset : 14u) + 4u * tags + NEXG_SHAPE_HDR(shape);
    d->payload_len = (uint16_t)(len - h);
    d->payload_off = (uint16_t)(len > h ? h : 0u);
    return 1;
}

/* Grouped sparse descriptors (out_kind NEXG_OUT_GROUPED): NEXG_OUT_SPARSE's
 * codes with the common part of each 64-frame group g = i / 64 stored once.
 * A group whose frames all share one non-exception code up to its two
 * verdict bits is "uniform": heads[g] = that code with bits 4..5 clear, and
 * its verdicts are two 64-bit masks (bit i % 64 = NEXG_SPARSE_IP_OK /
 * NEXG_SPARSE_L4_OK of frame i); nothing else of the group is written
 * (17 B per 64 frames on single-shape traffic). Any other group is mixed and
 * stores its 1-B codes and exceptions as NEXG_OUT_SPARSE does, with heads[g]
 * = 0; or heads[g] = NEXG_GROUPED_TILE_RUN (the packed-batch kernel's form):
 * then the exceptions of its 256-frame tile T = i / 256 sit in one run, frame
 * i's at exc[256 T + k], k = the code-0 frames of [256 T, i) (one write burst
 * per tile instead of one per group: DESIGN.md §6 round 6). Every
 * area is written densely (a head byte per group, 16 B of masks per group):
 * interleaving them with the codes costs partial-line writes.
 * `out` (16-B aligned) holds
 *   heads : uint8_t[G]                     at out            (G = groups)
 *   masks : uint32_t[G][4] {ip lo, ip hi, l4 lo, l4 hi} at out + NEXG_GROUPED_MASK_OFFSET(count)
 *   codes : uint8_t[count]                 at out + NEXG_GROUPED_CODE_OFFSET(count)
 *   exc   : nexg_desc[count] (capacity)    at out + NEXG_GROUPED_EXC_OFFSET(count)
 * nexg_grouped_code gives frame i's NEXG_OUT_SPARSE code (then
 * nexg_sparse_decode), nexg_grouped_exc_slot the exc index of a code-0
 * frame; nexg_grouped_expand restores nexg_desc[count] on the device. */
#define NEXG_OUT_GROUPED 7
#define NEXG_GROUPED_GROUPS(count) ((((uint64_t)(count)) + 63u) >> 6)
#define NEXG_GROUPED_MASK_OFFSET(count) ((NEXG_GROUPED_GROUPS(count) + 15u) & ~(uint64_t)15u)
#define NEXG_GROUPED_CODE_OFFSET(count) (NEXG_GROUPED_MASK_OFFSET(count) + 16u * NEXG_GROUPED_GROUPS(count))
#define NEXG_GROUPED_EXC_OFFSET(count) ((NEXG_GROUPED_CODE_OFFSET(count) + (uint64_t)(count) + 15u) & ~(uint64_t)15u)
#define NEXG_GROUPED_BYTES(count) (NEXG_GROUPED_EXC_OFFSET(count) + 8u * (uint64_t)(count))
/* head of a mixed group whose exceptions are kept per 256-frame tile (its
 * shape bits are 0, so it is never a uniform group's head) */
#define NEXG_GROUPED_TILE_RUN 0x80u

/* frame i's NEXG_OUT_SPARSE code from a NEXG_OUT_GROUPED output (host side) */
static inline uint8_t nexg_grouped_code(const void* out, uint64_t count, uint64_t i) {
    const uint8_t* o = (const uint8_t*)out;
    const uint64_t g = i >> 6;
    const uint8_t head = o[g];
    if (!head || head == NEXG_GROUPED_TILE_RUN) return o[NEXG_GROUPED_CODE_OFFSET(count) + i];
    const uint8_t* m = o + NEXG_GROUPED_MASK_OFFSET(count) + 16u * g;
    /* the masks are little-endian words: bit b of a 64-bit mask is bit b % 8
     * of its byte b / 8 */
    const uint32_t b = (uint32_t)(i & 63u), byte = b >> 3, sh = b & 7u;
    const uint32_t ip = (m[byte] >> sh) & 1u, l4 = (m[8u + byte] >> sh) & 1u;
    return (uint8_t)(head | (ip ? NEXG_SPARSE_IP_OK : 0u) | (l4 ? NEXG_SPARSE_L4_OK : 0u));
}

/* index in the exc area of frame i's descriptor when its code is 0 (host
 * side): its group's run (heads[g] = 0) or its tile's (NEXG_GROUPED_TILE_RUN) */
static inline uint64_t nexg_grouped_exc_slot(const void* out, uint64_t count, uint64_t i) {
    const uint8_t* o = (const uint8_t*)out;
    const uint64_t first = o[i >> 6] == NEXG_GROUPED_TILE_RUN ? (i & ~(uint64_t)255u) : (i & ~(uint64_t)63u);
    uint64_t k = 0;
    for (uint64_t j = first; j < i; j++) k += nexg_grouped_code(out, count, j) == 0u;
    return first + k;
}

/* FrameSlice::try_from_buf (frame.rs:84-287) per frame, out_kind
 * NEXG_OUT_SLICE, 16 bytes: layer boundaries only, no checksums. FrameSlice
 * has no ParseMode (NEXG_PARSE_STRICT is ignored) and reports every inner
 * failure as an error; its walk differs from Frame's (AH is walked, ICMP
 * needs 4 B, UDP length is not checked). Ranges are frame-relative:
 *   datalink  = [0, 14)                          if NEXG_S_DATALINK
 *   network   = [l3_off, l3_off + l3_len)        if NEXG_S_NETWORK
 *   transport = [l3_off + l3_len, + l4_len)      if NEXG_S_TRANSPORT
 *   payload   = [payload_off, payload_off + payload_len)  (on success)
 * ethertype = EtherType::value(), ip_protocol (bits 8..15) =
 * IpNextProtocol::value() (143..252 -> 255). Status bits 24..26 as for
 * Frame: BufferTooShort / InvalidLength / Malformed / Truncated / BAD_EXTENT. */
#define NEXG_S_DATALINK (1u << 0)
#define NEXG_S_NETWORK (1u << 1)
#define NEXG_S_TRANSPORT (1u << 2)
#define NEXG_S_ETHERTYPE (1u << 3)
#define NEXG_S_IP_PROTOCOL (1u << 4)
#define NEXG_S_PROTO_SHIFT 8
typedef struct nexg_slice {
    uint32_t flags;
    uint16_t l3_off, l3_len, l4_len;
    uint16_t payload_off, payload_len;
    uint16_t ethertype;
} nexg_slice;

/* ---- frame batch layout ------------------------------------------------
 * Frame i occupies data[off(i), off(i)+len(i)):
 *   offsets == NULL : off(i) = i*stride
 *   offsets != NULL : off(i) = offsets[i]
 *   lengths != NULL : len(i) = lengths[i]
 *   lengths == NULL : len(i) = stride (offsets == NULL)
 *                     or offsets[i+1]-offsets[i] (offsets has count+1 entries)
 * Every len(i) must be <= 65535 (frames are at most one IPv4 datagram; the
 * reference's default read buffer is 4096, nex-datalink/src/lib.rs:229).
 * data_bytes bounds every frame extent: a frame reaching past data+data_bytes
 * gets NEXG_ERR_BAD_EXTENT. Device loads are whole 16-B aligned blocks: the
 * kernels read only inside the 16-B aligned blocks that overlap
 * [data, data + data_bytes) (bytes of those blocks outside the range may be
 * read and are ignored; such a block cannot cross a page, so this never
 * faults). All pointers are device pointers.
 *
 * hints: NEXG_FRAMES_MONOTONE (offsets + lengths layouts) promises that
 * offsets are nondecreasing and frames do not overlap, with small gaps
 * between consecutive frames (e.g. the 16-B record headers a capture file
 * keeps in place, nexg_pcap_read_raw). Such batches are streamed as
 * contiguous spans (gap bytes are read and ignored) instead of by the
 * two-pass explicit-length kernels. The kernels verify the promise per
 * 256-frame group and fall back to per-frame reads where it fails, so a
 * wrong hint costs speed, never correctness. */
#define NEXG_FRAMES_MONOTONE 0x1u
/* NEXG_FRAMES_OFFSETS32: `offsets` points to uint32_t entries (4 bytes per
 * frame instead of 8; any 4-B aligned address). offsets32[i] is offset(i)
 * modulo 2^32. When data_bytes > 0xFFFFFFFF the table is followed, at the
 * first 8-B aligned address past its count + 1 entries, by one uint64_t per
 * 256 frames, base[k] = offset(256 k) in full (nexg_offsets32_bases), and
 * offset(i) = base[i / 256] + (uint32_t)(offsets32[i] - (uint32_t)base[i / 256]):
 * every frame (and, packed, the end of its group) lies within 4 GiB after
 * its group's first frame, which packed and monotone batches satisfy by
 * construction. nexg_offsets32_bytes gives the whole table's size. */
#define NEXG_FRAMES_OFFSETS32 0x2u
typedef struct nexg_frames {
    const uint8_t* data;
    uint64_t data_bytes;
    const uint64_t* offsets;
    const uint32_t* lengths;
    uint32_t stride;
    uint32_t hints; /* NEXG_FRAMES_* */
    uint64_t count;
} nexg_frames;

/* NEXG_FRAMES_OFFSETS32 table of `count` frames: count + 1 uint32 entries,
 * then (for batches over 4 GiB) ceil((count + 1) / 256) uint64 group bases
 * at the next 8-B boundary. */
static inline const uint64_t* nexg_offsets32_bases(const void* table, uint64_t count) {
    const uintptr_t end = (uintptr_t)table + 4u * (uintptr_t)(count + 1u);
    return (const uint64_t*)((end + 7u) & ~(uintptr_t)7u);
}
static inline uint64_t nexg_offsets32_bytes(uint64_t count, int with_bases) {
    const uint64_t b = (4u * (count + 1u) + 7u) & ~(uint64_t)7u;
    return with_bases ? b + 8u * ((count + 1u + 255u) / 256u) : 4u * (count + 1u);
}

/* ---- context ----------------------------------------------------------- */
typedef struct nexg_ctx nexg_ctx;

int nexg_abi_version(void);
const char* nexg_strerror(int status);
/* Binds `device` (HIP ordinal); fails with NEXG_EDEVICE unless it is gfx950. */
int nexg_ctx_create(int device, nexg_ctx** out);
int nexg_ctx_destroy(nexg_ctx* ctx);
/* Message of the last failing call on ctx ("" if none). */
const char* nexg_ctx_last_error(const nexg_ctx* ctx);
/* Number of compute units of the bound device (for grid sizing by callers). */
int nexg_ctx_cu_count(const nexg_ctx* ctx);

/* ---- hot path ----------------------------------------------------------
 * Frame::try_from_buf_with_mode on every frame + checksum verification.
 * out_kind NEXG_OUT_DESC   -> out is nexg_desc[count]
 * out_kind NEXG_OUT_RECORD -> out is nexg_record[count]
 * out_kind NEXG_OUT_SLICE  -> out is nexg_slice[count] (FrameSlice, above) */
int nexg_parse_batch(nexg_ctx* ctx, const nexg_frames* frames,
                     const nexg_parse_option* option, int out_kind, void* out,
                     void* stream);

/* util::checksum(buf_i, skipword) for every buffer (util.rs:65-78). */
int nexg_checksum_batch(nexg_ctx* ctx, const nexg_frames* bufs,
                        uint32_t skipword, uint16_t* out, void* stream);

/* nexg_desc[count] from a NEXG_OUT_SPARSE result of the same batch and parse
 * option (codes + exceptions, layout above). Stream-ordered, device pointers. */
int nexg_sparse_expand(nexg_ctx* ctx, const nexg_frames* frames, const nexg_parse_option* option,
                       const void* sparse, nexg_desc* out, void* stream);
/* The same from a NEXG_OUT_GROUPED result. */
int nexg_grouped_expand(nexg_ctx* ctx, const nexg_frames* frames, const nexg_parse_option* option,
                        const void* grouped, nexg_desc* out, void* stream);

/* ---- in-place checksum fix-up (mutable views) -------------
 * Rewrites checksum fields inside the frames, with the raw-buffer semantics
 * of the reference's mutable views, composed the way
 * examples/mutable_chaining.rs:19-63 chains them (payload_mut of each layer
 * is the buffer of the next):
 *   MutableEthernetPacket (>= 14 B; payload = bytes after 14)
 *   EtherType 0x0800 -> MutableIpv4Packet::new (ipv4.rs:540-566: >= 20 B,
 *     IHL >= 5, IHL*4 <= len, total 0 or >= IHL*4); recompute_checksum
 *     (ipv4.rs:669-679: util::checksum(raw[..header_len], 5) into bytes
 *     10..11); payload_mut = [hl, hl + total_len - hl) with total_len = 0 ->
 *     len, else min(total, len) (ipv4.rs:591-596, 697-704)
 *   EtherType 0x86DD -> MutableIpv6Packet::new (>= 40 B); payload_mut =
 *     every byte after 40 (ipv6.rs:423-426; extension headers not walked)
 *   protocol / next header (raw byte) 17 -> MutableUdpPacket::new (udp.rs:
 *     101-121) + recompute_checksum with the enclosing IP addresses as
 *     context (udp.rs:338-369: pseudo-header sum over the WHOLE payload_mut
 *     slice, skipword 3, into bytes 6..7); 6 -> MutableTcpPacket (tcp.rs:
 *     857-876, 1009-1040, skipword 8, bytes 16..17); 1 (IPv4 only) ->
 *     MutableIcmpPacket (icmp.rs:267-273 via IcmpPacket::from_buf, >= 8 B;
 *     icmp.rs:372-377 util::checksum(raw, 1), bytes 2..3); 58 (IPv6 only) ->
 *     MutableIcmpv6Packet (icmpv6.rs:316-322, 450-470).
 * A view whose constructor returns None is skipped. `which` selects
 * NEXG_FIX_IP and/or NEXG_FIX_L4. With parse flag NEXG_PARSE_FROM_IP the IP
 * header starts at ip_offset and the version nibble picks the family.
 * The bytes of frames->data are rewritten in place (the batch's data must be
 * writable device memory; frames must not overlap). out (optional, may be
 * NULL): nexg_fixup[count]. */
#define NEXG_FIX_IP 0x1u
#define NEXG_FIX_L4 0x2u
typedef struct nexg_fixup {
    uint8_t done;   /* NEXG_FIX_* bits of the fields written                 */
    uint8_t proto;  /* L4 protocol number whose view was built (0 if none)  */
    uint16_t ip_csum; /* value written at IPv4 bytes 10..11 (if NEXG_FIX_IP) */
    uint16_t l4_csum; /* value written into the L4 header (if NEXG_FIX_L4)   */
    uint16_t l4_off;  /* frame offset of the L4 header                       */
} nexg_fixup;
int nexg_recompute_checksums_batch(nexg_ctx* ctx, const nexg_frames* frames,
                                   const nexg_parse_option* option, uint32_t which,
                                   nexg_fixup* out, void* stream);

/* ---- option lists ---------------------------------------
 * The Vec fields of Frame's headers, decoded on the device into fixed-capacity
 * arrays: Ipv4Header.options (ipv4.rs:442-508: EOL is kept and ends the list,
 * NOP is kept, an option without room for its length / with length < 2 / past
 * the header ends the walk) and TcpHeader.options (tcp.rs:767-818). Option k
 * starts at frame byte ip_opt_off + ip_pos[k] (tcp_opt_off + tcp_pos[k]); its
 * type/kind is that byte; EOL and NOP (IPv4: number = byte & 0x1f in {0, 1};
 * TCP: kind in {0, 1}) are one byte long, every other option's length is the
 * next byte and its data the length - 2 bytes after that. Counts are 0 for an
 * absent header (nexg_record flags); they equal the record's ip_nopt /
 * l4_nopt. An options area is at most 40 bytes, so 40 entries always suffice. */
typedef struct nexg_options {
    uint8_t n_ip;          /* Ipv4Header.options.len()                       */
    uint8_t n_tcp;         /* TcpHeader.options.len()                        */
    uint16_t ip_opt_off;   /* frame offset of the IPv4 options (l3_off + 20) */
    uint16_t tcp_opt_off;  /* frame offset of the TCP options (l4_off + 20)  */
    uint16_t reserved;
    uint8_t ip_pos[40];
    uint8_t tcp_pos[40];
    uint8_t pad[8];
} nexg_options;

/* Option lists for a batch already parsed with NEXG_OUT_RECORD (any parse
 * mode): records[i] must be frame i's record. Device pointers, stream-ordered. */
int nexg_decode_options(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records,
                        nexg_options* out, void* stream);

/* ---- tunnel decapsulation (VXLAN, GRE) --------------------------------------
 * Frame::try_from_buf stops at the outer UDP / IP header; the reference's
 * tunnel parsers VxlanPacket::try_from_buf (vxlan.rs:28-65) and
 * GrePacket::try_from_buf (gre.rs:32-107) read Frame.payload. Here a second
 * pass over a batch already parsed with NEXG_OUT_RECORD (any parse option)
 * locates each tunnel's inner frame inside the outer batch, with no copy of
 * frame bytes: {frames->data, frames->data_bytes, inner_off, inner_len, count}
 * is itself a valid nexg_frames table (offsets + lengths; monotone whenever
 * the outer batch's offsets are nondecreasing), and nexg_decap_select compacts
 * it by inner class into the tables nexg_parse_batch takes: inner Ethernet
 * with the default option, inner IP with NEXG_PARSE_FROM_IP, ip_offset 0.
 *
 * Candidates (only the record's own fields decide):
 *   VXLAN  NEXG_DECAP_VXLAN set; status 0, NEXG_L_UDP, dst_port == the VXLAN
 *          port. Fewer than 8 payload bytes: kind VXLAN, status MALFORMED (the
 *          reference returns None). The I flag is not looked at (nor does the
 *          reference); flags reports the byte.
 *   GRE    NEXG_DECAP_GRE set; status 0, NEXG_L_IPV4 or NEXG_L_IPV6, no
 *          transport / ICMP / ICMPv6 layer, ip_proto == 47: Frame.payload is
 *          the IP payload (frame.rs:466-468, 511-513). Fewer than 4 bytes, or
 *          an optional 4-B field (checksum + offset when C or R, key when K,
 *          sequence when S, in that order) cut short: MALFORMED; the routing
 *          bit: MALFORMED once the other optional fields were consumed.
 *          Version and zero flags are not checked (flags reports them). The
 *          checksum and offset words stay readable at outer frame bytes
 *          [payload_off + 4, payload_off + 8).
 * An accepted tunnel (kind != 0, status 0) gets inner_off = off(i) +
 * payload_off + hdr_len (absolute in frames->data) and inner_len =
 * payload_len - hdr_len (may be 0). Every other frame (not a candidate,
 * malformed tunnel, error status, bad extent) gets inner_off = off(i) (0 where
 * off(i) is undefined), inner_len = 0, and every nexg_tunnel field not named
 * above 0. Records are caller memory: one whose payload_off + payload_len
 * exceeds len(i) makes its frame a non-candidate, and nothing outside the
 * frame's own extent is read (the 16-B block rule of the frame batch layout
 * applies). */
#define NEXG_TUN_NONE 0
#define NEXG_TUN_VXLAN 1
#define NEXG_TUN_GRE 2
#define NEXG_INNER_OTHER 0     /* not a frame this library parses */
#define NEXG_INNER_ETHERNET 1  /* VXLAN; GRE protocol_type 0x6558 */
#define NEXG_INNER_IPV4 2      /* GRE protocol_type 0x0800 */
#define NEXG_INNER_IPV6 3      /* GRE protocol_type 0x86DD */
#define NEXG_DECAP_VXLAN 0x1u
#define NEXG_DECAP_GRE 0x2u
typedef struct nexg_decap_option {
    uint32_t which;       /* NEXG_DECAP_* */
    uint16_t vxlan_port;  /* UDP destination port; 0 means 4789 */
    uint16_t reserved;    /* must be 0 */
} nexg_decap_option;
typedef struct nexg_tunnel {  /* 16 bytes */
    uint8_t kind;     /* NEXG_TUN_* */
    uint8_t status;   /* NEXG_FRAME_OK, or NEXG_ERR_MALFORMED where the reference's try_from_buf returns None */
    uint8_t inner;    /* NEXG_INNER_* */
    uint8_t hdr_len;  /* VXLAN 8; GRE 4 + 4*(C|R) + 4*K + 4*S */
    uint16_t flags;   /* VXLAN: the flags byte; GRE: the first 16 bits as read */
    uint16_t proto;   /* GRE protocol_type; VXLAN 0 */
    uint32_t id;      /* VXLAN vni (24 bits); GRE key, 0 if absent */
    uint32_t aux;     /* VXLAN reserved1 << 8 | reserved2; GRE sequence, 0 if absent */
} nexg_tunnel;

/* records[i] = frame i's record from a NEXG_OUT_RECORD parse of the same
 * batch (16-B aligned). option NULL = both tunnel kinds, port 4789. Outputs
 * hold `count` entries: tunnels 16-B, inner_off 8-B, inner_len 4-B aligned.
 * NEXG_EINVAL: a NULL pointer with count > 0, reserved != 0, unknown `which`
 * bits, a misaligned output. count == 0 launches nothing. Device pointers,
 * stream-ordered. */
int nexg_decap_batch(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records,
                     const nexg_decap_option* option, nexg_tunnel* tunnels,
                     uint64_t* inner_off, uint32_t* inner_len, void* stream);

/* Order-preserving compaction of a decap result by inner class: frame i is
 * selected when tunnels[i].status == 0, tunnels[i].kind != 0 and
 * inner_mask & (1u << tunnels[i].inner) is nonzero. For the k-th selected
 * frame in index order out_index[k] = i, out_off[k] = inner_off[i],
 * out_len[k] = inner_len[i]; *out_count (device memory, 8-B aligned) = the
 * number selected. The output arrays have capacity `count`; count must not
 * exceed 2^32 - 1 (NEXG_EINVAL). workspace: caller-owned device memory (4-B
 * aligned) of at least the bytes the helper below gives (NEXG_EINVAL when
 * smaller): one u32 counter per 256-frame tile, turned into the tiles'
 * exclusive scan in place. Deterministic: ballots and scans decide positions,
 * no atomics. Three kernels on `stream`. */
int nexg_decap_select(nexg_ctx* ctx, const nexg_tunnel* tunnels, const uint64_t* inner_off,
                      const uint32_t* inner_len, uint64_t count, uint32_t inner_mask,
                      uint32_t* out_index, uint64_t* out_off, uint32_t* out_len,
                      uint64_t* out_count, void* workspace, uint64_t workspace_bytes, void* stream);
/* one u32 per 256-frame tile, rounded up to whole 256-tile scan chunks, + 16 B */
static inline uint64_t nexg_decap_select_workspace(uint64_t count) {
    const uint64_t tiles = (count + 255u) / 256u;
    return 4u * ((tiles + 255u) / 256u * 256u) + 16u;
}

/* ---- tunnel encapsulation (VXLAN, GRE; extension) -----------------------------
 * The other direction of the section above: every frame of a table is copied
 * into a new buffer behind an outer Ethernet / IPv4 or IPv6 / UDP + VXLAN or GRE
 * header, the bytes the reference's builders give when composed as
 * examples/udp_ping.rs composes them: EthernetPacketBuilder(Ipv4PacketBuilder
 * or Ipv6PacketBuilder(UdpPacketBuilder(VxlanPacket::to_bytes))), vxlan.rs:73-84,
 * and for GRE the IP builder with protocol 47 around GrePacket::to_bytes,
 * gre.rs:115-160. Up to 16 tunnel specs per call; tunnel_index[i] (device
 * memory, one byte per frame, usually the out_rule of nexg_select_batch: rule j
 * gets tunnel j) picks frame i's, NULL means spec 0 for every frame. Two calls,
 * as the gather: nexg_encap_plan lays the outputs out, the host reads the
 * total and allocates, nexg_encap_frames fills.
 *
 * Per frame i, in this order:
 *  1 spec     t = tunnel_index ? tunnel_index[i] : 0. An extent that leaves
 *             [0, data_bytes) or a length above 65535 (the gather's rule):
 *             output length 0, status NEXG_ERR_BAD_EXTENT, row.tunnel = t.
 *             t >= n_tunnels: a pass-through, the frame copied unchanged, row
 *             {0, NEXG_TUNNEL_NONE, 0, 0, 0, 0}; the index never reaches past
 *             the set.
 *  2 payload  VXLAN, and GRE without NEXG_ENCAP_GRE_L3: the whole frame,
 *             protocol_type 0x6558. GRE_L3 with len < 14: status
 *             NEXG_ERR_BUFFER_TOO_SHORT, output length 0; otherwise
 *             protocol_type = the big-endian u16 at bytes 12..13, whatever its
 *             value, and the payload is bytes [14, len). m = the payload's
 *             length.
 *  3 length   H = 14 + (20 | 40) + (VXLAN: 8 + 8 | GRE: 4 + 4 K + 4 S).
 *             H + m > 65535: status NEXG_ERR_INVALID_LENGTH, output length 0
 *             (an outer frame is itself a valid nexg_frames entry). Otherwise
 *             the output length is H + m.
 *  4 header   Ethernet: eth_dst, eth_src, 0x0800 / 0x86DD. IPv4: IHL 5, byte 1
 *             = tos, total length H - 14 + m, identification ip_id, ip_flags in
 *             the top 3 bits of word 3, fragment offset 0, ttl, protocol 17 /
 *             47, the header checksum of ipv4::checksum. IPv6: traffic class
 *             tos, flow_label, payload_length H - 54 + m, next header 17 / 47,
 *             hop limit ttl. UDP: src_port (+ flows[i].hash % port_span under
 *             NEXG_ENCAP_FLOW_PORT, RFC 7348's entropy), dst_port (0: 4789),
 *             length 16 + m, checksum 0, or under NEXG_ENCAP_UDP_CSUM
 *             udp::checksum over the pseudo-header, the UDP header, the VXLAN
 *             header and the payload; a computed 0 stays 0.
 *             VXLAN: 08 00 00 00 vni[3] 00. GRE: K << 13 | S << 12 (version 0,
 *             no C / R bit), protocol_type, the key (K), seq_base + i mod 2^32
 *             (S; i is the frame's index in the table).
 *  5 pads     the bytes from the frame's end up to out_offsets[i + 1] are
 *             zero (fewer than 16 with the plan's offsets; at most 15 are
 *             written).
 * Out of scope: Geneve, NVGRE, the GRE checksum and routing, outer VLAN tags,
 * an incrementing IPv4 id, fixing inner checksums; nested encapsulation is the
 * pass run twice, and fragmentation to an MTU the section below. */
#define NEXG_ENCAP_VXLAN 1
#define NEXG_ENCAP_GRE 2
#define NEXG_ENCAP_UDP_CSUM  0x01u /* VXLAN: compute the outer UDP checksum (default: field 0) */
#define NEXG_ENCAP_FLOW_PORT 0x02u /* VXLAN: src port = src_port + flows[i].hash % port_span */
#define NEXG_ENCAP_GRE_KEY   0x04u /* GRE: K bit, key = id */
#define NEXG_ENCAP_GRE_SEQ   0x08u /* GRE: S bit, sequence = seq_base + i (mod 2^32), i the frame's index in the table */
#define NEXG_ENCAP_GRE_L3    0x10u /* GRE: drop the inner Ethernet header; protocol_type = its EtherType */
#define NEXG_ENCAP_MAX_TUNNELS 16
#define NEXG_TUNNEL_NONE 0xFFu
typedef struct nexg_tunnel_spec {   /* 96 bytes */
    uint8_t kind;                   /* NEXG_ENCAP_VXLAN / _GRE */
    uint8_t family;                 /* outer IP: 4 or 6 */
    uint8_t ttl;                    /* IPv4 ttl / IPv6 hop limit */
    uint8_t tos;                    /* IPv4 byte 1 / IPv6 traffic class */
    uint32_t flags;                 /* NEXG_ENCAP_* */
    uint8_t eth_dst[6], eth_src[6];
    uint8_t src[16], dst[16];       /* network order; family 4 uses the first 4 bytes */
    uint16_t src_port, dst_port;    /* VXLAN; dst_port 0 means 4789 */
    uint16_t port_span;             /* FLOW_PORT: 1..65536-src_port; else 0 */
    uint16_t ip_id;                 /* IPv4 identification */
    uint32_t id;                    /* VXLAN vni (24 bits) / GRE key */
    uint32_t seq_base;
    uint32_t flow_label;            /* IPv6, 20 bits */
    uint8_t ip_flags;               /* IPv4, 3 bits (DF = 2) */
    uint8_t reserved[23];           /* must be 0 */
} nexg_tunnel_spec;
typedef struct nexg_tunnels {       /* host memory, read during the call only */
    uint32_t n_tunnels, reserved;
    nexg_tunnel_spec tunnels[NEXG_ENCAP_MAX_TUNNELS];
} nexg_tunnels;
typedef struct nexg_encapped {      /* 8 bytes */
    uint8_t status;                 /* NEXG_FRAME_OK / NEXG_ERR_* */
    uint8_t tunnel;                 /* the spec used, NEXG_TUNNEL_NONE for a pass-through */
    uint8_t hdr_len;                /* bytes put before the payload (0 for pass-through / error) */
    uint8_t reserved;
    uint16_t src_port, l4_csum;     /* VXLAN: the values written; else 0 */
} nexg_encapped;
struct nexg_flow; /* the rows of nexg_flow_batch, declared with the flow section below */

/* Host only. NEXG_EINVAL: n_tunnels 0 or above 16; an unknown kind or family;
 * unknown flag bits; a VXLAN flag (UDP_CSUM, FLOW_PORT) on a GRE spec or a GRE
 * flag on a VXLAN spec; a VXLAN id above 24 bits; flow_label above 20 bits;
 * ip_flags above 7; FLOW_PORT with port_span 0 or src_port + port_span >
 * 65536; port_span != 0 without FLOW_PORT; a nonzero reserved field. */
int nexg_tunnels_check(const nexg_tunnels* set);

/* out_offsets[i] (count + 1 entries, 8-B aligned) = the sum over j < i of
 * frame j's output length rounded up to `align` (1, 4, 8 or 16);
 * out_offsets[count] = the total; out_len[i] (optional) = the output length.
 * workspace: as the gather plan's (8-B aligned). count <= 2^32 - 1; count == 0
 * writes out_offsets[0] = 0 and launches nothing else. Scans only, no atomics.
 * Three kernels on `stream`. */
int nexg_encap_plan(nexg_ctx* ctx, const nexg_frames* frames, const nexg_tunnels* set, const uint8_t* tunnel_index,
                    uint32_t align, uint64_t* out_offsets, uint32_t* out_len, void* workspace, uint64_t workspace_bytes,
                    void* stream);
static inline uint64_t nexg_encap_plan_workspace(uint64_t count) {
    const uint64_t tiles = (count + 255u) / 256u;
    return 8u * ((tiles + 255u) / 256u * 256u) + 16u;
}

/* Frame i's outer frame at out_data (16-B aligned) + out_offsets[i], the pads
 * zero; rows[i] (optional, 8-B aligned) says what was written. flows: the rows
 * of nexg_flow_batch over the same table (8-B aligned), needed when a spec has
 * NEXG_ENCAP_FLOW_PORT (NEXG_EINVAL when NULL then and count > 0), else ignored. No store
 * lands at or past out_cap or outside [out_offsets[i], out_offsets[i + 1]),
 * whatever out_offsets holds (it is caller memory), and the output is never
 * read. Source reads follow the 16-B block rule and never leave a frame's
 * blocks; the inner bytes are read once, the UDP checksum summed from the
 * loads that feed the copy. A frame cut short by out_cap or by an
 * out_offsets[i + 1] below its end has its bytes below the cut, but its UDP
 * checksum field and rows[i].l4_csum are undefined under NEXG_ENCAP_UDP_CSUM
 * (the sum covers what was copied). Deterministic, no atomics, no workspace.
 * NEXG_EINVAL also for a NULL out_offsets with count > 0, a NULL out_data with
 * out_cap > 0, a misaligned pointer, count > 2^32 - 1. count == 0 launches
 * nothing. With align 1, {out_data, total, out_offsets} is a packed batch;
 * with a larger align, {out_data, total, out_offsets, out_len} an offsets +
 * lengths batch (monotone). One kernel on `stream`. */
int nexg_encap_frames(nexg_ctx* ctx, const nexg_frames* frames, const nexg_tunnels* set, const uint8_t* tunnel_index,
                      const struct nexg_flow* flows, const uint64_t* out_offsets, uint8_t* out_data, uint64_t out_cap,
                      nexg_encapped* rows, void* stream);

/* ---- IPv4 fragmentation to an MTU (RFC 791 section 3.2; extension) --------------
 * What makes the output of the passes above fit a link: every IPv4 frame of a
 * table whose total length exceeds `mtu` is cut into pieces that each carry the
 * frame's Ethernet and IPv4 header, the bytes the reference's Ipv4PacketBuilder
 * gives for each piece's fields (Ipv4Flags::{DontFragment, MoreFragments},
 * fragment_offset, ipv4::checksum). The first one-to-many pass: a frame becomes
 * 0..8183 output frames, so the plan scans twice (output frames, output bytes)
 * and the fill writes a frame table with the input frame of each piece, the
 * index nexg_gather_rows takes to carry per-frame rows (rule, tunnel, flow) to
 * the pieces.
 *
 * Per frame i, in this order:
 *  1 extent   An extent that leaves [0, data_bytes) or a length above 65535
 *             (the gather's rule): 0 pieces, status NEXG_ERR_BAD_EXTENT, kind
 *             NEXG_FRAG_NONE.
 *  2 IPv6     bytes 12..13 are 0x86DD, len >= 54, version 6 and 40 +
 *             payload_length <= len - 14: 0 pieces and kind NEXG_FRAG_TOO_BIG
 *             when 40 + payload_length > mtu (routers never fragment IPv6),
 *             else a pass-through.
 *  3 not IPv4 bytes 12..13 are not 0x0800, len < 34, version != 4, IHL < 5,
 *             14 + hl > len (hl = 4 IHL), total length TL < hl, or 14 + TL > len:
 *             a pass-through, one output frame, the whole input frame copied
 *             unchanged, kind NEXG_FRAG_PASS. VLAN-tagged frames fall here.
 *  4 fits     TL <= mtu: a pass-through (the bytes past 14 + TL are copied too).
 *  5 DF       the DF bit set and NEXG_FRAG_IGNORE_DF absent: 0 pieces, kind
 *             NEXG_FRAG_TOO_BIG, status NEXG_FRAME_OK (the host builds the ICMP
 *             "fragmentation required" message from the row).
 *  6 split    D = TL - hl, p = (mtu - hl) & ~7, n = ceil(D / p); fo0 and MF0 are
 *             the input's own fragment offset and MF bit (an input that is
 *             already a fragment is split further). fo0 + (n - 1) p / 8 > 8191:
 *             0 pieces, status NEXG_ERR_INVALID_LENGTH, kind NEXG_FRAG_NONE.
 *             Otherwise kind NEXG_FRAG_SPLIT and piece k (0 <= k < n) is the 14
 *             Ethernet bytes, the hl header bytes and data bytes [k p, k p + d_k)
 *             of the input's IP payload, d_k = min(p, D - k p); its length is
 *             14 + hl + d_k (input bytes past 14 + TL are dropped; no padding to
 *             60 bytes). In the header: total length hl + d_k; identification,
 *             TOS, TTL, protocol, addresses and the reserved flag bit unchanged;
 *             DF unchanged, or cleared in every piece under IGNORE_DF; MF 1 for
 *             k < n - 1 and MF0 for the last piece; fragment offset fo0 + k p / 8;
 *             the checksum recomputed as ipv4::checksum over the piece's header.
 *             Piece 0 keeps its options. In pieces k >= 1 the options are walked
 *             from byte 20 to hl: type 0 stops the walk (the rest stays as it
 *             is), type 1 advances one byte, otherwise L is the next byte, L < 2
 *             or L above the bytes left stops the walk, a type with bit 7 (copied)
 *             clear has all its L bytes set to 0x01, and the walk advances by L.
 *             The header keeps its length, as Linux's forward path does.
 *  7 pads     each output frame's start is rounded up to `align`; the pads are
 *             zero.
 * Out of scope: IPv6 fragment headers, reassembly, VLAN-tagged or tunnelled
 * inner headers, padding to the Ethernet minimum, building the ICMP / ICMPv6
 * error, a per-frame MTU, fixing L4 checksums (they do not change). */
#define NEXG_FRAG_NONE 0     /* no output frame: an error status */
#define NEXG_FRAG_PASS 1     /* one output frame, the input copied unchanged */
#define NEXG_FRAG_SPLIT 2    /* `pieces` output frames */
#define NEXG_FRAG_TOO_BIG 3  /* no output frame: over the MTU and not to be fragmented (DF, IPv6) */
#define NEXG_FRAG_IGNORE_DF 0x1u
typedef struct nexg_frag_option {  /* host memory, read during the call only */
    uint32_t mtu;                  /* the largest IP total length, 68..65535 */
    uint32_t flags;                /* NEXG_FRAG_* */
    uint32_t align;                /* 1, 4, 8 or 16 */
    uint32_t reserved;             /* must be 0 */
} nexg_frag_option;
typedef struct nexg_fragged {      /* 16 bytes, one per input frame */
    uint8_t status;                /* NEXG_FRAME_OK / NEXG_ERR_* */
    uint8_t kind;                  /* NEXG_FRAG_* */
    uint8_t hdr_len;               /* hl of a split frame, else 0 */
    uint8_t reserved;
    uint16_t pieces;               /* output frames: 0, 1 or n */
    uint16_t piece_data;           /* p of a split frame, else 0 */
    uint32_t first;                /* index of its first output frame */
    uint32_t reserved2;
} nexg_fragged;

/* Host only. NEXG_EINVAL: NULL, mtu outside 68..65535, unknown flag bits, an
 * align other than 1, 4, 8 or 16, a nonzero reserved. */
int nexg_frag_option_check(const nexg_frag_option* option);

/* out_first[i] (count + 1 entries, 4-B aligned) = the number of output frames
 * of the frames before i, out_bytes[i] (count + 1 entries, 8-B aligned) = the
 * sum of their output frames' lengths, each rounded up to option->align; the
 * totals are in the last entries. rows[i] (optional, 16-B aligned) reports
 * frame i. workspace: caller-owned device memory (8-B aligned) of at least the
 * bytes the helper below gives (NEXG_EINVAL when smaller): two u64 per 256-frame
 * tile, turned into the tiles' exclusive scans in place. Scans only, no atomics.
 * count == 0 writes the two zeros and launches nothing else. NEXG_EINVAL also
 * for count > 2^32 - 1. The output frames are numbered with 32 bits; the call
 * does not wait for the device, so it cannot return an error for a total that
 * only the device knows: the total is summed in 64 bits, and out_first[count]
 * == 2^32 - 1 says that it is 2^32 - 1 or more (a 65535-byte frame gives up to
 * 8183 pieces, at mtu 68 and hl 60). The other prefixes then wrapped and are
 * of no use: fragment a part of the table. (nexg_fragment_frames keeps its
 * bounds whatever it is given.) Four kernels on `stream`. */
int nexg_fragment_plan(nexg_ctx* ctx, const nexg_frames* frames, const nexg_frag_option* option, uint32_t* out_first,
                       uint64_t* out_bytes, nexg_fragged* rows, void* workspace, uint64_t workspace_bytes, void* stream);
static inline uint64_t nexg_fragment_plan_workspace(uint64_t count) {
    const uint64_t tiles = (count + 255u) / 256u;
    return 16u * ((tiles + 255u) / 256u * 256u) + 16u;
}

/* The output frames of frame i at out_data (16-B aligned) + out_bytes[i] on,
 * each start rounded up to option->align and the pads zero, and for its k-th
 * piece, f = out_first[i] + k: out_offsets[f] (out_count + 1 entries, 8-B
 * aligned) = where it starts, out_len[f] its length, out_src[f] = i (4-B
 * aligned, out_count entries each); out_offsets[out_count] = out_bytes[count].
 * out_first and out_bytes are caller memory: whatever they hold, no byte store
 * lands at or past out_cap or outside frame i's [out_bytes[i], out_bytes[i + 1]),
 * no table store lands at an index at or above min(out_first[i + 1], out_count),
 * and every loop is bounded by the shape recomputed from the frame's own bytes.
 * Source reads follow the 16-B block rule and never leave a frame's blocks; the
 * payload is read once. The output is never read. Deterministic, no atomics,
 * no workspace. NEXG_EINVAL: an invalid option, a NULL out_first, out_bytes or
 * out_offsets, a NULL out_len or out_src with out_count > 0, a NULL out_data
 * with out_cap > 0, a misaligned pointer, count or out_count > 2^32 - 1.
 * count == 0 launches nothing but the copy of the total. With align 1,
 * {out_data, total, out_offsets} is a packed batch that nexg_parse_batch,
 * nexg_encap_plan, nexg_rewrite_batch and nexg_tx_send_batch take as it
 * stands; with a larger align, {out_data, total, out_offsets, out_len} an
 * offsets + lengths batch (monotone). One kernel on `stream`. */
int nexg_fragment_frames(nexg_ctx* ctx, const nexg_frames* frames, const nexg_frag_option* option,
                         const uint32_t* out_first, const uint64_t* out_bytes, uint64_t out_count, uint64_t* out_offsets,
                         uint32_t* out_len, uint32_t* out_src, uint8_t* out_data, uint64_t out_cap, void* stream);

/* ---- DNS messages ------------------------------------------------------------
 * Frame::try_from_buf stops at the UDP header; the reference's DNS parser
 * DnsPacket::try_from_buf (dns.rs:1166-1259) reads Frame.payload, as its
 * example caller does (dns_dump.rs:97-101). Here a second pass over a batch
 * already parsed with NEXG_OUT_RECORD (any parse option) walks each DNS
 * message in place: nexg_dns_batch writes one nexg_dns summary per frame and
 * the prefix sums that place a variable number of entries per frame;
 * nexg_dns_entries walks again and writes one nexg_dns_entry per query and
 * resource record. Names are not decoded on the device: an entry gives the
 * offsets at which a host decoder (decode_dns_name, dns.rs:1303-1390) starts.
 *
 * Candidates (only the record's own fields decide): status 0, NEXG_L_UDP,
 * payload_len > 0, payload_off + payload_len <= len(i), and src_port == port
 * or dst_port == port, or NEXG_DNS_ANY_UDP (dns_dump.rs:98-100 tries every
 * UDP payload that is not empty). A non-candidate (bad extent included) gets
 * an all-zero nexg_dns but for `first`.
 *
 * A candidate's message M of n = payload_len bytes, as dns.rs:1166-1259 with
 * DnsQueryPacket::from_buf_mut (dns.rs:752-790) and
 * DnsResponsePacket::from_buf_mut (dns.rs:904-945):
 *   n < 12: status NEXG_ERR_BUFFER_TOO_SHORT (dns.rs:1167-1173), every other
 *     field 0 (flags8 too), no entries.
 *   Header bytes 0..11 give id, flags, qd, an, ns, ar; pos = 12.
 *   Each of qd queries: labels until a zero length byte; a length byte L is a
 *     plain length whatever its top bits (0xC0..0xFF are NOT compression
 *     pointers here, dns.rs:759-769); pos >= n before a length byte, n - pos < L
 *     after one, or n - pos < 4 after the zero byte fail the whole message
 *     (dns.rs:1228-1231, "DNS query section"): status NEXG_ERR_MALFORMED;
 *     flags8 bit 0, msg_off, msg_len, id, flags, qd, an, ns, ar are kept,
 *     n_*, rest_off are 0 and there are no entries.
 *   Then an, ns, ar records: a section stops silently when n - pos < 12
 *     (dns.rs:905-907, 1213-1221), and since the cursor does not move every
 *     later section then parses 0 records too; flags8 bit 1 is set when fewer
 *     records were parsed than declared. A record is always name_tag u16,
 *     type, class, ttl u32, data_len (an uncompressed owner name is read as
 *     these 12 bytes all the same) and pos advances by
 *     12 + min(n - pos - 12, data_len) (dns.rs:929-931).
 *   rest_off = pos at the end: DnsPacket.payload is M[rest_off, n).
 *
 * Entries follow message order (queries, answers, authorities, additionals).
 * With T = ceil(count / 256) tiles, tile_first has T + 1 elements (device
 * memory, 8-B aligned): tile_first[t] = the number of entries of frames
 * [0, 256 t), tile_first[T] = the batch total. The k-th entry of frame i has
 * index tile_first[i >> 8] + dns[i].first + k. Positions come from scans
 * alone (no atomics): the output is the same on every run.
 *
 * Query fields: type and class at M[off + name .. + 4), the qname bytes are
 * M[off, off + name). Record data: M[off + 12, off + 12 + min(data_len,
 * msg_len - off - 12)).
 *
 * Records, summaries and tile_first are caller memory: nothing outside a
 * frame's own extent is read (msg_off + msg_len is clamped to it and every
 * bound is re-checked from the bytes), and nexg_dns_entries stores nothing at
 * or past entries_cap, whatever the summaries hold. */
#define NEXG_DNS_ANY_UDP 0x1u /* dns_dump.rs:98-100: try every UDP frame with a non-empty payload */
typedef struct nexg_dns_option {
    uint32_t flags;    /* NEXG_DNS_*; unknown bits -> NEXG_EINVAL */
    uint16_t port;     /* UDP source OR destination port; 0 means 53 */
    uint16_t reserved; /* must be 0 */
} nexg_dns_option;
typedef struct nexg_dns { /* 32 bytes per frame */
    uint8_t status;    /* NEXG_FRAME_OK | NEXG_ERR_BUFFER_TOO_SHORT (< 12 B, dns.rs:1167-1173)
                          | NEXG_ERR_MALFORMED ("DNS query section", dns.rs:1228-1231) */
    uint8_t flags8;    /* bit 0 candidate (with at least 12 bytes); bit 1 a record section ended early */
    uint16_t msg_off;  /* frame-relative offset of the DNS message (= record payload_off) */
    uint16_t msg_len;  /* = record payload_len */
    uint16_t id;
    uint16_t flags;    /* header bytes 2..3 as a BE value (QR, opcode, AA, TC, RD, RA, Z, AD, CD, rcode) */
    uint16_t qd, an, ns, ar;        /* declared counts, header bytes 4..11 */
    uint16_t n_q, n_an, n_ns, n_ar; /* queries.len(), responses.len(), authorities.len(), additionals.len() */
    uint16_t rest_off; /* message-relative offset of DnsPacket.payload; its length = msg_len - rest_off */
    uint32_t first;    /* entries of this frame's tile before this frame (see tile_first) */
} nexg_dns;
typedef struct nexg_dns_entry { /* 16 bytes per query / resource record */
    uint8_t section;    /* 0 query, 1 answer, 2 authority, 3 additional */
    uint8_t flags8;     /* bit 0: record data cut short (safe_data_len < data_len, dns.rs:929) */
    uint16_t off;       /* message-relative offset of the entry's first byte */
    uint16_t type;      /* qtype / rtype value */
    uint16_t dns_class; /* qclass / rclass value */
    uint32_t ttl;       /* record ttl; query 0 */
    uint16_t name;      /* query: qname.len() including the zero byte; record: name_tag */
    uint16_t data_len;  /* record: declared data_len; query 0 */
} nexg_dns_entry;

/* ceil(count / 256) + 1 u64 elements */
static inline uint64_t nexg_dns_tile_first_bytes(uint64_t count) { return 8u * ((count + 255u) / 256u + 1u); }

/* records[i] = frame i's record from a NEXG_OUT_RECORD parse of the same
 * batch (16-B aligned). option NULL = port 53, no flags. `out` holds `count`
 * summaries (16-B aligned), tile_first the bytes the helper above gives (8-B
 * aligned). NEXG_EINVAL: a NULL pointer with count > 0, reserved != 0, unknown
 * flag bits, a misaligned output, count > 2^32 - 1. count == 0 writes
 * tile_first[0] = 0 and nothing else. Two kernels on `stream`. Device
 * pointers, stream-ordered. */
int nexg_dns_batch(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records,
                   const nexg_dns_option* option, nexg_dns* out, uint64_t* tile_first, void* stream);

/* One entry per query / resource record of every frame whose summary is a
 * candidate with status 0, at tile_first[i >> 8] + dns[i].first + k; entry
 * indices at or past entries_cap are not written (the batch total is
 * tile_first's last element). At most n_q + n_an + n_ns + n_ar entries per
 * frame. entries: 16-B aligned; NULL with entries_cap 0 is valid and launches
 * nothing. NEXG_EINVAL: a NULL pointer with count > 0, NULL entries with a
 * nonzero capacity, a misaligned pointer, count > 2^32 - 1. */
int nexg_dns_entries(nexg_ctx* ctx, const nexg_frames* frames, const nexg_dns* dns,
                     const uint64_t* tile_first, nexg_dns_entry* entries, uint64_t entries_cap, void* stream);

/* ---- frame selection by rule, and gather (extension) --------------------------
 * The reference has no filter (examples/dump.rs prints every frame); like
 * NEXG_PARSE_VLAN this is an extension, and the text below is its whole
 * specification (nex_amd/select.py match_host / gather_host restate it on the
 * host). nexg_select_batch picks frames of a batch already parsed with
 * NEXG_OUT_RECORD by tests on the record's fields and writes a frame table
 * over the same bytes; nexg_gather_plan / nexg_gather_frames copy the selected
 * frames into one dense buffer, nexg_gather_rows compacts any per-frame rows.
 *
 * A filter is 1..16 rules. A rule is a conjunction of tests; a frame matches
 * the filter when some rule matches; NEXG_FILTER_INVERT flips the verdict.
 * The flags test ((record.flags & flags_mask) == flags_value; 0 / 0 is always
 * true; it covers the layer bits, the NEXG_C_* verdicts, NEXG_L_VLAN and the
 * status in bits 24..26) is always evaluated, the others when their bit is set
 * in `tests`:
 *   NEXG_RULE_PROTO      NEXG_L_IPV4 or NEXG_L_IPV6, and record.ip_proto == ip_proto
 *   NEXG_RULE_SRC_PORT   NEXG_L_TCP or NEXG_L_UDP, and src_port in [sport_lo, sport_hi]
 *   NEXG_RULE_DST_PORT   NEXG_L_TCP or NEXG_L_UDP, and dst_port in [dport_lo, dport_hi]
 *   NEXG_RULE_ANY_PORT   NEXG_L_TCP or NEXG_L_UDP, and either port in [sport_lo, sport_hi]
 *                        (dport_lo / dport_hi must be 0; not with SRC_PORT / DST_PORT)
 *   NEXG_RULE_SRC_ADDR   the source address matches the first src_bits bits of src
 *   NEXG_RULE_DST_ADDR   the destination address matches the first dst_bits bits of dst
 *   NEXG_RULE_ANY_ADDR   either address matches the first src_bits bits of src
 *                        (dst_bits must be 0; not with SRC_ADDR / DST_ADDR)
 *   NEXG_RULE_TCP_FLAGS  NEXG_L_TCP and (record.l4_type & tcp_mask) == tcp_value
 *   NEXG_RULE_LENGTH     len_lo <= len(i) <= len_hi, len(i) as the frame table gives it
 * Address tests, family 4: the frame must have NEXG_L_IPV4; the addresses are
 * record.ip_src / ip_dst (an ARP frame never matches: pick those with the flags
 * test). Family 6: the frame must have NEXG_L_IPV6, a valid extent and
 * l3_off + 40 <= len(i); the addresses are frame bytes [l3_off + 8, l3_off + 24)
 * and [l3_off + 24, l3_off + 40) (the record does not carry them). The port
 * tests need a TCP or UDP layer because the record reuses the port fields for
 * ARP. A record whose status is not 0 carries an error payload in its address,
 * port and type fields: for such a frame every test but the flags test and the
 * length test is false.
 *
 * Records are caller memory: nothing outside a frame's own extent is read (the
 * 16-B block rule of the frame batch layout applies), and a record whose l3_off
 * points past its frame simply fails the family-6 address tests. A filter
 * without a family-6 rule reads no frame byte.
 *
 * NEXG_EINVAL (nexg_filter_check says which): n_rules 0 or above 16, unknown
 * `tests` or `flags` bits, reserved != 0, an address test with a family other
 * than 4 or 6, prefix bits above the family's width, lo > hi in a range under
 * test, the exclusive combinations above. */
#define NEXG_RULE_PROTO 0x1u
#define NEXG_RULE_SRC_PORT 0x2u
#define NEXG_RULE_DST_PORT 0x4u
#define NEXG_RULE_ANY_PORT 0x8u
#define NEXG_RULE_SRC_ADDR 0x10u
#define NEXG_RULE_DST_ADDR 0x20u
#define NEXG_RULE_ANY_ADDR 0x40u
#define NEXG_RULE_TCP_FLAGS 0x80u
#define NEXG_RULE_LENGTH 0x100u
#define NEXG_RULE_ALL 0x1FFu
#define NEXG_FILTER_INVERT 0x1u
#define NEXG_FILTER_MAX_RULES 16
#define NEXG_RULE_NONE 0xFFu /* out_rule under NEXG_FILTER_INVERT */
typedef struct nexg_rule {      /* 64 bytes */
    uint32_t flags_mask;        /* (record.flags & flags_mask) == flags_value; 0/0 always true */
    uint32_t flags_value;
    uint32_t tests;             /* NEXG_RULE_*; unknown bits -> NEXG_EINVAL */
    uint8_t ip_proto;           /* NEXG_RULE_PROTO */
    uint8_t tcp_mask, tcp_value; /* NEXG_RULE_TCP_FLAGS */
    uint8_t family;             /* address tests: 4 or 6 */
    uint8_t src_bits, dst_bits; /* prefix lengths: 0..32 / 0..128 */
    uint16_t reserved;          /* must be 0 */
    uint16_t sport_lo, sport_hi, dport_lo, dport_hi; /* inclusive ranges */
    uint16_t len_lo, len_hi;    /* NEXG_RULE_LENGTH */
    uint8_t src[16], dst[16];   /* network order; family 4 uses the first 4 bytes */
} nexg_rule;
typedef struct nexg_filter { /* host memory; read during the call, not after it */
    uint32_t n_rules;
    uint32_t flags; /* NEXG_FILTER_* */
    nexg_rule rules[NEXG_FILTER_MAX_RULES];
} nexg_filter;

/* NEXG_OK when nexg_select_batch would accept the filter, else NEXG_EINVAL.
 * Host only: no context, no device. */
int nexg_filter_check(const nexg_filter* filter);

/* Order-preserving selection. records[i] = frame i's record (16-B aligned;
 * e.g. the inner records with an inner table from nexg_decap_batch). For the
 * k-th selected frame in index order out_index[k] = i, out_off[k] = off(i),
 * out_len[k] = len(i) exactly as the input table defines them for any layout
 * (a length above 2^32 - 1 is stored as 2^32 - 1), out_rule[k] (optional, may
 * be NULL) = the lowest matching rule index, NEXG_RULE_NONE under
 * NEXG_FILTER_INVERT; *out_count (device memory, 8-B aligned) = the number
 * selected. {frames->data, frames->data_bytes, out_off, out_len, *out_count}
 * is then a valid offsets + lengths table over the same bytes, monotone
 * whenever the input was packed, fixed-stride or monotone. The output arrays
 * have capacity `count` (out_off 8-B, out_index / out_len 4-B aligned); count
 * must not exceed 2^32 - 1. workspace: caller-owned device memory (4-B
 * aligned) of at least nexg_select_workspace(count) bytes, one u32 per
 * 256-frame tile. Positions come from ballots, ranks and scans only (no
 * atomics): a run repeats bit for bit. count == 0 writes *out_count = 0 and
 * launches nothing else. The scatter bounds every store by `count`, whatever
 * the workspace holds. NEXG_EINVAL: an invalid filter or frame table, a NULL
 * pointer, a misaligned pointer, a short workspace. Three kernels on `stream`. */
int nexg_select_batch(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records,
                      const nexg_filter* filter, uint32_t* out_index, uint64_t* out_off, uint32_t* out_len,
                      uint8_t* out_rule, uint64_t* out_count, void* workspace, uint64_t workspace_bytes,
                      void* stream);
static inline uint64_t nexg_select_workspace(uint64_t count) {
    const uint64_t tiles = (count + 255u) / 256u;
    return 4u * ((tiles + 255u) / 256u * 256u) + 16u;
}

/* Gather, in two calls (as nexg_dns_batch / nexg_dns_entries: the host reads
 * one total, allocates, then fills). `sel` is any frame table, usually the one
 * nexg_select_batch wrote. copied(k) = len(k), or 0 when the frame's extent
 * leaves [0, data_bytes) or its length exceeds 65535.
 *
 * nexg_gather_plan: out_offsets[k] (count + 1 entries, 8-B aligned) = the sum
 * over j < k of copied(j) rounded up to `align` (1, 4, 8 or 16);
 * out_offsets[count] = the total; out_len[k] (optional, may be NULL) =
 * copied(k). workspace: device memory (8-B aligned) of at least
 * nexg_gather_plan_workspace(count) bytes, one u64 per 256-frame tile. count
 * must not exceed 2^32 - 1. count == 0 writes out_offsets[0] = 0. Scans only,
 * no atomics. Three kernels on `stream`.
 *
 * nexg_gather_frames: bytes [out_offsets[k], out_offsets[k] + copied(k)) of
 * out_data (16-B aligned) become frame k's bytes, the pad bytes up to
 * out_offsets[k + 1] zero. No byte at or past out_cap is stored, whatever
 * out_offsets holds (it is caller memory), and bytes from the total up to
 * out_cap are left alone. Source reads follow the 16-B block rule and never
 * leave a frame's blocks. With align 1, {out_data, total, out_offsets} is a
 * packed batch; with a larger align, {out_data, total, out_offsets, out_len}
 * an offsets + lengths batch (monotone).
 *
 * nexg_gather_rows: out row k = rows[index[k]] when index[k] < rows_count,
 * zeros otherwise, for k < n (n <= 2^32 - 1). row_bytes is 4, 8, 16, 32 or
 * 64; rows and out are aligned to min(row_bytes, 16), index to 4. It compacts
 * records, nexg_tunnel, nexg_dns, descriptors and flags words by the index
 * nexg_select_batch returned. n == 0 launches nothing. */
int nexg_gather_plan(nexg_ctx* ctx, const nexg_frames* sel, uint32_t align, uint64_t* out_offsets,
                     uint32_t* out_len, void* workspace, uint64_t workspace_bytes, void* stream);
static inline uint64_t nexg_gather_plan_workspace(uint64_t count) {
    const uint64_t tiles = (count + 255u) / 256u;
    return 8u * ((tiles + 255u) / 256u * 256u) + 16u;
}
int nexg_gather_frames(nexg_ctx* ctx, const nexg_frames* sel, const uint64_t* out_offsets, uint8_t* out_data,
                       uint64_t out_cap, void* stream);
int nexg_gather_rows(nexg_ctx* ctx, const void* rows, uint32_t row_bytes, uint64_t rows_count,
                     const uint32_t* index, uint64_t n, void* out, void* stream);

/* ---- fixed-string match on frame bytes (extension) -----------------------------
 * The reference has no payload search; like the selection above this is an
 * extension, and the text below is its whole specification
 * (nex_amd/match.py match_host / match_rows_host / match_select_host restate
 * it on the host). nexg_match_batch looks for up to 32 byte strings of 1..16
 * bytes in every frame's payload (or in the whole frame) and gives a row per
 * frame; nexg_match_select compacts the frame table by the rows' masks into
 * the kind of table nexg_select_batch writes, which parse, decap, dns, flow,
 * the gather calls and nexg_match_batch itself take as it stands.
 *
 * The region of frame i. With NEXG_MATCH_FRAME it is [0, len(i)): `records`
 * may be NULL and is not read. Otherwise it is [payload_off, payload_off +
 * payload_len) of records[i], when the record's status is 0, payload_len > 0
 * and payload_off + payload_len <= len(i). Every other frame has an empty
 * region: an error status, a record that points past its frame, and under
 * either flag an extent that leaves [0, data_bytes) or a length above 65535.
 * A frame with an empty region gets the row {0, 0, NEXG_PAT_NONE, 0}.
 *
 * Pattern p occurs at region-relative position q, in a region of n bytes,
 * when q + len_p <= n, off_lo <= q <= off_hi, and region[q + k] == bytes[k]
 * for every k < len_p; under NEXG_PAT_NOCASE both sides first map the bytes
 * 0x41..0x5A to themselves | 0x20 and nothing else (0x40, 0x5B, 0x60, 0x7B
 * and bytes from 0x80 up stay as they are). Occurrences may overlap; the
 * position window bounds the start only: off_lo = off_hi = 0 is "starts
 * with", 0..65535 "anywhere".
 *
 * Records are caller memory: nothing outside a frame's own extent is read
 * (the 16-B block rule of the frame batch layout applies). In a packed batch
 * a pattern that only the next frame's first bytes would complete, or one
 * that begins in the header bytes before payload_off, does not occur.
 *
 * NEXG_EINVAL for a set (nexg_patterns_check tells): n_patterns 0 or above
 * 32, a len of 0 or above 16, nonzero bytes past len, unknown flag bits of a
 * pattern or of the set, nonzero reserved bytes, off_lo > off_hi. */
#define NEXG_MATCH_MAX_PATTERNS 32
#define NEXG_MATCH_MAX_LEN 16
#define NEXG_PAT_NOCASE 0x1u  /* per pattern: ASCII letters compare case-insensitively */
#define NEXG_MATCH_FRAME 0x1u /* per set: the region is the whole frame; default: Frame.payload */
#define NEXG_PAT_NONE 0xFFu   /* first_pat of a row whose mask is 0 */
typedef struct nexg_pattern { /* 32 bytes */
    uint8_t bytes[16];        /* the first `len` are compared; the rest must be 0 */
    uint8_t len;              /* 1..16 */
    uint8_t flags;            /* NEXG_PAT_*; unknown bits -> NEXG_EINVAL */
    uint16_t off_lo, off_hi;  /* the occurrence starts at a region-relative position in [off_lo, off_hi] */
    uint8_t reserved[10];     /* must be 0 */
} nexg_pattern;
typedef struct nexg_patterns { /* host memory; read during the call, not after it; 1032 bytes */
    uint32_t n_patterns;       /* 1..32 */
    uint32_t flags;            /* NEXG_MATCH_*; unknown bits -> NEXG_EINVAL */
    nexg_pattern pat[NEXG_MATCH_MAX_PATTERNS];
} nexg_patterns;
typedef struct nexg_match { /* 8 bytes per frame */
    uint32_t mask;          /* bit p: pattern p occurs in the region */
    uint16_t first_off;     /* FRAME-relative offset of the earliest occurrence of any pattern; 0 if mask == 0 */
    uint8_t first_pat;      /* the lowest pattern index among those occurring at first_off; NEXG_PAT_NONE if mask == 0 */
    uint8_t reserved;       /* 0 */
} nexg_match;

/* NEXG_OK when nexg_match_batch would accept the set, else NEXG_EINVAL.
 * Host only: no context, no device. */
int nexg_patterns_check(const nexg_patterns* set);

/* out[i] = frame i's row. records[i] = frame i's record (16-B aligned; under
 * NEXG_MATCH_FRAME any pointer, NULL too: it is not read); out: 8-B aligned,
 * `count` entries; count must not exceed 2^32 - 1. count == 0 launches
 * nothing. A row is the OR of its occurrences' bits and the minimum of their
 * (first_off << 8 | pattern) keys, gathered with workgroup-local (LDS) atomics
 * whose result does not depend on the order of arrival: a run repeats bit for
 * bit. NEXG_EINVAL: an invalid set or frame table, NULL or misaligned records
 * without NEXG_MATCH_FRAME, a NULL or misaligned out. One kernel on `stream`. */
int nexg_match_batch(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records,
                     const nexg_patterns* set, nexg_match* out, void* stream);

/* Order-preserving selection by the rows. matches[i] (8-B aligned) = frame
 * i's row; frame i is selected when
 *   (any_mask == 0 || (mask & any_mask) != 0) && (mask & all_mask) == all_mask
 *   && (mask & none_mask) == 0
 * so all-zero masks select every frame. For the k-th selected frame in index
 * order out_index[k] = i, out_off[k] = off(i), out_len[k] = len(i) exactly as
 * the input table defines them for any layout (a length above 2^32 - 1 is
 * stored as 2^32 - 1); *out_count (device memory, 8-B aligned) = the number
 * selected. {frames->data, frames->data_bytes, out_off, out_len, *out_count}
 * is then a valid offsets + lengths table over the same bytes, monotone
 * whenever the input was packed, fixed-stride or monotone. The output arrays
 * have capacity `count` (out_off 8-B, out_index / out_len 4-B aligned); count
 * must not exceed 2^32 - 1. workspace: caller-owned device memory (4-B
 * aligned) of at least nexg_match_select_workspace(count) bytes, one u32 per
 * 256-frame tile. Positions come from ballots, ranks and scans only (no
 * atomics): a run repeats bit for bit. count == 0 writes *out_count = 0 and
 * launches nothing else. The scatter bounds every store by `count`, whatever
 * the workspace holds. NEXG_EINVAL: an invalid frame table, a NULL pointer, a
 * misaligned pointer, a short workspace. Three kernels on `stream`. */
int nexg_match_select(nexg_ctx* ctx, const nexg_frames* frames, const nexg_match* matches,
                      uint32_t any_mask, uint32_t all_mask, uint32_t none_mask, uint32_t* out_index,
                      uint64_t* out_off, uint32_t* out_len, uint64_t* out_count, void* workspace,
                      uint64_t workspace_bytes, void* stream);
static inline uint64_t nexg_match_select_workspace(uint64_t count) {
    const uint64_t tiles = (count + 255u) / 256u;
    return 4u * ((tiles + 255u) / 256u * 256u) + 16u;
}

/* ---- header rewrite (mutable setters, the other half of SURVEY.md a20) ----------
 * nexg_rewrite_batch changes header fields of the frames in place, with the
 * semantics of the reference's mutable setters under ChecksumMode::Automatic
 * (checksum.rs:8-14, ipv4.rs:621-626: every set recomputes the checksum):
 * MutableEthernetPacket::set_destination / set_source, MutableIpv4Packet::
 * set_source / set_destination / set_ttl / set_dscp / set_ecn,
 * MutableIpv6Packet::set_source / set_destination / set_hop_limit /
 * set_traffic_class, MutableTcpPacket / MutableUdpPacket::set_source /
 * set_destination (examples/mutable_chaining.rs is the example caller). An
 * action names the fields and their values; a set holds up to 16 actions, and
 * a per-frame index picks one: with the out_rule of nexg_select_batch as the
 * index, rule j of a filter gets action j. The text below is the whole
 * specification (nex_amd/rewrite.py rewrite_host restates it on the host).
 *
 * Per frame i, in this order:
 * 1. Action. a = action_index ? action_index[i] : 0. If a >= n_actions
 *    (NEXG_ACTION_NONE and any other value: the index is caller memory and
 *    never indexes past the set) the frame is untouched and its row is
 *    {0, 0, NEXG_ACTION_NONE, 0, 0}. A frame whose extent is invalid (the
 *    fix-up's rule: it leaves [0, data_bytes) or is longer than 65535) is
 *    untouched and gets {0, 0, a, 0, 0}.
 * 2. Views: exactly those of the fix-up above. The Ethernet view: not
 *    NEXG_PARSE_FROM_IP, len >= 14. The IPv4 view under MutableIpv4Packet::
 *    new's conditions, the IPv6 view (>= 40 B, payload = everything after 40,
 *    extension headers not walked), L = the IP header's offset (14, or
 *    ip_offset with NEXG_PARSE_FROM_IP, where the version nibble picks the
 *    family). The UDP / TCP / ICMP / ICMPv6 views over the IP view's payload
 *    [P, P + m) under the fix-up's length conditions. In INCREMENTAL mode
 *    only, an IPv4 frame whose 13-bit fragment offset is not 0 has no L4 view
 *    (a later fragment holds no L4 header).
 * 3. Fields: each is written when its bit is set and its view exists. MACs
 *    need the Ethernet view. Addresses need the IP view of action.family
 *    (IPv4: bytes L+12.. and L+16..; IPv6: L+8.. and L+24..). TTL: IPv4 byte
 *    L+8, IPv6 byte L+7. TOS: IPv4 byte L+1; IPv6 traffic class = the low
 *    nibble of byte L and the high nibble of byte L+1. Ports need the UDP or
 *    TCP view: bytes P..P+1 and P+2..P+3, big-endian. `applied` gets the bit
 *    of every field written, whether or not the value changed (the reference
 *    marks a checksum dirty on every set).
 * 4. Dirty checksums. IPv4 header: the IPv4 view exists and any of IP_SRC,
 *    IP_DST, TTL, DEC_TTL, TOS was applied. L4: an L4 view exists and a port
 *    was applied, or an address was applied and the protocol is not ICMPv4 (1:
 *    no pseudo-header; ICMPv6 has one). IPv6 TTL and TOS dirty nothing.
 * 5. Default mode (flags == 0, RECOMPUTE): the frame's final bytes are the
 *    edited bytes passed through nexg_recompute_checksums_batch with `which` =
 *    the dirty set. Like the reference's views it knows nothing of fragments.
 * 6. NEXG_REWRITE_INCREMENTAL: RFC 1624 eqn. 3 on the stored value,
 *    HC' = ~fold(~HC + sum(~m_k + m'_k)) over the 16-bit words of every
 *    applied field the checksum covers (IPv4 header: the words at L+0 (TOS),
 *    L+8 (TTL) and the address words; L4: the pseudo-header address words and
 *    the port words); fold is the end-around carry fold to 16 bits. A UDP view
 *    over IPv4 whose stored checksum is 0 ("none") keeps 0 and `fixed` does
 *    not get NEXG_FIX_L4. There is no 0 -> 0xFFFF mapping (the reference has
 *    none). A frame whose stored checksums were the fix-up's
 *    values comes out byte-identical to RECOMPUTE; a wrong checksum stays
 *    wrong by the same amount. Only header bytes are used: at most the
 *    Ethernet, IP and first 20 L4 bytes. The kernel loads them as the frame's
 *    first 16-B blocks (at most six) and never sums the payload.
 *
 * Stores touch only the bytes of the fields and checksum fields named above,
 * as single bytes; every other byte of frames->data keeps its value, the gaps
 * between frames included. Frames must not overlap (then the result is
 * unspecified, but no store leaves a frame's own extent). No atomics: a run
 * repeats bit for bit. Reads follow the 16-B block rule of the frame batch
 * layout. count == 0 launches nothing; one kernel on `stream`; no workspace.
 *
 * NEXG_EINVAL for a set (nexg_actions_check tells): n_actions 0 or above 16,
 * unknown flags or sets bits, nonzero reserved, SET_TTL together with
 * DEC_TTL, DEC_TTL with ttl == 0, an address set with a family other than 4
 * or 6, a nonzero family without an address set, SET_TOS with tos_mask == 0
 * or tos & ~tos_mask. sets == 0 is valid: the "leave it" action of a rule.
 * From nexg_rewrite_batch itself: a NULL frames, option or actions, an
 * invalid frame table, a misaligned out. */
#define NEXG_SET_ETH_DST  0x001u  /* frame bytes 0..5  = eth_dst */
#define NEXG_SET_ETH_SRC  0x002u  /* frame bytes 6..11 = eth_src */
#define NEXG_SET_IP_SRC   0x004u
#define NEXG_SET_IP_DST   0x008u
#define NEXG_SET_SRC_PORT 0x010u
#define NEXG_SET_DST_PORT 0x020u
#define NEXG_SET_TTL      0x040u  /* IPv4 ttl / IPv6 hop limit = ttl */
#define NEXG_DEC_TTL      0x080u  /* ... = old > ttl ? old - ttl : 0 */
#define NEXG_SET_TOS      0x100u  /* IPv4 byte 1 / IPv6 traffic class = (old & ~tos_mask) | tos */
#define NEXG_SET_ALL      0x1FFu
#define NEXG_REWRITE_INCREMENTAL 0x1u   /* nexg_actions.flags */
#define NEXG_REWRITE_MAX_ACTIONS 16
#define NEXG_ACTION_NONE 0xFFu
typedef struct nexg_action {      /* 64 bytes */
    uint32_t sets;                /* NEXG_SET_* / NEXG_DEC_TTL */
    uint8_t family;               /* 4 or 6 with an address set, else 0 */
    uint8_t ttl, tos, tos_mask;
    uint16_t src_port, dst_port;  /* host order values */
    uint8_t eth_dst[6], eth_src[6];
    uint8_t src[16], dst[16];     /* network order; family 4 uses the first 4 bytes */
    uint8_t reserved[8];          /* must be 0 */
} nexg_action;
typedef struct nexg_actions {     /* host memory, 1032 bytes; read during the call only */
    uint32_t n_actions, flags;
    nexg_action actions[NEXG_REWRITE_MAX_ACTIONS];
} nexg_actions;
typedef struct nexg_rewritten {   /* 8 bytes */
    uint16_t applied;             /* NEXG_SET_* / NEXG_DEC_TTL bits of the fields written */
    uint8_t fixed;                /* NEXG_FIX_IP / NEXG_FIX_L4: checksum fields written */
    uint8_t action;               /* the action used, NEXG_ACTION_NONE if none */
    uint16_t ip_csum, l4_csum;    /* values written (0 where not written) */
} nexg_rewritten;

/* NEXG_OK when nexg_rewrite_batch would accept the set, else NEXG_EINVAL.
 * Host only: no context, no device. */
int nexg_actions_check(const nexg_actions* actions);

/* action_index: device memory, `count` entries, or NULL (action 0 for every
 * frame). out (optional, 8-B aligned): nexg_rewritten[count]. The batch's
 * data must be writable device memory. */
int nexg_rewrite_batch(nexg_ctx* ctx, const nexg_frames* frames, const nexg_parse_option* option,
                       const nexg_actions* actions, const uint8_t* action_index, nexg_rewritten* out,
                       void* stream);

/* ---- flow keys, RSS hash and flow-affine partition (extension) -----------------
 * The reference has no flow notion; like the selection above this is an
 * extension, and the text below is its whole specification
 * (nex_amd/flow.py flow_host / partition_host / sort_host / groups_host
 * restate it on the host).
 * nexg_flow_batch gives every frame of a batch already parsed with
 * NEXG_OUT_RECORD (any parse option; an inner table from nexg_decap_batch with
 * its inner records works too) an 8-byte flow row: the Toeplitz RSS hash of its
 * addresses and ports, as NICs, DPDK and the Linux drivers compute it.
 * nexg_flow_partition splits a frame table into up to 256 buckets by that hash,
 * stably, so that every flow lands whole in one bucket.
 *
 * Which frames have a flow. Only the record decides. status must be 0, and
 * the frame needs NEXG_L_IPV4, or (without NEXG_L_IPV4) NEXG_L_IPV6 with a
 * valid extent and l3_off + 40 <= len(i). Every other frame (ARP,
 * Ethernet-only, an error status, a bad extent, a record whose l3_off points
 * past its frame) gets an all-zero row.
 *
 * Addresses. IPv4: record.ip_src and ip_dst as four big-endian bytes each.
 * IPv6: frame bytes [l3_off + 8, l3_off + 24) and [l3_off + 24, l3_off + 40)
 * (the record does not carry them; the 16-B block rule of the frame batch
 * layout applies and nothing outside the frame's own blocks is read).
 *
 * Ports join the key when the record has NEXG_L_TCP or NEXG_L_UDP and
 * NEXG_FLOW_NO_PORTS is clear, except for an IPv4 frame with
 * (ip_word & 0x3FFF) != 0 (MF set, or a fragment offset): NICs leave the ports
 * out there as well, so all fragments of a datagram hash alike. That gives
 * `kind` its _L4 value or the plain one. Nothing else is special-cased: an
 * IPv6 fragment header is not detected (the parser gives such a frame no
 * transport layer, so it hashes on its addresses), and IPv6 extension-header
 * address options (home address, routing header) are not followed.
 *
 * Key bytes: source address, destination address, then src_port and dst_port
 * as two big-endian bytes each: 8, 12, 32 or 36 bytes. Under
 * NEXG_FLOW_SYMMETRIC the byte string (source address, src_port) is compared
 * with (destination address, dst_port), the addresses alone when the ports are
 * not part of the key; when the source side is greater the endpoints are
 * exchanged before hashing and `swapped` is 1, so both directions of a
 * conversation get one key.
 *
 * Hash: the Toeplitz RSS hash with a 320-bit key K. For every set bit of the
 * key bytes, bit s counted from the most significant bit of byte 0, the 32 key
 * bits K[s, s + 32) are XORed into the 32-bit result. 36 input bytes reach key
 * bit 319: 40 key bytes always suffice. The default key is the Microsoft RSS
 * verification key NEXG_FLOW_DEFAULT_KEY, so a hash computed here equals the
 * one such hardware put in the descriptor; NEXG_FLOW_KEY takes option->key
 * instead.
 *
 * NEXG_EINVAL: unknown flag bits, reserved != 0, a NULL pointer with
 * count > 0, a misaligned pointer (records 16 B, out 8 B). count == 0 launches
 * nothing. One kernel on `stream`. */
#define NEXG_FLOW_SYMMETRIC 0x1u /* both directions of a conversation get one key */
#define NEXG_FLOW_NO_PORTS 0x2u  /* 2-tuple only */
#define NEXG_FLOW_KEY 0x4u       /* use option->key; else NEXG_FLOW_DEFAULT_KEY */
#define NEXG_FLOW_DEFAULT_KEY                                                                     \
    {0x6d, 0x5a, 0x56, 0xda, 0x25, 0x5b, 0x0e, 0xc2, 0x41, 0x67, 0x25, 0x3d, 0x43, 0xa3, 0x8f, 0xb0, \
     0xd0, 0xca, 0x2b, 0xcb, 0xae, 0x7b, 0x30, 0xb4, 0x77, 0xcb, 0x2d, 0xa3, 0x80, 0x30, 0xf2, 0x0c, \
     0x6a, 0x42, 0xb7, 0x3b, 0xbe, 0xac, 0x01, 0xfa}
typedef struct nexg_flow_option { /* host memory; read during the call, not after it */
    uint32_t flags;    /* NEXG_FLOW_*; unknown bits -> NEXG_EINVAL */
    uint32_t reserved; /* must be 0 */
    uint8_t key[40];   /* NEXG_FLOW_KEY */
} nexg_flow_option;
enum { NEXG_FLOW_NONE = 0, NEXG_FLOW_IPV4 = 1, NEXG_FLOW_IPV4_L4 = 2, NEXG_FLOW_IPV6 = 3, NEXG_FLOW_IPV6_L4 = 4 };
typedef struct nexg_flow { /* 8 bytes */
    uint32_t hash;    /* Toeplitz hash of the key bytes; 0 for NEXG_FLOW_NONE */
    uint8_t kind;     /* NEXG_FLOW_* */
    uint8_t proto;    /* record.ip_proto; 0 for NONE */
    uint8_t swapped;  /* 1 when NEXG_FLOW_SYMMETRIC exchanged the endpoints */
    uint8_t reserved; /* 0 */
} nexg_flow;
int nexg_flow_batch(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records,
                    const nexg_flow_option* option /* NULL = defaults */, nexg_flow* out /* 8-B aligned */,
                    void* stream);

/* Stable split of a frame table into `buckets` (1..256) buckets:
 * bucket(i) = flows[i].hash % buckets (frames without a flow have hash 0 and
 * fall into bucket 0). The output is ordered by bucket, then by frame index.
 * bucket_first[b] (buckets + 1 entries, device memory, 8-B aligned) = the
 * number of frames in buckets below b; bucket_first[buckets] = count. For the
 * k-th output entry out_index[k] = i, and out_off[k] / out_len[k] (both NULL,
 * or both given) = off(i) / len(i) exactly as nexg_select_batch stores them.
 * For every b, {data, data_bytes, out_off + bucket_first[b], out_len +
 * bucket_first[b], bucket_first[b + 1] - bucket_first[b]} is a frame table
 * that parse, decap, dns, select and gather take as it stands, monotone
 * whenever the input was packed, fixed-stride or monotone; nexg_gather_rows
 * with out_index reorders records or any other per-frame rows to match. The
 * output arrays have capacity `count` (out_off 8-B, out_index / out_len 4-B
 * aligned); count must not exceed 2^32 - 1.
 *
 * The partition works on tiles of NEXG_FLOW_TILE = 1024 frames: a count
 * kernel writes one histogram per tile, bucket-major (buckets x tiles u32
 * counters), a three-kernel hierarchical scan (sums of 1024-counter chunks,
 * a scan of the chunk sums, the add-back) turns them into the global base of
 * every (bucket, tile) pair, and a scatter kernel recomputes each frame's
 * stable rank inside its tile. Positions come from ballots, ranks and scans
 * only (no atomics): a run repeats bit for bit. `flows` and the workspace are
 * caller memory: every store is bounded by `count`, whatever they hold.
 * workspace: device memory (8-B aligned) of at least
 * nexg_flow_partition_workspace(count, buckets) bytes. count == 0 writes
 * bucket_first[0..buckets] = 0 and launches nothing else. NEXG_EINVAL:
 * buckets outside 1..256, an invalid frame table, a NULL or misaligned
 * pointer (flows 8 B), only one of out_off / out_len NULL, a short workspace.
 * Five kernels on `stream`. */
#define NEXG_FLOW_TILE 1024u
int nexg_flow_partition(nexg_ctx* ctx, const nexg_frames* frames, const nexg_flow* flows, uint32_t buckets,
                        uint32_t* out_index, uint64_t* out_off, uint32_t* out_len, uint64_t* bucket_first,
                        void* workspace, uint64_t workspace_bytes, void* stream);
/* 8 B (the scan's total), one u32 per chunk of 1024 counters, then the
 * buckets x ceil(count / 1024) counters */
static inline uint64_t nexg_flow_partition_workspace(uint64_t count, uint32_t buckets) {
    const uint64_t tiles = (count + NEXG_FLOW_TILE - 1u) / NEXG_FLOW_TILE;
    const uint64_t counters = tiles * buckets;
    const uint64_t chunks = (counters + 1023u) / 1024u;
    return 8u + 4u * ((chunks + 1u) & ~(uint64_t)1u) + 4u * counters;
}

/* Per-flow counters: sort a batch by flow hash, then reduce it to one row per
 * run of equal hashes.
 *
 * nexg_flow_sort: out_index[k] (count entries, 4-B aligned) = the frame number
 * of the k-th frame when the frames are ordered by (flows[i].hash ascending,
 * i ascending). All frames take part; frames without a flow have hash 0 and
 * come first. It is a stable LSD radix sort: four 8-bit digit passes over
 * (hash, index) pairs held in the workspace, each pass the partition's count
 * kernel, three-kernel counter scan and scatter at 256 buckets; the first pass
 * makes the pairs from `flows`, the last stores the frame numbers alone.
 * Positions come from ballots, ranks and scans only (no atomics): a run
 * repeats bit for bit. `flows` and the workspace are caller memory: every
 * store is bounded by `count`, whatever they hold between the passes.
 * workspace: device memory (8-B aligned) of at least the sort's workspace
 * helper's bytes. count == 0 launches nothing. NEXG_EINVAL: count > 2^32 - 1,
 * a NULL or misaligned pointer (flows 8 B, out_index 4 B, workspace 8 B), a
 * short workspace. Twenty kernels on `stream`. */
int nexg_flow_sort(nexg_ctx* ctx, const nexg_flow* flows, uint64_t count, uint32_t* out_index, void* workspace,
                   uint64_t workspace_bytes, void* stream);
/* the partition's workspace at 256 buckets, then two buffers of `count`
 * 8-byte pairs */
static inline uint64_t nexg_flow_sort_workspace(uint64_t count) {
    return nexg_flow_partition_workspace(count, 256u) + 16u * count;
}

/* nexg_flow_groups: a group is a maximal run of equal flows[order[k]].hash in
 * `order` (nexg_flow_sort's out_index); groups are numbered in run order, so
 * ascending by hash. *out_count (device memory, 8-B aligned) = the number of
 * groups, written even when it exceeds groups_cap; rows at or past groups_cap
 * are not stored. out_group (optional, count entries, 4-B aligned):
 * out_group[order[k]] = the group number of position k, defined when `order`
 * is a permutation.
 *
 * The key of a frame is (kind, proto, key bytes), recomputed from its record
 * and frame bytes exactly as nexg_flow_batch documents above under `option`'s
 * NEXG_FLOW_SYMMETRIC / NEXG_FLOW_NO_PORTS (which frames have a flow, the IPv4
 * fragment rule, the IPv6 addresses from [l3_off + 8, l3_off + 40), the
 * exchange of the endpoints); the Toeplitz key plays no part. Two frames
 * without a flow have equal keys. `mixed` counts the positions k of the group
 * other than its first whose key differs from the key of position k - 1:
 * mixed == 0 if and only if the group is exactly one flow, and a nonzero
 * `mixed` marks a 32-bit hash collision, which the caller resolves from the
 * members order[first .. first + packets).
 *
 * `order`, `flows`, `records` and the workspace are caller memory. An order
 * entry >= count stands for a frame with an all-zero flow row, no key and
 * length 0: nothing is read for it and it gets no out_group store. Nothing
 * outside a frame's own 16-B blocks is read, and no store leaves
 * out[0, groups_cap), out_group[0, count) or *out_count.
 *
 * One kernel per sorted position computes a head flag (the hash differs from
 * the position before), a break flag (same hash, another key) and the length,
 * and scans them inside its 256-position tile; one-workgroup scans of the
 * tiles' totals, a kernel that numbers the groups, and one lane per group
 * taking differences of the prefixes follow. The work is linear in `count`
 * however the groups are sized; no atomics. count == 0 writes *out_count = 0
 * and launches nothing else. NEXG_EINVAL: unknown option flag bits,
 * reserved != 0, a NULL or misaligned pointer (records 16 B, out 16 B, flows /
 * out_count / workspace 8 B, order / out_group 4 B), an invalid frame table,
 * count > 2^32 - 1, a short workspace. Six kernels on `stream`. */
typedef struct nexg_flow_group { /* 32 bytes */
    uint32_t hash;        /* flows[first_index].hash */
    uint8_t kind, proto;  /* flows[first_index].kind / .proto */
    uint8_t flags8;       /* bit 0: mixed != 0 */
    uint8_t reserved;     /* 0 */
    uint32_t first;       /* position in `order` of the group's first member */
    uint32_t packets;     /* members: order[first .. first + packets) */
    uint64_t bytes;       /* sum of len(i) over the members with a valid extent (else 0) */
    uint32_t mixed;       /* members whose key differs from the member before them in the group */
    uint32_t first_index; /* order[first]: the group's earliest frame */
} nexg_flow_group;
int nexg_flow_groups(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records, const nexg_flow* flows,
                     const nexg_flow_option* option /* as given to nexg_flow_batch; NULL = defaults */,
                     const uint32_t* order, nexg_flow_group* out, uint64_t groups_cap, uint32_t* out_group,
                     uint64_t* out_count, void* workspace, uint64_t workspace_bytes, void* stream);
/* 16 B (two scan totals), per 256-position tile a u64 and two u32 (padded to
 * an even count), per position a u64 of in-tile prefixes and a u32 group start */
static inline uint64_t nexg_flow_groups_workspace(uint64_t count) {
    const uint64_t tiles = (count + 255u) / 256u;
    const uint64_t tp = (tiles + 1u) & ~(uint64_t)1u;
    return 16u + 8u * tiles + 8u * count + 8u * tp + 4u * ((count + 1u) & ~(uint64_t)1u);
}

/* The flow table: per-flow counters across batches. A table is an array of
 * 64-byte entries in device memory, strictly ascending by `hash`, one entry
 * per hash. The merge takes a table and the groups of one batch
 * (nexg_flow_groups' rows, so strictly ascending by hash as well) and writes
 * the new table: table_out = the union of table_in[0, n_in) and
 * groups[0, n_groups) by hash, ascending. It is a pure function of its
 * inputs: table_in is not changed, and a caller keeps two buffers and swaps
 * them.
 *
 * A hash in both: the entry is table_in's with `packets` and `bytes`
 * increased by the group's and last_epoch = epoch. MIXED is set when it was
 * set already, or the group has mixed != 0 (its flags8 bit 0), or the
 * group's key differs from the entry's (kind, proto, key): all 36 key bytes
 * are compared, so an entry's padding must be zero, as the merge writes it.
 * The group's key is the (kind, proto, key bytes) of frame `first_index`,
 * recomputed from its record and frame bytes exactly as the groups pass
 * recomputes keys, under `option`'s NEXG_FLOW_SYMMETRIC / NEXG_FLOW_NO_PORTS
 * (the Toeplitz key plays no part). So MIXED is set if and only if two or
 * more distinct keys have ever been counted under the hash; a collision is
 * flagged, never silently merged, and the entry keeps the first key seen.
 *
 * A hash only in the groups: a new entry with the group's hash, packets and
 * bytes, the recomputed key (kind, proto, the key bytes zero-padded to 36),
 * MIXED from the group's flags8 bit 0, and last_epoch = epoch.
 *
 * A hash only in table_in: the entry is copied unchanged when
 * last_epoch >= min_epoch and dropped otherwise (a plain unsigned compare,
 * no wrap-around; min_epoch = 0 keeps everything). A matched entry is never
 * dropped. This is the timeout: the caller picks what an epoch is (a batch
 * number, seconds) and passes min_epoch = epoch - timeout.
 *
 * The group of frames without a flow (hash 0, kind NEXG_FLOW_NONE, empty key)
 * is not special: it gets an entry like any other, and a real flow that
 * hashes to 0 marks it MIXED.
 *
 * *out_count (device memory, 8-B aligned) = the size of the union, written
 * even when it exceeds table_cap; rows at or past table_cap are not stored.
 * out_slot (optional, n_groups entries, 4-B aligned): out_slot[j] = the
 * position in the union of group j's entry, stored for every j whatever the
 * capacity; with nexg_flow_groups' out_group it maps a frame to its entry.
 *
 * Caller memory: a first_index >= frames->count is a frame without a flow,
 * and nothing is read for it (an empty frame table with such groups merges
 * made-up rows). If table_in or groups are not ascending the result is
 * unspecified, but even then every store stays inside
 * table_out[0, table_cap), out_slot[0, n_groups) and *out_count, and nothing
 * outside the arrays given, or outside a frame's own 16-B blocks, is read.
 *
 * A merge-path merge, without atomics (positions come from ranks and scans
 * only, so a run repeats bit for bit). The merged order is by hash, a table
 * entry before the group of the same hash. Per 256-position tile of that
 * order one workgroup finds the tile's split of the two arrays by a binary
 * search along its diagonal, stages the two runs' hashes in LDS, ranks each
 * element against the other run there (which also tells whether its hash is
 * in both), and scans the "leaves an entry" flags (a kept table entry, a
 * group with a new hash); a one-workgroup scan of the tiles' totals gives
 * every tile's first slot and *out_count; the write kernel builds each
 * surviving position's entry and stores it with 16-byte stores.
 * n_in == 0 && n_groups == 0 writes *out_count = 0 and launches nothing
 * else. workspace: device memory (8-B aligned) of at least the table
 * workspace helper's bytes. NEXG_EINVAL: unknown option flag bits,
 * reserved != 0, a NULL or misaligned pointer (records / groups / table_in /
 * table_out 16 B, out_count / workspace 8 B, out_slot 4 B), table_out
 * overlapping table_in, n_in or n_groups above 2^31 - 1, an invalid frame
 * table, a short workspace. Three kernels on `stream`. */
#define NEXG_FLOW_ENTRY_MIXED 0x1u
typedef struct nexg_flow_entry { /* 64 bytes, 16-B aligned */
    uint32_t hash;
    uint8_t kind, proto; /* of the recomputed key of the first frame ever seen under this hash */
    uint8_t flags8;      /* bit 0 NEXG_FLOW_ENTRY_MIXED: more than one key has been seen under this hash */
    uint8_t reserved;    /* 0 */
    uint8_t key[36];     /* that key's bytes (0, 8, 12, 32 or 36 of them), zero-padded */
    uint32_t last_epoch; /* `epoch` of the last merge that touched the entry */
    uint64_t packets;
    uint64_t bytes;
} nexg_flow_entry;
int nexg_flow_table_merge(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records,
                          const nexg_flow_option* option /* as given to nexg_flow_batch; NULL = defaults */,
                          const nexg_flow_group* groups, uint64_t n_groups, const nexg_flow_entry* table_in,
                          uint64_t n_in, uint32_t epoch, uint32_t min_epoch, nexg_flow_entry* table_out,
                          uint64_t table_cap, uint32_t* out_slot, uint64_t* out_count, void* workspace,
                          uint64_t workspace_bytes, void* stream);
/* per position of the merged order (n_in + n_groups of them) a u64, then a
 * u32 per 256-position tile (padded to an even count) */
static inline uint64_t nexg_flow_table_workspace(uint64_t n_in, uint64_t n_groups) {
    const uint64_t n = n_in + n_groups;
    const uint64_t tiles = (n + 255u) / 256u;
    return 8u * n + 4u * ((tiles + 1u) & ~(uint64_t)1u);
}

/* ---- IPv4 reassembly (RFC 791 section 3.2's way back; extension) ------------------
 * The inverse of nexg_fragment_*: the IPv4 fragments of a frame table are
 * grouped into datagrams, and every datagram whose pieces are all in the table
 * becomes one output frame. The first many-to-one pass: a group of input
 * frames, found by sorting, becomes one output frame. The reference has no
 * reassembly; this text is the whole specification, restated in plain Python
 * by nex_amd.reassemble.reassemble_host. No records are needed: the rules read
 * the frame's own bytes, as the fragment pass does.
 *
 * Per frame i, in this order:
 *  1 extent   An extent that leaves [0, data_bytes) or a length above 65535: no
 *             output, status NEXG_ERR_BAD_EXTENT, kind NEXG_REASM_NONE.
 *  2 not IPv4 nexg_fragment_plan's rule 3: bytes 12..13 are not 0x0800, len < 34,
 *             version != 4, IHL < 5, 14 + hl > len, TL < hl, or 14 + TL > len:
 *             kind NEXG_REASM_PASS, one output frame, the whole input copied
 *             unchanged. IPv6 and VLAN-tagged frames fall here.
 *  3 whole    MF clear and fragment offset 0: NEXG_REASM_PASS (the bytes past
 *             14 + TL are copied too).
 *  4 fragment otherwise. fo is the 13-bit offset, mf the MF bit, d = TL - hl; the
 *             key is (source address, destination address, protocol,
 *             identification), compared exactly.
 *
 * Datagrams. The fragments of one key form a datagram; its members are ordered
 * by (fo ascending, frame number ascending). It is complete when member 0 has
 * fo == 0; for every k >= 1, 8 fo_k == 8 fo_(k-1) + d_(k-1) and d_(k-1) >= 8 (no
 * gap, no overlap, no duplicate); MF is set on every member but the last and
 * clear on the last, and the last has d >= 1; hl_0 + 8 fo_last + d_last <= 65535;
 * and its hash run is not mixed (below).
 *   complete   Member 0 is the head, kind NEXG_REASM_HEAD, the others are
 *              NEXG_REASM_PART. One output frame stands at the head's place:
 *              output frames are ordered by the input index of the PASS or
 *              HEAD frame that produces them. Its length is 14 + hl_0 + D, D =
 *              8 fo_last + d_last. Bytes 0..13 and the hl_0 header bytes come
 *              from the head, options included; each member's data bytes
 *              [14 + hl_k, 14 + hl_k + d_k) land at 14 + hl_0 + 8 fo_k. In the
 *              header the total length is hl_0 + D, bytes 6..7 become old &
 *              0xC000 (reserved and DF kept, MF cleared, offset 0) and the
 *              checksum is recomputed as ipv4::checksum. Everything else in
 *              the other members' Ethernet and IP headers is ignored, as are
 *              input bytes past 14 + TL. Input header checksums are not
 *              verified: select on NEXG_C_IP_OK first for that.
 *   incomplete every member is NEXG_REASM_HELD, no output frame, status
 *              NEXG_FRAME_OK: the bytes stay where they are for the caller to
 *              carry into a later batch (nexg_reasm_held).
 *
 * Finding the groups. A 32-bit hash is taken over 12 key bytes: the source
 * address, the destination address, then 0, the protocol, 0, 0 (the protocol
 * where nexg_flow_batch has the source port, 0 for the destination port): the
 * Toeplitz hash of nexg_flow_batch with NEXG_FLOW_DEFAULT_KEY. The
 * identification is not hashed. The fragments are ordered by (hash,
 * identification, fo, frame number) with nexg_flow_sort's stable radix passes:
 * four 8-bit digit passes over id << 13 | fo, then four over the hash starting
 * from that order. A run of equal (hash, identification) is one datagram
 * unless two members' exact keys differ: such a run is mixed (a 32-bit hash
 * collision between two address pairs that use one identification at once),
 * every member of it is NEXG_REASM_HELD with flag NEXG_REASM_COLLISION and none
 * is reassembled on the device; the caller resolves those few frames
 * (reassemble_host does it exactly). Heads, breaks and contiguity are found
 * per sorted position, a group's verdict by prefix differences: the work is
 * linear in the count however the groups are sized. Deterministic, no atomics.
 *
 * Out of scope: IPv6 fragment headers; overlap or duplicate resolution (a
 * retransmitted fragment makes its datagram HELD); resolving a mixed run on the
 * device; verifying input checksums; fixing L4 checksums; VLAN-tagged or
 * tunnelled inner headers; TCP stream reassembly; a hash table across batches
 * (carrying over is done by re-submitting the held frames). */
#define NEXG_REASM_NONE 0  /* no output frame: an error status */
#define NEXG_REASM_PASS 1  /* one output frame, the input copied unchanged */
#define NEXG_REASM_HEAD 2  /* member 0 of a complete datagram: its output frame stands here */
#define NEXG_REASM_PART 3  /* another member of a complete datagram */
#define NEXG_REASM_HELD 4  /* a fragment of an incomplete datagram or of a mixed run */
#define NEXG_REASM_COLLISION 0x1u
typedef struct nexg_reasm {        /* 16 bytes, one per input frame */
    uint8_t status;                /* NEXG_FRAME_OK / NEXG_ERR_* */
    uint8_t kind;                  /* NEXG_REASM_* */
    uint8_t hdr_len;               /* hl of a fragment, else 0 */
    uint8_t flags;                 /* NEXG_REASM_COLLISION */
    uint16_t members;              /* HEAD: member count, else 0 */
    uint16_t data_len;             /* HEAD: D, the datagram's data bytes, else 0 (what the fill's head
                                      takes the total length, the checksum and out_len from) */
    uint32_t out;                  /* PASS / HEAD / PART: index of the output frame it went into, else 0xFFFFFFFF */
    uint32_t head;                 /* HEAD / PART: input index of the head, else 0xFFFFFFFF */
} nexg_reasm;

/* Classify, sort, group, then two scans. out_first[i] (count + 1 entries, 4-B
 * aligned) = the number of output frames of the frames before i (each frame
 * gives 0 or 1), out_bytes[i] (count + 1 entries, 8-B aligned) = the sum of
 * their output frames' lengths, each rounded up to `align` (1, 4, 8 or 16);
 * the totals are in the last entries. rows[i] (required, 16-B aligned) reports
 * frame i. workspace: caller-owned device memory (16-B aligned) of at least the
 * bytes the helper below gives (NEXG_EINVAL when smaller): nexg_flow_sort's
 * workspace, then 32 B of classification, two sort keys, a mark, the order, an
 * output length and a group start per frame, and four values per 256-frame
 * tile. Scans only, no atomics. count == 0 writes the two zeros and launches
 * nothing else. NEXG_EINVAL also for count > 2^32 - 1, a NULL or misaligned
 * pointer, an align other than 1, 4, 8 or 16. 51 kernels on `stream`, 40 of them
 * the eight radix passes. */
int nexg_reasm_plan(nexg_ctx* ctx, const nexg_frames* frames, uint32_t align, uint32_t* out_first, uint64_t* out_bytes,
                    nexg_reasm* rows, void* workspace, uint64_t workspace_bytes, void* stream);
static inline uint64_t nexg_reasm_plan_workspace(uint64_t count) {
    const uint64_t tiles = (count + 255u) / 256u;
    const uint64_t even = (count + 1u) & ~(uint64_t)1u, even_tiles = (tiles + 1u) & ~(uint64_t)1u;
    const uint64_t sort = (nexg_flow_sort_workspace(count) + 15u) & ~(uint64_t)15u;
    return sort + 56u * count + 24u * tiles + 32u + 12u * even + 4u * even_tiles;
}

/* The fill. A PASS frame is copied to out_data (16-B aligned) + out_bytes[i];
 * a HEAD writes its datagram's header (total length, flags / offset and
 * checksum fixed) and its own data there; a PART copies its data to
 * out_bytes[h] + 14 + rows[h].hdr_len + 8 fo with h = rows[i].head and fo, d
 * from its own bytes; the member with MF clear writes the zero pad behind the
 * datagram. For the output frame f = out_first[i] of a PASS or HEAD frame:
 * out_offsets[f] (out_count + 1 entries, 8-B aligned) = where it starts,
 * out_len[f] its length, out_src[f] = i (4-B aligned, out_count entries each),
 * the index nexg_gather_rows takes to carry per-frame rows to the output;
 * out_offsets[out_count] = out_bytes[count]. rows, out_first and out_bytes are
 * caller memory: whatever they hold, no byte store lands at or past out_cap or
 * outside [out_bytes[h], out_bytes[h + 1]) of the head h < count it names (h =
 * i for PASS and HEAD), no table store lands at an index at or above
 * min(out_first[i + 1], out_count), and every loop is bounded by the frame's
 * own bytes. A rows[i].data_len that is not its datagram's D changes the
 * total length (bytes 16..17) and the checksum (bytes 24..25) of that head's
 * output header and its out_len, and nothing else: no bound depends on it.
 * Pads are zero. With a consistent plan every byte of an output
 * frame is written exactly once. The output is never read. Source reads follow
 * the 16-B block rule. Deterministic, no atomics, no workspace. NEXG_EINVAL: an
 * align other than 1, 4, 8 or 16, a NULL rows (count > 0), out_first, out_bytes
 * or out_offsets, a NULL out_len or out_src with out_count > 0, a NULL
 * out_data with out_cap > 0, a misaligned pointer, count or out_count > 2^32 -
 * 1. count == 0 launches nothing but the copy of the total. With align 1,
 * {out_data, total, out_offsets} is a packed batch that nexg_parse_batch,
 * nexg_decap_batch and nexg_fragment_plan take as it stands; with a larger
 * align, {out_data, total, out_offsets, out_len} an offsets + lengths batch
 * (monotone). One kernel on `stream`. */
int nexg_reasm_frames(nexg_ctx* ctx, const nexg_frames* frames, uint32_t align, const nexg_reasm* rows,
                      const uint32_t* out_first, const uint64_t* out_bytes, uint64_t out_count, uint64_t* out_offsets,
                      uint32_t* out_len, uint32_t* out_src, uint8_t* out_data, uint64_t out_cap, void* stream);

/* The NEXG_REASM_HELD frames as a frame table, in order: nexg_select_batch's
 * compaction with rows[i].kind == NEXG_REASM_HELD as the predicate. `count` is
 * the number of rows and must be frames->count (NEXG_EINVAL otherwise).
 * out_index[k] (4-B aligned) = the frame number, out_off[k] (8-B aligned) /
 * out_len[k] its table entry, *out_count (device memory, 8-B aligned) the
 * number held; the outputs hold `count` entries. workspace: caller-owned
 * device memory (4-B aligned) of at least the bytes the helper below gives.
 * The table goes to nexg_gather_plan / nexg_parse_batch as it stands. Three
 * kernels on `stream`; count == 0 launches the scan alone. */
int nexg_reasm_held(nexg_ctx* ctx, const nexg_frames* frames, const nexg_reasm* rows, uint64_t count,
                    uint32_t* out_index, uint64_t* out_off, uint32_t* out_len, uint64_t* out_count, void* workspace,
                    uint64_t workspace_bytes, void* stream);
static inline uint64_t nexg_reasm_held_workspace(uint64_t count) {
    const uint64_t tiles = (count + 255u) / 256u;
    return 4u * ((tiles + 255u) / 256u * 256u) + 16u;
}

/* ---- calibration (not a reference entry point) ---------------------------
 * The HBM stream ceilings the parse kernels are measured against, on the
 * caller's own buffer and box: `bytes` (a multiple of 16384) read with the
 * parse kernels' load shape (16-B non-temporal loads, 16-KiB tile per
 * 256-lane workgroup). out_per_64 = 8: for every 64 B read, 8 B written
 * (the nexg_desc stream shape): out[i] = {x, i} with x the XOR of the four
 * 16-B chunks lane i % 256 of tile i / 256 loaded (chunks i%256 + 256k).
 * out_per_64 = 9: the same stream capped at the fixed-stride parse kernel's
 * occupancy (6 workgroups per CU, by dynamic LDS; 8 runs 8 per CU).
 * out_per_64 = 0: read only; out[tile] = XOR of the tile's dwords (4 B per
 * 16 KiB). bench.py reports the headline kernel against both.
 * out_per_64 = 64: write only (the builders' copy-out shape: 16-B
 * non-temporal stores, 16 KiB per workgroup); `data` is not read (may be
 * NULL), `out` (16-B aligned) receives `bytes` bytes: dwords {tile, chunk, 0, 0}
 * per 16-B chunk. bench.py reports the serialize path against it. */
int nexg_probe_stream(nexg_ctx* ctx, const void* data, uint64_t bytes, uint32_t out_per_64,
                      void* out, void* stream);

/* Calibration (not a reference entry point): the clock a parse of this batch
 * runs at. Runs the span kernel that nexg_parse_batch runs for the batch
 * (packed layouts and monotone capture records; NEXG_EINVAL for any other
 * layout) with NEXG_OUT_GROUPED into `out` (NEXG_GROUPED_BYTES(count),
 * 16-B aligned: the same bytes nexg_parse_batch writes), in an
 * instance that also stores 8 u64 per 256-frame workgroup into `stamps`
 * (device, ceil(count / 256) * 8 entries, 8-B aligned): s_memtime (shader
 * clock ticks of the workgroup's XCD) at [0] entry, [1] after the span check,
 * [2] after the sub-tile loop, [3] after the fast path, [4] after the generic
 * section, [5] exit; s_memrealtime (100 MHz) at [6] entry and [7] exit. A
 * workgroup's clock is ([5] - [0]) / ([7] - [6]) x 100 MHz. The product
 * kernels contain no stamp. */
int nexg_probe_span_clock(nexg_ctx* ctx, const nexg_frames* frames, const nexg_parse_option* option,
                          void* out, uint64_t* stamps, void* stream);

/* Calibration (not a reference entry point): dependent HBM load latency.
 * Writes a ring into `buf` (device, `bytes` >= 4 MiB, 16-B aligned; 64-B
 * line i holds the index of line (i + 16411) mod (bytes / 64)) and has one lane
 * chase it for `steps` (1..2^20) dependent loads from line `start`, alone
 * (loaded = 0) or while 4 workgroups per CU stream-read the buffer (loaded =
 * 1: the conditions of a parse kernel's dependent loads). out (device, 4 u64,
 * 8-B aligned): [0] shader-clock ticks and [1] 100-MHz ticks over the chain;
 * per step = [1] / steps x 10 ns. The App. C mix's generic section waits on
 * such loads. */
int nexg_probe_latency(nexg_ctx* ctx, void* buf, uint64_t bytes, uint32_t steps, uint32_t start, uint32_t loaded,
                       uint64_t* out, void* stream);

/* ---- serialize path (udp_ping.rs:68-109 shape) -------------------------- */
typedef struct nexg_udp4_build {
    const uint32_t* src_ip;   /* per frame, IPv4 address as BE u32 value, or
                                 NULL -> def_src_ip (udp_ping: one source)   */
    const uint32_t* dst_ip;   /* per frame                                    */
    const uint16_t* src_port; /* per frame, or NULL -> def_src_port           */
    const uint16_t* dst_port; /* per frame, or NULL -> def_dst_port           */
    const uint16_t* ip_id;    /* per frame, or NULL -> def_ip_id              */
    const uint8_t* src_mac;   /* 6 bytes per frame, or NULL -> def_src_mac    */
    const uint8_t* dst_mac;   /* 6 bytes per frame, or NULL -> def_dst_mac    */
    const uint8_t* payload;   /* UDP payload shared by all frames (may be NULL) */
    uint32_t payload_len;
    uint16_t def_src_port, def_dst_port, def_ip_id;
    uint8_t def_src_mac[6], def_dst_mac[6];
    uint8_t ttl;      /* Ipv4PacketBuilder default 64 (builder/ipv4.rs:37)   */
    uint8_t ip_flags; /* 3-bit flags; udp_ping uses DontFragment = 0b010     */
    uint8_t dscp_ecn; /* dscp<<2|ecn, builder default 0                      */
    uint8_t reserved;
    uint32_t def_src_ip; /* source when src_ip is NULL (BE u32 value); sits in
                            what was padding, so the struct is unchanged in size */
    uint64_t count;
} nexg_udp4_build;

/* Writes frame i (42 + payload_len bytes) at out + i*out_stride.
 * NEXG_ERANGE if 28 + payload_len > 65535 (builder/udp.rs:83, ipv4.rs:153). */
int nexg_build_udp4_batch(nexg_ctx* ctx, const nexg_udp4_build* params,
                          uint8_t* out, uint32_t out_stride, void* stream);

/* The same build with each frame's tuple as one 16-B record (array of
 * structs, 16-B aligned): one 16-B load per frame instead of five arrays.
 * Ports and id are u16 values, addresses BE u32 values as above. */
typedef struct nexg_udp4_tuple {
    uint32_t src_ip, dst_ip;
    uint16_t src_port, dst_port;
    uint16_t ip_id, reserved;
} nexg_udp4_tuple;

/* nexg_build_udp4_batch with frame i's src_ip / dst_ip / src_port / dst_port /
 * ip_id from tuples[i] (params->count tuples); MACs, ttl, flags, dscp_ecn and
 * payload from params, whose per-frame arrays must all be NULL (NEXG_EINVAL
 * otherwise, or when tuples is NULL or not 16-B aligned). Same bytes as
 * nexg_build_udp4_batch on the same values. */
int nexg_build_udp4_tuples(nexg_ctx* ctx, const nexg_udp4_build* params, const nexg_udp4_tuple* tuples,
                           uint8_t* out, uint32_t out_stride, void* stream);

/* ---- udp_ping IPv6 branch (examples/udp_ping.rs:83-89) ---------------------
 * UdpPacketBuilder::build over IPv6 (builder/udp.rs:67-95; checksum =
 * udp::ipv6_checksum, udp.rs:480-505) -> Ipv6PacketBuilder::to_bytes
 * (builder/ipv6.rs:89-152; Ipv6Packet::to_bytes ipv6.rs:50-75) ->
 * EthernetPacketBuilder (EtherType 0x86DD). Frame = 62 + payload_len bytes. */
typedef struct nexg_udp6_build {
    const uint8_t* src_ip;    /* 16 bytes per frame, network order            */
    const uint8_t* dst_ip;    /* 16 bytes per frame                           */
    const uint16_t* src_port; /* per frame, or NULL -> def_src_port           */
    const uint16_t* dst_port; /* per frame, or NULL -> def_dst_port           */
    const uint8_t* src_mac;   /* 6 bytes per frame, or NULL -> def_src_mac    */
    const uint8_t* dst_mac;   /* 6 bytes per frame, or NULL -> def_dst_mac    */
    const uint8_t* payload;   /* UDP payload shared by all frames (may be NULL) */
    uint32_t payload_len;
    uint32_t flow_label;      /* low 20 bits (Ipv6PacketBuilder::flow_label masks) */
    uint16_t def_src_port, def_dst_port;
    uint8_t def_src_mac[6], def_dst_mac[6];
    uint8_t hop_limit;        /* Ipv6PacketBuilder default 64 (builder/ipv6.rs:33) */
    uint8_t traffic_class;    /* builder default 0                            */
    uint8_t src_shared;       /* 1: src_ip holds ONE address, the source of every
                                 frame (udp_ping's probe batch: one interface
                                 address, a destination per frame)            */
    uint8_t reserved;
    uint64_t count;
} nexg_udp6_build;

/* Writes frame i (62 + payload_len bytes) at out + i*out_stride.
 * NEXG_ERANGE if 8 + payload_len > 65535 (builder/udp.rs:83, builder/ipv6.rs:137).
 * With src_shared and every other per-frame array NULL (the probe batch) the
 * kernel reads 16 B per frame (dst_ip) and nothing else. */
int nexg_build_udp6_batch(nexg_ctx* ctx, const nexg_udp6_build* params,
                          uint8_t* out, uint32_t out_stride, void* stream);

/* ---- tcp_ping / icmp_ping ---------------------------------
 * IP + Ethernet layer shared by these builders: Ipv4PacketBuilder (IHL 5,
 * builder/ipv4.rs:94-170) or Ipv6PacketBuilder (builder/ipv6.rs:89-152), then
 * EthernetPacketBuilder (builder/ethernet.rs:63-70). */
typedef struct nexg_ip_build {
    const uint8_t* src_ip;    /* per frame: 4 B (family 4) or 16 B (family 6), network order, 4-B aligned */
    const uint8_t* dst_ip;
    const uint16_t* ip_id;    /* family 4: per frame, or NULL -> def_ip_id */
    const uint8_t* src_mac;   /* 6 B per frame, or NULL -> def_src_mac */
    const uint8_t* dst_mac;
    uint32_t family;          /* 4 or 6 */
    uint32_t flow_label;      /* family 6, low 20 bits */
    uint16_t def_ip_id;
    uint8_t def_src_mac[6], def_dst_mac[6];
    uint8_t ttl;              /* IPv4 TTL / IPv6 hop limit (builders default 64) */
    uint8_t ip_flags;         /* IPv4 3-bit flags (tcp_ping/icmp_ping: DontFragment 0b010) */
    uint8_t tos;              /* IPv4 dscp<<2|ecn / IPv6 traffic class */
    uint8_t src_shared;       /* 1: src_ip holds ONE address (4 or 16 B), the source of
                                 every frame: the probe batches of tcp_ping / icmp_ping
                                 (tcp_ping.rs:108-163, icmp_ping.rs:67-120: one interface
                                 address, a destination per target) */
    uint8_t reserved[2];
} nexg_ip_build;

/* TcpPacketBuilder::build (builder/tcp.rs:93-158; tcp.rs:521-575 to_bytes:
 * options zero-padded to 4 B, data offset = (20 + padded) / 4; checksum
 * tcp::checksum, tcp.rs:1207-1269), composed as examples/tcp_ping.rs:111-163.
 * Frame = 14 + (20|40) + 20 + padded options + payload_len bytes. */
typedef struct nexg_tcp_build {
    nexg_ip_build ip;
    const uint16_t* src_port; /* per frame, or NULL -> def_src_port */
    const uint16_t* dst_port;
    const uint32_t* seq;      /* per frame, or NULL -> def_seq */
    const uint32_t* ack;
    const uint8_t* payload;   /* shared by all frames (may be NULL) */
    uint32_t payload_len;
    uint32_t def_seq, def_ack;
    uint16_t def_src_port, def_dst_port;
    uint16_t window, urgent_ptr;
    uint8_t flags;
    uint8_t options_len;      /* encoded TcpOptionPacket bytes in options[] */
    uint8_t options[40];
    uint8_t reserved[2];
    uint64_t count;
} nexg_tcp_build;

/* IcmpPacketBuilder / Icmpv6PacketBuilder with echo_fields (builder/icmp.rs:
 * 14-86, builder/icmpv6.rs:14-90; checksums icmp.rs:429-432 / icmpv6.rs:
 * 589-599), composed as examples/icmp_ping.rs:67-102. Frame = 14 + (20|40)
 * + 8 + payload_len bytes. */
typedef struct nexg_icmp_echo_build {
    nexg_ip_build ip;
    const uint16_t* identifier; /* per frame, or NULL -> def_identifier */
    const uint16_t* sequence;   /* per frame, or NULL -> def_sequence */
    const uint8_t* payload;
    uint32_t payload_len;
    uint16_t def_identifier, def_sequence;
    uint8_t icmp_type, icmp_code; /* EchoRequest: 8/0 (IPv4), 128/0 (IPv6) */
    uint8_t reserved[2];
    uint64_t count;
} nexg_icmp_echo_build;

/* NEXG_ERANGE on BuildError::LengthOverflow (padded options > 40; segment >
 * 65515 (IPv4) / 65535 (IPv6); ICMP > 65515 / 65535). Probe batches: with
 * ip.src_shared set and every other per-frame array NULL (ports, seq / ack,
 * identifier / sequence, ip_id, MACs) the kernels read only dst_ip per frame
 * (4 / 16 B), as the tcp_ping / icmp_ping probes of one host vary only the
 * target. */
int nexg_build_tcp_batch(nexg_ctx* ctx, const nexg_tcp_build* params, uint8_t* out,
                         uint32_t out_stride, void* stream);
int nexg_build_icmp_echo_batch(nexg_ctx* ctx, const nexg_icmp_echo_build* params,
                               uint8_t* out, uint32_t out_stride, void* stream);

/* ---- arp / ndp probes (the callers examples/arp.rs, examples/ndp.rs) -------
 * ArpPacketBuilder::new(sender_mac, sender_ip, target_ip) (builder/arp.rs:
 * 18-37; build() rejects hw_addr_len != 6 / proto_addr_len != 4 with
 * InvalidFieldLength, :101-118 -> NEXG_EINVAL) serialised by ArpPacket::
 * to_bytes (arp.rs:385-399) behind EthernetPacketBuilder (EtherType 0x0806),
 * as examples/arp.rs:59-67 composes it. Frame = 14 + 28 = 42 bytes. */
typedef struct nexg_arp_build {
    const uint8_t* sender_ip;  /* 4 B per frame (network order), or NULL -> def_sender_ip */
    const uint8_t* target_ip;  /* 4 B per frame */
    const uint8_t* sender_mac; /* 6 B per frame, or NULL -> def_sender_mac (also the Ethernet source) */
    const uint8_t* target_mac; /* 6 B per frame, or NULL -> def_target_mac (builder: zero) */
    const uint8_t* eth_dst;    /* 6 B per frame, or NULL -> def_eth_dst (arp.rs: broadcast) */
    uint8_t def_sender_ip[4];
    uint8_t def_sender_mac[6], def_target_mac[6], def_eth_dst[6];
    uint16_t hardware_type;    /* ArpHardwareType::Ethernet = 1 */
    uint16_t protocol_type;    /* EtherType::Ipv4 = 0x0800 */
    uint16_t operation;        /* ArpOperation::Request = 1 */
    uint8_t hw_addr_len;       /* must be 6 */
    uint8_t proto_addr_len;    /* must be 4 */
    uint64_t count;
} nexg_arp_build;
int nexg_build_arp_batch(nexg_ctx* ctx, const nexg_arp_build* params, uint8_t* out,
                         uint32_t out_stride, void* stream);

/* NdpPacketBuilder::new(src_mac, src_ip, dst_ip).build() (builder/ndp.rs:
 * 30-84): a NeighborSolicit (type 135, code 0, reserved 0, target = dst_ip,
 * one SourceLLAddr option of length 1 carrying src_mac; icmpv6.rs:1385-1400)
 * with icmpv6::checksum over src_ip -> dst_ip (icmpv6.rs:589-599), inside
 * Ipv6PacketBuilder (next header 58) and EthernetPacketBuilder (0x86DD), as
 * examples/ndp.rs:82-108 composes it (hop limit 255; Ethernet destination
 * 33:33 + the target's last four bytes, ipv6_multicast_mac, ndp.rs:25-35).
 * ip.family must be 6; ip.dst_ip is the target; the option's MAC is the
 * Ethernet source. Frame = 14 + 40 + 32 = 86 bytes. */
typedef struct nexg_ndp_ns_build {
    nexg_ip_build ip;
    uint32_t eth_dst_multicast; /* 1: Ethernet destination from the target (ndp.rs); 0: ip.dst_mac / def */
    uint32_t reserved;
    uint64_t count;
} nexg_ndp_ns_build;
int nexg_build_ndp_ns_batch(nexg_ctx* ctx, const nexg_ndp_ns_build* params, uint8_t* out,
                            uint32_t out_stride, void* stream);

/* ---- capture-file batch ingest ---------------------------
 * Replaces nex-datalink's pcap::from_file channel (nex-datalink/src/pcap.rs:
 * 95-109) read one frame per RawReceiver::next (pcap.rs:178-190): each call
 * copies the next records' captured bytes back to back into a host buffer
 * (pinned for the H2D pipeline) and writes the packed offset table, ready for
 * nexg_parse_batch (offsets without lengths). Classic pcap (µs/ns, either
 * byte order) and pcapng (SHB, IDB, EPB, SPB, OPB). Host-side only. */
typedef struct nexg_pcap nexg_pcap;
int nexg_pcap_open(const char* path, nexg_pcap** out);
/* LINKTYPE of the file (first interface for pcapng): 1 = Ethernet; 101 =
 * raw IP (parse with NEXG_PARSE_FROM_IP, ip_offset 0). */
int nexg_pcap_linktype(const nexg_pcap* p);
const char* nexg_pcap_last_error(const nexg_pcap* p);
/* Up to max_frames records: frame k at data + offsets[k], offsets[n] = end
 * (offsets holds max_frames + 1 entries); ts_ns (optional) receives
 * timestamps in ns. *n_frames = 0 at end of file. A record that does not fit
 * data_cap waits for the next call (NEXG_ERANGE if not even one fits).
 * NEXG_EINVAL on a malformed or truncated file, after the complete records
 * before the damage were delivered. */
int nexg_pcap_read_batch(nexg_pcap* p, uint8_t* data, uint64_t data_cap, uint64_t* offsets,
                         uint64_t max_frames, uint64_t* ts_ns, uint64_t* n_frames);
/* In-place shape: the next file bytes are read straight into buf (up to cap,
 * one copy from the page cache) and the records found there are described by
 * offsets[k] / lengths[k] into buf (record headers stay in place; parse with
 * this offsets + lengths layout). Bytes of a record cut at the end of buf are
 * carried to the next call. *bytes_used = bytes of buf holding complete
 * records; *n_frames == 0 and *bytes_used == 0 means end of file. */
int nexg_pcap_read_raw(nexg_pcap* p, uint8_t* buf, uint64_t cap, uint64_t* offsets,
                       uint32_t* lengths, uint64_t max_frames, uint64_t* ts_ns,
                       uint64_t* n_frames, uint64_t* bytes_used);
/* Zero-copy shape: no read at all. nexg_pcap_map maps the file read-only
 * (the page cache itself; *data, *size = file bytes, *first = offset of the
 * first record or block). nexg_pcap_walk_mapped describes the records in the
 * window [from, from + max_bytes) of the mapping: offsets[k] (relative to
 * `from`) / lengths[k], *next = the offset after the last complete record
 * (the next call's `from`). The caller registers the mapping for DMA
 * (hipHostRegister) and copies [from, *next) to the GPU as is: the same
 * in-place layout as read_raw (record headers between frames, monotone), at
 * PCIe rate with no host copy. End of file when *next == size. Classic pcap
 * uses nexg_pcap_set_read_threads for the parallel walk. Use one shape per
 * reader: the mapped walk does not move the file position. */
int nexg_pcap_map(nexg_pcap* p, const uint8_t** data, uint64_t* size, uint64_t* first);
int nexg_pcap_walk_mapped(nexg_pcap* p, uint64_t from, uint64_t max_bytes, uint64_t* offsets,
                          uint32_t* lengths, uint64_t max_frames, uint64_t* ts_ns, uint64_t* n_frames,
                          uint64_t* next);
/* read_raw's file reads split over up to `threads` (1..64) parallel preads
 * of >= 4-MiB pieces (default 1), and for classic pcap the record walk of a
 * read (or mapped window) of >= 8 MiB split over as many threads, eight
 * interleaved chunks each (speculative chunk starts, stitched; a
 * disagreement re-walks that chunk). Results are identical for any count.
 * (read_batch stays single-threaded: parallel record copies into pinned
 * staging measured 2.5-4x slower on the GPU boxes, profiles/r01_ingest/threads.) */
int nexg_pcap_set_read_threads(nexg_pcap* p, uint32_t threads);
int nexg_pcap_close(nexg_pcap* p);

/* ---- live datalink batch rx / tx ---------------------------
 * The reference's Linux channel (nex-datalink/src/linux.rs:102-218) hands one
 * frame per RawReceiver::next (poll + recvfrom into a 4096-B buffer,
 * linux.rs:356-397) and sends one per RawSender::send (poll + sendto,
 * linux.rs:302-346); its scale-out is PACKET_FANOUT (lib.rs:70-131,
 * linux.rs:154-193). Here an AF_PACKET socket with the same Config knobs
 * (read_buffer_size, promiscuous, linux_fanout, read timeout) fills whole
 * batches: the TPACKET_V3 mmap ring (blocks of frames retired by the kernel)
 * or recvmmsg, copied into the caller's (pinned) buffer in the packed layout
 * nexg_pcap_read_batch produces (offsets only, parse with SpanTile). Each
 * frame is its first min(len, read_buffer_size) bytes, as recvfrom into the
 * reference's read buffer truncates it. One rx per GPU in one fanout group
 * is the multi-GPU ingest. Host-side only; needs
 * CAP_NET_RAW (open fails with NEXG_EPERM without it). */
#define NEXG_RX_RING 0u  /* TPACKET_V3 mmap ring (default)                   */
#define NEXG_RX_MMSG 1u  /* recvmmsg into read_buffer_size slots             */
/* FanoutType (nex-datalink/src/lib.rs:70-90) = PACKET_FANOUT_* */
#define NEXG_FANOUT_HASH 0u
#define NEXG_FANOUT_LB 1u
#define NEXG_FANOUT_CPU 2u
#define NEXG_FANOUT_ROLLOVER 3u
#define NEXG_FANOUT_RND 4u
#define NEXG_FANOUT_QM 5u
#define NEXG_FANOUT_FLAG_ROLLOVER 0x1000u /* FanoutOption.rollover */
#define NEXG_FANOUT_FLAG_DEFRAG 0x8000u   /* FanoutOption.defrag   */
/* rx flags: drop the loopback echo of frames this host sends (sll_pkttype
 * PACKET_OUTGOING); the reference keeps them (recvfrom discards sockaddr_ll,
 * linux.rs:358), so the default is to keep them too. */
#define NEXG_RX_SKIP_OUTGOING 0x1u
typedef struct nexg_rx_config {
    uint32_t read_buffer_size; /* Config.read_buffer_size (default 4096, lib.rs:229) */
    int32_t read_timeout_ms;   /* Config.read_timeout; -1 = wait (default)          */
    uint32_t promiscuous;      /* Config.promiscuous (default 1)                    */
    uint32_t fanout;           /* 1: join linux_fanout group below                  */
    uint32_t fanout_type;      /* NEXG_FANOUT_* | NEXG_FANOUT_FLAG_*               */
    uint32_t fanout_group;     /* FanoutOption.group_id                             */
    uint32_t mode;             /* NEXG_RX_RING / NEXG_RX_MMSG                       */
    uint32_t ring_block_size;  /* TPACKET_V3 block bytes (default 1 MiB)            */
    uint32_t ring_blocks;      /* blocks in the ring (default 64)                   */
    uint32_t ring_block_tov_ms;/* block retire timeout (default 2 ms)               */
    uint32_t flags;            /* NEXG_RX_*                                         */
    uint32_t reserved;
} nexg_rx_config;
typedef struct nexg_rx nexg_rx;
typedef struct nexg_tx nexg_tx;
void nexg_rx_config_default(nexg_rx_config* cfg);
int nexg_rx_open(const char* ifname, const nexg_rx_config* cfg, nexg_rx** out);
/* Up to max_frames frames (bytes packed: frame k at data + offsets[k],
 * offsets[n] = end; offsets holds max_frames + 1 entries); waits up to the
 * read timeout for the first frame (*n_frames = 0 on timeout), then takes
 * whatever the ring / socket already holds. ts_ns optional. NEXG_ERANGE
 * (nothing taken) when data_cap cannot hold the next frame (ring mode) or one
 * read_buffer_size slot (recvmmsg mode): a retry with a larger buffer
 * resumes at that frame. */
int nexg_rx_next_batch(nexg_rx* rx, uint8_t* data, uint64_t data_cap, uint64_t* offsets,
                       uint64_t max_frames, uint64_t* ts_ns, uint64_t* n_frames);
/* PACKET_STATISTICS since the last call: frames seen, frames dropped. */
int nexg_rx_stats(nexg_rx* rx, uint64_t* packets, uint64_t* drops);
int nexg_rx_close(nexg_rx* rx);
/* The ring walker on one retired TPACKET_V3 block (struct tpacket_block_desc
 * + tpacket3_hdr chain, linux/if_packet.h), from packet `first` on: frames
 * appended to the packed batch at data[*pos...] with offsets[*n...] until
 * max_frames / data_cap; *next_pkt = the first packet not taken (== the
 * block's num_pkts when done). What nexg_rx_next_batch runs on each block;
 * exported so the walk is tested on synthetic blocks without a socket. */
int nexg_tpacket3_walk(const uint8_t* block, uint64_t block_bytes, uint32_t first, uint32_t snap,
                       uint32_t flags, uint8_t* data, uint64_t data_cap, uint64_t* pos,
                       uint64_t* offsets, uint64_t max_frames, uint64_t* ts_ns, uint64_t* n,
                       uint32_t* next_pkt);
int nexg_tx_open(const char* ifname, nexg_tx** out);
/* Sends frames (host memory, the nexg_frames layout: offsets NULL -> stride)
 * with sendmmsg, up to 1024 per system call, waiting for POLLOUT as
 * RawSender::send does; *n_sent = frames the kernel accepted. */
int nexg_tx_send_batch(nexg_tx* tx, const uint8_t* data, const uint64_t* offsets, const uint32_t* lengths,
                       uint32_t stride, uint64_t count, uint64_t* n_sent);
int nexg_tx_close(nexg_tx* tx);

/* ---- synthetic workloads --------------------------
 * Frame i of a workload depends only on (seed, first_index + i), so shards
 * regenerate identically on any GPU count. */
#define NEXG_WL_UDP64 1 /* 64-B Eth/IPv4/UDP, 1/16 with a flipped checksum bit */
#define NEXG_WL_IMIX 2  /* 64/576/1500 at 7:4:1 over {v4,v6}x{TCP,UDP,ICMP}   */

/* Frame length of each frame of the workload (device lengths[count]). */
int nexg_gen_lengths(nexg_ctx* ctx, int workload, uint64_t seed,
                     uint64_t first_index, uint64_t count, uint32_t* lengths,
                     void* stream);
/* Writes frame i at data + offsets[i] (offsets NULL -> i*stride). */
int nexg_gen_frames(nexg_ctx* ctx, int workload, uint64_t seed,
                    uint64_t first_index, uint64_t count, uint8_t* data,
                    const uint64_t* offsets, uint32_t stride, void* stream);
/* SER parameter tuples: src_ip, dst_ip, src_port, dst_port, ip_id. */
int nexg_gen_udp4_params(nexg_ctx* ctx, uint64_t seed, uint64_t first_index,
                         uint64_t count, uint32_t* src_ip, uint32_t* dst_ip,
                         uint16_t* src_port, uint16_t* dst_port,
                         uint16_t* ip_id, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NEXG_H */
