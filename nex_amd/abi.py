"""Python mirror of include/nexg.h: constants, ctypes structs, numpy dtypes.

Layouts here must match include/nexg.h byte for byte; tests/test_abi.py checks
the sizes against the C compiler's view.
"""
import ctypes

import numpy as np

ABI_VERSION = 1

# call status
OK, EINVAL, ENOMEM, EDEVICE, ELAUNCH, ERANGE, EPERM, EIO = 0, -1, -2, -3, -4, -5, -6, -7

# per-frame status: ParseError kind (nex-packet/src/parse.rs:51-97)
FRAME_OK = 0
ERR_BUFFER_TOO_SHORT = 1
ERR_INVALID_LENGTH = 2
ERR_MALFORMED = 3
ERR_TRUNCATED = 4
ERR_BAD_EXTENT = 7

PARSE_STRICT = 0x1
PARSE_FROM_IP = 0x2
PARSE_VLAN = 0x4  # extension: unwrap up to two 802.1Q/802.1ad/QinQ tags (not Frame semantics)

L_ETHERNET = 1 << 0
L_ARP = 1 << 1
L_IP = 1 << 2
L_IPV4 = 1 << 3
L_IPV6 = 1 << 4
L_ICMP = 1 << 5
L_ICMPV6 = 1 << 6
L_TRANSPORT = 1 << 7
L_TCP = 1 << 8
L_UDP = 1 << 9
C_IP_CHECKED = 1 << 10
C_IP_OK = 1 << 11
C_IP_PANIC = 1 << 12
C_L4_CHECKED = 1 << 13
C_L4_OK = 1 << 14
L_VLAN = 1 << 15
STATUS_SHIFT = 24
VERDICT_ERR = L_ARP | L_IP  # NEXG_VERDICT_ERR: never both in a parsed Frame

OUT_DESC = 1
OUT_RECORD = 2
OUT_SLICE = 3
OUT_FLAGS = 4  # nexg_desc.flags only (include/nexg.h)
OUT_VERDICT = 5  # lossless 2-B form of the flags word (include/nexg.h)
OUT_SPARSE = 6  # 1-B shape codes + per-64-frame exception slots (include/nexg.h)
OUT_GROUPED = 7  # SPARSE with uniform 64-frame groups as a head byte + 2 verdict masks
GROUPED_TILE_RUN = 0x80  # NEXG_GROUPED_TILE_RUN: a mixed group whose exceptions run per 256-frame tile

# NEXG_FRAMES_* hints (nexg_frames.hints)
FRAMES_MONOTONE = 0x1
FRAMES_OFFSETS32 = 0x2  # u32 offset table (+ 64-bit group bases over 4 GiB)


def offsets32_layout(count, with_bases):
    """(u32 entries, byte offset of the u64 group bases, base count, total
    bytes) of a NEXG_FRAMES_OFFSETS32 table for `count` frames whose table
    starts 8-B aligned (include/nexg.h nexg_offsets32_bytes)."""
    n = count + 1
    base_off = (4 * n + 7) // 8 * 8
    nb = (n + 255) // 256 if with_bases else 0
    return n, base_off, nb, (base_off + 8 * nb) if with_bases else 4 * n


def offsets32_table(offsets64, data_bytes):
    """numpy u64 offsets (count + 1 entries) -> the NEXG_FRAMES_OFFSETS32
    table as a uint8 array: offsets mod 2^32, then (data_bytes > 0xFFFFFFFF)
    the full offset of every 256th frame."""
    o = np.asarray(offsets64, dtype=np.uint64)
    count = len(o) - 1
    with_bases = data_bytes > 0xFFFFFFFF
    n, base_off, nb, total = offsets32_layout(count, with_bases)
    buf = np.zeros(total, np.uint8)
    buf[: 4 * n].view(np.uint32)[:] = (o & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    if with_bases:
        buf[base_off:].view(np.uint64)[:] = o[::256]
    return buf


def offsets32_decode(table, count, data_bytes):
    """The full u64 offsets (count + 1) of a NEXG_FRAMES_OFFSETS32 table
    (uint8 array), as the kernels read it."""
    t = np.asarray(table, np.uint8)
    with_bases = data_bytes > 0xFFFFFFFF
    n, base_off, nb, _ = offsets32_layout(count, with_bases)
    lo = t[: 4 * n].view(np.uint32).astype(np.uint64)
    if not with_bases:
        return lo
    b = t[base_off: base_off + 8 * nb].view(np.uint64)[np.arange(n) >> 8]
    return b + ((lo - (b & np.uint64(0xFFFFFFFF))) & np.uint64(0xFFFFFFFF))

# NEXG_OUT_SPARSE code byte
SPARSE_IP_OK = 0x10
SPARSE_L4_OK = 0x20
SPARSE_TAG_SHIFT = 6
SHAPE_EXCEPTION, SHAPE_IP_NONE = 0, 10
_V4 = L_ETHERNET | L_IP | L_IPV4 | C_IP_CHECKED
_V6 = L_ETHERNET | L_IP | L_IPV6
#: NEXG_SHAPE_FLAGS / NEXG_SHAPE_HDR (include/nexg.h), indexed by shape 0..15
SHAPE_FLAGS = np.array([
    0,
    _V4 | L_TRANSPORT | L_UDP | C_L4_CHECKED, _V4 | L_TRANSPORT | L_TCP | C_L4_CHECKED, _V4 | L_ICMP | C_L4_CHECKED,
    _V6 | L_TRANSPORT | L_UDP | C_L4_CHECKED, _V6 | L_TRANSPORT | L_TCP | C_L4_CHECKED, _V6 | L_ICMPV6 | C_L4_CHECKED,
    L_ETHERNET, _V4, _V6, L_ETHERNET | L_IP,
    1 << STATUS_SHIFT, 2 << STATUS_SHIFT, 3 << STATUS_SHIFT, 4 << STATUS_SHIFT, 7 << STATUS_SHIFT], np.uint32)
SHAPE_HDR = np.array([0, 28, 40, 24, 48, 60, 44, 0, 20, 40, 0, 0, 0, 0, 0, 0], np.int64)


def sparse_exc_offset(count):
    """NEXG_SPARSE_EXC_OFFSET: byte offset of the exception slots."""
    return (int(count) + 15) & ~15


def sparse_bytes(count):
    """NEXG_SPARSE_BYTES: size of a NEXG_OUT_SPARSE output."""
    return sparse_exc_offset(count) + 8 * int(count)


def grouped_offsets(count):
    """NEXG_GROUPED_{MASK,CODE,EXC}_OFFSET and NEXG_GROUPED_BYTES."""
    g = (int(count) + 63) >> 6
    mask = (g + 15) & ~15
    code = mask + 16 * g
    exc = (code + int(count) + 15) & ~15
    return mask, code, exc, exc + 8 * int(count)


def grouped_codes(buf, count):
    """Every frame's NEXG_OUT_SPARSE code from a NEXG_OUT_GROUPED output
    (nexg_grouped_code, vectorised)."""
    buf = np.asarray(buf, np.uint8)
    mask, code, _, _ = grouped_offsets(count)
    G = (count + 63) >> 6
    i = np.arange(count)
    g = i >> 6
    head = buf[:G].astype(np.int64)[g]
    m = buf[mask:mask + 16 * G].copy().view("<u8").reshape(-1, 2)
    b = (i & 63).astype(np.uint64)
    ip = (m[g, 0] >> b) & np.uint64(1)
    l4 = (m[g, 1] >> b) & np.uint64(1)
    uni = head | np.where(ip != 0, SPARSE_IP_OK, 0) | np.where(l4 != 0, SPARSE_L4_OK, 0)
    mixed = (head == 0) | (head == GROUPED_TILE_RUN)
    return np.where(mixed, buf[code:code + count].astype(np.int64), uni)


def grouped_to_desc(buf, count, lengths, parse_flags=0, ip_offset=0):
    """nexg_desc[count] from a NEXG_OUT_GROUPED output (uint8 host array)."""
    buf = np.asarray(buf, np.uint8)
    _, _, exc, _ = grouped_offsets(count)
    G = (count + 63) >> 6
    run = buf[:G][np.arange(count) >> 6] == GROUPED_TILE_RUN
    return codes_to_desc(grouped_codes(buf, count), buf[exc:exc + 8 * count].view(DESC_DTYPE), count, lengths,
                         parse_flags, ip_offset, tile_run=run)


def sparse_to_desc(buf, count, lengths, parse_flags=0, ip_offset=0):
    """nexg_desc[count] from a NEXG_OUT_SPARSE output (uint8 host array):
    nexg_sparse_decode per code, exceptions looked up per 64-frame group.
    `lengths` = every frame's length (int array)."""
    buf = np.asarray(buf, np.uint8)
    return codes_to_desc(buf[:count].astype(np.int64),
                         buf[sparse_exc_offset(count):sparse_exc_offset(count) + 8 * count].view(DESC_DTYPE),
                         count, lengths, parse_flags, ip_offset)


def codes_to_desc(codes, exc, count, lengths, parse_flags=0, ip_offset=0, tile_run=None):
    """nexg_sparse_decode over every code; code-0 frames take the k-th
    exception of their 64-frame group (exc = the exception slots), or of
    their 256-frame tile where `tile_run` (per frame) is set
    (NEXG_GROUPED_TILE_RUN groups)."""
    lengths = np.asarray(lengths, np.int64)[:count]
    shape, tags = codes & 0xF, (codes >> SPARSE_TAG_SHIFT) & 3
    out = np.zeros(count, DESC_DTYPE)
    fl = SHAPE_FLAGS[shape].astype(np.int64)
    pay = (shape >= 1) & (shape < SHAPE_IP_NONE)
    fl |= np.where(pay & ((codes & SPARSE_IP_OK) != 0), C_IP_OK, 0)
    fl |= np.where(pay & ((codes & SPARSE_L4_OK) != 0), C_L4_OK, 0)
    fl |= np.where((pay | (shape == SHAPE_IP_NONE)) & (tags > 0), L_VLAN, 0)
    base = ip_offset if parse_flags & PARSE_FROM_IP else 14
    h = base + 4 * tags + SHAPE_HDR[shape]
    plen = np.where(pay, lengths - h, 0)
    out["flags"] = fl.astype(np.uint32)
    out["payload_len"] = (plen & 0xFFFF).astype(np.uint16)
    out["payload_off"] = np.where(pay & (lengths > h), h, 0).astype(np.uint16)
    ex = np.nonzero(shape == SHAPE_EXCEPTION)[0]
    if len(ex):
        unit = np.full(len(ex), 64, np.int64) if tile_run is None else np.where(tile_run[ex], 256, 64)
        start = ex // unit * unit  # the first frame of the exception's group or tile
        first = np.searchsorted(ex, start)  # index in ex of that run's first exception
        rank = np.arange(len(ex)) - first
        out[ex] = exc[start + rank]
    return out

# FrameSlice presence bits (nexg_slice.flags)
S_DATALINK = 1 << 0
S_NETWORK = 1 << 1
S_TRANSPORT = 1 << 2
S_ETHERTYPE = 1 << 3
S_IP_PROTOCOL = 1 << 4
S_PROTO_SHIFT = 8

WL_UDP64 = 1
WL_IMIX = 2

#: seed of the synthetic workloads ("nex")
DEFAULT_SEED = 0x6E6578


#: NEXG_CTX_* -> the reference's ParseError context string (include/nexg.h)
ERR_CONTEXTS = (None, "Ethernet packet", "Frame dummy Ethernet classification", "IPv4 packet",
                "IPv4 packet version", "IPv4 header length", "IPv4 header", "IPv4 total length",
                "IPv4 options", "IPv4 option length", "IPv6 packet", "IPv6 packet version", "IPv6 payload",
                "IPv6 extension header", "IPv6 routing header", "IPv6 fragment header")


def status_of(flags):
    return (np.asarray(flags) >> STATUS_SHIFT) & 0x7


DESC_DTYPE = np.dtype([("flags", "<u4"), ("payload_off", "<u2"), ("payload_len", "<u2")])
assert DESC_DTYPE.itemsize == 8

SLICE_DTYPE = np.dtype([("flags", "<u4"), ("l3_off", "<u2"), ("l3_len", "<u2"), ("l4_len", "<u2"),
                        ("payload_off", "<u2"), ("payload_len", "<u2"), ("ethertype", "<u2")])
assert SLICE_DTYPE.itemsize == 16
FLAGS_DTYPE = np.dtype([("flags", "<u4")])
VERDICT_DTYPE = np.dtype([("verdict", "<u2")])


def verdict_to_flags(v):
    """NEXG_VERDICT_FLAGS (include/nexg.h): the flags words of 2-B verdicts."""
    v = np.asarray(v).astype(np.uint32)
    err = (v & VERDICT_ERR) == VERDICT_ERR
    return np.where(err, ((v >> 3) & 7) << STATUS_SHIFT, v).astype(np.uint32)
OPTIONS_DTYPE = np.dtype([("n_ip", "u1"), ("n_tcp", "u1"), ("ip_opt_off", "<u2"), ("tcp_opt_off", "<u2"),
                          ("reserved", "<u2"), ("ip_pos", "u1", 40), ("tcp_pos", "u1", 40), ("pad", "u1", 8)])
assert OPTIONS_DTYPE.itemsize == 96

RECORD_DTYPE = np.dtype([
    ("flags", "<u4"), ("payload_off", "<u2"), ("payload_len", "<u2"),
    ("packet_len", "<u2"), ("ethertype", "<u2"), ("l3_off", "<u2"), ("l4_off", "<u2"),
    ("ip_ver_ihl", "u1"), ("ip_tos", "u1"), ("ip_length", "<u2"),
    ("ip_word", "<u4"),
    ("ip_ttl", "u1"), ("ip_proto", "u1"), ("ip_nopt", "u1"), ("l4_nopt", "u1"),
    ("ip_src", "<u4"), ("ip_dst", "<u4"),
    ("ip_csum", "<u2"), ("ip_csum_calc", "<u2"), ("l4_csum", "<u2"), ("l4_csum_calc", "<u2"),
    ("src_port", "<u2"), ("dst_port", "<u2"), ("l4_length", "<u2"),
    ("l4_type", "u1"), ("l4_code", "u1"),
    ("tcp_seq", "<u4"), ("tcp_ack", "<u4"), ("tcp_window", "<u2"), ("tcp_urg", "<u2"),
])
assert RECORD_DTYPE.itemsize == 64


class Frames(ctypes.Structure):
    """struct nexg_frames"""
    _fields_ = [
        ("data", ctypes.c_void_p),
        ("data_bytes", ctypes.c_uint64),
        ("offsets", ctypes.c_void_p),
        ("lengths", ctypes.c_void_p),
        ("stride", ctypes.c_uint32),
        ("hints", ctypes.c_uint32),
        ("count", ctypes.c_uint64),
    ]


class ParseOptionC(ctypes.Structure):
    """struct nexg_parse_option"""
    _fields_ = [("flags", ctypes.c_uint32), ("ip_offset", ctypes.c_uint32)]


class Udp4Build(ctypes.Structure):
    """struct nexg_udp4_build"""
    _fields_ = [
        ("src_ip", ctypes.c_void_p),
        ("dst_ip", ctypes.c_void_p),
        ("src_port", ctypes.c_void_p),
        ("dst_port", ctypes.c_void_p),
        ("ip_id", ctypes.c_void_p),
        ("src_mac", ctypes.c_void_p),
        ("dst_mac", ctypes.c_void_p),
        ("payload", ctypes.c_void_p),
        ("payload_len", ctypes.c_uint32),
        ("def_src_port", ctypes.c_uint16),
        ("def_dst_port", ctypes.c_uint16),
        ("def_ip_id", ctypes.c_uint16),
        ("def_src_mac", ctypes.c_uint8 * 6),
        ("def_dst_mac", ctypes.c_uint8 * 6),
        ("ttl", ctypes.c_uint8),
        ("ip_flags", ctypes.c_uint8),
        ("dscp_ecn", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8),
        ("def_src_ip", ctypes.c_uint32),
        ("count", ctypes.c_uint64),
    ]


#: struct nexg_udp4_tuple (16 B): the AoS per-frame tuple of nexg_build_udp4_tuples
UDP4_TUPLE_DTYPE = np.dtype([("src_ip", "<u4"), ("dst_ip", "<u4"), ("src_port", "<u2"), ("dst_port", "<u2"),
                             ("ip_id", "<u2"), ("reserved", "<u2")])


class Udp6Build(ctypes.Structure):
    """struct nexg_udp6_build"""
    _fields_ = [
        ("src_ip", ctypes.c_void_p),
        ("dst_ip", ctypes.c_void_p),
        ("src_port", ctypes.c_void_p),
        ("dst_port", ctypes.c_void_p),
        ("src_mac", ctypes.c_void_p),
        ("dst_mac", ctypes.c_void_p),
        ("payload", ctypes.c_void_p),
        ("payload_len", ctypes.c_uint32),
        ("flow_label", ctypes.c_uint32),
        ("def_src_port", ctypes.c_uint16),
        ("def_dst_port", ctypes.c_uint16),
        ("def_src_mac", ctypes.c_uint8 * 6),
        ("def_dst_mac", ctypes.c_uint8 * 6),
        ("hop_limit", ctypes.c_uint8),
        ("traffic_class", ctypes.c_uint8),
        ("src_shared", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8),
        ("count", ctypes.c_uint64),
    ]


class IpBuild(ctypes.Structure):
    """struct nexg_ip_build"""
    _fields_ = [
        ("src_ip", ctypes.c_void_p), ("dst_ip", ctypes.c_void_p), ("ip_id", ctypes.c_void_p),
        ("src_mac", ctypes.c_void_p), ("dst_mac", ctypes.c_void_p),
        ("family", ctypes.c_uint32), ("flow_label", ctypes.c_uint32), ("def_ip_id", ctypes.c_uint16),
        ("def_src_mac", ctypes.c_uint8 * 6), ("def_dst_mac", ctypes.c_uint8 * 6),
        ("ttl", ctypes.c_uint8), ("ip_flags", ctypes.c_uint8), ("tos", ctypes.c_uint8),
        ("src_shared", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 2),
    ]


class TcpBuild(ctypes.Structure):
    """struct nexg_tcp_build"""
    _fields_ = [
        ("ip", IpBuild),
        ("src_port", ctypes.c_void_p), ("dst_port", ctypes.c_void_p), ("seq", ctypes.c_void_p),
        ("ack", ctypes.c_void_p), ("payload", ctypes.c_void_p), ("payload_len", ctypes.c_uint32),
        ("def_seq", ctypes.c_uint32), ("def_ack", ctypes.c_uint32),
        ("def_src_port", ctypes.c_uint16), ("def_dst_port", ctypes.c_uint16),
        ("window", ctypes.c_uint16), ("urgent_ptr", ctypes.c_uint16),
        ("flags", ctypes.c_uint8), ("options_len", ctypes.c_uint8), ("options", ctypes.c_uint8 * 40),
        ("reserved", ctypes.c_uint8 * 2), ("count", ctypes.c_uint64),
    ]


class IcmpEchoBuild(ctypes.Structure):
    """struct nexg_icmp_echo_build"""
    _fields_ = [
        ("ip", IpBuild),
        ("identifier", ctypes.c_void_p), ("sequence", ctypes.c_void_p), ("payload", ctypes.c_void_p),
        ("payload_len", ctypes.c_uint32), ("def_identifier", ctypes.c_uint16),
        ("def_sequence", ctypes.c_uint16), ("icmp_type", ctypes.c_uint8), ("icmp_code", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 2), ("count", ctypes.c_uint64),
    ]


class ArpBuild(ctypes.Structure):
    """struct nexg_arp_build"""
    _fields_ = [
        ("sender_ip", ctypes.c_void_p), ("target_ip", ctypes.c_void_p), ("sender_mac", ctypes.c_void_p),
        ("target_mac", ctypes.c_void_p), ("eth_dst", ctypes.c_void_p),
        ("def_sender_ip", ctypes.c_uint8 * 4), ("def_sender_mac", ctypes.c_uint8 * 6),
        ("def_target_mac", ctypes.c_uint8 * 6), ("def_eth_dst", ctypes.c_uint8 * 6),
        ("hardware_type", ctypes.c_uint16), ("protocol_type", ctypes.c_uint16), ("operation", ctypes.c_uint16),
        ("hw_addr_len", ctypes.c_uint8), ("proto_addr_len", ctypes.c_uint8), ("count", ctypes.c_uint64),
    ]


class NdpNsBuild(ctypes.Structure):
    """struct nexg_ndp_ns_build"""
    _fields_ = [("ip", IpBuild), ("eth_dst_multicast", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("count", ctypes.c_uint64)]


# in-place checksum fix-up (nexg_recompute_checksums_batch)
FIX_IP = 0x1
FIX_L4 = 0x2
FIXUP_DTYPE = np.dtype([("done", "u1"), ("proto", "u1"), ("ip_csum", "<u2"), ("l4_csum", "<u2"),
                        ("l4_off", "<u2")])
assert FIXUP_DTYPE.itemsize == 8

# tunnel decapsulation (nexg_decap_batch / nexg_decap_select)
TUN_NONE, TUN_VXLAN, TUN_GRE = 0, 1, 2
INNER_OTHER, INNER_ETHERNET, INNER_IPV4, INNER_IPV6 = 0, 1, 2, 3
DECAP_VXLAN = 0x1
DECAP_GRE = 0x2
VXLAN_PORT = 4789  # what nexg_decap_option.vxlan_port = 0 means
TUNNEL_DTYPE = np.dtype([("kind", "u1"), ("status", "u1"), ("inner", "u1"), ("hdr_len", "u1"), ("flags", "<u2"),
                         ("proto", "<u2"), ("id", "<u4"), ("aux", "<u4")])
assert TUNNEL_DTYPE.itemsize == 16


class DecapOption(ctypes.Structure):
    """struct nexg_decap_option"""
    _fields_ = [("which", ctypes.c_uint32), ("vxlan_port", ctypes.c_uint16), ("reserved", ctypes.c_uint16)]


def decap_select_workspace(count):
    """nexg_decap_select_workspace: bytes of nexg_decap_select's workspace."""
    return select_workspace(count)


# tunnel encapsulation (nexg_encap_plan / nexg_encap_frames; an extension: the
# reference builds one packet at a time)
ENCAP_VXLAN, ENCAP_GRE = 1, 2
ENCAP_UDP_CSUM, ENCAP_FLOW_PORT, ENCAP_GRE_KEY, ENCAP_GRE_SEQ, ENCAP_GRE_L3 = 0x01, 0x02, 0x04, 0x08, 0x10
ENCAP_VXLAN_FLAGS = ENCAP_UDP_CSUM | ENCAP_FLOW_PORT
ENCAP_GRE_FLAGS = ENCAP_GRE_KEY | ENCAP_GRE_SEQ | ENCAP_GRE_L3
ENCAP_MAX_TUNNELS = 16
TUNNEL_NONE = 0xFF
ENCAPPED_DTYPE = np.dtype([("status", "u1"), ("tunnel", "u1"), ("hdr_len", "u1"), ("reserved", "u1"),
                           ("src_port", "<u2"), ("l4_csum", "<u2")])
assert ENCAPPED_DTYPE.itemsize == 8


class TunnelSpecC(ctypes.Structure):
    """struct nexg_tunnel_spec"""
    _fields_ = [("kind", ctypes.c_uint8), ("family", ctypes.c_uint8), ("ttl", ctypes.c_uint8), ("tos", ctypes.c_uint8),
                ("flags", ctypes.c_uint32), ("eth_dst", ctypes.c_uint8 * 6), ("eth_src", ctypes.c_uint8 * 6),
                ("src", ctypes.c_uint8 * 16), ("dst", ctypes.c_uint8 * 16), ("src_port", ctypes.c_uint16),
                ("dst_port", ctypes.c_uint16), ("port_span", ctypes.c_uint16), ("ip_id", ctypes.c_uint16),
                ("id", ctypes.c_uint32), ("seq_base", ctypes.c_uint32), ("flow_label", ctypes.c_uint32),
                ("ip_flags", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 23)]


class TunnelsC(ctypes.Structure):
    """struct nexg_tunnels"""
    _fields_ = [("n_tunnels", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("tunnels", TunnelSpecC * ENCAP_MAX_TUNNELS)]


assert ctypes.sizeof(TunnelSpecC) == 96 and ctypes.sizeof(TunnelsC) == 8 + 16 * 96


def encap_plan_workspace(count):
    """nexg_encap_plan_workspace: bytes of nexg_encap_plan's workspace (the gather plan's)."""
    return gather_plan_workspace(count)


# IPv4 fragmentation to an MTU (nexg_fragment_plan / nexg_fragment_frames; an
# extension: the reference has the fields, not the procedure)
FRAG_NONE, FRAG_PASS, FRAG_SPLIT, FRAG_TOO_BIG = 0, 1, 2, 3
FRAG_IGNORE_DF = 0x1
FRAG_MTU_MIN, FRAG_MTU_MAX = 68, 65535
FRAGGED_DTYPE = np.dtype([("status", "u1"), ("kind", "u1"), ("hdr_len", "u1"), ("reserved", "u1"), ("pieces", "<u2"),
                          ("piece_data", "<u2"), ("first", "<u4"), ("reserved2", "<u4")])
assert FRAGGED_DTYPE.itemsize == 16


class FragOptionC(ctypes.Structure):
    """struct nexg_frag_option"""
    _fields_ = [("mtu", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("align", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


def fragment_plan_workspace(count):
    """nexg_fragment_plan_workspace: bytes of nexg_fragment_plan's workspace."""
    tiles = (int(count) + 255) // 256
    return 16 * ((tiles + 255) // 256 * 256) + 16


FRAG_TOTAL_OVERFLOW = 0xFFFFFFFF  # out_first[count] of nexg_fragment_plan: 2^32 - 1 output frames or more


# DNS messages (nexg_dns_batch / nexg_dns_entries)
DNS_ANY_UDP = 0x1
DNS_PORT = 53  # what nexg_dns_option.port = 0 means
DNS_CANDIDATE = 0x1    # nexg_dns.flags8
DNS_SECTION_SHORT = 0x2
DNS_DATA_CUT = 0x1     # nexg_dns_entry.flags8
DNS_QUERY, DNS_ANSWER, DNS_AUTHORITY, DNS_ADDITIONAL = 0, 1, 2, 3  # nexg_dns_entry.section
DNS_DTYPE = np.dtype([("status", "u1"), ("flags8", "u1"), ("msg_off", "<u2"), ("msg_len", "<u2"), ("id", "<u2"),
                      ("flags", "<u2"), ("qd", "<u2"), ("an", "<u2"), ("ns", "<u2"), ("ar", "<u2"), ("n_q", "<u2"),
                      ("n_an", "<u2"), ("n_ns", "<u2"), ("n_ar", "<u2"), ("rest_off", "<u2"), ("first", "<u4")])
assert DNS_DTYPE.itemsize == 32
DNS_ENTRY_DTYPE = np.dtype([("section", "u1"), ("flags8", "u1"), ("off", "<u2"), ("type", "<u2"),
                            ("dns_class", "<u2"), ("ttl", "<u4"), ("name", "<u2"), ("data_len", "<u2")])
assert DNS_ENTRY_DTYPE.itemsize == 16


class DnsOption(ctypes.Structure):
    """struct nexg_dns_option"""
    _fields_ = [("flags", ctypes.c_uint32), ("port", ctypes.c_uint16), ("reserved", ctypes.c_uint16)]


def dns_tile_first_bytes(count):
    """nexg_dns_tile_first_bytes: bytes of nexg_dns_batch's tile_first."""
    return 8 * ((int(count) + 255) // 256 + 1)

# frame selection by rule and gather (nexg_select_batch / nexg_gather_*; an
# extension: the reference has no filter)
RULE_PROTO, RULE_SRC_PORT, RULE_DST_PORT, RULE_ANY_PORT = 0x1, 0x2, 0x4, 0x8
RULE_SRC_ADDR, RULE_DST_ADDR, RULE_ANY_ADDR = 0x10, 0x20, 0x40
RULE_TCP_FLAGS, RULE_LENGTH = 0x80, 0x100
RULE_ALL = 0x1FF
FILTER_INVERT = 0x1
FILTER_MAX_RULES = 16
RULE_NONE = 0xFF  # out_rule under FILTER_INVERT
GATHER_ALIGNS = (1, 4, 8, 16)
GATHER_ROW_BYTES = (4, 8, 16, 32, 64)


class RuleC(ctypes.Structure):
    """struct nexg_rule"""
    _fields_ = [("flags_mask", ctypes.c_uint32), ("flags_value", ctypes.c_uint32), ("tests", ctypes.c_uint32),
                ("ip_proto", ctypes.c_uint8), ("tcp_mask", ctypes.c_uint8), ("tcp_value", ctypes.c_uint8),
                ("family", ctypes.c_uint8), ("src_bits", ctypes.c_uint8), ("dst_bits", ctypes.c_uint8),
                ("reserved", ctypes.c_uint16), ("sport_lo", ctypes.c_uint16), ("sport_hi", ctypes.c_uint16),
                ("dport_lo", ctypes.c_uint16), ("dport_hi", ctypes.c_uint16), ("len_lo", ctypes.c_uint16),
                ("len_hi", ctypes.c_uint16), ("src", ctypes.c_uint8 * 16), ("dst", ctypes.c_uint8 * 16)]


class FilterC(ctypes.Structure):
    """struct nexg_filter"""
    _fields_ = [("n_rules", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("rules", RuleC * FILTER_MAX_RULES)]


assert ctypes.sizeof(RuleC) == 64 and ctypes.sizeof(FilterC) == 1032


def select_workspace(count):
    """nexg_select_workspace: bytes of nexg_select_batch's workspace."""
    tiles = (int(count) + 255) // 256
    return 4 * ((tiles + 255) // 256 * 256) + 16


def gather_plan_workspace(count):
    """nexg_gather_plan_workspace: bytes of nexg_gather_plan's workspace."""
    tiles = (int(count) + 255) // 256
    return 8 * ((tiles + 255) // 256 * 256) + 16


# fixed-string match on frame bytes (nexg_match_batch / nexg_match_select; an
# extension: the reference has no payload search)
MATCH_MAX_PATTERNS = 32
MATCH_MAX_LEN = 16
PAT_NOCASE = 0x1
MATCH_FRAME = 0x1
PAT_NONE = 0xFF  # first_pat of a row whose mask is 0
MATCH_DTYPE = np.dtype([("mask", "<u4"), ("first_off", "<u2"), ("first_pat", "u1"), ("reserved", "u1")])
assert MATCH_DTYPE.itemsize == 8


class PatternC(ctypes.Structure):
    """struct nexg_pattern"""
    _fields_ = [("bytes", ctypes.c_uint8 * 16), ("len", ctypes.c_uint8), ("flags", ctypes.c_uint8),
                ("off_lo", ctypes.c_uint16), ("off_hi", ctypes.c_uint16), ("reserved", ctypes.c_uint8 * 10)]


class PatternsC(ctypes.Structure):
    """struct nexg_patterns"""
    _fields_ = [("n_patterns", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("pat", PatternC * MATCH_MAX_PATTERNS)]


assert ctypes.sizeof(PatternC) == 32 and ctypes.sizeof(PatternsC) == 1032


def match_select_workspace(count):
    """nexg_match_select_workspace: bytes of nexg_match_select's workspace."""
    return select_workspace(count)


# header rewrite (nexg_rewrite_batch: the mutable setters under ChecksumMode::Automatic)
SET_ETH_DST, SET_ETH_SRC, SET_IP_SRC, SET_IP_DST = 0x001, 0x002, 0x004, 0x008
SET_SRC_PORT, SET_DST_PORT, SET_TTL, DEC_TTL, SET_TOS = 0x010, 0x020, 0x040, 0x080, 0x100
SET_ALL = 0x1FF
REWRITE_INCREMENTAL = 0x1
REWRITE_MAX_ACTIONS = 16
ACTION_NONE = 0xFF
REWRITTEN_DTYPE = np.dtype([("applied", "<u2"), ("fixed", "u1"), ("action", "u1"), ("ip_csum", "<u2"),
                            ("l4_csum", "<u2")])
assert REWRITTEN_DTYPE.itemsize == 8


class ActionC(ctypes.Structure):
    """struct nexg_action"""
    _fields_ = [("sets", ctypes.c_uint32), ("family", ctypes.c_uint8), ("ttl", ctypes.c_uint8),
                ("tos", ctypes.c_uint8), ("tos_mask", ctypes.c_uint8), ("src_port", ctypes.c_uint16),
                ("dst_port", ctypes.c_uint16), ("eth_dst", ctypes.c_uint8 * 6), ("eth_src", ctypes.c_uint8 * 6),
                ("src", ctypes.c_uint8 * 16), ("dst", ctypes.c_uint8 * 16), ("reserved", ctypes.c_uint8 * 8)]


class ActionsC(ctypes.Structure):
    """struct nexg_actions"""
    _fields_ = [("n_actions", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("actions", ActionC * REWRITE_MAX_ACTIONS)]


assert ctypes.sizeof(ActionC) == 64 and ctypes.sizeof(ActionsC) == 1032


# flow keys, RSS hash and flow-affine partition (nexg_flow_batch /
# nexg_flow_partition; an extension: the reference has no flow notion)
FLOW_SYMMETRIC, FLOW_NO_PORTS, FLOW_KEY = 0x1, 0x2, 0x4
FLOW_ALL = 0x7
FLOW_NONE, FLOW_IPV4, FLOW_IPV4_L4, FLOW_IPV6, FLOW_IPV6_L4 = 0, 1, 2, 3, 4
FLOW_TILE = 1024  # NEXG_FLOW_TILE: frames per partition tile
FLOW_MAX_BUCKETS = 256
FLOW_DTYPE = np.dtype([("hash", "<u4"), ("kind", "u1"), ("proto", "u1"), ("swapped", "u1"), ("reserved", "u1")])
assert FLOW_DTYPE.itemsize == 8


class FlowOptionC(ctypes.Structure):
    """struct nexg_flow_option"""
    _fields_ = [("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("key", ctypes.c_uint8 * 40)]


assert ctypes.sizeof(FlowOptionC) == 48


def flow_partition_workspace(count, buckets):
    """nexg_flow_partition_workspace: bytes of nexg_flow_partition's workspace."""
    counters = (int(count) + FLOW_TILE - 1) // FLOW_TILE * int(buckets)
    chunks = (counters + 1023) // 1024
    return 8 + 4 * ((chunks + 1) & ~1) + 4 * counters


# per-flow counters (nexg_flow_sort / nexg_flow_groups)
FLOW_GROUP_MIXED = 0x1  # nexg_flow_group.flags8 bit 0: mixed != 0
FLOW_GROUP_DTYPE = np.dtype([("hash", "<u4"), ("kind", "u1"), ("proto", "u1"), ("flags8", "u1"), ("reserved", "u1"),
                             ("first", "<u4"), ("packets", "<u4"), ("bytes", "<u8"), ("mixed", "<u4"),
                             ("first_index", "<u4")])
assert FLOW_GROUP_DTYPE.itemsize == 32


def flow_sort_workspace(count):
    """nexg_flow_sort_workspace: bytes of nexg_flow_sort's workspace."""
    return flow_partition_workspace(count, 256) + 16 * int(count)


def flow_groups_workspace(count):
    """nexg_flow_groups_workspace: bytes of nexg_flow_groups' workspace."""
    count = int(count)
    tiles = (count + 255) // 256
    return 16 + 8 * tiles + 8 * count + 8 * ((tiles + 1) & ~1) + 4 * ((count + 1) & ~1)


# the flow table across batches (nexg_flow_table_merge)
FLOW_ENTRY_MIXED = 0x1  # nexg_flow_entry.flags8 bit 0: more than one key seen under the hash
FLOW_ENTRY_DTYPE = np.dtype([("hash", "<u4"), ("kind", "u1"), ("proto", "u1"), ("flags8", "u1"), ("reserved", "u1"),
                             ("key", "u1", (36,)), ("last_epoch", "<u4"), ("packets", "<u8"), ("bytes", "<u8")])
assert FLOW_ENTRY_DTYPE.itemsize == 64


def flow_table_workspace(n_in, n_groups):
    """nexg_flow_table_workspace: bytes of nexg_flow_table_merge's workspace."""
    n = int(n_in) + int(n_groups)
    tiles = (n + 255) // 256
    return 8 * n + 4 * ((tiles + 1) & ~1)


# IPv4 reassembly (nexg_reasm_plan / nexg_reasm_frames / nexg_reasm_held; an
# extension: the reference has no reassembly)
REASM_NONE, REASM_PASS, REASM_HEAD, REASM_PART, REASM_HELD = 0, 1, 2, 3, 4
REASM_COLLISION = 0x1
REASM_NO_INDEX = 0xFFFFFFFF  # nexg_reasm.out / .head of a frame that has none
REASM_DTYPE = np.dtype([("status", "u1"), ("kind", "u1"), ("hdr_len", "u1"), ("flags", "u1"), ("members", "<u2"),
                        ("data_len", "<u2"), ("out", "<u4"), ("head", "<u4")])
assert REASM_DTYPE.itemsize == 16


def reasm_plan_workspace(count):
    """nexg_reasm_plan_workspace: bytes of nexg_reasm_plan's workspace."""
    count = int(count)
    tiles = (count + 255) // 256
    even, even_tiles = (count + 1) & ~1, (tiles + 1) & ~1
    sort = (flow_sort_workspace(count) + 15) & ~15
    return sort + 56 * count + 24 * tiles + 32 + 12 * even + 4 * even_tiles


def reasm_held_workspace(count):
    """nexg_reasm_held_workspace: bytes of nexg_reasm_held's workspace."""
    return select_workspace(count)


#: static inline helpers of include/nexg.h (header-only, not exported)
HEADER_INLINE = ("nexg_sparse_decode", "nexg_grouped_code", "nexg_grouped_exc_slot", "nexg_offsets32_bases",
                 "nexg_offsets32_bytes", "nexg_decap_select_workspace", "nexg_dns_tile_first_bytes",
                 "nexg_select_workspace", "nexg_match_select_workspace", "nexg_gather_plan_workspace", "nexg_encap_plan_workspace",
                 "nexg_fragment_plan_workspace", "nexg_flow_partition_workspace",
                 "nexg_flow_sort_workspace", "nexg_flow_groups_workspace", "nexg_flow_table_workspace",
                 "nexg_reasm_plan_workspace", "nexg_reasm_held_workspace")

#: every symbol include/nexg.h declares (tests check the .so exports them)
EXPORTED_SYMBOLS = (
    "nexg_abi_version", "nexg_strerror", "nexg_ctx_create", "nexg_ctx_destroy",
    "nexg_ctx_last_error", "nexg_ctx_cu_count", "nexg_parse_batch", "nexg_checksum_batch", "nexg_decode_options", "nexg_probe_stream",
    "nexg_decap_batch", "nexg_decap_select", "nexg_dns_batch", "nexg_dns_entries",
    "nexg_filter_check", "nexg_select_batch", "nexg_gather_plan", "nexg_gather_frames", "nexg_gather_rows",
    "nexg_patterns_check", "nexg_match_batch", "nexg_match_select",
    "nexg_actions_check", "nexg_rewrite_batch",
    "nexg_tunnels_check", "nexg_encap_plan", "nexg_encap_frames",
    "nexg_frag_option_check", "nexg_fragment_plan", "nexg_fragment_frames",
    "nexg_flow_batch", "nexg_flow_partition", "nexg_flow_sort", "nexg_flow_groups",
    "nexg_flow_table_merge",
    "nexg_reasm_plan", "nexg_reasm_frames", "nexg_reasm_held",
    "nexg_probe_span_clock", "nexg_probe_latency",
    "nexg_sparse_expand", "nexg_grouped_expand", "nexg_recompute_checksums_batch",
    "nexg_rx_config_default", "nexg_rx_open", "nexg_rx_next_batch", "nexg_rx_stats", "nexg_rx_close",
    "nexg_tpacket3_walk", "nexg_tx_open", "nexg_tx_send_batch", "nexg_tx_close",
    "nexg_build_udp4_batch", "nexg_build_udp4_tuples", "nexg_build_udp6_batch", "nexg_build_tcp_batch",
    "nexg_build_icmp_echo_batch", "nexg_build_arp_batch", "nexg_build_ndp_ns_batch", "nexg_pcap_open", "nexg_pcap_linktype", "nexg_pcap_last_error",
    "nexg_pcap_read_batch", "nexg_pcap_read_raw", "nexg_pcap_map", "nexg_pcap_walk_mapped", "nexg_pcap_set_read_threads", "nexg_pcap_close", "nexg_gen_lengths", "nexg_gen_frames", "nexg_gen_udp4_params",
)
