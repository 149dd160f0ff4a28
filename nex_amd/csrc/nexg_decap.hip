// nexg_decap.hip — tunnel decapsulation on gfx950 (include/nexg.h): a second
// pass over a batch already parsed with NEXG_OUT_RECORD that locates each
// VXLAN / GRE tunnel's inner frame inside the outer batch
// (VxlanPacket::try_from_buf vxlan.rs:28-65, GrePacket::try_from_buf
// gre.rs:32-107 on Frame.payload), and the order-preserving compaction of the
// result by inner class. No frame byte is copied: the outputs are offset +
// length tables over the outer batch's data that nexg_parse_batch takes as
// they stand. Record fields, the header bytes as big-endian words and the
// compaction itself (count, scan, scatter) come from table_kernels.hpp: the
// select is its rule on a nexg_tunnel's first dword.
#include "table_kernels.hpp"

namespace nexg {

static_assert(sizeof(nexg_tunnel) == 16, "nexg_tunnel is 16 bytes (include/nexg.h)");
static_assert(sizeof(nexg_decap_option) == 8, "nexg_decap_option is 8 bytes (include/nexg.h)");

// k_decap: one lane per frame. Per lane 48 B of its record (the three 16-B
// quarters that hold flags / payload_off / payload_len, ip_proto, dst_port),
// up to 16 tunnel-header bytes as big-endian words (frame_be_words), and one 16-B + one 8-B + one 4-B non-temporal store; consecutive lanes write
// consecutive addresses. The candidate test and the GRE flag walk are integer
// selects: the reference's sequential "remaining < 4" checks (gre.rs:57-77)
// fail exactly when the payload is shorter than the closed-form header length.
__global__ __launch_bounds__(256) void k_decap(ParseArgs a, const nexg_record* recs, uint32_t which, uint32_t vxlan_port,
                                               nexg_tunnel* tunnels, uint64_t* inner_off, uint32_t* inner_len) {
    typedef uint32_t v2u __attribute__((ext_vector_type(2)));
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    if (idx >= a.count) return;
    const RecQuarter<0> q0 = rec_quarter<0>(recs + idx);
    const RecQuarter<1> q1 = rec_quarter<1>(recs + idx);
    const RecQuarter<2> q2 = rec_quarter<2>(recs + idx);
    uint64_t off;
    uint32_t len;
    const bool ext = frame_extent(a, idx, off, len);
    const uint32_t flags = rec_dw<kRecFlags>(q0), ip_proto = rec_proto(rec_dw<kRecProto>(q1)),
                   dst_port = rec_dport(rec_dw<kRecPorts>(q2));
    uint32_t poff, plen;
    rec_payload(rec_dw<kRecPayload>(q0), poff, plen);
    // the record is caller memory: clamp to the frame's own extent before any load
    const bool ok = ext && rec_status(flags) == 0u && poff + plen <= len;
    const bool vx = ok && (which & NEXG_DECAP_VXLAN) && (flags & NEXG_L_UDP) && dst_port == vxlan_port;
    const bool gre = ok && !vx && (which & NEXG_DECAP_GRE) && (flags & (NEXG_L_IPV4 | NEXG_L_IPV6)) &&
                     !(flags & (NEXG_L_TRANSPORT | NEXG_L_ICMP | NEXG_L_ICMPV6)) && ip_proto == 47u;
    // header bytes wanted: VXLAN its 8, GRE up to 16 of the payload (the flag
    // bits that size it are in the first dword: no second, dependent load)
    const uint32_t need = vx ? (plen >= 8u ? 8u : 0u) : gre ? (plen >= 4u ? (plen < 16u ? plen : 16u) : 0u) : 0u;
    uint32_t w[4];  // header bytes 4j..4j+3 as big-endian values
    frame_be_words(reinterpret_cast<uint64_t>(a.data) + off + poff, need != 0u, need, w);

    // VXLAN (vxlan.rs:34-50): flags u8, reserved1 u24, vni u24, reserved2 u8
    // GRE (gre.rs:38-77): flags u16, protocol_type u16, then checksum + offset
    // when C or R, key when K, sequence when S
    const uint32_t gflags = w[0] >> 16, gproto = w[0] & 0xFFFFu;
    const uint32_t cr = ((gflags >> 15) | (gflags >> 14)) & 1u, K = (gflags >> 13) & 1u, S = (gflags >> 12) & 1u;
    const uint32_t ghl = 4u + 4u * (cr + K + S);
    const bool gbad = gre && (plen < ghl || ((gflags >> 14) & 1u));  // plen < 4 included (need = 0 -> ghl = 4)
    const bool vbad = vx && plen < 8u;
    const bool acc = (vx && !vbad) || (gre && !gbad);
    const uint32_t kw = cr ? w[2] : w[1];                       // the word after the checksum + offset, if any
    const uint32_t sw = (cr + K) == 2u ? w[3] : (cr + K) == 1u ? w[2] : w[1];
    const uint32_t ginner = gproto == 0x6558u ? NEXG_INNER_ETHERNET : gproto == 0x0800u ? NEXG_INNER_IPV4
                            : gproto == 0x86DDu ? NEXG_INNER_IPV6 : NEXG_INNER_OTHER;
    const uint32_t kind = vx ? NEXG_TUN_VXLAN : gre ? NEXG_TUN_GRE : NEXG_TUN_NONE;
    const uint32_t hl = acc ? (vx ? 8u : ghl) : 0u;
    u32x4 t;
    t.x = kind | ((vbad || gbad) ? (uint32_t)NEXG_ERR_MALFORMED << 8 : 0u) |
          (acc ? (vx ? (uint32_t)NEXG_INNER_ETHERNET : ginner) << 16 : 0u) | (hl << 24);
    t.y = acc ? (vx ? (w[0] >> 24) : (gflags | (gproto << 16))) : 0u;
    t.z = acc ? (vx ? (w[1] >> 8) : (K ? kw : 0u)) : 0u;
    t.w = acc ? (vx ? (((w[0] & 0xFFFFFFu) << 8) | (w[1] & 0xFFu)) : (S ? sw : 0u)) : 0u;
    const uint64_t io = ext ? off + (acc ? poff + hl : 0u) : 0ull;
    __builtin_nontemporal_store(t, reinterpret_cast<u32x4*>(tunnels) + idx);
    __builtin_nontemporal_store(v2u{(uint32_t)io, (uint32_t)(io >> 32)}, reinterpret_cast<v2u*>(inner_off) + idx);
    __builtin_nontemporal_store(acc ? plen - hl : 0u, inner_len + idx);
}

hipError_t launch_decap(const ParseArgs& a, const nexg_record* recs, uint32_t which, uint32_t vxlan_port,
                        nexg_tunnel* tunnels, uint64_t* inner_off, uint32_t* inner_len, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    const uint64_t blocks = (a.count + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_decap, dim3((uint32_t)blocks), dim3(kTile), 0, s, a, recs, which, vxlan_port, tunnels,
                       inner_off, inner_len);
    return hipGetLastError();
}

// ---- nexg_decap_select: table_kernels.hpp's compaction with this selector ----

struct DecapPick {
    const nexg_tunnel* tunnels;
    const uint64_t* inner_off;
    const uint32_t* inner_len;
    uint64_t n;
    uint32_t inner_mask;
    struct Picked {};
    static constexpr bool kTagged = false;
    NEXG_HD uint64_t count() const { return n; }
    // first dword of a nexg_tunnel: kind | status << 8 | inner << 16 | hdr_len << 24
    __device__ __forceinline__ bool pick(uint64_t idx, Picked&) const {
        const uint32_t h = NEXG_GLOBAL(uint32_t, tunnels)[idx * 4u];
        const uint32_t inner = (h >> 16) & 0xFFu;
        return (h & 0xFFu) != 0u && (h & 0xFF00u) == 0u && inner < 32u && ((inner_mask >> inner) & 1u) != 0u;
    }
    __device__ __forceinline__ void entry(uint64_t idx, const Picked&, uint64_t& off, uint32_t& len) const {
        off = NEXG_GLOBAL(uint64_t, inner_off)[idx];
        len = NEXG_GLOBAL(uint32_t, inner_len)[idx];
    }
};

hipError_t launch_decap_select(const nexg_tunnel* tunnels, const uint64_t* inner_off, const uint32_t* inner_len,
                               uint64_t count, uint32_t inner_mask, uint32_t* out_index, uint64_t* out_off,
                               uint32_t* out_len, uint64_t* out_count, void* workspace, hipStream_t s) {
    return launch_compact(DecapPick{tunnels, inner_off, inner_len, count, inner_mask}, out_index, out_off, out_len,
                          nullptr, out_count, workspace, s);
}

}  // namespace nexg
