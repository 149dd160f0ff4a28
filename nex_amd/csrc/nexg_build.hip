// nexg_build.hip — serialize path: the builders with one lane per frame
// (udp4, udp6, tcp / icmp echo, arp, ndp) and their launchers. The pieces they
// share are in build_core.hpp; probe batches built from a template are in
// nexg_build_probe.hip.
//
// k_build_udp4: the examples/udp_ping.rs:68-109 composition
//   UdpPacketBuilder::build (builder/udp.rs:67-95: length = 8 + payload,
//   checksum via udp::checksum over to_bytes with skipword 3, computed 0 kept)
//   -> Ipv4PacketBuilder::to_bytes (builder/ipv4.rs:94-170: IHL 5, total
//   length, ipv4::checksum) -> EthernetPacketBuilder::to_bytes
//   (builder/ethernet.rs:68, ethernet.rs:211-216)
// on one lane per tuple. Frames are assembled in LDS and leave the CU as
// coalesced 16-B stores of the tile's contiguous output range.
#include <stdlib.h>

#include "build_core.hpp"

namespace nexg {

struct BuildArgs {
    nexg_udp4_build p;
    uint8_t* out;
    uint32_t out_stride;
    const nexg_udp4_tuple* tuples;  // AOS builds: one 16-B tuple per frame
    uint32_t tile_order;            // tile_index order (nexg_internal.hpp)
};

// Dynamic LDS beside k_build_udp4<64>'s 16-KiB static tile so that 5
// workgroups fit a CU's 160 KiB instead of 8 (at most 32 KiB each): fewer
// concurrent write streams per CU. 16M udp_ping frames in contiguous eighths
// (profiles/r04/occupancy/builder_occupancy_ab.log): probe batch 0.887-0.891
// of 8 TB/s written against 0.743 at 8 per CU, full tuples 0.717-0.719 against
// 0.681; 4 per CU the same, 6 and 7 in between. NEXG_BUILD_LDS_PAD overrides
// (measurement).
constexpr uint32_t kBuildCapPad = 160u * 1024u / 5u - (kBuildTile * 64u + 16u) - 256u;
uint32_t build_lds_pad() {
    static const uint32_t pad = [] {
#ifdef NEXG_AB_KNOBS
        const char* e = getenv("NEXG_BUILD_LDS_PAD");
#else
        const char* e = nullptr;  // product build: no environment overrides
#endif
        if (!e) return kBuildCapPad;
        const long v = atol(e);  // clamped: a negative or oversized pad fails every build launch
        return v <= 0 ? 0u : v >= (long)kBuildCapPad ? kBuildCapPad : (uint32_t)v;
    }();
    return pad;
}

// MAXS = largest stride the LDS tile holds (0: direct global writes).
// FULL: per-tuple address, port and id arrays present, MACs from the defaults —
// every parameter load is unconditional, so a lane issues all five before its
// first wait (the general form waits once per optional array).
// PROBE: the udp_ping probe batch (udp_ping.rs:30-31, 68-109 per target): only
// dst_ip is per frame; source address, ports, id and MACs are the batch's.
// AOS: the per-frame tuple as one 16-B record (nexg_udp4_tuple), read with one
// plain dwordx4 load per lane instead of five SoA loads (a non-temporal load
// measured slower).
template <uint32_t MAXS, bool FULL = false, bool PROBE = false, bool AOS = false>
__global__ __launch_bounds__(256) void k_build_udp4(BuildArgs a) {
    constexpr bool STAGED = MAXS != 0;
    __shared__ __attribute__((aligned(16))) uint8_t smem[STAGED ? kBuildTile * MAXS : 16];
    const nexg_udp4_build& p = a.p;
    const BuildTile<kBuildTile> t(a.tile_order);
    const uint32_t nf = t.frames(p.count);
    const uint32_t tid = threadIdx.x;
    const uint64_t i = t.lane();
    const uint32_t flen = 42u + p.payload_len;
    __shared__ uint32_t s_pay;
    // (the ICMP/TCP builder's wave-0 small-payload path measured slower here:
    // 1-5 B payloads 0.43-0.47 of 8 TB/s against 0.52-0.55 in one session,
    // profiles/r05/payload/: udp_ping's lean per-lane work does not hide it)
    const uint64_t pw = shared_payload_sum(p.payload, p.payload_len, &s_pay);
    if (tid < nf) {
        const u32x4 tv = AOS ? reinterpret_cast<const u32x4*>(a.tuples)[i] : u32x4{0, 0, 0, 0};
        const uint32_t dst = AOS ? tv.y : p.dst_ip[i];
        const uint32_t src = AOS ? tv.x : FULL ? p.src_ip[i] : PROBE ? p.def_src_ip : (p.src_ip ? p.src_ip[i] : p.def_src_ip);
        const uint32_t sp = AOS ? tv.z & 0xFFFFu : FULL ? p.src_port[i] : PROBE ? p.def_src_port : (p.src_port ? p.src_port[i] : p.def_src_port);
        const uint32_t dp = AOS ? tv.z >> 16 : FULL ? p.dst_port[i] : PROBE ? p.def_dst_port : (p.dst_port ? p.dst_port[i] : p.def_dst_port);
        const uint32_t id = AOS ? tv.w & 0xFFFFu : FULL ? p.ip_id[i] : PROBE ? p.def_ip_id : (p.ip_id ? p.ip_id[i] : p.def_ip_id);
        const uint32_t ulen = 8u + p.payload_len, total = 20u + ulen;
        const uint64_t addr = (uint64_t)(src >> 16) + (src & 0xFFFFu) + (dst >> 16) + (dst & 0xFFFFu);
        // udp.rs:443-477 on to_bytes(): pseudo + sport + dport + length (+ payload)
        const uint32_t ucs = fold_complement(addr + 17u + ulen + sp + dp + ulen + pw);
        // ipv4.rs:932-938 on to_bytes()[..20]
        const uint32_t w0 = (0x45u << 8) | p.dscp_ecn, w3 = ((uint32_t)(p.ip_flags & 7u)) << 13;
        const uint32_t w4 = ((uint32_t)p.ttl << 8) | 17u;
        const uint32_t ics = fold_complement(addr + w0 + total + id + w3 + w4);
        uint8_t h[42];
        for (int k = 0; k < 6; k++) {
            h[k] = !FULL && !PROBE && !AOS && p.dst_mac ? p.dst_mac[i * 6 + k] : p.def_dst_mac[k];
            h[6 + k] = !FULL && !PROBE && !AOS && p.src_mac ? p.src_mac[i * 6 + k] : p.def_src_mac[k];
        }
        h[12] = 0x08; h[13] = 0x00;
        h[14] = (uint8_t)(w0 >> 8); h[15] = (uint8_t)w0;
        h[16] = (uint8_t)(total >> 8); h[17] = (uint8_t)total;
        h[18] = (uint8_t)(id >> 8); h[19] = (uint8_t)id;
        h[20] = (uint8_t)(w3 >> 8); h[21] = 0;
        h[22] = p.ttl; h[23] = 17;
        h[24] = (uint8_t)(ics >> 8); h[25] = (uint8_t)ics;
        h[26] = (uint8_t)(src >> 24); h[27] = (uint8_t)(src >> 16); h[28] = (uint8_t)(src >> 8); h[29] = (uint8_t)src;
        h[30] = (uint8_t)(dst >> 24); h[31] = (uint8_t)(dst >> 16); h[32] = (uint8_t)(dst >> 8); h[33] = (uint8_t)dst;
        h[34] = (uint8_t)(sp >> 8); h[35] = (uint8_t)sp;
        h[36] = (uint8_t)(dp >> 8); h[37] = (uint8_t)dp;
        h[38] = (uint8_t)(ulen >> 8); h[39] = (uint8_t)ulen;
        h[40] = (uint8_t)(ucs >> 8); h[41] = (uint8_t)ucs;
        if (STAGED) {
            const uint32_t d0 = tid * a.out_stride;
            uint8_t* d = smem + d0;
            uint32_t hw[21];
#pragma unroll
            for (int k = 0; k < 21; k++) hw[k] = (uint32_t)h[2 * k] | ((uint32_t)h[2 * k + 1] << 8);
            lds_put_frame_hw<21>(smem, d0, hw);  // dword writes at either parity of d0
            for (uint32_t k = 0; k < p.payload_len; k++) d[42 + k] = p.payload[k];
            for (uint32_t k = flen; k < a.out_stride; k++) d[k] = 0;
        } else {
            uint8_t* d = a.out + i * (uint64_t)a.out_stride;
#pragma unroll
            for (int k = 0; k < 42; k++) d[k] = h[k];
            for (uint32_t k = 0; k < p.payload_len; k++) d[42 + k] = p.payload[k];
        }
    }
    build_finish<STAGED>(smem, t, nf, a.out, a.out_stride);
}

// ---- udp_ping IPv6 branch: builder/udp.rs:67-95 over IPv6 (udp.rs:480-505),
// Ipv6PacketBuilder::to_bytes (builder/ipv6.rs:89-152, ipv6.rs:50-75),
// EthernetPacketBuilder; 62 + payload_len bytes per frame.
struct Build6Args {
    nexg_udp6_build p;
    uint8_t* out;
    uint32_t out_stride;
    uint32_t tile_order;  // tile_index order (nexg_internal.hpp), as k_build_udp4
};

// udp_ping's IPv6 probe batch (p.src_shared: src_ip holds one address, dst_ip
// one per frame) reads 16 B per frame when its other arrays are NULL.
template <uint32_t MAXS>
__global__ __launch_bounds__(256) void k_build_udp6(Build6Args a) {
    constexpr bool STAGED = MAXS != 0;
    __shared__ __attribute__((aligned(16))) uint8_t smem[STAGED ? kBuildTile * MAXS : 16];
    const nexg_udp6_build& p = a.p;
    const BuildTile<kBuildTile> t(a.tile_order);
    const uint32_t nf = t.frames(p.count);
    const uint32_t tid = threadIdx.x;
    const uint64_t i = t.lane();
    __shared__ uint32_t s_pay;
    const uint64_t pw = shared_payload_sum(p.payload, p.payload_len, &s_pay);
    if (tid < nf) {
        uint32_t sw[4], dw[4];
        load_addrs<4>(p.src_ip, p.dst_ip, p.src_shared, i, sw, dw);
        const uint32_t sp = per_or_def(p.src_port, i, p.def_src_port);
        const uint32_t dp = per_or_def(p.dst_port, i, p.def_dst_port);
        const uint32_t ulen = 8u + p.payload_len;
        // util.rs:111-133 pseudo-header: address segments (as LE halves x 256),
        // next header 17, length; then sport, dport, length, payload (skipword 3)
        uint32_t addr_le = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) addr_le += halves(sw[k]) + halves(dw[k]);
        const uint32_t ucs = fold_complement(256ull * addr_le + 17u + ulen + sp + dp + ulen + pw);
        uint32_t hw[31];
        emit_eth(hw, p.dst_mac, p.def_dst_mac, p.src_mac, p.def_src_mac, i, 0xDD86u);  // EtherType 0x86DD
        emit_ipv6(hw, p.traffic_class, p.flow_label, ulen, 17u, p.hop_limit, sw, dw);
        hw[27] = bswap16(sp);
        hw[28] = bswap16(dp);
        hw[29] = bswap16(ulen);
        hw[30] = bswap16(ucs);  // computed 0 stays 0 (Q18)
        const FrameAt f = frame_at<STAGED>(smem, a.out, i, a.out_stride);
        put_frame<STAGED>(f.base, f.d0, a.out_stride, hw, p.payload, p.payload_len);
    }
    build_finish<STAGED>(smem, t, nf, a.out, a.out_stride);
}

// ---- tcp_ping / icmp_ping: one kernel per (family, L4 kind) ----------------
// The header is a compile-time halfword layout (Ethernet 7, IPv4 10 / IPv6 20,
// TCP 10 / ICMP echo 4) built in registers, then the shared TCP options and
// payload; checksums in closed form: per-frame words + the options word sum
// (host-computed, passed in) + the payload word sum (computed once per
// workgroup into LDS). Arguments: L4Args (build_core.hpp).
// PROBE: a tcp_ping / icmp_ping probe batch (ip.src_shared, every other
// per-frame array NULL): only the destination is read per frame (4 / 16 B);
// source, ports, seq / ack, identifier / sequence, id and MACs are the batch's.
template <int FAM, int KIND, uint32_t MAXS, bool PROBE = false>
__global__ __launch_bounds__(256) void k_build_l4(L4Args a) {
    constexpr bool STAGED = MAXS != 0;
    constexpr int NIP = FAM == 4 ? 10 : 20;             // IP header halfwords
    constexpr int NL4 = KIND == kL4Tcp ? 10 : 4;        // fixed L4 header halfwords
    constexpr int NH = 7 + NIP + NL4;
    static_assert(NH % 2 == 1, "lds_put_halfwords takes an odd halfword count");
    __shared__ __attribute__((aligned(16))) uint8_t smem[STAGED ? kBuildTile * MAXS : 16];
    __shared__ uint32_t s_pay;
    const uint32_t tid = threadIdx.x;
    const BuildTile<kBuildTile> t(a.tile_order);
    const uint32_t nf = t.frames(a.count);
    const uint64_t i = t.lane();
    const bool small = a.payload_len <= kSmallPay;  // uniform
    SmallPayload spay{};
    uint32_t pay_sum = 0;
    __shared__ uint32_t s_payw[kSmallPay / 4 + 1];  // the staged words, then their sum
    if (small && STAGED) {
        // staged tile: wave 0 realigns and sums the payload once for the
        // workgroup (the other waves skip ~100 VALU instructions each): icmp_ping's
        // 47-B batch 0.525 -> 0.70 of 8 TB/s written (profiles/r05/payload/)
        if (a.payload_len) {  // uniform
            if (tid < 64u) {
                load_small_payload(a.payload, a.payload_len, spay, pay_sum);
                stage_small_payload(spay, s_payw);
                if (tid == 0) s_payw[kSmallPay / 4] = pay_sum;
            }
            __syncthreads();
            pay_sum = s_payw[kSmallPay / 4];
        }
    } else if (small) {
        load_small_payload(a.payload, a.payload_len, spay, pay_sum);
        if (STAGED && a.payload_len) stage_small_payload(spay, s_payw);
    } else {
        pay_sum = shared_payload_sum(a.payload, a.payload_len, &s_pay);
    }
    const uint32_t l4_hdr = KIND == kL4Tcp ? 20u + a.opt_padded : 8u;
    const uint32_t l4_len = l4_hdr + a.payload_len;
    const uint32_t flen = 14u + 2u * NIP + l4_len;
    if (tid < nf) {
        const nexg_ip_build& ip = a.ip;
        constexpr uint32_t AW = FAM == 4 ? 1u : 4u;  // address dwords
        uint32_t sw[AW], dw[AW];
        load_addrs<AW>(ip.src_ip, ip.dst_ip, PROBE || ip.src_shared, i, sw, dw);
        uint32_t addr_le = 0;  // address words as LE halves: x256 gives the BE sum (mod 0xFFFF)
#pragma unroll
        for (int k = 0; k < (FAM == 4 ? 1 : 4); k++) addr_le += halves(sw[k]) + halves(dw[k]);
        const uint32_t proto = KIND == kL4Tcp ? 6u : (FAM == 4 ? 1u : 58u);
        uint32_t hw[NH];
        // Ethernet and IPv6 headers written out here, not by emit_eth / emit_ipv6:
        // with the emitters the IPv6 echo instances split two of their dwordx4
        // address loads and regrouped the kernel-argument loads, and icmp6 echo
        // ran 0.297 ms against 0.276 (profiles/build_refactor/README.md)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint8_t* dm = PROBE ? nullptr : ip.dst_mac;
            const uint8_t* sm = PROBE ? nullptr : ip.src_mac;
            const uint32_t b0 = per_or_def(dm, i * 6 + 2 * k, ip.def_dst_mac[2 * k]);
            const uint32_t b1 = per_or_def(dm, i * 6 + 2 * k + 1, ip.def_dst_mac[2 * k + 1]);
            const uint32_t c0 = per_or_def(sm, i * 6 + 2 * k, ip.def_src_mac[2 * k]);
            const uint32_t c1 = per_or_def(sm, i * 6 + 2 * k + 1, ip.def_src_mac[2 * k + 1]);
            hw[k] = b0 | (b1 << 8);
            hw[3 + k] = c0 | (c1 << 8);
        }
        hw[6] = FAM == 4 ? 0x0008u : 0xDD86u;
        // ---- L4 header + checksum ----
        uint64_t sum;
        constexpr int L = 7 + NIP;  // first L4 halfword
        if constexpr (KIND == kL4Tcp) {
            const uint32_t sp = PROBE ? a.def_sport : per_or_def(a.sport, i, a.def_sport);
            const uint32_t dp = PROBE ? a.def_dport : per_or_def(a.dport, i, a.def_dport);
            const uint32_t sq = PROBE ? a.def_seq : per_or_def(a.seq, i, a.def_seq);
            const uint32_t ak = PROBE ? a.def_ack : per_or_def(a.ack, i, a.def_ack);
            const uint32_t w6 = ((l4_hdr / 4u) << 12) | (a.flags & 0xFFu);
            sum = sp + dp + (sq >> 16) + (sq & 0xFFFFu) + (ak >> 16) + (ak & 0xFFFFu) + w6 + a.window + a.urg +
                a.opt_sum + pay_sum;
            hw[L + 0] = bswap16(sp); hw[L + 1] = bswap16(dp);
            hw[L + 2] = bswap16(sq >> 16); hw[L + 3] = bswap16(sq & 0xFFFFu);
            hw[L + 4] = bswap16(ak >> 16); hw[L + 5] = bswap16(ak & 0xFFFFu);
            hw[L + 6] = bswap16(w6); hw[L + 7] = bswap16(a.window);
            hw[L + 9] = bswap16(a.urg);
        } else {
            const uint32_t id = PROBE ? a.def_ident : per_or_def(a.ident, i, a.def_ident);
            const uint32_t sq = PROBE ? a.def_seqno : per_or_def(a.seqno, i, a.def_seqno);
            const uint32_t w0 = (a.icmp_type << 8) | a.icmp_code;
            sum = w0 + id + sq + pay_sum;
            hw[L + 0] = bswap16(w0);
            hw[L + 2] = bswap16(id); hw[L + 3] = bswap16(sq);
        }
        if (FAM == 6 || KIND == kL4Tcp) sum += 256ull * addr_le + proto + l4_len;  // pseudo-header
        const uint32_t cs = fold_complement(sum);  // computed 0 stays 0 (Q18)
        hw[KIND == kL4Tcp ? L + 8 : L + 1] = bswap16(cs);
        // ---- IP header ----
        if constexpr (FAM == 4) {
            const uint32_t total = 20u + l4_len, id = PROBE ? ip.def_ip_id : per_or_def(ip.ip_id, i, ip.def_ip_id);
            const uint32_t w0 = (0x45u << 8) | ip.tos, w3 = ((uint32_t)(ip.ip_flags & 7u)) << 13;
            const uint32_t w4 = ((uint32_t)ip.ttl << 8) | proto;
            const uint32_t ics = fold_complement(256ull * addr_le + w0 + total + id + w3 + w4);
            hw[7] = bswap16(w0); hw[8] = bswap16(total); hw[9] = bswap16(id); hw[10] = bswap16(w3);
            hw[11] = bswap16(w4); hw[12] = bswap16(ics);
            hw[13] = sw[0] & 0xFFFFu; hw[14] = sw[0] >> 16; hw[15] = dw[0] & 0xFFFFu; hw[16] = dw[0] >> 16;
        } else {
            const uint32_t fl = ip.flow_label & 0xFFFFFu, tc = ip.tos;
            hw[7] = ((6u << 4) | (tc >> 4)) | ((((tc & 0xFu) << 4) | (fl >> 16)) << 8);
            hw[8] = ((fl >> 8) & 0xFFu) | ((fl & 0xFFu) << 8);
            hw[9] = bswap16(l4_len);
            hw[10] = proto | ((uint32_t)ip.ttl << 8);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                hw[11 + 2 * k] = sw[k] & 0xFFFFu; hw[12 + 2 * k] = sw[k] >> 16;
                hw[19 + 2 * k] = dw[k] & 0xFFFFu; hw[20 + 2 * k] = dw[k] >> 16;
            }
        }
        // ---- write: fixed halfwords, options, payload, zero gap (the options
        // and the three payload forms are this kernel's: not put_frame's one run)
        const FrameAt f = frame_at<STAGED>(smem, a.out, i, a.out_stride);
        uint8_t* const base = f.base;
        const uint32_t d0 = f.d0;
        const bool odd = (a.out_stride & 1u) != 0;
        put_frame_head<STAGED>(base, d0, hw);
        uint32_t p = d0 + 2u * NH;
        if (KIND == kL4Tcp) {
            // unrolled over the 40-B maximum with a uniform guard: constant
            // kernarg offsets become scalar loads, where a run-time index made
            // one vector load + vmcnt(0) wait per option halfword pair
#pragma unroll
            for (uint32_t k = 0; k < 40u; k += 2)
                if (k < a.opt_padded) put_hw(base, p + k, a.options[k] | ((uint32_t)a.options[k + 1] << 8), odd);
            p += a.opt_padded;
        }
        if (small && STAGED) {
            const uint8_t* pb = reinterpret_cast<const uint8_t*>(s_payw);
            for (uint32_t k = 0; k < a.payload_len; k++) base[p + k] = pb[k];
        } else if (small) {
#pragma unroll
            for (uint32_t k = 0; k < kSmallPay; k++)
                if (k < a.payload_len) base[p + k] = (uint8_t)spay.byte(k);
        } else {
            for (uint32_t k = 0; k < a.payload_len; k++) base[p + k] = a.payload[k];
        }
        put_frame_gap<STAGED>(base, d0, a.out_stride, flen);
    }
    build_finish<STAGED>(smem, t, nf, a.out, a.out_stride);
}

template <int FAM, int KIND, bool PROBE>
static void launch_l4_form(const L4Args& a, dim3 grid, hipStream_t s) {
    const bool staged = build_staged(a.out, a.out_stride);
    const dim3 blk(kBuildTile);
    // IPv6: 16-KiB tile + build_lds_pad() -> 5 workgroups per CU (icmp6 echo
    // 0.29 -> 0.26 ms at 16M frames); IPv4 shapes run faster at 8 per CU (tcp
    // SYN 0.21 vs 0.24-0.26 ms, icmp echo 0.132 vs 0.140; profiles/r04/builders/)
    // ICMP probe batches (odd frame lengths, 47 / 67 B) run faster at 8 per CU:
    // 0.437 / 0.570 of 8 TB/s written against 0.385 / 0.485 (profiles/r05/probe/)
    const uint32_t pad = (FAM == 6 || PROBE) && !(PROBE && KIND == kL4Icmp) ? build_lds_pad() : 0u;
    if (staged && a.out_stride <= 64u)
        hipLaunchKernelGGL((k_build_l4<FAM, KIND, 64, PROBE>), grid, blk, pad, s, a);
    else if (staged && a.out_stride <= 80u)  // tcp_ping's 66 B: a 20-KiB tile (7 per CU) instead of 32 KiB (4)
        hipLaunchKernelGGL((k_build_l4<FAM, KIND, 80, PROBE>), grid, blk, pad > 4096u ? pad - 4096u : 0u, s, a);
    else if (staged)
        hipLaunchKernelGGL((k_build_l4<FAM, KIND, kBuildMaxStride, PROBE>), grid, blk, 0, s, a);
    else
        hipLaunchKernelGGL((k_build_l4<FAM, KIND, 0, PROBE>), grid, blk, 0, s, a);
}

template <int FAM, int KIND>
static hipError_t launch_l4_fam(L4Args& a, dim3 grid, hipStream_t s) {
    // the probe batch: one source, a destination per frame, nothing else per
    // frame. It reads 4 / 16 B per frame, as udp_ping's probe batch, and takes
    // that builder's tile order (contiguous eighths); the forms with several
    // parameter arrays keep l4_build_tile_order()
    const bool probe = a.ip.src_shared && !a.ip.ip_id && !a.ip.src_mac && !a.ip.dst_mac &&
                       (KIND == kL4Tcp ? !a.sport && !a.dport && !a.seq && !a.ack : !a.ident && !a.seqno);
    // the template kernel's status (its explicit checks and its launch's
    // hipGetLastError, which also clears HIP's error state) is the result
    hipError_t e = hipSuccess;
    if (probe && try_probe_l4(a, KIND, a.out, a.out_stride, s, e)) return e;
    if (probe) {
        a.tile_order = build_tile_order();
        launch_l4_form<FAM, KIND, true>(a, grid, s);
    } else {
        launch_l4_form<FAM, KIND, false>(a, grid, s);
    }
    return hipGetLastError();
}

static hipError_t launch_l4(L4Args& a, int kind, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    dim3 grid;
    if (hipError_t e = build_grid(a.count, kBuildTile, grid)) return e;
    a.tile_order = l4_build_tile_order();
    if (kind == kL4Tcp)
        return a.ip.family == 4 ? launch_l4_fam<4, kL4Tcp>(a, grid, s) : launch_l4_fam<6, kL4Tcp>(a, grid, s);
    return a.ip.family == 4 ? launch_l4_fam<4, kL4Icmp>(a, grid, s) : launch_l4_fam<6, kL4Icmp>(a, grid, s);
}

hipError_t launch_build_tcp(const nexg_tcp_build& p, uint8_t* out, uint32_t out_stride, hipStream_t s) {
    L4Args a{};
    a.ip = p.ip;
    a.sport = p.src_port; a.dport = p.dst_port; a.seq = p.seq; a.ack = p.ack;
    a.def_seq = p.def_seq; a.def_ack = p.def_ack; a.def_sport = p.def_src_port; a.def_dport = p.def_dst_port;
    a.window = p.window; a.urg = p.urgent_ptr; a.flags = p.flags;
    a.opt_padded = (p.options_len + 3u) & ~3u;
    for (uint32_t k = 0; k < 40; k++) a.options[k] = k < p.options_len ? p.options[k] : 0;
    for (uint32_t k = 0; k < a.opt_padded; k += 2) a.opt_sum += ((uint32_t)a.options[k] << 8) | a.options[k + 1];
    a.payload = p.payload; a.payload_len = p.payload_len; a.count = p.count;
    a.out = out; a.out_stride = out_stride;
    return launch_l4(a, kL4Tcp, s);
}

hipError_t launch_build_icmp_echo(const nexg_icmp_echo_build& p, uint8_t* out, uint32_t out_stride,
                                  hipStream_t s) {
    L4Args a{};
    a.ip = p.ip;
    a.ident = p.identifier; a.seqno = p.sequence; a.def_ident = p.def_identifier; a.def_seqno = p.def_sequence;
    a.icmp_type = p.icmp_type; a.icmp_code = p.icmp_code;
    a.payload = p.payload; a.payload_len = p.payload_len; a.count = p.count;
    a.out = out; a.out_stride = out_stride;
    return launch_l4(a, kL4Icmp, s);
}

// ---- arp / ndp probes ------------------------------------------------------
// One lane per frame: the frame's halfwords (memory order, low byte first)
// assembled in registers, written to the LDS tile and copied out coalesced
// like the other builders. 6-B address fields are read bytewise (any
// alignment); IPv6 addresses as dwords (4-B aligned, nexg_ip_build). Tiles in
// grid order.

struct ArpArgs {
    nexg_arp_build p;
    uint8_t* out;
    uint32_t out_stride;
};

// builder/arp.rs:18-37 + arp.rs:385-399 behind Ethernet (examples/arp.rs:59-67)
template <uint32_t MAXS>
__global__ __launch_bounds__(256) void k_build_arp(ArpArgs a) {
    constexpr bool STAGED = MAXS != 0;
    __shared__ __attribute__((aligned(16))) uint8_t smem[STAGED ? kBuildTile * MAXS : 16];
    const nexg_arp_build& p = a.p;
    const BuildTile<kBuildTile> t(0);
    const uint32_t nf = t.frames(p.count);
    const uint32_t tid = threadIdx.x;
    const uint64_t i = t.lane();
    if (tid < nf) {
        uint32_t hw[21];
        emit_eth(hw, p.eth_dst, p.def_eth_dst, p.sender_mac, p.def_sender_mac, i, 0x0608u);  // EtherType 0x0806
        hw[7] = bswap16(p.hardware_type);
        hw[8] = bswap16(p.protocol_type);
        hw[9] = (uint32_t)p.hw_addr_len | ((uint32_t)p.proto_addr_len << 8);
        hw[10] = bswap16(p.operation);
#pragma unroll
        for (int k = 0; k < 3; k++) hw[11 + k] = hw[3 + k];  // sender_hw_addr
        const uint8_t* tip = p.target_ip + 4u * i;
#pragma unroll
        for (int k = 0; k < 2; k++)
            hw[14 + k] = per_or_def(p.sender_ip, 4u * i + 2 * k, p.def_sender_ip[2 * k]) |
                         (per_or_def(p.sender_ip, 4u * i + 2 * k + 1, p.def_sender_ip[2 * k + 1]) << 8);
#pragma unroll
        for (int k = 0; k < 3; k++) hw[16 + k] = mac_halfword(p.target_mac, p.def_target_mac, i, k);
        hw[19] = (uint32_t)tip[0] | ((uint32_t)tip[1] << 8);
        hw[20] = (uint32_t)tip[2] | ((uint32_t)tip[3] << 8);
        const FrameAt f = frame_at<STAGED>(smem, a.out, i, a.out_stride);
        put_frame<STAGED>(f.base, f.d0, a.out_stride, hw, nullptr, 0);
    }
    build_finish<STAGED>(smem, t, nf, a.out, a.out_stride);
}

struct NdpArgs {
    nexg_ndp_ns_build p;
    uint8_t* out;
    uint32_t out_stride;
};

// builder/ndp.rs:30-84 (NS + SourceLLAddr option, icmpv6::checksum) inside
// Ipv6PacketBuilder + EthernetPacketBuilder (examples/ndp.rs:82-108)
template <uint32_t MAXS>
__global__ __launch_bounds__(256) void k_build_ndp_ns(NdpArgs a) {
    constexpr bool STAGED = MAXS != 0;
    constexpr int NH = 43;  // 86 B
    __shared__ __attribute__((aligned(16))) uint8_t smem[STAGED ? kBuildTile * MAXS : 16];
    const nexg_ndp_ns_build& p = a.p;
    const nexg_ip_build& ip = p.ip;
    const BuildTile<kBuildTile> t(0);
    const uint32_t nf = t.frames(p.count);
    const uint32_t tid = threadIdx.x;
    const uint64_t i = t.lane();
    if (tid < nf) {
        uint32_t sw[4], dw[4];
        load_addrs<4>(ip.src_ip, ip.dst_ip, false, i, sw, dw);  // a source per frame
        uint32_t hw[NH];
        // Ethernet destination: given, or 33:33 + target bytes 12..15 (ndp.rs:25-35)
        const bool mc = p.eth_dst_multicast != 0;
        emit_eth(hw, mc ? nullptr : ip.dst_mac, ip.def_dst_mac, ip.src_mac, ip.def_src_mac, i, 0xDD86u);
        if (mc) {
            hw[0] = 0x3333u;
            hw[1] = dw[3] & 0xFFFFu;
            hw[2] = dw[3] >> 16;
        }
        emit_ipv6(hw, ip.tos, ip.flow_label, 32u, 58u, ip.ttl, sw, dw);  // payload 32, next header 58
        // NeighborSolicit: type 135 code 0, checksum, reserved 0, target = dst, option 1 / len 1 / MAC
        constexpr int L = 27;
        hw[L + 0] = 135u;
        hw[L + 2] = 0u; hw[L + 3] = 0u;
#pragma unroll
        for (int k = 0; k < 8; k++) hw[L + 4 + k] = hw[19 + k];
        hw[L + 12] = 0x0101u;
#pragma unroll
        for (int k = 0; k < 3; k++) hw[L + 13 + k] = hw[3 + k];
        // icmpv6::checksum (util.rs:91-137): pseudo-header (src, dst, length 32, next header 58)
        // + the message with its checksum word skipped; memory-order halfwords are
        // little-endian, x256 gives the big-endian sum (mod 0xFFFF)
        uint32_t le = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) le += hw[11 + k];   // src + dst
#pragma unroll
        for (int k = 0; k < 8; k++) le += hw[L + 4 + k];  // target
#pragma unroll
        for (int k = 0; k < 3; k++) le += hw[L + 13 + k]; // MAC
        hw[L + 1] = bswap16(fold_complement(256ull * le + 58u + 32u + (135u << 8) + 0x0101u));
        const FrameAt f = frame_at<STAGED>(smem, a.out, i, a.out_stride);
        put_frame<STAGED>(f.base, f.d0, a.out_stride, hw, nullptr, 0);
    }
    build_finish<STAGED>(smem, t, nf, a.out, a.out_stride);
}

// --------------------------------------------------------------- launchers
// Each picks its kernel by build_staged and the stride's tile band, one
// workgroup per tile (build_grid).

hipError_t launch_build_arp(const nexg_arp_build& p, uint8_t* out, uint32_t out_stride, hipStream_t s) {
    if (p.count == 0) return hipSuccess;
    ArpArgs a{p, out, out_stride};
    dim3 grid;
    if (hipError_t e = build_grid(p.count, kBuildTile, grid)) return e;
    const dim3 blk(kBuildTile);
    const bool staged = build_staged(out, out_stride);
    if (staged && out_stride <= 64u) hipLaunchKernelGGL(k_build_arp<64>, grid, blk, 0, s, a);
    else if (staged) hipLaunchKernelGGL(k_build_arp<kBuildMaxStride>, grid, blk, 0, s, a);
    else hipLaunchKernelGGL(k_build_arp<0>, grid, blk, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_build_ndp_ns(const nexg_ndp_ns_build& p, uint8_t* out, uint32_t out_stride, hipStream_t s) {
    if (p.count == 0) return hipSuccess;
    NdpArgs a{p, out, out_stride};
    dim3 grid;
    if (hipError_t e = build_grid(p.count, kBuildTile, grid)) return e;
    const dim3 blk(kBuildTile);
    if (build_staged(out, out_stride)) hipLaunchKernelGGL(k_build_ndp_ns<kBuildMaxStride>, grid, blk, 0, s, a);
    else hipLaunchKernelGGL(k_build_ndp_ns<0>, grid, blk, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_build_udp4_tuples(const nexg_udp4_build& p, const nexg_udp4_tuple* tuples, uint8_t* out,
                                    uint32_t out_stride, hipStream_t s) {
    if (p.count == 0) return hipSuccess;
    BuildArgs a{p, out, out_stride, tuples, build_tile_order()};
    dim3 grid;
    if (hipError_t e = build_grid(p.count, kBuildTile, grid)) return e;
    const dim3 blk(kBuildTile);
    const bool staged = build_staged(out, out_stride);
    if (staged && out_stride <= 64u)
        hipLaunchKernelGGL((k_build_udp4<64, false, false, true>), grid, blk, build_lds_pad(), s, a);
    else if (staged)
        hipLaunchKernelGGL((k_build_udp4<kBuildMaxStride, false, false, true>), grid, blk, 0, s, a);
    else
        hipLaunchKernelGGL((k_build_udp4<0, false, false, true>), grid, blk, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_build_udp4(const nexg_udp4_build& p, uint8_t* out, uint32_t out_stride,
                             hipStream_t s) {
    if (p.count == 0) return hipSuccess;
    BuildArgs a{p, out, out_stride, nullptr, build_tile_order()};
    dim3 grid;
    if (hipError_t e = build_grid(p.count, kBuildTile, grid)) return e;
    const dim3 blk(kBuildTile);
    const bool staged = build_staged(out, out_stride);
    const bool full = p.src_ip && p.src_port && p.dst_port && p.ip_id && !p.src_mac && !p.dst_mac;
    const bool probe = !p.src_ip && !p.src_port && !p.dst_port && !p.ip_id && !p.src_mac && !p.dst_mac;
    // the udp_ping shapes: a 16-KiB tile + build_lds_pad() -> 5 workgroups per CU
    // (the probe batch stays per lane: 0.84-0.85 of 8 TB/s written against
    // 0.69-0.83 for the template kernel, profiles/r05/probe/)
    const uint32_t pad = build_lds_pad();
    if (staged && out_stride <= 64u && full)
        hipLaunchKernelGGL((k_build_udp4<64, true>), grid, blk, pad, s, a);
    else if (staged && out_stride <= 64u && probe)
        hipLaunchKernelGGL((k_build_udp4<64, false, true>), grid, blk, pad, s, a);
    else if (staged && out_stride <= 64u)
        hipLaunchKernelGGL(k_build_udp4<64>, grid, blk, 0, s, a);
    else if (staged)
        hipLaunchKernelGGL(k_build_udp4<kBuildMaxStride>, grid, blk, 0, s, a);
    else
        hipLaunchKernelGGL(k_build_udp4<0>, grid, blk, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_build_udp6(const nexg_udp6_build& p, uint8_t* out, uint32_t out_stride,
                             hipStream_t s) {
    if (p.count == 0) return hipSuccess;
    Build6Args a{p, out, out_stride, l4_build_tile_order()};
    dim3 grid;
    if (hipError_t e = build_grid(p.count, kBuildTile, grid)) return e;
    const dim3 blk(kBuildTile);
    const bool staged = build_staged(out, out_stride);
    const bool probe = p.src_shared && !p.src_port && !p.dst_port && !p.src_mac && !p.dst_mac;
    hipError_t e = hipSuccess;
    if (probe && try_probe_udp6(p, out, out_stride, s, e)) return e;
    if (probe) a.tile_order = build_tile_order();  // udp_ping's probe batch order (see launch_l4_fam)
    // a 16-KiB tile for the udp_ping shapes + build_lds_pad(): 5 workgroups per CU (0.279 -> 0.253 ms)
    // (a probe batch reaching here has a misaligned output or a long frame:
    // the per-lane kernel's src_shared branch takes it)
    if (staged && out_stride <= 64u)
        hipLaunchKernelGGL(k_build_udp6<64>, grid, blk, build_lds_pad(), s, a);
    else if (staged)
        hipLaunchKernelGGL(k_build_udp6<kBuildMaxStride>, grid, blk, 0, s, a);
    else
        hipLaunchKernelGGL(k_build_udp6<0>, grid, blk, 0, s, a);
    return hipGetLastError();
}

}  // namespace nexg

#if NEXG_PROBE_TIMING
// measurement builds only. The stamp buffer is one device variable, and the
// library has a code object per translation unit (no relocatable device code),
// so the template kernels are compiled into this unit; nexg_build_probe.hip on
// its own is empty in such a build.
#define NEXG_BUILD_ONE_UNIT 1
#include "nexg_build_probe.hip"

// copy the builders' workgroup stamps to the host
extern "C" int nexg_debug_build_stamps(uint64_t* host, uint64_t n, int reset) {
    if (n > 8ull * nexg::kStampWgs) n = 8ull * nexg::kStampWgs;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(nexg::g_build_stamps), n * 8u, 0, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    if (reset) {
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(nexg::g_build_stamps)) != hipSuccess ||
            hipMemset(p, 0, 8ull * 8u * nexg::kStampWgs) != hipSuccess)
            return -1;
    }
    return 0;
}
#endif
