// nexg_build_probe.hip — serialize path, probe batches: the frames of a batch
// with one source and a destination per frame, built from one template
// (k_build_probe, k_build_lane), the host side that makes the template from
// the builders' arguments, and the launchers (try_probe_*, build_core.hpp).
#include <stdlib.h>

#include "build_core.hpp"

// (a -DNEXG_PROBE_TIMING=1 build compiles this file as part of nexg_build.hip)
#if !NEXG_PROBE_TIMING || defined(NEXG_BUILD_ONE_UNIT)

namespace nexg {

// ---- probe batches: one template + a per-frame patch ----------------------
// Every frame of a probe batch (one source, a destination per frame, every
// other field the batch's) is one template with the destination address and
// the checksums over it patched. The host builds the template (one frame
// period P = out_stride, with destination, checksums and the device-resident
// source / payload bytes 0) and its base sums and passes it in the kernel
// arguments; a workgroup reads it by scalar loads, merges in the source and
// payload (scalar loads: every workgroup reads the same line, which as vector
// loads makes one L2 channel the bottleneck), lays the period out in LDS and
// fills its tile with it (one ds_write_b128 per 16-B chunk, realigned by
// v_alignbyte), patches each frame (the other builders' closed-form sums: the
// batch base sum plus the destination's halfwords), and copies the tile out
// with 16-B non-temporal stores.
// Used for tcp_ping (IPv4 / IPv6) and udp_ping's IPv6 batch, where it beats
// the per-lane builders (tcp_ping 0.72-0.89 of 8 TB/s written against
// 0.70-0.73); udp_ping's IPv4 batch and the ICMP shapes stay per lane
// (profiles/r05/probe/). A persistent sweep over the tiles and one-wave
// workgroups were measured and lose (writes at 0.65-0.72 of 8 TB/s in a
// sweep, tools/writebench.hip).
#ifndef NEXG_PROBE_TEMPLATE
#define NEXG_PROBE_TEMPLATE 1  // 0: the per-lane builders for probe batches too (A/B builds)
#endif
constexpr uint32_t kProbeMaxP = 128;

struct ProbeArgs {
    uint32_t tmpl[kProbeMaxP / 4];  // one period (the frame with destination, checksums and device bytes 0, zero pad)
    uint64_t ip_sum;           // IPv4 header: congruent sum of every word but the destination's (and a device source's)
    uint64_t l4_sum;           // L4: the same, without the payload
    const uint8_t* dst;        // per-frame destination: DW dwords each, 4-B aligned
    const uint8_t* src;        // the batch's source on the device (DW dwords), written in at src_off; or NULL
    const uint8_t* payload;    // device payload (<= kSmallPay bytes), written in at pay_off
    uint8_t* out;
    uint64_t count;
    uint32_t period;           // out_stride (<= kProbeMaxP)
    uint32_t dst_off, ip_ck_off, l4_ck_off;  // byte offsets in the frame; a checksum offset 0 = none
    uint32_t l4_dst;           // the L4 checksum covers the addresses (all but ICMPv4)
    uint32_t dst_value;        // udp_ping IPv4: dst is a u32 value (bytes reversed in the frame, BE halves summed)
    uint32_t src_off, ip_src;  // device source offset; the source is in the IPv4 header checksum
    uint32_t pay_off, pay_len;
    uint32_t tile_order;
};

// halfword v (big-endian: high byte first in memory) at LDS byte position p
__device__ __forceinline__ void lds_put_be16(uint8_t* lds, uint32_t p, uint32_t v) {
    if (p & 1u) {
        lds[p] = (uint8_t)(v >> 8);
        lds[p + 1] = (uint8_t)v;
    } else {
        *reinterpret_cast<uint16_t*>(lds + p) = (uint16_t)bswap16(v);
    }
}
// dword d of network-order bytes (as loaded little-endian) at LDS position p
__device__ __forceinline__ void lds_put_net32(uint8_t* lds, uint32_t p, uint32_t d) {
    lds_put_be16(lds, p, bswap16(d & 0xFFFFu));
    lds_put_be16(lds, p + 2u, bswap16(d >> 16));
}

// A workgroup of WAVES waves builds a tile of kT = 64 WAVES frames (one per
// lane). KCH = ceil(P / 16): the 16-B pattern chunks per lane (kT frames x P
// bytes = kT P / 16 chunks), written unconditionally. With one wave per
// workgroup the barriers below are wave barriers (no s_barrier).
template <uint32_t DW, uint32_t KCH, uint32_t WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_build_probe(ProbeArgs a) {
    constexpr uint32_t kT = 64u * WAVES;
    extern __shared__ __attribute__((aligned(16))) uint8_t s_tile[];  // kT x P, then the pattern
    const uint32_t t = threadIdx.x, P = a.period;
    // (1) once per workgroup, the period in LDS: wave 0 composes template
    // bytes [0, P + 24) (the period and the start of its next copy, so a 20-B
    // window at any offset < P is contiguous): the template dwords come from
    // the kernel arguments by scalar loads and reach their lanes by a cndmask
    // chain and ds_bpermute; the device payload and source bytes are loaded
    // into place, so they are part of the pattern and not patched per frame
    uint8_t* const tp = s_tile + KCH * 16u * kT;  // 2 x kProbeMaxP + 32 B
    // this lane's destination goes in flight (clamped index: an unconditional
    // load; lanes past the batch's end reload its last frame)
    const BuildTile<kT> g(a.tile_order);
    uint32_t dw[DW];
    {
        const uint64_t i = g.lane();
        const auto* d4 = NEXG_GLOBAL(uint32_t, a.dst + 4u * DW * (i < a.count ? i : a.count - 1u));
#pragma unroll
        for (uint32_t k = 0; k < DW; k++) dw[k] = d4[k];
    }
    // the batch's device source by scalar loads (uniform addresses through the
    // scalar cache: a vector load of one line by every workgroup of the grid
    // makes that line's L2 channel the bottleneck) and its BE word sum
    uint32_t sx[DW], ssum = 0;
#pragma unroll
    for (uint32_t k = 0; k < DW; k++) sx[k] = 0;
    if (a.src) {  // 4-B aligned
#pragma unroll
        for (uint32_t k = 0; k < DW; k++) sx[k] = uniform_u32(a.src)[k];
#pragma unroll
        for (uint32_t k = 0; k < DW; k++) ssum += bswap16(sx[k] & 0xFFFFu) + bswap16(sx[k] >> 16);
    }
    uint32_t* const psum_lds = reinterpret_cast<uint32_t*>(tp) + (kProbeMaxP + 32u) / 4u;  // past the pattern
    if (t < 64u) {
        // the payload (scalar loads) realigned and summed by wave 0 only; its
        // sum reaches the other waves through LDS
        SmallPayload spay;
        uint32_t psum0;
        load_small_payload(a.payload, a.pay_len, spay, psum0);  // realigned words, 0 past pay_len
        if (t == 0) *psum_lds = psum0;
        // template, source and payload words handed to lane k by cndmask
        // chains, then each pattern byte picked by ds_bpermute from the lane
        // holding it (one per source: the source lane returns its own copy of
        // the operand, so the operand cannot depend on the reading lane)
        uint32_t v = 0, sv = 0, pv = 0;
#pragma unroll
        for (uint32_t k = 0; k < kProbeMaxP / 4; k++) v = t == k ? a.tmpl[k] : v;
#pragma unroll
        for (uint32_t k = 0; k < DW; k++) sv = t == k ? sx[k] : sv;
#pragma unroll
        for (uint32_t k = 0; k < kSmallPay / 4; k++) pv = t == k ? spay.w[k] : pv;
        uint32_t d = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t j = 4u * t + i, jm = j >= P ? j - P : j;
            const uint32_t pi = jm - a.pay_off, si = jm - a.src_off;  // wrap: huge when before
            const bool in_p = pi < a.pay_len, in_s = a.src && si < 4u * DW;
            const uint32_t xt = (uint32_t)__shfl(v, (int)(jm >> 2));
            const uint32_t xs = (uint32_t)__shfl(sv, (int)((si >> 2) & 63u));
            const uint32_t xp = (uint32_t)__shfl(pv, (int)((pi >> 2) & 63u));
            const uint32_t x = in_p ? xp >> (8u * (pi & 3u)) : in_s ? xs >> (8u * (si & 3u)) : xt >> (8u * (jm & 3u));
            d |= (x & 0xFFu) << (8u * i);
        }
        if (4u * t < P + 24u) reinterpret_cast<uint32_t*>(tp)[t] = d;
    }
    __syncthreads();
    const uint32_t psum = *psum_lds;
    const uint32_t step = (16u * kT) % P, r0 = (16u * t) % P;
    // the pattern over the tile: chunk c = bytes [(16 c) mod P, + 16) of the
    // period, five dword reads realigned by v_alignbyte
    auto fill = [&]() {
        uint32_t r = r0;
#pragma unroll
        for (uint32_t k = 0; k < KCH; k++) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(tp + (r & ~3u));
            const uint32_t sh = r & 3u;
            const uint4 c = make_uint4(__builtin_amdgcn_alignbyte(w[1], w[0], sh),
                                       __builtin_amdgcn_alignbyte(w[2], w[1], sh),
                                       __builtin_amdgcn_alignbyte(w[3], w[2], sh),
                                       __builtin_amdgcn_alignbyte(w[4], w[3], sh));
            reinterpret_cast<uint4*>(s_tile)[t + kT * k] = c;
            r += step;
            r = r >= P ? r - P : r;
        }
    };
    // this lane's frame: the destination and the checksums over it
    auto patch = [&](const uint32_t (&cur)[DW]) {
        uint8_t* f = s_tile + t * P;
        uint32_t dsum = 0;
#pragma unroll
        for (uint32_t k = 0; k < DW; k++) dsum += halves(cur[k]);
        uint64_t D;
        if (a.dst_value) {  // a u32 value: network order in the frame, its BE halves summed
            lds_put_be16(f, a.dst_off, cur[0] >> 16);
            lds_put_be16(f, a.dst_off + 2u, cur[0] & 0xFFFFu);
            D = dsum;
        } else {  // network-order bytes as stored: LE halves x 256
#pragma unroll
            for (uint32_t k = 0; k < DW; k++) lds_put_net32(f, a.dst_off + 4u * k, cur[k]);
            D = 256ull * dsum;
        }
        const uint64_t S = ssum;
        if (a.ip_ck_off) lds_put_be16(f, a.ip_ck_off, fold_complement(a.ip_sum + (a.ip_src ? S : 0u) + D));
        if (a.l4_ck_off) lds_put_be16(f, a.l4_ck_off, fold_complement(a.l4_sum + psum + (a.l4_dst ? S + D : 0u)));
    };
    // (2) fill, patch, copy out: one tile per workgroup (a persistent sweep
    // over the tiles writes at 0.65-0.72 of 8 TB/s against 0.77-0.83 for one
    // tile per workgroup, tools/writebench.hip, profiles/r05/writebench/)
    const uint32_t nf = g.frames(a.count);
    NEXG_BUILD_STAMP(1);
    fill();
    __syncthreads();
    NEXG_BUILD_STAMP(2);
    if (t < nf) patch(dw);
    __syncthreads();
    NEXG_BUILD_STAMP(3);
    build_copy_out<kT>(s_tile, a.out + g.first * P, nf * P);
    build_stamp_exit();
}

// ---- probe batches, frame per lane: k_build_lane ---------------------------
// The probe template as k_build_probe takes it, but each lane writes its own
// frame into the LDS tile as whole dwords of the tile, so that odd frame
// periods (icmp_ping's 47 B) cost no byte or halfword stores and there is no
// separate fill pass or patch barrier:
//  * the template dwords (the host's, followed by the next frame's first 8
//    bytes) are uniform: the device source and payload are merged into them
//    by scalar loads at compile-time offsets in every wave (no barrier);
//  * lane t's frame starts at tile byte t P, s = t P mod 4 bytes into its
//    first dword. Frame dword F[j] (frame bytes [4j, 4j + 4)) gets the lane's
//    destination and the checksums over it OR-ed in at the shape's
//    compile-time offsets; tile dword (t P >> 2) + j is
//    v_alignbyte(F[j], F[j - 1], 4 - s) (F[j] when s = 0);
//  * a lane writes the dwords from the first one that starts inside its frame
//    to the one holding its last byte; that last dword's other bytes are the
//    next frame's head (the Ethernet addresses: batch constants), so every
//    tile dword has exactly one writer and no lane needs a neighbour's bytes.
// Then one barrier and the tile leaves with 16-B non-temporal stores.
// MINP <= P <= MAXP: the frame dwords every lane writes are known at compile
// time (no exec mask per dword); the last one or two are per lane.
template <int FAM, int KIND, uint32_t MAXP, uint32_t MINP = 0>
__global__ __launch_bounds__(256) void k_build_lane(ProbeArgs a) {
    constexpr uint32_t DW = FAM == 4 ? 1u : 4u;              // destination dwords
    constexpr uint32_t SRC = FAM == 4 ? 26u : 22u;           // source address offset (= 2 mod 4)
    constexpr uint32_t DST = FAM == 4 ? 30u : 38u;           // destination offset (= 2 mod 4)
    constexpr uint32_t L3 = FAM == 4 ? 20u : 40u;
    constexpr uint32_t L4CK = 14u + L3 + (KIND == kL4Tcp ? 16u : 2u);  // L4 checksum offset
    constexpr uint32_t PAY = 14u + L3 + 8u;                  // ICMP payload offset (= 2 mod 4)
    constexpr bool L4DST = !(FAM == 4 && KIND == kL4Icmp);   // ICMPv4 sums the message alone
    constexpr uint32_t NF = MAXP / 4u + 3u;                  // frame dwords + the next frame's head
    static_assert(SRC % 4u == 2u && DST % 4u == 2u && PAY % 4u == 2u, "halfword-shifted fields");
    static_assert(KIND != kL4Icmp || MAXP >= PAY, "the period holds the ICMP header");
    extern __shared__ __attribute__((aligned(16))) uint8_t s_tile[];  // 256 x P + 16
    const uint32_t t = threadIdx.x, P = a.period;
    const BuildTile<kBuildTile> g(a.tile_order);
    const uint32_t nf = g.frames(a.count);
    uint32_t dw[DW];
    {  // this lane's destination in flight first (clamped: lanes past the end reload the last)
        const uint64_t i = g.lane();
        const auto* d4 = NEXG_GLOBAL(uint32_t, a.dst + 4u * DW * (i < a.count ? i : a.count - 1u));
#pragma unroll
        for (uint32_t k = 0; k < DW; k++) dw[k] = d4[k];
    }
    // uniform: the template with the batch's device source and payload merged
    uint32_t F[NF];
#pragma unroll
    for (uint32_t k = 0; k < NF; k++) F[k] = a.tmpl[k];
    uint32_t ssum = 0;
    {
        uint32_t sx[DW];
#pragma unroll
        for (uint32_t k = 0; k < DW; k++) sx[k] = uniform_u32(a.src)[k];
#pragma unroll
        for (uint32_t k = 0; k < DW; k++) {
            ssum += bswap16(sx[k] & 0xFFFFu) + bswap16(sx[k] >> 16);
            F[SRC / 4u + k] |= sx[k] << 16;
            F[SRC / 4u + k + 1u] |= sx[k] >> 16;
        }
    }
    uint64_t psum = 0;
    if (KIND == kL4Icmp && a.pay_len) {  // uniform: scalar loads and SALU only
        // (load_small_payload's v_alignbyte / v_perm forms put ~250 VALU
        // instructions in every wave; 64-bit scalar shifts, and the payload's
        // word sum as 256 x its LE halves, congruent mod 0xFFFF, stay scalar)
        constexpr uint32_t NP = (MAXP - PAY + 3u) / 4u;  // payload dwords a period can hold
        const uint64_t pa = reinterpret_cast<uint64_t>(a.payload);
        const uint32_t n = a.pay_len, sh = 8u * (uint32_t)(pa & 3u), nw = ((uint32_t)(pa & 3u) + n + 3u) >> 2;
        const uniform_u32_ptr src = uniform_u32(reinterpret_cast<const void*>(pa & ~3ull));
        uint32_t raw[NP + 1];
#pragma unroll
        for (uint32_t k = 0; k < NP + 1u; k++) raw[k] = k < nw ? src[k] : 0u;  // none past the payload
        uint32_t le = 0;
#pragma unroll
        for (uint32_t k = 0; k < NP; k++) {
            const uint32_t x = (uint32_t)((((uint64_t)raw[k + 1] << 32) | raw[k]) >> sh);
            const uint32_t w = 4u * k + 4u <= n ? x : 4u * k >= n ? 0u : x & ((1u << (8u * (n - 4u * k))) - 1u);
            le += (w & 0xFFFFu) + (w >> 16);
            if (PAY / 4u + k < NF) F[PAY / 4u + k] |= w << 16;
            if (PAY / 4u + k + 1u < NF) F[PAY / 4u + k + 1u] |= w >> 16;
        }
        psum = 256ull * le;  // the payload starts at an even offset: BE word sum (mod 0xFFFF)
    }
    const uint64_t S = ssum;
    if (!L4DST) {  // ICMPv4: one checksum for the batch
        const uint32_t ck = fold_complement(a.l4_sum + psum);
        F[L4CK / 4u] |= bswap16(ck) << (8u * (L4CK % 4u));
    }
    if (t < nf) {
        // the lane's frame: destination (network-order bytes, LE halves x 256) and checksums
        uint32_t dsum = 0;
#pragma unroll
        for (uint32_t k = 0; k < DW; k++) {
            dsum += halves(dw[k]);
            F[DST / 4u + k] |= dw[k] << 16;
            F[DST / 4u + k + 1u] |= dw[k] >> 16;
        }
        const uint64_t D = 256ull * dsum;
        if (FAM == 4) F[6] |= bswap16(fold_complement(a.ip_sum + S + D));  // bytes 24-25
        if (L4DST) F[L4CK / 4u] |= bswap16(fold_complement(a.l4_sum + psum + S + D)) << (8u * (L4CK % 4u));
        // frame start s' = 1..4 bytes into tile dword qb = (t P - s') / 4 (s' = 4
        // when t P is dword-aligned), so tile dword qb + j = frame bytes
        // [4j - s', 4j - s' + 4) = v_alignbyte(F[j], F[j - 1], (4 - s') mod 4) for
        // every lane alike; j = 0 is the previous frame's (its writer's), j runs
        // to the dword holding byte P - 1: j <= (P - 1 + s') / 4, which is
        // lane-dependent only for the last one or two j
        const uint32_t b0 = t * P, s1 = ((b0 + 3u) & 3u) + 1u, sh = (4u - s1) & 3u;
        const uint32_t jend = (P - 1u + s1) >> 2, jlo = P >> 2, jhi = (P + 3u) >> 2;
        uint32_t* const tw = reinterpret_cast<uint32_t*>(s_tile) + ((b0 + 4u - s1) >> 2) - 1u;
        // fully unrolled (a `break` here rolls the loop back up with dynamic
        // register indexing of F): j <= MINP / 4 unconditionally, then uniform
        // and per-lane guards
#pragma unroll
        for (uint32_t j = 1; j < NF; j++) {
            const uint32_t v = __builtin_amdgcn_alignbyte(F[j], F[j - 1u], sh);
            if (j <= MINP / 4u) tw[j] = v;
            else if (j <= jlo) tw[j] = v;
            else if (j <= jhi && j <= jend) tw[j] = v;
        }
    }
    build_finish<true>(s_tile, g, nf, a.out, P);
}

// ---- host: probe templates (the bytes the per-lane builders write, with the
// destination, checksums and payload zero) and their base sums
namespace {
void put_be16(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 8);
    p[1] = (uint8_t)v;
}
uint64_t be_halves(const uint8_t* p, uint32_t n) {  // BE words of n (even) bytes
    uint64_t s = 0;
    for (uint32_t k = 0; k < n; k += 2) s += ((uint32_t)p[k] << 8) | p[k + 1];
    return s;
}
void probe_eth(uint8_t* t, const uint8_t* dmac, const uint8_t* smac, uint32_t ethertype) {
    for (int k = 0; k < 6; k++) {
        t[k] = dmac[k];
        t[6 + k] = smac[k];
    }
    put_be16(t + 12, ethertype);
}
// IPv4 header (builder/ipv4.rs:94-170) with destination and checksum zero;
// returns the BE word sum of the rest (the header checksum's base)
uint64_t probe_ipv4(uint8_t* h, uint32_t tos, uint32_t total, uint32_t id, uint32_t flags, uint32_t ttl,
                    uint32_t proto, const uint8_t* src) {
    h[0] = 0x45; h[1] = (uint8_t)tos;
    put_be16(h + 2, total);
    put_be16(h + 4, id);
    put_be16(h + 6, (flags & 7u) << 13);
    h[8] = (uint8_t)ttl; h[9] = (uint8_t)proto;
    put_be16(h + 10, 0);
    for (int k = 0; k < 4; k++) { h[12 + k] = src[k]; h[16 + k] = 0; }
    return be_halves(h, 20);
}
// IPv6 header (builder/ipv6.rs:89-152) with the destination zero
void probe_ipv6(uint8_t* h, uint32_t tc, uint32_t flow, uint32_t plen, uint32_t next, uint32_t hop, const uint8_t* src) {
    const uint32_t fl = flow & 0xFFFFFu;
    h[0] = (uint8_t)(0x60u | (tc >> 4)); h[1] = (uint8_t)(((tc & 0xFu) << 4) | (fl >> 16));
    h[2] = (uint8_t)(fl >> 8); h[3] = (uint8_t)fl;
    put_be16(h + 4, plen);
    h[6] = (uint8_t)next; h[7] = (uint8_t)hop;
    for (int k = 0; k < 16; k++) { h[8 + k] = src[k]; h[24 + k] = 0; }
}

bool probe_launch_ok(uint32_t flen, uint32_t period, uint32_t pay_len, const uint8_t* out) {
    return NEXG_PROBE_TEMPLATE && period <= kProbeMaxP && flen <= period && pay_len <= kSmallPay &&
           (reinterpret_cast<uint64_t>(out) & 15u) == 0;
}

// Probe kernel shape (measurement overrides, read once): NEXG_PROBE_WAVES
// waves per workgroup (1 or 4), NEXG_PROBE_WGS workgroups per CU set by the
// dynamic LDS (160 KiB per CU; 0 = only the tile's LDS).
uint32_t probe_env(const char* name, uint32_t def, uint32_t lo, uint32_t hi) {
#ifdef NEXG_AB_KNOBS
    const char* e = getenv(name);
#else
    (void)name;
    const char* e = nullptr;  // product build: no environment overrides
#endif
    const long x = e ? strtol(e, nullptr, 10) : -1;
    return x >= (long)lo && x <= (long)hi ? (uint32_t)x : def;
}
uint32_t probe_waves() {
    static const uint32_t v = probe_env("NEXG_PROBE_WAVES", 4u, 1u, 4u) == 1u ? 1u : 4u;
    return v;
}
uint32_t probe_wgs_per_cu() {
    // 1 or 2 per CU would ask more than a workgroup's 64 KiB of LDS: 3 at least
    static const uint32_t v = [] { const uint32_t w = probe_env("NEXG_PROBE_WGS", 5u, 0u, 64u);
                                   return w && w < 3u ? 3u : w; }();
    return v;
}

// kProbeMaxP template bytes as the kernel argument's little-endian dwords
void pack_template(ProbeArgs& a, const uint8_t* bytes) {
    for (uint32_t k = 0; k < kProbeMaxP / 4; k++)
        a.tmpl[k] = (uint32_t)bytes[4 * k] | ((uint32_t)bytes[4 * k + 1] << 8) | ((uint32_t)bytes[4 * k + 2] << 16) |
                    ((uint32_t)bytes[4 * k + 3] << 24);
}

// fault injection for the error-path test (tests/test_gpu_probe_batches.py): knobs build only
bool probe_fail_injected() {
#ifdef NEXG_AB_KNOBS
    return probe_env("NEXG_PROBE_FAIL", 0u, 0u, 1u) == 1u;
#else
    return false;
#endif
}

// tmpl: one period (P bytes, zero past the frame), one tile per workgroup
hipError_t launch_probe(ProbeArgs& a, const uint8_t* tmpl, uint32_t dw, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    const uint32_t P = a.period;
    pack_template(a, tmpl);
    const uint32_t waves = probe_waves(), kT = 64u * waves;
    dim3 g;
    if (hipError_t e = build_grid(a.count, kT, g)) return e;
    if (probe_fail_injected()) return hipErrorInvalidValue;
    const uint32_t need = (P + 15u) / 16u;  // 16-B chunks per lane, rounded to an instantiated KCH
    const uint32_t kch = need <= 3u ? 3u : need <= 6u ? need : 8u;
    const uint32_t lds = build_lds_for_wgs(kch * 16u * kT + 2u * kProbeMaxP + 32u, probe_wgs_per_cu());
    a.tile_order = probe_tile_order();
    const dim3 b(kT);
#define NEXG_PROBE_LAUNCH(DW, K)                                                     \
    do {                                                                             \
        if (waves == 1u) hipLaunchKernelGGL((k_build_probe<DW, K, 1>), g, b, lds, s, a); \
        else hipLaunchKernelGGL((k_build_probe<DW, K, 4>), g, b, lds, s, a);             \
    } while (0)
    if (dw == 1) {
        if (kch == 3) NEXG_PROBE_LAUNCH(1, 3); else if (kch == 4) NEXG_PROBE_LAUNCH(1, 4);
        else if (kch == 5) NEXG_PROBE_LAUNCH(1, 5); else if (kch == 6) NEXG_PROBE_LAUNCH(1, 6);
        else NEXG_PROBE_LAUNCH(1, 8);
    } else {
        if (kch == 3) NEXG_PROBE_LAUNCH(4, 3); else if (kch == 4) NEXG_PROBE_LAUNCH(4, 4);
        else if (kch == 5) NEXG_PROBE_LAUNCH(4, 5); else if (kch == 6) NEXG_PROBE_LAUNCH(4, 6);
        else NEXG_PROBE_LAUNCH(4, 8);
    }
#undef NEXG_PROBE_LAUNCH
    return hipGetLastError();
}

// Workgroups per CU of k_build_lane, set by its dynamic LDS (NEXG_LANE_WGS
// overrides in the knobs build; 0 = the tile's LDS only): icmp_ping's 47-B
// batch, 16M frames, in one process (profiles/r06/lane/lane_ab2.log): 0.693
// of 8 TB/s written at 3 per CU, 0.663-0.667 at 4, 0.662 at 5, 0.654-0.661
// at 6, against 0.58 for k_build_l4
uint32_t lane_wgs_per_cu() {
    static const uint32_t v = probe_env("NEXG_LANE_WGS", 3u, 0u, 64u);
    return v;
}

// k_build_lane: tmpl = one period P <= kLaneMaxP; the kernel's template is the
// period followed by its first 8 bytes (the next frame's head)
constexpr uint32_t kLaneMaxP = 96;
bool lane_launch_ok(uint32_t flen, uint32_t period, uint32_t pay_len, const uint8_t* out) {
    return period <= kLaneMaxP && flen <= period && pay_len <= kSmallPay && (reinterpret_cast<uint64_t>(out) & 15u) == 0;
}

hipError_t launch_lane(ProbeArgs& a, const uint8_t* tmpl, int fam, int kind, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    const uint32_t P = a.period;
    uint8_t d[kProbeMaxP] = {0};
    for (uint32_t k = 0; k < P; k++) d[k] = tmpl[k];
    for (uint32_t k = 0; k < 8u; k++) d[P + k] = tmpl[k];
    pack_template(a, d);
    dim3 g;
    if (hipError_t e = build_grid(a.count, kBuildTile, g)) return e;
    if (probe_fail_injected()) return hipErrorInvalidValue;
    // dynamic LDS: the tile (+ the last lane's tail dword), raised to set the
    // workgroups per CU (as k_build_probe)
    const uint32_t lds = build_lds_for_wgs(kBuildTile * P + 16u, lane_wgs_per_cu());
    a.tile_order = build_tile_order();
    const dim3 b(kBuildTile);
    // the unrolled frame-dword count follows the period: instances for
    // 44-48 B (icmp_ping, 47 B), 64-68 B (its IPv6 form, 67 B; tcp_ping, 66 B)
    // and any period up to 96 B
    const bool p48 = P >= 44u && P <= 48u, p68 = P >= 64u && P <= 68u;
#define NEXG_LANE(F, K)                                                                           \
    do {                                                                                          \
        if (p68) hipLaunchKernelGGL((k_build_lane<F, K, 68, 64>), g, b, lds, s, a);               \
        else hipLaunchKernelGGL((k_build_lane<F, K, kLaneMaxP>), g, b, lds, s, a);                \
    } while (0)
    if (kind == kL4Icmp && fam == 4 && p48) hipLaunchKernelGGL((k_build_lane<4, kL4Icmp, 48, 44>), g, b, lds, s, a);
    else if (kind == kL4Icmp && fam == 4) NEXG_LANE(4, kL4Icmp);
    else if (kind == kL4Icmp) return hipErrorInvalidValue;  // ICMPv6: try_probe_l4 never sends it here, no instance
    else if (fam == 4) NEXG_LANE(4, kL4Tcp);
    else NEXG_LANE(6, kL4Tcp);
#undef NEXG_LANE
    return hipGetLastError();
}
}  // namespace

// udp_ping's IPv6 probe batch (src_shared, dst per frame): builder/udp.rs:67-95
// over IPv6 (udp.rs:480-505) as k_build_udp6 sums it
bool try_probe_udp6(const nexg_udp6_build& p, uint8_t* out, uint32_t out_stride, hipStream_t s, hipError_t& e) {
    const uint32_t flen = 62u + p.payload_len;
    if (!probe_launch_ok(flen, out_stride, p.payload_len, out)) return false;
    ProbeArgs a{};
    uint8_t t[kProbeMaxP] = {0};
    const uint8_t zero[16] = {0};
    const uint32_t ulen = 8u + p.payload_len;
    probe_eth(t, p.def_dst_mac, p.def_src_mac, 0x86DD);
    probe_ipv6(t + 14, p.traffic_class, p.flow_label, ulen, 17, p.hop_limit, zero);
    uint8_t* u = t + 54;
    put_be16(u, p.def_src_port); put_be16(u + 2, p.def_dst_port); put_be16(u + 4, ulen); put_be16(u + 6, 0);
    a.l4_sum = 17u + ulen + (uint64_t)p.def_src_port + p.def_dst_port + ulen;
    a.src = p.src_ip; a.src_off = 22; a.ip_src = 0;
    a.dst = p.dst_ip; a.dst_off = 38;
    a.payload = p.payload; a.pay_off = 62; a.pay_len = p.payload_len;
    a.out = out; a.count = p.count; a.period = out_stride;
    a.l4_ck_off = 60; a.l4_dst = 1;
    e = launch_probe(a, t, 4, s);
    return true;
}

// tcp_ping / icmp_ping probe batches (ip.src_shared, dst per frame): the
// layouts and sums of k_build_l4
bool try_probe_l4(const L4Args& l, int kind, uint8_t* out, uint32_t out_stride, hipStream_t s, hipError_t& e) {
    const nexg_ip_build& ip = l.ip;
    const bool v4 = ip.family == 4;
    const uint32_t l3 = v4 ? 20u : 40u;
    const uint32_t l4_hdr = kind == kL4Tcp ? 20u + l.opt_padded : 8u;
    const uint32_t l4_len = l4_hdr + l.payload_len;
    const uint32_t flen = 14u + l3 + l4_len;
    // icmp_ping IPv4: k_build_lane (whole-dword tile writes at any frame
    // period); tcp_ping: k_build_probe (0.72-0.89 of 8 TB/s written, round 5).
    // Measurement overrides (knobs build): NEXG_PROBE_ICMP = 1 the template
    // kernel, 2 the per-lane k_build_l4; NEXG_PROBE_LANE_TCP = 1 k_build_lane
    // for tcp_ping (no payload)
    static const uint32_t icmp_path = probe_env("NEXG_PROBE_ICMP", 0u, 0u, 2u);
    static const bool tcp_lane = probe_env("NEXG_PROBE_LANE_TCP", 0u, 0u, 1u) == 1u;
    // (ICMPv6's 67 B ran 0.634-0.637 in k_build_lane against 0.656 per lane in
    // k_build_l4, tcp_ping 0.69-0.70 against 0.80 in k_build_probe: both stay)
    const bool lane = kind == kL4Icmp ? icmp_path == 0u && v4 && lane_launch_ok(flen, out_stride, l.payload_len, out)
                                      : tcp_lane && l.payload_len == 0 && lane_launch_ok(flen, out_stride, 0, out);
    if (!lane && ((kind != kL4Tcp && icmp_path != 1u) || !probe_launch_ok(flen, out_stride, l.payload_len, out)))
        return false;
    ProbeArgs a{};
    uint8_t t[kProbeMaxP] = {0};
    const uint8_t zero[16] = {0};
    const uint32_t proto = kind == kL4Tcp ? 6u : (v4 ? 1u : 58u);
    probe_eth(t, ip.def_dst_mac, ip.def_src_mac, v4 ? 0x0800 : 0x86DD);
    if (v4) a.ip_sum = probe_ipv4(t + 14, ip.tos, 20u + l4_len, ip.def_ip_id, ip.ip_flags, ip.ttl, proto, zero);
    else probe_ipv6(t + 14, ip.tos, ip.flow_label, l4_len, proto, ip.ttl, zero);
    uint8_t* h = t + 14 + l3;
    uint64_t sum;
    if (kind == kL4Tcp) {
        const uint32_t w6 = ((l4_hdr / 4u) << 12) | (l.flags & 0xFFu);
        put_be16(h, l.def_sport); put_be16(h + 2, l.def_dport);
        put_be16(h + 4, l.def_seq >> 16); put_be16(h + 6, l.def_seq & 0xFFFFu);
        put_be16(h + 8, l.def_ack >> 16); put_be16(h + 10, l.def_ack & 0xFFFFu);
        put_be16(h + 12, w6); put_be16(h + 14, l.window); put_be16(h + 16, 0); put_be16(h + 18, l.urg);
        for (uint32_t k = 0; k < l.opt_padded; k++) h[20 + k] = l.options[k];
        sum = (uint64_t)l.def_sport + l.def_dport + (l.def_seq >> 16) + (l.def_seq & 0xFFFFu) + (l.def_ack >> 16) +
              (l.def_ack & 0xFFFFu) + w6 + l.window + l.urg + l.opt_sum;
        a.l4_ck_off = 14 + l3 + 16;
    } else {
        const uint32_t w0 = (l.icmp_type << 8) | l.icmp_code;
        put_be16(h, w0); put_be16(h + 2, 0); put_be16(h + 4, l.def_ident); put_be16(h + 6, l.def_seqno);
        sum = (uint64_t)w0 + l.def_ident + l.def_seqno;
        a.l4_ck_off = 14 + l3 + 2;
    }
    const bool pseudo = !v4 || kind == kL4Tcp;  // ICMPv4 sums the message alone
    if (pseudo) sum += proto + l4_len;
    a.l4_sum = sum;
    a.l4_dst = pseudo ? 1u : 0u;
    a.ip_ck_off = v4 ? 24u : 0u;
    a.ip_src = v4 ? 1u : 0u;
    a.src = ip.src_ip; a.src_off = v4 ? 26u : 22u;
    a.dst = ip.dst_ip; a.dst_off = v4 ? 30u : 38u;
    a.payload = l.payload; a.pay_off = 14 + l3 + l4_hdr; a.pay_len = l.payload_len;
    a.out = out; a.count = l.count; a.period = out_stride;
    e = lane ? launch_lane(a, t, ip.family, kind, s) : launch_probe(a, t, v4 ? 1u : 4u, s);
    return true;
}

}  // namespace nexg

#endif  // !NEXG_PROBE_TIMING || NEXG_BUILD_ONE_UNIT
