// nexg_dns.hip — the DNS message pass on gfx950 (include/nexg.h): a second
// pass over a batch already parsed with NEXG_OUT_RECORD that walks each UDP
// payload as DnsPacket::try_from_buf does (dns.rs:1166-1259, with
// DnsQueryPacket::from_buf_mut dns.rs:752-790 and
// DnsResponsePacket::from_buf_mut dns.rs:904-945). nexg_dns_batch writes one
// 32-B summary per frame and the entry counts' prefix sums (a CSR-style row
// table in two levels: per frame within its 256-frame tile, per tile within
// the batch); nexg_dns_entries walks again and stores one 16-B entry per query
// / resource record at the position the sums give. Positions come from scans
// alone (block_excl_scan and k_tile_scan of table_kernels.hpp): no atomics, the
// same output on every run.
#include "table_kernels.hpp"

namespace nexg {

static_assert(sizeof(nexg_dns) == 32, "nexg_dns is 32 bytes (include/nexg.h)");
static_assert(sizeof(nexg_dns_entry) == 16, "nexg_dns_entry is 16 bytes (include/nexg.h)");
static_assert(sizeof(nexg_dns_option) == 8, "nexg_dns_option is 8 bytes (include/nexg.h)");

struct DnsWalk {
    uint32_t n_q, n_an, n_ns, n_ar;  // queries.len(), responses.len(), authorities.len(), additionals.len()
    uint32_t pos;                    // the cursor: DnsPacket.payload starts here
    bool fail;                       // parse_queries returned None ("DNS query section")
};

__device__ __forceinline__ uint32_t dns_be16(const uint8_t* m, uint32_t p) {
    const auto* g = NEXG_GLOBAL(uint8_t, m);
    return ((uint32_t)g[p] << 8) | g[p + 1];
}

// The walk over message m[0, n), n >= 12, from byte 12: up to `cq` queries,
// then up to `c1`, `c2`, `c3` records. Every load is of a byte p < n, checked
// against n from the bytes themselves, and every loop iteration advances pos by
// at least 1 with pos <= n <= 65535: it terminates on any bytes and any counts.
// EMIT: entry k of the walk goes to ent[base + k] when that index is below cap.
template <bool EMIT>
__device__ __forceinline__ DnsWalk dns_walk(const uint8_t* m, uint32_t n, uint32_t cq, uint32_t c1, uint32_t c2,
                                            uint32_t c3, nexg_dns_entry* ent, uint64_t base, uint64_t cap) {
    const auto* g = NEXG_GLOBAL(uint8_t, m);
    DnsWalk w{0u, 0u, 0u, 0u, 12u, false};
    uint32_t pos = 12u;
    uint64_t k = base;
    for (uint32_t q = 0; q < cq && !w.fail; q++) {
        const uint32_t start = pos;
        // dns.rs:755-770: a length byte is a plain length, 0xC0..0xFF included
        for (;;) {
            if (pos >= n) {
                w.fail = true;
                break;
            }
            const uint32_t L = g[pos];
            pos++;
            if (L == 0u) break;
            if (n - pos < L) {
                w.fail = true;
                break;
            }
            pos += L;
        }
        if (w.fail || n - pos < 4u) {  // dns.rs:772-774
            w.fail = true;
            break;
        }
        if (EMIT) {
            if (k < cap) {
                const u32x4 e{start << 16, dns_be16(m, pos) | (dns_be16(m, pos + 2u) << 16), 0u, pos - start};
                __builtin_nontemporal_store(e, reinterpret_cast<u32x4*>(ent) + k);
            }
            k++;
        }
        pos += 4u;
        w.n_q++;
    }
    if (!w.fail) {
#pragma unroll
        for (uint32_t s = 1; s <= 3u; s++) {
            const uint32_t c = s == 1u ? c1 : s == 2u ? c2 : c3;
            uint32_t got = 0;
            for (; got < c; got++) {
                if (n - pos < 12u) break;  // dns.rs:905-907: the section ends, the cursor stays
                const uint32_t dl = dns_be16(m, pos + 10u);
                const uint32_t room = n - pos - 12u;
                if (EMIT) {
                    if (k < cap) {
                        const uint32_t ttl = (dns_be16(m, pos + 6u) << 16) | dns_be16(m, pos + 8u);
                        const u32x4 e{s | (dl > room ? 0x100u : 0u) | (pos << 16),
                                      dns_be16(m, pos + 2u) | (dns_be16(m, pos + 4u) << 16), ttl,
                                      dns_be16(m, pos) | (dl << 16)};
                        __builtin_nontemporal_store(e, reinterpret_cast<u32x4*>(ent) + k);
                    }
                    k++;
                }
                pos += 12u + (dl < room ? dl : room);  // dns.rs:929-931
            }
            if (s == 1u) w.n_an = got;
            else if (s == 2u) w.n_ns = got;
            else w.n_ar = got;
        }
    }
    w.pos = pos;
    return w;
}

// k_dns_walk: one lane per frame, 256-frame workgroups. Per lane the two 16-B
// quarters of its record that hold flags / payload_off / payload_len and the
// ports, the walk's dependent byte loads, then the workgroup's exclusive scan
// of the per-lane entry counts (block_excl_scan: lanes past the batch take part
// with count 0) and the 32-B summary as two adjacent 16-B non-temporal stores:
// consecutive lanes write consecutive addresses.
__global__ __launch_bounds__(256) void k_dns_walk(ParseArgs a, const nexg_record* recs, uint32_t any_udp, uint32_t port,
                                                  nexg_dns* out, uint64_t* tile_first) {
    __shared__ uint32_t s_w[4];
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    const bool valid = idx < a.count;
    uint32_t status = 0, f8 = 0, poff = 0, plen = 0, id = 0, hflags = 0, qd = 0, an = 0, ns = 0, ar = 0;
    DnsWalk w{0u, 0u, 0u, 0u, 0u, false};
    if (valid) {
        const RecQuarter<0> q0 = rec_quarter<0>(recs + idx);
        const RecQuarter<2> q2 = rec_quarter<2>(recs + idx);
        uint64_t off;
        uint32_t len;
        const bool ext = frame_extent(a, idx, off, len);
        const uint32_t flags = rec_dw<kRecFlags>(q0), ports = rec_dw<kRecPorts>(q2);
        const uint32_t sport = rec_sport(ports), dport = rec_dport(ports);
        rec_payload(rec_dw<kRecPayload>(q0), poff, plen);
        // the record is caller memory: clamp to the frame's own extent before any load
        const bool cand = ext && rec_status(flags) == 0u && (flags & NEXG_L_UDP) && plen > 0u &&
                          poff + plen <= len && (any_udp || sport == port || dport == port);
        if (!cand) {
            poff = plen = 0u;
        } else if (plen < 12u) {  // dns.rs:1167-1173
            status = NEXG_ERR_BUFFER_TOO_SHORT;
            poff = plen = 0u;
        } else {
            const uint8_t* m = a.data + off + poff;
            f8 = 1u;
            id = dns_be16(m, 0u), hflags = dns_be16(m, 2u);
            qd = dns_be16(m, 4u), an = dns_be16(m, 6u), ns = dns_be16(m, 8u), ar = dns_be16(m, 10u);
            w = dns_walk<false>(m, plen, qd, an, ns, ar, nullptr, 0ull, 0ull);
            if (w.fail) {  // dns.rs:1228-1231: the header is kept, nothing else
                status = NEXG_ERR_MALFORMED;
                w = DnsWalk{0u, 0u, 0u, 0u, 0u, true};
            } else if (w.n_an < an || w.n_ns < ns || w.n_ar < ar) {
                f8 |= 2u;
            }
        }
    }
    const uint32_t v = w.n_q + w.n_an + w.n_ns + w.n_ar;  // <= 65535 / 5 per lane: a tile's total fits 32 bits
    uint32_t total;
    const uint32_t first = block_excl_scan(v, s_w, total);
    if (threadIdx.x == 0) tile_first[blockIdx.x] = total;
    if (!valid) return;
    const u32x4 lo{status | (f8 << 8) | (poff << 16), plen | (id << 16), hflags | (qd << 16), an | (ns << 16)};
    const u32x4 hi{ar | (w.n_q << 16), w.n_an | (w.n_ns << 16), w.n_ar | (w.pos << 16), first};
    __builtin_nontemporal_store(lo, reinterpret_cast<u32x4*>(out) + idx * 2u);
    __builtin_nontemporal_store(hi, reinterpret_cast<u32x4*>(out) + idx * 2u + 1u);
}

// k_dns_fill: one lane per frame; the same walk with the stores switched on.
// The summary and tile_first are caller memory: the message is clamped to the
// frame's own extent, the walk re-checks every bound from the bytes and stops
// after the summary's own counts, and an entry is stored only at an index
// below cap (the index is 64-bit: a wrapped sum is still compared with cap).
__global__ __launch_bounds__(256) void k_dns_fill(ParseArgs a, const nexg_dns* dns, const uint64_t* tile_first,
                                                  nexg_dns_entry* entries, uint64_t cap) {
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    if (idx >= a.count) return;
    const uint8_t* sp = reinterpret_cast<const uint8_t*>(dns + idx);
    const uint4 lo = load16<true>(sp), hi = load16<true>(sp + 16);
    if ((lo.x & 0xFFu) != 0u || !(lo.x & 0x100u)) return;  // status != 0 or no candidate
    uint64_t off;
    uint32_t len;
    if (!frame_extent(a, idx, off, len)) return;
    uint32_t mo = lo.x >> 16, n = lo.y & 0xFFFFu;
    mo = mo < len ? mo : len;
    n = n < len - mo ? n : len - mo;
    if (n < 12u) return;
    const uint64_t base = NEXG_GLOBAL(uint64_t, tile_first)[idx >> 8] + hi.w;
    (void)dns_walk<true>(a.data + off + mo, n, hi.x >> 16, hi.y & 0xFFFFu, hi.y >> 16, hi.z & 0xFFFFu, entries, base,
                         cap);
}

hipError_t launch_dns(const ParseArgs& a, const nexg_record* recs, uint32_t any_udp, uint32_t port, nexg_dns* out,
                      uint64_t* tile_first, hipStream_t s) {
    const uint64_t tiles = (a.count + kTile - 1) / kTile;
    if (tiles)
        hipLaunchKernelGGL(k_dns_walk, dim3((uint32_t)tiles), dim3(kTile), 0, s, a, recs, any_udp, port, out,
                           tile_first);
    // the tile totals become their exclusive scan in place, the batch total behind them (tiles == 0: tile_first[0] = 0)
    hipLaunchKernelGGL(k_tile_scan<uint64_t>, dim3(1), dim3(kTile), 0, s, tile_first, tiles, tile_first + tiles);
    return hipGetLastError();
}

hipError_t launch_dns_entries(const ParseArgs& a, const nexg_dns* dns, const uint64_t* tile_first,
                              nexg_dns_entry* entries, uint64_t cap, hipStream_t s) {
    if (a.count == 0 || cap == 0) return hipSuccess;
    const uint64_t tiles = (a.count + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_dns_fill, dim3((uint32_t)tiles), dim3(kTile), 0, s, a, dns, tile_first, entries, cap);
    return hipGetLastError();
}

}  // namespace nexg
