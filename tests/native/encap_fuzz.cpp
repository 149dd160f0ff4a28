// TEST INFRASTRUCTURE ONLY: the per-frame core of nexg_encap_plan /
// nexg_encap_frames (nex_amd/csrc/encap_core.hpp: shape, header template and
// patches, chunk copy, checksum, header chunks), built for the host with
// AddressSanitizer + UBSan.
//
//   encap_fuzz FILE   the corpus as tests/test_encap_core.py writes it: per case
//                     a nexg_tunnels, u32 source phase mask, u32 destination
//                     phase mask, u32 frame count, then per frame u32 length,
//                     u32 tunnel number, u32 index in the table, u32 flow hash,
//                     u32 expected output length, u32 extent accepted (0: the
//                     frame's extent leaves the data; no bytes follow for it and
//                     its source address is one nothing is allocated at), the
//                     bytes, the bytes expected and the 8-byte row expected.
// Every frame is run at each of the 16 x 16 byte phases the masks name: the
// inner frame in a heap allocation that covers exactly the 16-B aligned blocks
// overlapping it, the output in one that covers exactly the blocks overlapping
// [lo, next), next = lo + the output length + a pad of 0..15, so any read or
// write outside them is a sanitizer report. The slack bytes of the output's
// blocks hold 0xA5 and must still hold it afterwards, the pad bytes must be 0.
// Each run is repeated with out_cap in the middle of the frame: the bytes below
// it are the expected ones, the bytes from it on untouched. Exit 0 = clean and
// equal.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../nex_amd/csrc/encap_core.hpp"

namespace {

// k_encap_frames' body (encap_core.hpp's encap_group_lane, the function the
// kernel calls) over one frame, the group's lanes one after the other. The
// lanes run twice: the first round collects every lane's share of the sum
// (its reduce gives 0 back), the second is given the group's sum, as the
// kernel's shuffles give it, and stores every chunk again with the checksum in
// place. Both rounds run under the sanitizers.
nexg_encapped run(const nexg::EncapSet& set, const nexg::EncapJob& job, uint32_t hash, uint8_t* out_data, uint64_t out_cap) {
    using namespace nexg;
    uint32_t sum = 0;
    nexg_encapped row{};
    for (uint32_t lane = 0; lane < kEncapLanes; lane++)
        (void)encap_group_lane(set.t, set.n, job, out_cap, out_data, lane, [&] { return hash; },
                               [&](uint32_t v) { sum += v; return 0u; });
    for (uint32_t lane = 0; lane < kEncapLanes; lane++) {
        const nexg_encapped r = encap_group_lane(set.t, set.n, job, out_cap, out_data, lane, [&] { return hash; },
                                                 [&](uint32_t) { return sum; });
        if (lane && memcmp(&r, &row, sizeof(r)) != 0) row.status = 0xEE;  // every lane returns the same row
        if (!lane) row = r;
    }
    return row;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    long bad = 0, frames = 0, cases = 0, runs = 0;
    nexg_tunnels set;
    while (fread(&set, sizeof(set), 1, fp) == 1) {
        if (nexg::check_tunnels(&set)) return 3;
        nexg::EncapSet es;
        nexg::prepare_tunnels(set, es);
        uint32_t head[3];
        if (fread(head, 4, 3, fp) != 3) return 2;
        const uint32_t sphases = head[0], dphases = head[1], count = head[2];
        cases++;
        std::vector<uint8_t> in, want;
        for (uint32_t i = 0; i < count; i++) {
            uint32_t fh[6];
            nexg_encapped want_row;
            if (fread(fh, 4, 6, fp) != 6) return 2;
            const uint32_t t = fh[1], index = fh[2], hash = fh[3], out_len = fh[4];
            const bool ext = fh[5] != 0;
            const uint32_t len = ext ? fh[0] : 0u;  // frame_extent gives length 0 with a rejected extent
            in.resize(len);
            want.resize(out_len);
            if (len && fread(in.data(), 1, len, fp) != len) return 2;
            if (out_len && fread(want.data(), 1, out_len, fp) != out_len) return 2;
            if (fread(&want_row, sizeof(want_row), 1, fp) != 1) return 2;
            frames++;
            for (uint32_t sp = 0; sp < 16; sp++) {
                if (!(sphases >> sp & 1u)) continue;
                const size_t sbytes = len ? (sp + len + 15u) / 16u * 16u : 16u;
                uint8_t* sblock = static_cast<uint8_t*>(aligned_alloc(16, sbytes));
                if (!sblock) return 2;
                memset(sblock, 0x5A, sbytes);
                // a rejected extent's offset is any number: an address far from every allocation, at every phase
                uint8_t* f = ext ? sblock + sp : reinterpret_cast<uint8_t*>(uintptr_t(0x1000) + sp);
                if (len) memcpy(f, in.data(), len);
                for (uint32_t dp = 0; dp < 16; dp++) {
                    if (!(dphases >> dp & 1u)) continue;
                    const uint32_t pad = (sp * 5u + dp * 3u + len) & 15u;
                    const uint64_t lo = 16u + dp, next = lo + out_len + pad;  // one block in front stays 0xA5
                    const size_t dbytes = (next + 15u) / 16u * 16u;
                    for (int cut = 0; cut < 2; cut++) {
                        if (cut && out_len < 2) continue;
                        const uint64_t cap = cut ? lo + out_len / 2u : dbytes;
                        // with a cap the blocks from the one that holds it on are not there at all
                        const size_t have = cut ? (cap + 15u) / 16u * 16u : dbytes;
                        uint8_t* out = static_cast<uint8_t*>(aligned_alloc(16, have));
                        if (!out) return 2;
                        memset(out, 0xA5, have);
                        nexg::EncapJob job{};
                        job.live = true;
                        job.ext = ext;
                        job.t = t;
                        job.len = len;
                        job.index = index;
                        job.src = reinterpret_cast<uint64_t>(f);
                        job.lo = lo;
                        job.next = next;
                        const nexg_encapped got = run(es, job, hash, out, cap);
                        runs++;
                        bool same = true;
                        if (!cut) same = memcmp(&got, &want_row, sizeof(got)) == 0;
                        for (size_t k = 0; k < have; k++) {
                            uint8_t w = 0xA5;
                            if (k >= lo && k < next && k < cap) w = k < lo + out_len ? want[k - lo] : 0;
                            // the checksum of a cut frame covers what was copied: its two bytes are not compared
                            if (cut && want_row.l4_csum && k >= lo + want_row.hdr_len - 10u && k < lo + want_row.hdr_len - 8u) continue;
                            if (out[k] != w) same = false;
                        }
                        if (!same && bad++ < 5)
                            fprintf(stderr, "case %ld frame %u (len %u, tunnel %u) phases %u -> %u cut %d: row {%u, %u, %u, %u, %04x} expected {%u, %u, %u, %u, %04x}\n",
                                    cases, i, len, t, sp, dp, cut, got.status, got.tunnel, got.hdr_len, got.src_port, got.l4_csum,
                                    want_row.status, want_row.tunnel, want_row.hdr_len, want_row.src_port, want_row.l4_csum);
                        free(out);
                    }
                }
                free(sblock);
            }
        }
    }
    fclose(fp);
    printf("cases %ld frames %ld runs %ld mismatches %ld\n", cases, frames, runs, bad);
    return bad ? 1 : 0;
}
