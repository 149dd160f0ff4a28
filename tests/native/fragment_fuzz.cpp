// TEST INFRASTRUCTURE ONLY: the per-frame core of nexg_fragment_plan /
// nexg_fragment_frames (nex_amd/csrc/fragment_core.hpp: shape, header templates,
// option walk, piece copy, table), built for the host with AddressSanitizer +
// UBSan.
//
//   fragment_fuzz FILE   the corpus as tests/test_fragment_core.py writes it: per
//                        case u32 mtu, flags, align, source phase mask,
//                        destination phase mask, frame count; per frame u32
//                        length, extent accepted (0: the frame's extent leaves
//                        the data; no bytes follow for it and its source address
//                        is one nothing is allocated at), index in the table,
//                        index of its first output frame, output frames, then
//                        the 16-byte row expected, the bytes, and per output
//                        frame u32 length and the bytes expected.
// Every frame is run at each of the 16 x 16 byte phases the masks name: the
// frame in a heap allocation that covers exactly the 16-B aligned blocks
// overlapping it, the output in one that covers exactly the blocks overlapping
// [lo, next), the three tables in allocations of exactly the entries the frame
// may write, so any read or write outside them is a sanitizer report. The
// output's slack bytes hold 0xA5 and must still hold it afterwards, the pads
// must be 0, the table entries in front of the frame's keep their sentinel.
// Each run is repeated with out_cap and out_first[i + 1] in the middle of the
// frame's output (the blocks and entries from the cut on are not there at all)
// and with out_bytes[i + 1] in the middle. Exit 0 = clean and equal.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../nex_amd/csrc/fragment_core.hpp"

namespace {

// k_fragment_frames' body over one frame: the three phases of fragment_core.hpp
// (the functions the kernel calls), the group's lanes one after the other, the
// kernel's barriers where one loop ends and the next begins.
void run(const nexg::FragJob& job, const nexg::FragShape& s, uint32_t align, const nexg::FragOut& out) {
    using namespace nexg;
    FragHdr H;
    memset(&H, 0xEE, sizeof(H));
    for (uint32_t lane = 0; lane < kFragLanes; lane++) frag_stage(job, s, H, lane);
    frag_walk(s, H);
    for (uint32_t lane = 0; lane < kFragLanes; lane++) frag_fill(job, s, H, align, out, lane);
}

struct Piece {
    std::vector<uint8_t> bytes;
};

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    long bad = 0, frames = 0, cases = 0, runs = 0, pieces_run = 0;
    uint32_t head[6];
    while (fread(head, 4, 6, fp) == 6) {
        const nexg_frag_option opt{head[0], head[1], head[2], 0};
        if (nexg::check_frag_option(&opt)) return 3;
        const uint32_t sphases = head[3], dphases = head[4], count = head[5];
        cases++;
        std::vector<uint8_t> in;
        for (uint32_t i = 0; i < count; i++) {
            uint32_t fh[5];
            nexg_fragged want_row;
            if (fread(fh, 4, 5, fp) != 5 || fread(&want_row, sizeof(want_row), 1, fp) != 1) return 2;
            const bool ext = fh[1] != 0;
            const uint32_t len = ext ? fh[0] : 0u, index = fh[2], first = fh[3], n = fh[4];
            in.resize(len);
            if (len && fread(in.data(), 1, len, fp) != len) return 2;
            std::vector<Piece> want(n);
            uint64_t out_bytes = 0, last_end = 0;
            std::vector<uint64_t> at(n);
            for (uint32_t k = 0; k < n; k++) {
                uint32_t pl;
                if (fread(&pl, 4, 1, fp) != 1) return 2;
                want[k].bytes.resize(pl);
                if (pl && fread(want[k].bytes.data(), 1, pl, fp) != pl) return 2;
                at[k] = out_bytes;
                last_end = out_bytes + pl;
                out_bytes += (pl + opt.align - 1u) & ~(opt.align - 1u);
            }
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
                const nexg::FragShape s = nexg::frag_shape(ext, len, reinterpret_cast<uint64_t>(f), opt.mtu, opt.flags);
                const nexg_fragged row = nexg::frag_row(s, first);
                if (memcmp(&row, &want_row, sizeof(row)) != 0 || s.n != n || nexg::frag_out_bytes(s, len, opt.align) != out_bytes) {
                    if (bad++ < 5)
                        fprintf(stderr, "case %ld frame %u (len %u) phase %u: row {%u, %u, %u, %u, %u, %u} bytes %u expected {%u, %u, %u, %u, %u, %u} bytes %llu\n",
                                cases, i, len, sp, row.status, row.kind, row.hdr_len, row.pieces, row.piece_data, row.first,
                                nexg::frag_out_bytes(s, len, opt.align), want_row.status, want_row.kind, want_row.hdr_len,
                                want_row.pieces, want_row.piece_data, want_row.first, (unsigned long long)out_bytes);
                    free(sblock);
                    continue;
                }
                for (uint32_t dp = 0; dp < 16; dp++) {
                    if (!(dphases >> dp & 1u)) continue;
                    const uint32_t pad = opt.align == 1u && n ? (sp * 5u + dp * 3u + len) & 15u : 0u;
                    const uint64_t lo = 16u + dp, end = lo + out_bytes + pad;  // one block in front stays 0xA5
                    // the image of [0, end): 0xA5 in front, the output frames, zero between and behind them
                    std::vector<uint8_t> image(end, 0xA5);
                    if (n) memset(image.data() + lo, 0, end - lo);
                    for (uint32_t k = 0; k < n; k++)
                        if (!want[k].bytes.empty()) memcpy(image.data() + lo + at[k], want[k].bytes.data(), want[k].bytes.size());
                    for (int cut = 0; cut < 3; cut++) {
                        if (cut && out_bytes < 2) continue;
                        const uint64_t mid = lo + out_bytes / 2u;
                        const uint64_t next = cut == 2 ? mid : end;
                        const uint64_t full = (next + 15u) / 16u * 16u;
                        const uint64_t cap = cut == 1 ? mid : full;
                        const uint64_t stop = cap < next ? cap : next;  // no store at or past it
                        // with a cut the blocks from the one that holds it on are not there at all
                        const size_t have = (stop + 15u) / 16u * 16u;
                        uint8_t* out = static_cast<uint8_t*>(aligned_alloc(16, have));
                        if (!out) return 2;
                        memset(out, 0xA5, have);
                        const uint32_t first_end = first + (cut == 1 ? n / 2u : n);
                        // out_count past first_end on the full run, so that first_end bounds; below it on the cut run
                        const uint64_t out_count = cut == 1 ? first_end : first_end + 3u;
                        std::vector<uint64_t> t_off(first_end + 1u, 0xA5A5A5A5A5A5A5A5ull);
                        std::vector<uint32_t> t_len(first_end + 1u, 0xA5A5A5A5u), t_src(first_end + 1u, 0xA5A5A5A5u);
                        nexg::FragJob job{};
                        job.live = true;
                        job.ext = ext;
                        job.len = len;
                        job.index = index;
                        job.src = reinterpret_cast<uint64_t>(f);
                        job.first = first;
                        job.first_end = cut == 1 ? first_end + 7u : first_end;  // the cut run: out_count is the lower bound
                        job.lo = lo;
                        job.next = next;
                        // the vectors hold first_end + 1 entries: the spare one keeps its sentinel
                        const nexg::FragOut o{t_off.data(), t_len.data(), t_src.data(), out, cap, out_count};
                        run(job, s, opt.align, o);
                        runs++;
                        pieces_run += n;
                        bool same = true;
                        for (size_t k = 0; k < have; k++) {
                            const uint8_t w = k < stop ? image[k] : 0xA5;
                            if (out[k] != w) same = false;
                        }
                        for (uint32_t e = 0; e <= first_end; e++) {
                            const bool mine = e >= first && e < first_end;
                            const uint64_t w_off = mine ? lo + at[e - first] : 0xA5A5A5A5A5A5A5A5ull;
                            const uint32_t w_len = mine ? (uint32_t)want[e - first].bytes.size() : 0xA5A5A5A5u;
                            const uint32_t w_src = mine ? index : 0xA5A5A5A5u;
                            if (t_off[e] != w_off || t_len[e] != w_len || t_src[e] != w_src) same = false;
                        }
                        if (!same && bad++ < 5)
                            fprintf(stderr, "case %ld (mtu %u align %u) frame %u (len %u, %u output frames, last ends at %llu) phases %u -> %u cut %d: bytes or table differ\n",
                                    cases, opt.mtu, opt.align, i, len, n, (unsigned long long)last_end, sp, dp, cut);
                        free(out);
                    }
                }
                free(sblock);
            }
        }
    }
    fclose(fp);
    printf("cases %ld frames %ld runs %ld pieces %ld mismatches %ld\n", cases, frames, runs, pieces_run, bad);
    return bad ? 1 : 0;
}
