// TEST INFRASTRUCTURE ONLY: the per-frame core of nexg_reasm_plan /
// nexg_reasm_frames (nex_amd/csrc/reasm_core.hpp: classification, hash, marks,
// verdict, header staging, copies, table), built for the host with
// AddressSanitizer + UBSan.
//
//   reasm_fuzz FILE   the corpus as tests/test_reasm_core.py writes it: per table
//                     u32 align, source phase mask, destination phase mask, frame
//                     count; per frame u32 length, extent accepted (0: the frame's
//                     extent leaves the data; no bytes follow and its source
//                     address is one nothing is allocated at) and the bytes; then
//                     the 16-byte rows expected (reassemble_host, exact=False),
//                     u32 output frames, and per output frame u32 length and the
//                     bytes expected.
// Plan side: at each source phase every frame stands in a heap allocation that
// covers exactly the 16-B aligned blocks overlapping it; the frames are
// classified (reasm_classify, reasm_info), ordered by (hash, id << 13 | fo,
// frame number) with std::stable_sort where the device has its radix passes,
// marked (reasm_mark) and judged (reasm_complete) as k_reasm_rows does, and the
// rows must equal the expected ones.
// Fill side: at each destination phase every output frame gets an allocation
// that covers exactly the blocks overlapping [lo, next); each frame that goes
// into it runs the kernel's three phases, lane by lane; the bytes, the pad and
// the table entry must equal the expected ones and the slack must keep 0xA5.
// Again with out_cap in the middle of the output frame (the blocks from the cut
// on are not there at all, out_count bars the table entry), with
// out_bytes[h + 1] in the middle, and with rows[i].head lying: each PART is run
// once more against the range of the next output frame, which alone is
// allocated. Any read or write outside the allocations is a sanitizer report.
// Exit 0 = clean and equal.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../nex_amd/csrc/reasm_core.hpp"

namespace {

using namespace nexg;

// k_reasm_frames' body over one frame
void run(const ReasmJob& job, const ReasmClass& c, const FragOut& out) {
    FragHdr H;
    memset(&H, 0xEE, sizeof(H));
    for (uint32_t lane = 0; lane < kReasmLanes; lane++) reasm_stage(job, c, H, lane);
    reasm_sum(job, c, H);
    for (uint32_t lane = 0; lane < kReasmLanes; lane++) reasm_fill(job, c, H, out, lane);
}

struct Frame {
    uint32_t len;
    bool ext;
    std::vector<uint8_t> bytes;
    uint8_t* block;  // the allocation at this phase
    uint64_t at;     // the address of byte 0
    ReasmClass c;
};

// k_reasm_mark + k_reasm_rows with sums in place of the scans
std::vector<nexg_reasm> plan(const std::vector<Frame>& fr) {
    const size_t n = fr.size();
    std::vector<ReasmInfo> info(n);
    for (size_t i = 0; i < n; i++) info[i] = reasm_info(fr[i].c, fr[i].ext ? fr[i].len : 0u);
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return info[a].hash != info[b].hash ? info[a].hash < info[b].hash : info[a].idfo < info[b].idfo;
    });
    std::vector<nexg_reasm> rows(n);
    size_t first = 0;
    while (first < n) {
        size_t next = first + 1;
        uint32_t brk = 0, bad = 0;
        const ReasmMark m0 = reasm_mark(info[order[first]], first > 0, info[order[first ? first - 1 : 0]]);
        bad += m0.bad;
        while (next < n) {
            const ReasmMark m = reasm_mark(info[order[next]], true, info[order[next - 1]]);
            if (m.head) break;
            brk += m.brk, bad += m.bad;
            next++;
        }
        const ReasmInfo &xh = info[order[first]], &xl = info[order[next - 1]];
        uint32_t D = 0;
        const bool frag = info_frag(xh);
        const bool complete = frag && reasm_complete(brk, bad, xh, xl, D);
        for (size_t k = first; k < next; k++) {
            const uint32_t i = order[k];
            nexg_reasm r{};
            r.out = r.head = 0xFFFFFFFFu;
            if (!frag) {
                r.status = (uint8_t)((info[i].shape >> 16) & 0xFFu);
                r.kind = (uint8_t)(info[i].shape >> 24);
            } else {
                r.kind = complete ? (k == first ? NEXG_REASM_HEAD : NEXG_REASM_PART) : NEXG_REASM_HELD;
                r.hdr_len = (uint8_t)info_hl(info[i]);
                r.flags = brk ? NEXG_REASM_COLLISION : 0;
                if (complete) r.head = order[first];
                if (complete && k == first) r.members = (uint16_t)(next - first), r.data_len = (uint16_t)D;
            }
            rows[i] = r;
        }
        first = next;
    }
    uint32_t f = 0;
    for (size_t i = 0; i < n; i++)
        if (rows[i].kind == NEXG_REASM_PASS || rows[i].kind == NEXG_REASM_HEAD) rows[i].out = f++;
    for (size_t i = 0; i < n; i++)
        if (rows[i].kind == NEXG_REASM_PART) rows[i].out = rows[rows[i].head].out;
    return rows;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    long bad = 0, tables = 0, frames = 0, runs = 0, lies = 0;
    uint32_t head[4];
    while (fread(head, 4, 4, fp) == 4) {
        const uint32_t align = head[0], sphases = head[1], dphases = head[2], count = head[3];
        tables++;
        std::vector<Frame> fr(count);
        for (Frame& f : fr) {
            uint32_t fh[2];
            if (fread(fh, 4, 2, fp) != 2) return 2;
            f.ext = fh[1] != 0;
            f.len = f.ext ? fh[0] : 0u;
            f.bytes.resize(f.len);
            if (f.len && fread(f.bytes.data(), 1, f.len, fp) != f.len) return 2;
        }
        std::vector<nexg_reasm> want_rows(count);
        if (count && fread(want_rows.data(), 16, count, fp) != count) return 2;
        uint32_t n_out;
        if (fread(&n_out, 4, 1, fp) != 1) return 2;
        std::vector<std::vector<uint8_t>> want(n_out);
        for (auto& w : want) {
            uint32_t l;
            if (fread(&l, 4, 1, fp) != 1) return 2;
            w.resize(l);
            if (l && fread(w.data(), 1, l, fp) != l) return 2;
        }
        frames += count;
        // the frames of each output frame
        std::vector<std::vector<uint32_t>> members(n_out);
        for (uint32_t i = 0; i < count; i++)
            if (want_rows[i].out < n_out) members[want_rows[i].out].push_back(i);
        for (uint32_t sp = 0; sp < 16; sp++) {
            if (!(sphases >> sp & 1u)) continue;
            for (Frame& f : fr) {
                const size_t sbytes = f.len ? (sp + f.len + 15u) / 16u * 16u : 16u;
                f.block = static_cast<uint8_t*>(aligned_alloc(16, sbytes));
                if (!f.block) return 2;
                memset(f.block, 0x5A, sbytes);
                // a rejected extent's offset is any number: an address far from every allocation
                f.at = f.ext ? reinterpret_cast<uint64_t>(f.block + sp) : uint64_t(0x1000) + sp;
                if (f.len) memcpy(f.block + sp, f.bytes.data(), f.len);
                f.c = reasm_classify(f.ext, f.len, f.at);
            }
            const std::vector<nexg_reasm> rows = plan(fr);
            bool rows_same = true;
            for (uint32_t i = 0; i < count; i++)
                if (memcmp(&rows[i], &want_rows[i], 16) != 0) {
                    rows_same = false;
                    if (bad++ < 5)
                        fprintf(stderr, "table %ld frame %u phase %u: row {%u %u %u %u %u %u %u %u} expected {%u %u %u %u %u %u %u %u}\n",
                                tables, i, sp, rows[i].status, rows[i].kind, rows[i].hdr_len, rows[i].flags, rows[i].members,
                                rows[i].data_len, rows[i].out, rows[i].head, want_rows[i].status, want_rows[i].kind,
                                want_rows[i].hdr_len, want_rows[i].flags, want_rows[i].members, want_rows[i].data_len,
                                want_rows[i].out, want_rows[i].head);
                }
            for (uint32_t dp = 0; rows_same && dp < 16; dp++) {
                if (!(dphases >> dp & 1u)) continue;
                for (uint32_t f = 0; f < n_out; f++) {
                    const uint32_t L = (uint32_t)want[f].size();
                    const uint64_t lo = 16u + dp, end = lo + ((L + align - 1u) & ~(align - 1u));  // one block in front stays 0xA5
                    std::vector<uint8_t> image(end, 0xA5);
                    memset(image.data() + lo, 0, end - lo);
                    if (L) memcpy(image.data() + lo, want[f].data(), L);
                    const uint32_t h = members[f].empty() ? 0u : (rows[members[f][0]].kind == NEXG_REASM_PART ? rows[members[f][0]].head
                                                                                                              : members[f][0]);
                    for (int cut = 0; cut < 4; cut++) {
                        if (cut && end - lo < 2) continue;
                        // cut 3: the PARTs alone, against the next output frame's range (rows[i].head lying)
                        const uint32_t g = cut == 3 ? (f + 1u) % n_out : f;
                        if (cut == 3 && (g == f || rows[h].kind != NEXG_REASM_HEAD)) continue;
                        const uint32_t Lg = (uint32_t)want[g].size();
                        const uint64_t g_end = lo + ((Lg + align - 1u) & ~(align - 1u));
                        const uint64_t mid = lo + (end - lo) / 2u;
                        const uint64_t next = cut == 2 ? mid : cut == 3 ? g_end : end;
                        const uint64_t full = (next + 15u) / 16u * 16u;
                        const uint64_t cap = cut == 1 ? mid : full;
                        const uint64_t stop = cap < next ? cap : next;  // no store at or past it
                        const size_t have = (stop + 15u) / 16u * 16u;
                        uint8_t* out = static_cast<uint8_t*>(aligned_alloc(16, have ? have : 16));
                        if (!out) return 2;
                        memset(out, 0xA5, have ? have : 16);
                        uint64_t t_off[3] = {0xA5A5A5A5A5A5A5A5ull, 0xA5A5A5A5A5A5A5A5ull, 0xA5A5A5A5A5A5A5A5ull};
                        uint32_t t_len[3] = {0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u}, t_src[3] = {0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u};
                        const FragOut o{t_off, t_len, t_src, out, cap, cut == 1 ? 1u : 5u};  // out_count 1 bars entry 1
                        for (uint32_t i : members[f]) {
                            if (cut == 3 && rows[i].kind != NEXG_REASM_PART) continue;
                            ReasmJob job{};
                            job.live = true;
                            job.ext = fr[i].ext;
                            job.len = fr[i].len;
                            job.index = i;
                            job.src = fr[i].at;
                            job.kind = rows[i].kind;
                            job.data_len = rows[i].data_len;
                            job.first = 1;
                            job.first_end = cut == 1 ? 9u : 2u;
                            job.named = true;
                            job.head_hl = cut == 3 ? 20u : rows[h].hdr_len;
                            job.lo = lo;
                            job.next = next;
                            run(job, fr[i].c, o);
                            runs++;
                            if (cut == 3) lies++;
                        }
                        bool same = true;
                        if (cut == 3) {  // whatever the part wrote, it wrote inside [lo, stop)
                            for (size_t k = 0; k < have; k++)
                                if ((k < lo || k >= stop) && out[k] != 0xA5) same = false;
                            if (t_off[1] != 0xA5A5A5A5A5A5A5A5ull) same = false;
                        } else {
                            for (size_t k = 0; k < have; k++)
                                if (out[k] != (k < stop ? image[k] : 0xA5)) same = false;
                            const bool entry = cut != 1;
                            if (t_off[1] != (entry ? lo : 0xA5A5A5A5A5A5A5A5ull) || t_len[1] != (entry ? L : 0xA5A5A5A5u) ||
                                t_src[1] != (entry ? h : 0xA5A5A5A5u))
                                same = false;
                        }
                        if (t_off[0] != 0xA5A5A5A5A5A5A5A5ull || t_off[2] != 0xA5A5A5A5A5A5A5A5ull || t_len[0] != 0xA5A5A5A5u ||
                            t_len[2] != 0xA5A5A5A5u || t_src[0] != 0xA5A5A5A5u || t_src[2] != 0xA5A5A5A5u)
                            same = false;
                        if (!same && bad++ < 5)
                            fprintf(stderr, "table %ld (align %u) output %u (len %u, head %u, %zu members) phases %u -> %u cut %d: bytes or table differ\n",
                                    tables, align, f, L, h, members[f].size(), sp, dp, cut);
                        free(out);
                    }
                }
            }
            for (Frame& f : fr) free(f.block);
        }
    }
    fclose(fp);
    printf("tables %ld frames %ld runs %ld lies %ld mismatches %ld\n", tables, frames, runs, lies, bad);
    return bad ? 1 : 0;
}
