// TEST INFRASTRUCTURE ONLY: the per-frame core of nexg_match_batch
// (nex_amd/csrc/match_core.hpp: region rule, fold, occurrence test, row), built
// for the host with AddressSanitizer + UBSan, against a naive memcmp loop.
//
//   match_fuzz FILE   the corpus as tests/test_match_core.py writes it: per case
//                     a nexg_patterns, a u32 frame count, then per frame u32
//                     length, u32 record flags, u32 payload dword, the bytes,
//                     and the 8-byte row the host contract expects. Each frame
//                     sits alone in a heap block that ends at its last byte.
//   then              random regions over a small alphabet that sit flush
//                     against the end of a heap allocation, random sets.
// Any read outside the region's frame is a sanitizer report; any row that
// differs from the naive loop's (or the file's) is counted. Exit 0 = clean and equal.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../nex_amd/csrc/match_core.hpp"

namespace {

struct Bytes {
    const uint8_t* g;
    uint32_t u8(uint32_t i) const { return g[i]; }
};

uint8_t fold(uint8_t b) { return b >= 'A' && b <= 'Z' ? (uint8_t)(b + 32) : b; }

// the text of include/nexg.h, one byte at a time
nexg_match naive(const nexg_patterns& s, const uint8_t* f, uint32_t start, uint32_t n) {
    nexg_match r{0, 0, NEXG_PAT_NONE, 0};
    uint32_t best = 0xFFFFFFFFu;
    for (uint32_t p = 0; p < s.n_patterns; p++) {
        const nexg_pattern& P = s.pat[p];
        for (uint32_t q = 0; q + P.len <= n; q++) {
            if (q < P.off_lo || q > P.off_hi) continue;
            bool same;
            if (P.flags & NEXG_PAT_NOCASE) {
                same = true;
                for (uint32_t k = 0; k < P.len && same; k++) same = fold(f[start + q + k]) == fold(P.bytes[k]);
            } else {
                same = memcmp(f + start + q, P.bytes, P.len) == 0;
            }
            if (!same) continue;
            r.mask |= 1u << p;
            const uint32_t key = (start + q) << 8 | p;
            if (key < best) best = key;
        }
    }
    if (r.mask) {
        r.first_off = (uint16_t)(best >> 8);
        r.first_pat = (uint8_t)(best & 0xFF);
    }
    return r;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n;
}

bool same_row(const nexg_match& a, const nexg_match& b) { return memcmp(&a, &b, sizeof(a)) == 0; }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long bad = 0, frames = 0, cases = 0, fuzzed = 0;
    nexg_patterns set;
    while (fread(&set, sizeof(set), 1, f) == 1) {
        nexg::MatchSet ms;
        if (nexg::prepare_patterns(&set, &ms)) return 3;
        uint32_t count;
        if (fread(&count, 4, 1, f) != 1) return 2;
        cases++;
        for (uint32_t i = 0; i < count; i++) {
            uint32_t head[3];
            nexg_match want;
            if (fread(head, 4, 3, f) != 3) return 2;
            const uint32_t len = head[0];
            uint8_t* buf = static_cast<uint8_t*>(malloc(len ? len : 1));  // ends at the frame's last byte
            if (len && fread(buf, 1, len, f) != len) return 2;
            if (fread(&want, sizeof(want), 1, f) != 1) return 2;
            uint32_t start, n;
            nexg::match_region(ms.flags, len > 65535u ? 0u : len, head[1], head[2], start, n);
            const nexg_match got = nexg::match_frame(ms, Bytes{buf}, start, n);
            frames++;
            if ((!same_row(got, want) || !same_row(got, naive(set, buf, start, n))) && bad++ < 5)
                fprintf(stderr, "case %ld frame %u: row {%x, %u, %u} expected {%x, %u, %u}\n", cases, i, got.mask,
                        got.first_off, got.first_pat, want.mask, want.first_off, want.first_pat);
            free(buf);
        }
    }
    fclose(f);
    // random regions flush against the end of their allocation
    static const uint8_t alphabet[] = {'a', 'A', 'b', 'B', 'z', 'Z', '@', '`', '[', '{', 0x00, 0xFF, 0xC1, 0xE1};
    for (int round = 0; round < 4000; round++) {
        nexg_patterns s;
        memset(&s, 0, sizeof(s));
        s.n_patterns = 1 + rnd(32);
        s.flags = rnd(2);
        for (uint32_t p = 0; p < s.n_patterns; p++) {
            nexg_pattern& P = s.pat[p];
            P.len = (uint8_t)(1 + rnd(rnd(4) ? 3 : 16));
            for (uint32_t k = 0; k < P.len; k++) P.bytes[k] = alphabet[rnd(rnd(3) ? 4 : sizeof(alphabet))];
            P.flags = (uint8_t)rnd(2);
            if (rnd(2)) {
                P.off_lo = (uint16_t)rnd(40);
                P.off_hi = (uint16_t)(P.off_lo + rnd(3) * rnd(30));
            } else {
                P.off_hi = 65535;
            }
        }
        nexg::MatchSet ms;
        if (nexg::prepare_patterns(&s, &ms)) return 3;
        const uint32_t len = rnd(120), poff = rnd(len + 1), plen = rnd(len - poff + 2);  // the payload may end one past the frame
        uint8_t* buf = static_cast<uint8_t*>(malloc(len ? len : 1));
        for (uint32_t k = 0; k < len; k++) buf[k] = alphabet[rnd(rnd(3) ? 4 : sizeof(alphabet))];
        uint32_t start, n;
        nexg::match_region(ms.flags, len, rnd(8) ? 0u : 3u << NEXG_STATUS_SHIFT, poff | plen << 16, start, n);
        if (start + n > len) return 4;  // the region rule let a region leave its frame
        const nexg_match got = nexg::match_frame(ms, Bytes{buf}, start, n);
        fuzzed++;
        if (!same_row(got, naive(s, buf, start, n)) && bad++ < 5) fprintf(stderr, "fuzz round %d differs\n", round);
        free(buf);
    }
    printf("cases %ld frames %ld fuzzed %ld mismatches %ld\n", cases, frames, fuzzed, bad);
    return bad ? 1 : 0;
}
