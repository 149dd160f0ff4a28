// TEST INFRASTRUCTURE ONLY: the per-frame core of nexg_rewrite_batch
// (nex_amd/csrc/rewrite_core.hpp: views, fields, dirty set, both checksum
// modes), built for the host with AddressSanitizer + UBSan.
//
//   rewrite_fuzz FILE   the corpus as tests/test_rewrite_core.py writes it: per
//                       case a nexg_actions, u32 parse flags, u32 ip_offset, u32
//                       phase mask, u32 frame count, then per frame u32 length,
//                       u32 action index, the bytes, the bytes expected after
//                       the call and the 8-byte row expected.
// Every frame is run at each of the 16 byte phases the case's mask names, in a
// heap allocation that covers exactly the 16-B aligned blocks overlapping the
// frame (include/nexg.h's block rule: the fix-up's sums load whole blocks), so
// any read or write outside them is a sanitizer report. The slack bytes of the
// blocks hold 0xA5 and must still hold it afterwards. Exit 0 = clean and equal.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../nex_amd/csrc/rewrite_core.hpp"

namespace {

// k_rewrite's per-lane part (nexg_rewrite.hip) over one frame
nexg_rewritten run(const nexg_actions& s, uint32_t ai, uint8_t* f, uint32_t len, uint32_t flags, uint32_t ip_offset) {
    nexg_rewritten rw{0, 0, NEXG_ACTION_NONE, 0, 0};
    if (ai >= s.n_actions) return rw;
    if (s.flags & NEXG_REWRITE_INCREMENTAL) {  // through the header window, as the kernel (its LDS column: an array here)
        uint32_t col[4 * nexg::kWindowBlocks];
        const nexg::HeaderWindow w = nexg::load_header_window(f, len, col, 1);
        return nexg::rewrite_frame<true>(f, w, len, flags, ip_offset, s.actions[ai], ai);
    }
    return nexg::rewrite_frame<false>(f, nexg::GlobalFrame{f}, len, flags, ip_offset, s.actions[ai], ai);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    long bad = 0, frames = 0, cases = 0, runs = 0;
    nexg_actions set;
    while (fread(&set, sizeof(set), 1, fp) == 1) {
        if (nexg::check_actions(&set)) return 3;
        uint32_t head[4];
        if (fread(head, 4, 4, fp) != 4) return 2;
        const uint32_t flags = head[0], ip_offset = head[1], phases = head[2], count = head[3];
        cases++;
        std::vector<uint8_t> in, want;
        for (uint32_t i = 0; i < count; i++) {
            uint32_t fh[2];
            nexg_rewritten want_row;
            if (fread(fh, 4, 2, fp) != 2) return 2;
            const uint32_t len = fh[0], ai = fh[1];
            in.resize(len);
            want.resize(len);
            if (len && (fread(in.data(), 1, len, fp) != len || fread(want.data(), 1, len, fp) != len)) return 2;
            if (fread(&want_row, sizeof(want_row), 1, fp) != 1) return 2;
            frames++;
            for (uint32_t phase = 0; phase < 16; phase++) {
                if (!(phases >> phase & 1u)) continue;
                const size_t bytes = len ? (phase + len + 15u) / 16u * 16u : 16u;
                uint8_t* block = static_cast<uint8_t*>(aligned_alloc(16, bytes));
                if (!block) return 2;
                memset(block, 0xA5, bytes);
                uint8_t* f = block + phase;
                if (len) memcpy(f, in.data(), len);
                const nexg_rewritten got = run(set, ai, f, len, flags, ip_offset);
                runs++;
                bool same = memcmp(&got, &want_row, sizeof(got)) == 0 && (len == 0 || memcmp(f, want.data(), len) == 0);
                for (size_t k = 0; k < bytes; k++)
                    if ((k < phase || k >= phase + len) && block[k] != 0xA5) same = false;
                if (!same && bad++ < 5)
                    fprintf(stderr, "case %ld frame %u (len %u, action %u) phase %u: row {%x, %u, %u, %04x, %04x} expected {%x, %u, %u, %04x, %04x}\n",
                            cases, i, len, ai, phase, got.applied, got.fixed, got.action, got.ip_csum, got.l4_csum,
                            want_row.applied, want_row.fixed, want_row.action, want_row.ip_csum, want_row.l4_csum);
                free(block);
            }
        }
    }
    fclose(fp);
    printf("cases %ld frames %ld runs %ld mismatches %ld\n", cases, frames, runs, bad);
    return bad ? 1 : 0;
}
