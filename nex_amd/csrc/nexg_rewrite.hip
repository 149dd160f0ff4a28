// nexg_rewrite.hip — nexg_rewrite_batch: header fields rewritten in place with
// the semantics of nex-packet's mutable setters under ChecksumMode::Automatic
// (include/nexg.h; the per-frame rule is rewrite_core.hpp). A match-action
// table's action half: rule j of a filter gets action j through action_index.
//
// One lane per frame, 256-frame tiles, extents through frame_extent as
// k_recompute takes them. The action set (<= 1 KiB) travels as a kernel
// argument and is staged into LDS once per workgroup: the copy loop is uniform
// over the actions, so the argument is only ever indexed by a scalar, and each
// lane then reads its own action from LDS.
//
// Two instances. RECOMPUTE reuses the fix-up's sums over the edited bytes and
// reads the payload only of a frame whose L4 checksum is dirty. INCREMENTAL
// updates the stored checksums by RFC 1624 eqn. 3 from the old and new words
// of the fields it writes: a lane loads its frame's first 16-B blocks (at most
// six, 96 B: the header window) with 16-B loads issued together into its own
// LDS column, reads the view conditions, the old field words and the stored
// checksums from there, and stores the fields and checksum words as bytes. An
// element-granular gather is uncoalesced by nature; whole aligned blocks, all
// in flight at once, are the widest form it has, and a lane's blocks share one
// or two cache lines. Byte stores only: a neighbouring frame's lane may own
// the rest of any wider word. No atomics, no workspace.
#include <string.h>

#include "parse_kernels.hpp"
#include "rewrite_core.hpp"

namespace nexg {

struct RewriteSet {  // nexg_actions' actions as dwords (nexg_action is 16 of them)
    uint32_t n, flags;
    uint32_t w[NEXG_REWRITE_MAX_ACTIONS][16];
};
static_assert(sizeof(nexg_action) == 64 && sizeof(RewriteSet) == sizeof(nexg_actions), "nexg_action is 16 dwords");

template <bool INCR>
__global__ __launch_bounds__(256) void k_rewrite(ParseArgs a, RewriteSet s, const uint8_t* action_index,
                                                 nexg_rewritten* out) {
    __shared__ uint32_t s_act[NEXG_REWRITE_MAX_ACTIONS][16];
    __shared__ uint32_t s_win[INCR ? 4 * kWindowBlocks : 1][kTile];  // INCREMENTAL: one header window column per lane
    const uint32_t t = threadIdx.x;
    for (uint32_t i = 0; i < s.n; i++) {  // uniform: action i stays in scalar registers
#pragma unroll
        for (uint32_t k = 0; k < 16; k++)
            if (t == i * 16u + k) s_act[i][k] = s.w[i][k];
    }
    __syncthreads();
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + t;
    if (idx >= a.count) return;
    const uint32_t ai = action_index ? (uint32_t)action_index[idx] : 0u;
    nexg_rewritten rw{0, 0, NEXG_ACTION_NONE, 0, 0};
    if (ai < s.n) {  // the index is caller memory: it never reaches past the set
        rw.action = (uint8_t)ai;
        uint64_t off;
        uint32_t len;
        if (frame_extent(a, idx, off, len)) {
            const nexg_action& A = *reinterpret_cast<const nexg_action*>(&s_act[ai][0]);
            uint8_t* f = const_cast<uint8_t*>(a.data) + off;
            if (INCR) {
                const HeaderWindow w = load_header_window(f, len, &s_win[0][t], kTile);
                rw = rewrite_frame<true>(f, w, len, a.opt_flags, a.ip_offset, A, ai);
            } else {
                rw = rewrite_frame<false>(f, GlobalFrame{f}, len, a.opt_flags, a.ip_offset, A, ai);
            }
        }
    }
    if (out) out[idx] = rw;
}

hipError_t launch_rewrite(const ParseArgs& a, const nexg_actions& actions, const uint8_t* action_index,
                          nexg_rewritten* out, hipStream_t st) {
    if (a.count == 0) return hipSuccess;
    RewriteSet s;
    memcpy(&s, &actions, sizeof(s));
    const uint64_t blocks = (a.count + kTile - 1) / kTile;
    if (s.flags & NEXG_REWRITE_INCREMENTAL)
        hipLaunchKernelGGL(k_rewrite<true>, dim3((uint32_t)blocks), dim3(kTile), 0, st, a, s, action_index, out);
    else
        hipLaunchKernelGGL(k_rewrite<false>, dim3((uint32_t)blocks), dim3(kTile), 0, st, a, s, action_index, out);
    return hipGetLastError();
}

}  // namespace nexg
