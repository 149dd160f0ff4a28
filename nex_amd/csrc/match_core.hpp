// match_core.hpp — the per-frame core of nexg_match_batch (include/nexg.h): the
// set in the form the kernel tests with, the region rule, the case fold, the
// occurrence test at one start position over a 16-byte window, the (offset,
// pattern) key a row is the minimum of, and the select predicate. k_match
// (nexg_match.hip) runs it on gfx950 over windows built in registers; the
// test-only host driver (tests/native/match_fuzz.cpp) runs the very same code
// over windows built byte by byte, through match_frame below.
// Plain host / device code: <stdint.h> and nexg.h only (a plain C++ compiler
// takes it too).
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "../../include/nexg.h"

#ifndef NEXG_HD
#ifdef __HIPCC__
#define NEXG_HD __host__ __device__ __forceinline__
#else
#define NEXG_HD inline
#endif
#endif

namespace nexg {

// A pattern as a kernel argument: its bytes as four big-endian words (byte 0
// on top of w[0], zero past len, already folded under NEXG_PAT_NOCASE).
struct MatchPat {  // 24 bytes
    uint32_t w[4];
    uint32_t meta;  // len | flags << 8
    uint32_t win;   // off_lo | off_hi << 16
};
struct MatchSet {
    uint32_t n, flags;  // flags: NEXG_MATCH_*
    MatchPat pat[NEXG_MATCH_MAX_PATTERNS];
};

// 0x41..0x5A -> | 0x20, every other byte as it is
NEXG_HD uint32_t match_fold(uint32_t b) { return b >= 0x41u && b <= 0x5Au ? b | 0x20u : b; }

// match_fold on each byte of a word
NEXG_HD uint32_t match_fold4(uint32_t x) {
    const uint32_t y = x & 0x7F7F7F7Fu;
    const uint32_t ge_a = y + 0x3F3F3F3Fu;  // bit 7 of a byte: its low seven bits >= 0x41
    const uint32_t gt_z = y + 0x25252525u;  // bit 7 of a byte: its low seven bits >= 0x5B
    return x | ((ge_a & ~gt_z & ~x & 0x80808080u) >> 2);
}

// nullptr when the set is valid (then *out, if given, is filled), else what is wrong with it
inline const char* prepare_patterns(const nexg_patterns* s, MatchSet* out) {
    if (!s) return "NULL pattern set";
    if (s->n_patterns == 0 || s->n_patterns > NEXG_MATCH_MAX_PATTERNS) return "patterns: n_patterns must be 1..32";
    if (s->flags & ~NEXG_MATCH_FRAME) return "patterns: unknown flag bits";
    MatchSet o{};
    o.n = s->n_patterns;
    o.flags = s->flags;
    for (uint32_t i = 0; i < s->n_patterns; i++) {
        const nexg_pattern& p = s->pat[i];
        if (p.len == 0 || p.len > NEXG_MATCH_MAX_LEN) return "pattern: len must be 1..16";
        for (uint32_t k = p.len; k < NEXG_MATCH_MAX_LEN; k++)
            if (p.bytes[k]) return "pattern: nonzero bytes past len";
        if (p.flags & ~NEXG_PAT_NOCASE) return "pattern: unknown flag bits";
        for (uint32_t k = 0; k < sizeof(p.reserved); k++)
            if (p.reserved[k]) return "pattern: reserved must be 0";
        if (p.off_lo > p.off_hi) return "pattern: off_lo > off_hi";
        MatchPat& d = o.pat[i];
        for (uint32_t k = 0; k < p.len; k++) {
            const uint32_t b = (p.flags & NEXG_PAT_NOCASE) ? match_fold(p.bytes[k]) : p.bytes[k];
            d.w[k >> 2] |= b << (24u - 8u * (k & 3u));
        }
        d.meta = (uint32_t)p.len | (uint32_t)p.flags << 8;
        d.win = (uint32_t)p.off_lo | (uint32_t)p.off_hi << 16;
    }
    if (out) *out = o;
    return nullptr;
}

// The region of a frame of `len` bytes (0 for an extent frame_extent refuses):
// [start, start + n). flags_dw / payload_dw: dwords 0 and 1 of the frame's
// record, not looked at under NEXG_MATCH_FRAME.
NEXG_HD void match_region(uint32_t set_flags, uint32_t len, uint32_t flags_dw, uint32_t payload_dw, uint32_t& start,
                          uint32_t& n) {
    start = 0u, n = len;
    if (set_flags & NEXG_MATCH_FRAME) return;
    const uint32_t poff = payload_dw & 0xFFFFu, plen = payload_dw >> 16;
    const bool ok = ((flags_dw >> NEXG_STATUS_SHIFT) & 7u) == 0u && plen > 0u && poff + plen <= len;
    start = ok ? poff : 0u;
    n = ok ? plen : 0u;
}

// Does pattern P occur at region-relative position q of a region of n bytes?
// ww: the 16 bytes at q as four big-endian words; bytes at or past n may hold
// anything (the length test leaves them out). wf: match_fold4 of ww.
NEXG_HD bool match_at(const MatchPat& P, const uint32_t (&ww)[4], const uint32_t (&wf)[4], uint32_t q, uint32_t n) {
    const uint32_t L = P.meta & 0xFFu, lo = P.win & 0xFFFFu, hi = P.win >> 16;
    const bool nocase = ((P.meta >> 8) & NEXG_PAT_NOCASE) != 0u;
    uint32_t diff = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
        const uint32_t kept = L <= 4u * i ? 0u : L - 4u * i >= 4u ? 4u : L - 4u * i;  // pattern bytes in word i
        const uint32_t km = kept == 0u ? 0u : 0xFFFFFFFFu << (8u * (4u - kept));
        diff |= ((nocase ? wf[i] : ww[i]) ^ P.w[i]) & km;
    }
    return diff == 0u && q + L <= n && q >= lo && q <= hi;
}

// a row is the OR of its occurrences' bits and the minimum of their keys
constexpr uint32_t kMatchNoKey = 0xFFFFFFFFu;
NEXG_HD uint32_t match_key(uint32_t frame_off, uint32_t p) { return frame_off << 8 | p; }
NEXG_HD nexg_match match_row(uint32_t mask, uint32_t key) {
    nexg_match r{0u, 0u, (uint8_t)NEXG_PAT_NONE, 0u};
    if (mask) {
        r.mask = mask;
        r.first_off = (uint16_t)(key >> 8);
        r.first_pat = (uint8_t)(key & 0xFFu);
    }
    return r;
}

// nexg_match_select's predicate
NEXG_HD bool match_selected(uint32_t mask, uint32_t any_mask, uint32_t all_mask, uint32_t none_mask) {
    return (any_mask == 0u || (mask & any_mask) != 0u) && (mask & all_mask) == all_mask && (mask & none_mask) == 0u;
}

// One frame start to end, every pattern at every position: the row of the
// region [start, start + n) of a frame whose bytes `f.u8(i)` gives, 0 <= i <
// start + n. Only bytes of the region are asked for.
template <typename F>
NEXG_HD nexg_match match_frame(const MatchSet& s, const F& f, uint32_t start, uint32_t n) {
    uint32_t mask = 0u, key = kMatchNoKey;
    for (uint32_t q = 0; q < n; q++) {
        uint32_t ww[4] = {0u, 0u, 0u, 0u}, wf[4];
        const uint32_t have = n - q < 16u ? n - q : 16u;
        for (uint32_t k = 0; k < have; k++) ww[k >> 2] |= (uint32_t)f.u8(start + q + k) << (24u - 8u * (k & 3u));
        for (uint32_t i = 0; i < 4; i++) wf[i] = match_fold4(ww[i]);
        for (uint32_t p = 0; p < s.n; p++) {
            if (!match_at(s.pat[p], ww, wf, q, n)) continue;
            mask |= 1u << p;
            const uint32_t k = match_key(start + q, p);
            key = k < key ? k : key;
        }
    }
    return match_row(mask, key);
}

}  // namespace nexg
