// nexg_api.hip — the C ABI declared in include/nexg.h.
//
// Validation, context handling and kernel selection only; every byte of frame
// data is processed by the gfx950 kernels in nexg_parse.hip / nexg_build.hip.
// There is deliberately no CPU fallback: a missing or non-gfx950 device makes
// nexg_ctx_create fail with NEXG_EDEVICE.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "encap_core.hpp"
#include "fragment_core.hpp"
#include "match_core.hpp"
#include "nexg_internal.hpp"
#include "rewrite_core.hpp"

struct nexg_ctx {
    int device;
    int cu_count;
    char arch[64];
    char last_error[256];
    void* scratch;          // device memory for per-call hand-offs (TwoPass tail sums)
    uint64_t scratch_bytes;
    hipEvent_t scratch_done;    // recorded after the last launch that used the scratch ...
    hipStream_t scratch_stream; // ... on this stream
    bool scratch_used;
};

namespace {

// Every entry point runs with the context's device current and restores the
// caller's afterwards: allocations and NULL-stream launches then land on the
// device the context is bound to, whichever device the thread had selected.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(const nexg_ctx* ctx) {
        if (ctx && hipGetDevice(&prev) == hipSuccess && prev != ctx->device)
            switched = hipSetDevice(ctx->device) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

// ctx scratch of at least `bytes` (grown, never shrunk; hipFree is
// device-synchronous, so no launch still reads the old block)
void* scratch(nexg_ctx* ctx, uint64_t bytes) {
    if (ctx->scratch_bytes >= bytes) return ctx->scratch;
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
    const uint64_t want = bytes < (1ull << 20) ? (1ull << 20) : bytes;
    if (hipMalloc(&ctx->scratch, want) != hipSuccess) {
        ctx->scratch = nullptr;
        return nullptr;
    }
    ctx->scratch_bytes = want;
    return ctx->scratch;
}

// The scratch is shared by every call on the context, whatever its stream:
// a call on another stream than the last user's waits for that user's launch
// (stream order alone covers calls on one stream).
hipError_t scratch_acquire(nexg_ctx* ctx, hipStream_t stream) {
    if (!ctx->scratch_used || ctx->scratch_stream == stream) return hipSuccess;
    return hipStreamWaitEvent(stream, ctx->scratch_done, 0);
}

hipError_t scratch_release(nexg_ctx* ctx, hipStream_t stream) {
    if (!ctx->scratch_done) {
        const hipError_t e = hipEventCreateWithFlags(&ctx->scratch_done, hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    const hipError_t e = hipEventRecord(ctx->scratch_done, stream);
    if (e != hipSuccess) return e;
    ctx->scratch_stream = stream;
    ctx->scratch_used = true;
    return hipSuccess;
}

int fail(nexg_ctx* ctx, int code, const char* fmt, const char* detail) {
    if (ctx) snprintf(ctx->last_error, sizeof(ctx->last_error), fmt, detail ? detail : "");
    return code;
}

int hip_status(nexg_ctx* ctx, hipError_t e, int code) {
    if (e == hipSuccess) return NEXG_OK;
    return fail(ctx, code, "HIP: %s", hipGetErrorString(e));
}

bool frames_valid(const nexg_frames* f) {
    if (!f) return false;
    if (f->count == 0) return true;
    if (!f->data) return false;
    if (!f->offsets && f->stride == 0) return false;
    if ((reinterpret_cast<uint64_t>(f->data) & 3u) != 0) return false;  // 4-B aligned base
    if ((f->hints & NEXG_FRAMES_OFFSETS32) && (reinterpret_cast<uint64_t>(f->offsets) & 3u) != 0) return false;
    return true;
}

nexg::ParseArgs to_args(const nexg_frames* f) {
    nexg::ParseArgs a{};
    a.data = f->data;
    a.data_bytes = f->data_bytes;
    a.offsets = f->offsets;
    a.lengths = f->lengths;
    a.stride = f->stride;
    a.count = f->count;
    a.hints = f->hints;
    if ((f->hints & NEXG_FRAMES_OFFSETS32) && f->offsets && f->data_bytes > 0xFFFFFFFFull)
        a.off_bases = nexg_offsets32_bases(f->offsets, f->count);
    return a;
}

nexg::ParseArgs parse_args(const nexg_frames* f, const nexg_parse_option* option) {
    nexg::ParseArgs a = to_args(f);
    a.opt_flags = option ? option->flags : 0u;
    a.ip_offset = option ? option->ip_offset : 0u;
    return a;
}

// ---- what the entries' checks share; the texts stay each entry's own --------

// one of the pointers has a bit of `mask` set (NULL is aligned)
template <typename... P>
bool misaligned(uint64_t mask, const P*... p) {
    return ((reinterpret_cast<uint64_t>(p) | ...) & mask) != 0;
}

// the second passes number frames with 32 bits
int check_count(nexg_ctx* ctx, const char* entry, uint64_t count) {
    if (count <= 0xFFFFFFFFull) return NEXG_OK;
    return fail(ctx, NEXG_EINVAL, "%s: more than 2^32 - 1 frames", entry);
}

// `have` bytes of workspace against `need`, what nexg_<entry>_workspace gives for `count`
int check_workspace(nexg_ctx* ctx, const char* entry, uint64_t count, uint64_t have, uint64_t need) {
    if (count == 0 || have >= need) return NEXG_OK;
    return fail(ctx, NEXG_EINVAL, "%1$s: workspace smaller than nexg_%1$s_workspace", entry);  // the name twice
}

// nexg_flow_option as nexg_flow_batch and nexg_flow_groups take it (NULL: no flags)
int flow_option_flags(nexg_ctx* ctx, const nexg_flow_option* option, uint32_t& flags) {
    flags = 0u;
    if (!option) return NEXG_OK;
    if (option->reserved != 0) return fail(ctx, NEXG_EINVAL, "flow option: reserved must be 0%s", nullptr);
    if ((option->flags & ~(NEXG_FLOW_SYMMETRIC | NEXG_FLOW_NO_PORTS | NEXG_FLOW_KEY)) != 0)
        return fail(ctx, NEXG_EINVAL, "flow option: unknown flag bits%s", nullptr);
    flags = option->flags;
    return NEXG_OK;
}

// every entry's tail: the caller's stream handle, and the launch's error as a status
hipStream_t as_stream(void* stream) { return static_cast<hipStream_t>(stream); }
int launched(nexg_ctx* ctx, hipError_t e) { return hip_status(ctx, e, NEXG_ELAUNCH); }

}  // namespace

extern "C" {

int nexg_abi_version(void) { return NEXG_ABI_VERSION; }

const char* nexg_strerror(int status) {
    switch (status) {
        case NEXG_OK: return "ok";
        case NEXG_EINVAL: return "invalid argument";
        case NEXG_ENOMEM: return "out of memory";
        case NEXG_EDEVICE: return "device error or device is not gfx950";
        case NEXG_ELAUNCH: return "kernel launch failed";
        case NEXG_ERANGE: return "length overflow (BuildError::LengthOverflow)";
        default: return "unknown status";
    }
}

int nexg_ctx_create(int device, nexg_ctx** out) {
    if (!out) return NEXG_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return NEXG_EDEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return NEXG_EDEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return NEXG_EDEVICE;
    nexg_ctx* c = static_cast<nexg_ctx*>(calloc(1, sizeof(nexg_ctx)));
    if (!c) return NEXG_ENOMEM;
    c->device = device;
    c->cu_count = prop.multiProcessorCount;
    snprintf(c->arch, sizeof(c->arch), "%s", prop.gcnArchName);
    *out = c;
    return NEXG_OK;
}

int nexg_ctx_destroy(nexg_ctx* ctx) {
    if (ctx && (ctx->scratch || ctx->scratch_done)) {
        DeviceGuard g(ctx);
        if (ctx->scratch) (void)hipFree(ctx->scratch);
        if (ctx->scratch_done) (void)hipEventDestroy(ctx->scratch_done);
    }
    free(ctx);
    return NEXG_OK;
}

const char* nexg_ctx_last_error(const nexg_ctx* ctx) { return ctx ? ctx->last_error : ""; }

int nexg_ctx_cu_count(const nexg_ctx* ctx) { return ctx ? ctx->cu_count : 0; }

int nexg_parse_batch(nexg_ctx* ctx, const nexg_frames* frames, const nexg_parse_option* option,
                     int out_kind, void* out, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (out_kind != NEXG_OUT_DESC && out_kind != NEXG_OUT_RECORD && out_kind != NEXG_OUT_SLICE &&
        out_kind != NEXG_OUT_FLAGS && out_kind != NEXG_OUT_VERDICT && out_kind != NEXG_OUT_SPARSE &&
        out_kind != NEXG_OUT_GROUPED)
        return fail(ctx, NEXG_EINVAL, "invalid out_kind%s", nullptr);
    if (frames->count && !out) return fail(ctx, NEXG_EINVAL, "NULL output%s", nullptr);
    const uint64_t align_mask = out_kind == NEXG_OUT_VERDICT ? 1u : out_kind == NEXG_OUT_FLAGS ? 3u
                                : out_kind == NEXG_OUT_DESC  ? 7u : 15u;
    if (misaligned(align_mask, out)) return fail(ctx, NEXG_EINVAL, "misaligned output%s", nullptr);
    DeviceGuard g(ctx);
    nexg::ParseArgs a = parse_args(frames, option);
    a.out = out;
    a.tile_order = nexg::tile_order_for(a);
    const nexg::ParseVariant v = nexg::choose_parse_variant(a);
    const hipStream_t st = as_stream(stream);
    if (nexg::parse_needs_tail(v, out_kind) && a.count) {
        a.tail = static_cast<uint32_t*>(scratch(ctx, a.count * 4u));
        if (!a.tail) return fail(ctx, NEXG_ENOMEM, "device scratch allocation failed%s", nullptr);
        if (int rc = launched(ctx, scratch_acquire(ctx, st))) return rc;
        if (int rc = launched(ctx, nexg::launch_parse(v, a, out_kind, st))) return rc;
        return launched(ctx, scratch_release(ctx, st));
    }
    return launched(ctx, nexg::launch_parse(v, a, out_kind, st));
}

static int sparse_expand(nexg_ctx* ctx, const nexg_frames* frames, const nexg_parse_option* option,
                         const void* sparse, nexg_desc* out, bool grouped, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (frames->count && (!sparse || !out)) return fail(ctx, NEXG_EINVAL, "NULL sparse input or output%s", nullptr);
    if (misaligned(15u, sparse) || misaligned(7u, out))
        return fail(ctx, NEXG_EINVAL, "misaligned sparse input or output%s", nullptr);
    DeviceGuard g(ctx);
    const nexg::ParseArgs a = parse_args(frames, option);
    return launched(ctx, nexg::launch_sparse_expand(a, static_cast<const uint8_t*>(sparse), out, grouped,
                                                    as_stream(stream)));
}

int nexg_sparse_expand(nexg_ctx* ctx, const nexg_frames* frames, const nexg_parse_option* option,
                       const void* sparse, nexg_desc* out, void* stream) {
    return sparse_expand(ctx, frames, option, sparse, out, false, stream);
}

int nexg_grouped_expand(nexg_ctx* ctx, const nexg_frames* frames, const nexg_parse_option* option,
                        const void* grouped, nexg_desc* out, void* stream) {
    return sparse_expand(ctx, frames, option, grouped, out, true, stream);
}

int nexg_recompute_checksums_batch(nexg_ctx* ctx, const nexg_frames* frames, const nexg_parse_option* option,
                                   uint32_t which, nexg_fixup* out, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if ((which & ~(NEXG_FIX_IP | NEXG_FIX_L4)) != 0) return fail(ctx, NEXG_EINVAL, "invalid fix-up selection%s", nullptr);
    if (misaligned(7u, out)) return fail(ctx, NEXG_EINVAL, "misaligned output%s", nullptr);
    DeviceGuard g(ctx);
    const nexg::ParseArgs a = parse_args(frames, option);
    return launched(ctx, nexg::launch_recompute(a, which, out, as_stream(stream)));
}

int nexg_actions_check(const nexg_actions* actions) {
    return nexg::check_actions(actions) ? NEXG_EINVAL : NEXG_OK;
}

int nexg_rewrite_batch(nexg_ctx* ctx, const nexg_frames* frames, const nexg_parse_option* option,
                       const nexg_actions* actions, const uint8_t* action_index, nexg_rewritten* out, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (!option) return fail(ctx, NEXG_EINVAL, "rewrite: NULL option%s", nullptr);
    if (const char* why = nexg::check_actions(actions)) return fail(ctx, NEXG_EINVAL, "rewrite: %s", why);
    if (misaligned(7u, out)) return fail(ctx, NEXG_EINVAL, "misaligned output%s", nullptr);
    if (frames->count == 0) return NEXG_OK;
    DeviceGuard g(ctx);
    const nexg::ParseArgs a = parse_args(frames, option);
    return launched(ctx, nexg::launch_rewrite(a, *actions, action_index, out, as_stream(stream)));
}

int nexg_checksum_batch(nexg_ctx* ctx, const nexg_frames* bufs, uint32_t skipword, uint16_t* out,
                        void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(bufs)) return fail(ctx, NEXG_EINVAL, "invalid buffer batch%s", nullptr);
    if (bufs->count && !out) return fail(ctx, NEXG_EINVAL, "NULL output%s", nullptr);
    nexg::ParseArgs a = to_args(bufs);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_checksum(a, skipword, out, as_stream(stream)));
}

int nexg_decode_options(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records,
                        nexg_options* out, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (frames->count && (!records || !out)) return fail(ctx, NEXG_EINVAL, "NULL records or output%s", nullptr);
    if (misaligned(15u, records, out)) return fail(ctx, NEXG_EINVAL, "misaligned records or output%s", nullptr);
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_decode_options(a, records, out, as_stream(stream)));
}

int nexg_decap_batch(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records,
                     const nexg_decap_option* option, nexg_tunnel* tunnels, uint64_t* inner_off,
                     uint32_t* inner_len, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    uint32_t which = NEXG_DECAP_VXLAN | NEXG_DECAP_GRE, port = 4789u;
    if (option) {
        if (option->reserved != 0) return fail(ctx, NEXG_EINVAL, "decap option: reserved must be 0%s", nullptr);
        if ((option->which & ~(NEXG_DECAP_VXLAN | NEXG_DECAP_GRE)) != 0)
            return fail(ctx, NEXG_EINVAL, "decap option: unknown tunnel kind bits%s", nullptr);
        which = option->which;
        if (option->vxlan_port) port = option->vxlan_port;
    }
    if (frames->count && (!records || !tunnels || !inner_off || !inner_len))
        return fail(ctx, NEXG_EINVAL, "NULL records or output%s", nullptr);
    if (misaligned(15u, records, tunnels) || misaligned(7u, inner_off) || misaligned(3u, inner_len))
        return fail(ctx, NEXG_EINVAL, "misaligned records or output%s", nullptr);
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_decap(a, records, which, port, tunnels, inner_off, inner_len, as_stream(stream)));
}

int nexg_decap_select(nexg_ctx* ctx, const nexg_tunnel* tunnels, const uint64_t* inner_off,
                      const uint32_t* inner_len, uint64_t count, uint32_t inner_mask, uint32_t* out_index,
                      uint64_t* out_off, uint32_t* out_len, uint64_t* out_count, void* workspace,
                      uint64_t workspace_bytes, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (int rc = check_count(ctx, "decap_select", count)) return rc;
    if (!out_count) return fail(ctx, NEXG_EINVAL, "NULL out_count%s", nullptr);
    if (count && (!tunnels || !inner_off || !inner_len || !out_index || !out_off || !out_len || !workspace))
        return fail(ctx, NEXG_EINVAL, "NULL input, output or workspace%s", nullptr);
    if (int rc = check_workspace(ctx, "decap_select", count, workspace_bytes, nexg_decap_select_workspace(count)))
        return rc;
    if (misaligned(15u, tunnels) || misaligned(7u, inner_off, out_off, out_count) ||
        misaligned(3u, inner_len, out_index, out_len, workspace))
        return fail(ctx, NEXG_EINVAL, "misaligned input, output or workspace%s", nullptr);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_decap_select(tunnels, inner_off, inner_len, count, inner_mask, out_index, out_off,
                                                   out_len, out_count, workspace, as_stream(stream)));
}

int nexg_dns_batch(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records,
                   const nexg_dns_option* option, nexg_dns* out, uint64_t* tile_first, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    uint32_t flags = 0u, port = 53u;
    if (option) {
        if (option->reserved != 0) return fail(ctx, NEXG_EINVAL, "dns option: reserved must be 0%s", nullptr);
        if ((option->flags & ~NEXG_DNS_ANY_UDP) != 0)
            return fail(ctx, NEXG_EINVAL, "dns option: unknown flag bits%s", nullptr);
        flags = option->flags;
        if (option->port) port = option->port;
    }
    if (int rc = check_count(ctx, "dns", frames->count)) return rc;
    if (frames->count && (!records || !out || !tile_first))
        return fail(ctx, NEXG_EINVAL, "NULL records or output%s", nullptr);
    if (misaligned(15u, records, out) || misaligned(7u, tile_first))
        return fail(ctx, NEXG_EINVAL, "misaligned records or output%s", nullptr);
    if (!tile_first) return NEXG_OK;  // an empty batch with nowhere to put its total
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_dns(a, records, flags & NEXG_DNS_ANY_UDP, port, out, tile_first, as_stream(stream)));
}

int nexg_dns_entries(nexg_ctx* ctx, const nexg_frames* frames, const nexg_dns* dns, const uint64_t* tile_first,
                     nexg_dns_entry* entries, uint64_t entries_cap, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (int rc = check_count(ctx, "dns", frames->count)) return rc;
    if (frames->count && (!dns || !tile_first)) return fail(ctx, NEXG_EINVAL, "NULL summaries or tile_first%s", nullptr);
    if (entries_cap && !entries) return fail(ctx, NEXG_EINVAL, "NULL entries with a nonzero capacity%s", nullptr);
    if (misaligned(15u, dns, entries) || misaligned(7u, tile_first))
        return fail(ctx, NEXG_EINVAL, "misaligned summaries, tile_first or entries%s", nullptr);
    if (!entries) return NEXG_OK;  // capacity 0: nothing to store
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_dns_entries(a, dns, tile_first, entries, entries_cap, as_stream(stream)));
}

int nexg_filter_check(const nexg_filter* filter) {
    return nexg::prepare_filter(filter, nullptr) ? NEXG_EINVAL : NEXG_OK;
}

int nexg_select_batch(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records,
                      const nexg_filter* filter, uint32_t* out_index, uint64_t* out_off, uint32_t* out_len,
                      uint8_t* out_rule, uint64_t* out_count, void* workspace, uint64_t workspace_bytes,
                      void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    nexg::SelFilter f;
    if (const char* why = nexg::prepare_filter(filter, &f)) return fail(ctx, NEXG_EINVAL, "select: %s", why);
    const uint64_t count = frames->count;
    if (int rc = check_count(ctx, "select", count)) return rc;
    if (!out_count) return fail(ctx, NEXG_EINVAL, "NULL out_count%s", nullptr);
    if (count && (!records || !out_index || !out_off || !out_len || !workspace))
        return fail(ctx, NEXG_EINVAL, "NULL records, output or workspace%s", nullptr);
    if (int rc = check_workspace(ctx, "select", count, workspace_bytes, nexg_select_workspace(count))) return rc;
    if (misaligned(15u, records) || misaligned(7u, out_off, out_count) || misaligned(3u, out_index, out_len, workspace))
        return fail(ctx, NEXG_EINVAL, "misaligned records, output or workspace%s", nullptr);
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_select(a, records, f, out_index, out_off, out_len, out_rule, out_count,
                                             workspace, as_stream(stream)));
}

int nexg_patterns_check(const nexg_patterns* set) {
    return nexg::prepare_patterns(set, nullptr) ? NEXG_EINVAL : NEXG_OK;
}

int nexg_match_batch(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records, const nexg_patterns* set,
                     nexg_match* out, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    nexg::MatchSet s;
    if (const char* why = nexg::prepare_patterns(set, &s)) return fail(ctx, NEXG_EINVAL, "match: %s", why);
    const uint64_t count = frames->count;
    if (int rc = check_count(ctx, "match", count)) return rc;
    if (count && !records && !(s.flags & NEXG_MATCH_FRAME))
        return fail(ctx, NEXG_EINVAL, "match: NULL records without NEXG_MATCH_FRAME%s", nullptr);
    if (count && !out) return fail(ctx, NEXG_EINVAL, "NULL output%s", nullptr);
    const bool reads_records = !(s.flags & NEXG_MATCH_FRAME);  // the whole-frame region never looks at them
    if ((reads_records && misaligned(15u, records)) || misaligned(7u, out))
        return fail(ctx, NEXG_EINVAL, "misaligned records or output%s", nullptr);
    if (count == 0) return NEXG_OK;
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_match(a, records, s, out, as_stream(stream)));
}

int nexg_match_select(nexg_ctx* ctx, const nexg_frames* frames, const nexg_match* matches, uint32_t any_mask,
                      uint32_t all_mask, uint32_t none_mask, uint32_t* out_index, uint64_t* out_off, uint32_t* out_len,
                      uint64_t* out_count, void* workspace, uint64_t workspace_bytes, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    const uint64_t count = frames->count;
    if (int rc = check_count(ctx, "match_select", count)) return rc;
    if (!out_count) return fail(ctx, NEXG_EINVAL, "NULL out_count%s", nullptr);
    if (count && (!matches || !out_index || !out_off || !out_len || !workspace))
        return fail(ctx, NEXG_EINVAL, "NULL rows, output or workspace%s", nullptr);
    if (int rc = check_workspace(ctx, "match_select", count, workspace_bytes, nexg_match_select_workspace(count))) return rc;
    if (misaligned(7u, matches, out_off, out_count) || misaligned(3u, out_index, out_len, workspace))
        return fail(ctx, NEXG_EINVAL, "misaligned rows, output or workspace%s", nullptr);
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_match_select(a, matches, any_mask, all_mask, none_mask, out_index, out_off, out_len,
                                                   out_count, workspace, as_stream(stream)));
}

int nexg_gather_plan(nexg_ctx* ctx, const nexg_frames* sel, uint32_t align, uint64_t* out_offsets,
                     uint32_t* out_len, void* workspace, uint64_t workspace_bytes, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(sel)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (align != 1 && align != 4 && align != 8 && align != 16)
        return fail(ctx, NEXG_EINVAL, "gather_plan: align must be 1, 4, 8 or 16%s", nullptr);
    const uint64_t count = sel->count;
    if (int rc = check_count(ctx, "gather_plan", count)) return rc;
    if (!out_offsets) return fail(ctx, NEXG_EINVAL, "NULL out_offsets%s", nullptr);
    if (count && !workspace) return fail(ctx, NEXG_EINVAL, "NULL workspace%s", nullptr);
    if (int rc = check_workspace(ctx, "gather_plan", count, workspace_bytes, nexg_gather_plan_workspace(count))) return rc;
    if (misaligned(7u, out_offsets, workspace) || misaligned(3u, out_len))
        return fail(ctx, NEXG_EINVAL, "misaligned output or workspace%s", nullptr);
    const nexg::ParseArgs a = to_args(sel);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_gather_plan(a, align, out_offsets, out_len, workspace, as_stream(stream)));
}

int nexg_gather_frames(nexg_ctx* ctx, const nexg_frames* sel, const uint64_t* out_offsets, uint8_t* out_data,
                       uint64_t out_cap, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(sel)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (int rc = check_count(ctx, "gather_frames", sel->count)) return rc;
    if (sel->count && !out_offsets) return fail(ctx, NEXG_EINVAL, "NULL out_offsets%s", nullptr);
    if (out_cap && !out_data) return fail(ctx, NEXG_EINVAL, "NULL out_data with a nonzero capacity%s", nullptr);
    if (misaligned(7u, out_offsets) || misaligned(15u, out_data))
        return fail(ctx, NEXG_EINVAL, "misaligned out_offsets or out_data%s", nullptr);
    const nexg::ParseArgs a = to_args(sel);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_gather_frames(a, out_offsets, out_data, out_cap, as_stream(stream)));
}

int nexg_tunnels_check(const nexg_tunnels* set) { return nexg::check_tunnels(set) ? NEXG_EINVAL : NEXG_OK; }

int nexg_encap_plan(nexg_ctx* ctx, const nexg_frames* frames, const nexg_tunnels* set, const uint8_t* tunnel_index,
                    uint32_t align, uint64_t* out_offsets, uint32_t* out_len, void* workspace, uint64_t workspace_bytes,
                    void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (const char* why = nexg::check_tunnels(set)) return fail(ctx, NEXG_EINVAL, "encap_plan: %s", why);
    if (align != 1 && align != 4 && align != 8 && align != 16)
        return fail(ctx, NEXG_EINVAL, "encap_plan: align must be 1, 4, 8 or 16%s", nullptr);
    const uint64_t count = frames->count;
    if (int rc = check_count(ctx, "encap_plan", count)) return rc;
    if (!out_offsets) return fail(ctx, NEXG_EINVAL, "NULL out_offsets%s", nullptr);
    if (count && !workspace) return fail(ctx, NEXG_EINVAL, "NULL workspace%s", nullptr);
    if (int rc = check_workspace(ctx, "encap_plan", count, workspace_bytes, nexg_encap_plan_workspace(count))) return rc;
    if (misaligned(7u, out_offsets, workspace) || misaligned(3u, out_len))
        return fail(ctx, NEXG_EINVAL, "misaligned output or workspace%s", nullptr);
    nexg::EncapSet es;
    nexg::prepare_tunnels(*set, es);
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_encap_plan(a, es, tunnel_index, align, out_offsets, out_len,
                                                 workspace, as_stream(stream)));
}

int nexg_encap_frames(nexg_ctx* ctx, const nexg_frames* frames, const nexg_tunnels* set, const uint8_t* tunnel_index,
                      const nexg_flow* flows, const uint64_t* out_offsets, uint8_t* out_data, uint64_t out_cap,
                      nexg_encapped* rows, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (const char* why = nexg::check_tunnels(set)) return fail(ctx, NEXG_EINVAL, "encap_frames: %s", why);
    if (int rc = check_count(ctx, "encap_frames", frames->count)) return rc;
    if (!flows && frames->count)
        for (uint32_t i = 0; i < set->n_tunnels; i++)
            if (set->tunnels[i].flags & NEXG_ENCAP_FLOW_PORT)
                return fail(ctx, NEXG_EINVAL, "encap_frames: a spec has FLOW_PORT and flows is NULL%s", nullptr);
    if (frames->count && !out_offsets) return fail(ctx, NEXG_EINVAL, "NULL out_offsets%s", nullptr);
    if (out_cap && !out_data) return fail(ctx, NEXG_EINVAL, "NULL out_data with a nonzero capacity%s", nullptr);
    if (misaligned(7u, out_offsets, flows, rows) || misaligned(15u, out_data))
        return fail(ctx, NEXG_EINVAL, "misaligned out_offsets, flows, rows or out_data%s", nullptr);
    if (frames->count == 0) return NEXG_OK;
    nexg::EncapSet es;
    nexg::prepare_tunnels(*set, es);
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_encap_frames(a, es, tunnel_index, flows, out_offsets, out_data, out_cap, rows,
                                                   as_stream(stream)));
}

int nexg_frag_option_check(const nexg_frag_option* option) { return nexg::check_frag_option(option) ? NEXG_EINVAL : NEXG_OK; }

int nexg_fragment_plan(nexg_ctx* ctx, const nexg_frames* frames, const nexg_frag_option* option, uint32_t* out_first,
                       uint64_t* out_bytes, nexg_fragged* rows, void* workspace, uint64_t workspace_bytes, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (const char* why = nexg::check_frag_option(option)) return fail(ctx, NEXG_EINVAL, "fragment_plan: %s", why);
    const uint64_t count = frames->count;
    if (int rc = check_count(ctx, "fragment_plan", count)) return rc;
    if (!out_first || !out_bytes) return fail(ctx, NEXG_EINVAL, "NULL out_first or out_bytes%s", nullptr);
    if (count && !workspace) return fail(ctx, NEXG_EINVAL, "NULL workspace%s", nullptr);
    if (int rc = check_workspace(ctx, "fragment_plan", count, workspace_bytes, nexg_fragment_plan_workspace(count))) return rc;
    if (misaligned(7u, out_bytes, workspace) || misaligned(3u, out_first) || misaligned(15u, rows))
        return fail(ctx, NEXG_EINVAL, "misaligned output, rows or workspace%s", nullptr);
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_fragment_plan(a, option->mtu, option->flags, option->align, out_first, out_bytes, rows,
                                                    workspace, as_stream(stream)));
}

int nexg_fragment_frames(nexg_ctx* ctx, const nexg_frames* frames, const nexg_frag_option* option,
                         const uint32_t* out_first, const uint64_t* out_bytes, uint64_t out_count, uint64_t* out_offsets,
                         uint32_t* out_len, uint32_t* out_src, uint8_t* out_data, uint64_t out_cap, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (const char* why = nexg::check_frag_option(option)) return fail(ctx, NEXG_EINVAL, "fragment_frames: %s", why);
    if (int rc = check_count(ctx, "fragment_frames", frames->count)) return rc;
    if (out_count > 0xFFFFFFFFull) return fail(ctx, NEXG_EINVAL, "fragment_frames: more than 2^32 - 1 output frames%s", nullptr);
    if (!out_first || !out_bytes || !out_offsets) return fail(ctx, NEXG_EINVAL, "NULL out_first, out_bytes or out_offsets%s", nullptr);
    if (out_count && (!out_len || !out_src)) return fail(ctx, NEXG_EINVAL, "NULL out_len or out_src%s", nullptr);
    if (out_cap && !out_data) return fail(ctx, NEXG_EINVAL, "NULL out_data with a nonzero capacity%s", nullptr);
    if (misaligned(7u, out_bytes, out_offsets) || misaligned(3u, out_first, out_len, out_src) || misaligned(15u, out_data))
        return fail(ctx, NEXG_EINVAL, "misaligned out_first, out_bytes, table or out_data%s", nullptr);
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_fragment_frames(a, option->mtu, option->flags, option->align, out_first, out_bytes,
                                                      out_count, out_offsets, out_len, out_src, out_data, out_cap,
                                                      as_stream(stream)));
}

int nexg_reasm_plan(nexg_ctx* ctx, const nexg_frames* frames, uint32_t align, uint32_t* out_first, uint64_t* out_bytes,
                    nexg_reasm* rows, void* workspace, uint64_t workspace_bytes, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (align != 1 && align != 4 && align != 8 && align != 16)
        return fail(ctx, NEXG_EINVAL, "reasm_plan: align must be 1, 4, 8 or 16%s", nullptr);
    const uint64_t count = frames->count;
    if (int rc = check_count(ctx, "reasm_plan", count)) return rc;
    if (!out_first || !out_bytes) return fail(ctx, NEXG_EINVAL, "NULL out_first or out_bytes%s", nullptr);
    if (count && (!rows || !workspace)) return fail(ctx, NEXG_EINVAL, "NULL rows or workspace%s", nullptr);
    if (int rc = check_workspace(ctx, "reasm_plan", count, workspace_bytes, nexg_reasm_plan_workspace(count))) return rc;
    if (misaligned(7u, out_bytes) || misaligned(3u, out_first) || misaligned(15u, rows, workspace))
        return fail(ctx, NEXG_EINVAL, "misaligned output, rows or workspace%s", nullptr);
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_reasm_plan(a, align, out_first, out_bytes, rows, workspace, as_stream(stream)));
}

int nexg_reasm_frames(nexg_ctx* ctx, const nexg_frames* frames, uint32_t align, const nexg_reasm* rows,
                      const uint32_t* out_first, const uint64_t* out_bytes, uint64_t out_count, uint64_t* out_offsets,
                      uint32_t* out_len, uint32_t* out_src, uint8_t* out_data, uint64_t out_cap, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (align != 1 && align != 4 && align != 8 && align != 16)
        return fail(ctx, NEXG_EINVAL, "reasm_frames: align must be 1, 4, 8 or 16%s", nullptr);
    if (int rc = check_count(ctx, "reasm_frames", frames->count)) return rc;
    if (out_count > 0xFFFFFFFFull) return fail(ctx, NEXG_EINVAL, "reasm_frames: more than 2^32 - 1 output frames%s", nullptr);
    if (!out_first || !out_bytes || !out_offsets) return fail(ctx, NEXG_EINVAL, "NULL out_first, out_bytes or out_offsets%s", nullptr);
    if (frames->count && !rows) return fail(ctx, NEXG_EINVAL, "NULL rows%s", nullptr);
    if (out_count && (!out_len || !out_src)) return fail(ctx, NEXG_EINVAL, "NULL out_len or out_src%s", nullptr);
    if (out_cap && !out_data) return fail(ctx, NEXG_EINVAL, "NULL out_data with a nonzero capacity%s", nullptr);
    if (misaligned(7u, out_bytes, out_offsets) || misaligned(3u, out_first, out_len, out_src) || misaligned(15u, out_data, rows))
        return fail(ctx, NEXG_EINVAL, "misaligned rows, out_first, out_bytes, table or out_data%s", nullptr);
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_reasm_frames(a, align, rows, out_first, out_bytes, out_count, out_offsets, out_len,
                                                   out_src, out_data, out_cap, as_stream(stream)));
}

int nexg_reasm_held(nexg_ctx* ctx, const nexg_frames* frames, const nexg_reasm* rows, uint64_t count, uint32_t* out_index,
                    uint64_t* out_off, uint32_t* out_len, uint64_t* out_count, void* workspace, uint64_t workspace_bytes,
                    void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (count != frames->count) return fail(ctx, NEXG_EINVAL, "reasm_held: count is not the table's%s", nullptr);
    if (int rc = check_count(ctx, "reasm_held", count)) return rc;
    if (!out_count) return fail(ctx, NEXG_EINVAL, "NULL out_count%s", nullptr);
    if (count && (!rows || !out_index || !out_off || !out_len || !workspace))
        return fail(ctx, NEXG_EINVAL, "NULL rows, output or workspace%s", nullptr);
    if (int rc = check_workspace(ctx, "reasm_held", count, workspace_bytes, nexg_reasm_held_workspace(count))) return rc;
    if (misaligned(15u, rows) || misaligned(7u, out_off, out_count) || misaligned(3u, out_index, out_len, workspace))
        return fail(ctx, NEXG_EINVAL, "misaligned rows, output or workspace%s", nullptr);
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_reasm_held(a, rows, out_index, out_off, out_len, out_count, workspace, as_stream(stream)));
}

int nexg_gather_rows(nexg_ctx* ctx, const void* rows, uint32_t row_bytes, uint64_t rows_count,
                     const uint32_t* index, uint64_t n, void* out, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (row_bytes != 4 && row_bytes != 8 && row_bytes != 16 && row_bytes != 32 && row_bytes != 64)
        return fail(ctx, NEXG_EINVAL, "gather_rows: row_bytes must be 4, 8, 16, 32 or 64%s", nullptr);
    if (n > 0xFFFFFFFFull) return fail(ctx, NEXG_EINVAL, "gather_rows: more than 2^32 - 1 rows%s", nullptr);
    if (n && (!index || !out || (rows_count && !rows)))
        return fail(ctx, NEXG_EINVAL, "NULL rows, index or output%s", nullptr);
    const uint64_t am = (row_bytes < 16u ? row_bytes : 16u) - 1u;
    if (misaligned(am, rows, out) || misaligned(3u, index))
        return fail(ctx, NEXG_EINVAL, "misaligned rows, index or output%s", nullptr);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_gather_rows(rows, row_bytes, rows_count, index, n, out, as_stream(stream)));
}

int nexg_flow_batch(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records,
                    const nexg_flow_option* option, nexg_flow* out, void* stream) {
    static const uint8_t default_key[40] = NEXG_FLOW_DEFAULT_KEY;
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    uint32_t flags;
    if (int rc = flow_option_flags(ctx, option, flags)) return rc;
    const uint8_t* key = (flags & NEXG_FLOW_KEY) ? option->key : default_key;
    if (frames->count && (!records || !out)) return fail(ctx, NEXG_EINVAL, "NULL records or output%s", nullptr);
    if (misaligned(15u, records) || misaligned(7u, out))
        return fail(ctx, NEXG_EINVAL, "misaligned records or output%s", nullptr);
    nexg::FlowKey k;
    for (uint32_t i = 0; i < 10; i++)
        k.w[i] = (uint32_t)key[4 * i] << 24 | (uint32_t)key[4 * i + 1] << 16 | (uint32_t)key[4 * i + 2] << 8 |
                 (uint32_t)key[4 * i + 3];
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_flow(a, records, flags, k, out, as_stream(stream)));
}

int nexg_flow_partition(nexg_ctx* ctx, const nexg_frames* frames, const nexg_flow* flows, uint32_t buckets,
                        uint32_t* out_index, uint64_t* out_off, uint32_t* out_len, uint64_t* bucket_first,
                        void* workspace, uint64_t workspace_bytes, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (buckets < 1u || buckets > 256u) return fail(ctx, NEXG_EINVAL, "flow_partition: buckets must be 1..256%s", nullptr);
    const uint64_t count = frames->count;
    if (int rc = check_count(ctx, "flow_partition", count)) return rc;
    if (!bucket_first) return fail(ctx, NEXG_EINVAL, "NULL bucket_first%s", nullptr);
    if ((out_off == nullptr) != (out_len == nullptr))
        return fail(ctx, NEXG_EINVAL, "flow_partition: out_off and out_len go together%s", nullptr);
    if (count && (!flows || !out_index || !workspace))
        return fail(ctx, NEXG_EINVAL, "NULL flows, output or workspace%s", nullptr);
    const uint64_t need = nexg_flow_partition_workspace(count, buckets);
    if (int rc = check_workspace(ctx, "flow_partition", count, workspace_bytes, need)) return rc;
    if (misaligned(7u, flows, out_off, bucket_first, workspace) || misaligned(3u, out_index, out_len))
        return fail(ctx, NEXG_EINVAL, "misaligned flows, output or workspace%s", nullptr);
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_flow_partition(a, flows, buckets, out_index, out_off, out_len, bucket_first,
                                                     workspace, as_stream(stream)));
}

int nexg_flow_sort(nexg_ctx* ctx, const nexg_flow* flows, uint64_t count, uint32_t* out_index, void* workspace,
                   uint64_t workspace_bytes, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (int rc = check_count(ctx, "flow_sort", count)) return rc;
    if (count && (!flows || !out_index || !workspace))
        return fail(ctx, NEXG_EINVAL, "NULL flows, output or workspace%s", nullptr);
    if (int rc = check_workspace(ctx, "flow_sort", count, workspace_bytes, nexg_flow_sort_workspace(count))) return rc;
    if (misaligned(7u, flows, workspace) || misaligned(3u, out_index))
        return fail(ctx, NEXG_EINVAL, "misaligned flows, output or workspace%s", nullptr);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_flow_sort(flows, count, out_index, workspace, as_stream(stream)));
}

int nexg_flow_groups(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records, const nexg_flow* flows,
                     const nexg_flow_option* option, const uint32_t* order, nexg_flow_group* out, uint64_t groups_cap,
                     uint32_t* out_group, uint64_t* out_count, void* workspace, uint64_t workspace_bytes, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    uint32_t flags;
    if (int rc = flow_option_flags(ctx, option, flags)) return rc;
    const uint64_t count = frames->count;
    if (int rc = check_count(ctx, "flow_groups", count)) return rc;
    if (!out_count) return fail(ctx, NEXG_EINVAL, "NULL out_count%s", nullptr);
    if (count && (!records || !flows || !order || !workspace || (groups_cap && !out)))
        return fail(ctx, NEXG_EINVAL, "NULL records, flows, order, output or workspace%s", nullptr);
    if (int rc = check_workspace(ctx, "flow_groups", count, workspace_bytes, nexg_flow_groups_workspace(count))) return rc;
    if (misaligned(15u, records, out) || misaligned(7u, flows, out_count, workspace) || misaligned(3u, order, out_group))
        return fail(ctx, NEXG_EINVAL, "misaligned records, flows, order, output or workspace%s", nullptr);
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_flow_groups(a, records, flows, flags, order, out, groups_cap, out_group, out_count,
                                                  workspace, as_stream(stream)));
}

int nexg_flow_table_merge(nexg_ctx* ctx, const nexg_frames* frames, const nexg_record* records,
                          const nexg_flow_option* option, const nexg_flow_group* groups, uint64_t n_groups,
                          const nexg_flow_entry* table_in, uint64_t n_in, uint32_t epoch, uint32_t min_epoch,
                          nexg_flow_entry* table_out, uint64_t table_cap, uint32_t* out_slot, uint64_t* out_count,
                          void* workspace, uint64_t workspace_bytes, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    uint32_t flags;
    if (int rc = flow_option_flags(ctx, option, flags)) return rc;
    if (n_in > 0x7FFFFFFFull || n_groups > 0x7FFFFFFFull)
        return fail(ctx, NEXG_EINVAL, "flow_table: more than 2^31 - 1 entries or groups%s", nullptr);
    if (!out_count) return fail(ctx, NEXG_EINVAL, "NULL out_count%s", nullptr);
    const uint64_t n = n_in + n_groups;
    if ((n_groups && (!groups || (frames->count && !records))) || (n_in && !table_in) || (table_cap && !table_out) ||
        (n && !workspace))
        return fail(ctx, NEXG_EINVAL, "NULL records, groups, table or workspace%s", nullptr);
    if (int rc = check_workspace(ctx, "flow_table", n, workspace_bytes, nexg_flow_table_workspace(n_in, n_groups))) return rc;
    if (misaligned(15u, records, groups, table_in, table_out) || misaligned(7u, out_count, workspace) ||
        misaligned(3u, out_slot))
        return fail(ctx, NEXG_EINVAL, "misaligned records, groups, table, output or workspace%s", nullptr);
    // table_out[0, table_cap) against table_in[0, n_in), as addresses (a capacity that runs past the
    // address space ends there)
    const uint64_t in0 = reinterpret_cast<uint64_t>(table_in), out0 = reinterpret_cast<uint64_t>(table_out);
    const uint64_t room = (~0ull - out0) / sizeof(nexg_flow_entry);
    const uint64_t out1 = out0 + (table_cap < room ? table_cap : room) * sizeof(nexg_flow_entry);
    if (n_in && table_cap && in0 < out1 && out0 < in0 + n_in * sizeof(nexg_flow_entry))
        return fail(ctx, NEXG_EINVAL, "flow_table: table_out overlaps table_in%s", nullptr);
    const nexg::ParseArgs a = to_args(frames);
    DeviceGuard g(ctx);
    return launched(ctx, nexg::launch_flow_table_merge(a, records, flags, groups, n_groups, table_in, n_in, epoch, min_epoch,
                                                       table_out, table_cap, out_slot, out_count, workspace,
                                                       as_stream(stream)));
}

int nexg_probe_stream(nexg_ctx* ctx, const void* data, uint64_t bytes, uint32_t out_per_64,
                      void* out, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    const bool wo = out_per_64 == 64;  // write-only: data unused
    if (bytes % 16384u != 0 || (bytes && ((!wo && !data) || !out)) ||
        (out_per_64 != 0 && out_per_64 != 8 && out_per_64 != 9 && !wo) || (reinterpret_cast<uint64_t>(data) & 15u) != 0 ||
        (reinterpret_cast<uint64_t>(out) & (wo ? 15u : 7u)) != 0)
        return fail(ctx, NEXG_EINVAL, "probe: bytes must be a multiple of 16384, buffers aligned%s", nullptr);
    if (bytes / 16384u > 0x7FFFFFFFull) return fail(ctx, NEXG_ERANGE, "probe: too many tiles%s", nullptr);
    DeviceGuard g(ctx);
    return hip_status(ctx, nexg::launch_probe_stream(static_cast<const uint8_t*>(data), bytes / 16384u,
                                                     out_per_64, out, static_cast<hipStream_t>(stream)),
                      NEXG_ELAUNCH);
}

int nexg_probe_span_clock(nexg_ctx* ctx, const nexg_frames* frames, const nexg_parse_option* option, void* out,
                          uint64_t* stamps, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!frames_valid(frames)) return fail(ctx, NEXG_EINVAL, "invalid frame batch%s", nullptr);
    if (frames->count && (!out || !stamps)) return fail(ctx, NEXG_EINVAL, "NULL output or stamps%s", nullptr);
    if (misaligned(15u, out) || misaligned(7u, stamps))
        return fail(ctx, NEXG_EINVAL, "misaligned output or stamps%s", nullptr);
    DeviceGuard g(ctx);
    nexg::ParseArgs a = parse_args(frames, option);
    a.out = out;
    a.tile_order = nexg::tile_order_for(a);
    a.stamps = stamps;
    if (nexg::choose_parse_variant(a) != nexg::ParseVariant::SpanTile)
        return fail(ctx, NEXG_EINVAL, "probe_span_clock: the batch does not take the span kernel%s", nullptr);
    return launched(ctx, nexg::launch_span_clock(a, as_stream(stream)));
}

int nexg_probe_latency(nexg_ctx* ctx, void* buf, uint64_t bytes, uint32_t steps, uint32_t start, uint32_t loaded,
                       uint64_t* out, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (!buf || !out || bytes < 64u * 65536u || bytes / 64u > 0xFFFFFFFFull || steps == 0 || steps > (1u << 20) ||
        (reinterpret_cast<uint64_t>(buf) & 15u) != 0 || (reinterpret_cast<uint64_t>(out) & 7u) != 0)
        return fail(ctx, NEXG_EINVAL, "probe_latency: buffer of at least 4 MiB (16-B aligned), 1..2^20 steps%s", nullptr);
    DeviceGuard g(ctx);
    // loaded: one reading workgroup per CU x 4, at most 64 passes over the buffer
    const uint32_t wgs = loaded ? (uint32_t)ctx->cu_count * 4u : 0u;
    return hip_status(ctx, nexg::launch_probe_latency(static_cast<uint32_t*>(buf), (uint32_t)(bytes / 64u), start, steps,
                                                      wgs, 64u, out, static_cast<hipStream_t>(stream)),
                      NEXG_ELAUNCH);
}

int nexg_build_udp4_batch(nexg_ctx* ctx, const nexg_udp4_build* p, uint8_t* out,
                          uint32_t out_stride, void* stream) {
    if (!ctx || !p) return NEXG_EINVAL;
    if (28ull + p->payload_len > 65535ull)
        return fail(ctx, NEXG_ERANGE, "UDP/IPv4 length overflow%s", nullptr);
    if (p->count && (!p->dst_ip || !out))
        return fail(ctx, NEXG_EINVAL, "NULL address array or output%s", nullptr);
    if (p->payload_len && !p->payload) return fail(ctx, NEXG_EINVAL, "NULL payload%s", nullptr);
    if (out_stride < 42u + p->payload_len)
        return fail(ctx, NEXG_EINVAL, "out_stride shorter than a frame%s", nullptr);
    DeviceGuard g(ctx);
    return hip_status(ctx, nexg::launch_build_udp4(*p, out, out_stride, static_cast<hipStream_t>(stream)),
                      NEXG_ELAUNCH);
}

int nexg_build_udp4_tuples(nexg_ctx* ctx, const nexg_udp4_build* p, const nexg_udp4_tuple* tuples, uint8_t* out,
                           uint32_t out_stride, void* stream) {
    if (!ctx || !p) return NEXG_EINVAL;
    if (28ull + p->payload_len > 65535ull)
        return fail(ctx, NEXG_ERANGE, "UDP/IPv4 length overflow%s", nullptr);
    if (p->src_ip || p->dst_ip || p->src_port || p->dst_port || p->ip_id || p->src_mac || p->dst_mac)
        return fail(ctx, NEXG_EINVAL, "per-frame arrays come from the tuples: pass NULL%s", nullptr);
    if (p->count && (!tuples || !out))
        return fail(ctx, NEXG_EINVAL, "NULL tuples or output%s", nullptr);
    if ((reinterpret_cast<uint64_t>(tuples) & 15u) != 0)
        return fail(ctx, NEXG_EINVAL, "tuples must be 16-B aligned%s", nullptr);
    if (p->payload_len && !p->payload) return fail(ctx, NEXG_EINVAL, "NULL payload%s", nullptr);
    if (out_stride < 42u + p->payload_len)
        return fail(ctx, NEXG_EINVAL, "out_stride shorter than a frame%s", nullptr);
    DeviceGuard g(ctx);
    return hip_status(ctx, nexg::launch_build_udp4_tuples(*p, tuples, out, out_stride, static_cast<hipStream_t>(stream)),
                      NEXG_ELAUNCH);
}

int nexg_build_udp6_batch(nexg_ctx* ctx, const nexg_udp6_build* p, uint8_t* out,
                          uint32_t out_stride, void* stream) {
    if (!ctx || !p) return NEXG_EINVAL;
    if (8ull + p->payload_len > 65535ull)
        return fail(ctx, NEXG_ERANGE, "UDP/IPv6 length overflow%s", nullptr);
    // src_ip is per frame here (no def_src_ip: only the IPv4 probe batch has one)
    if (p->count && (!p->src_ip || !p->dst_ip || !out))
        return fail(ctx, NEXG_EINVAL, "NULL address array or output%s", nullptr);
    if (((reinterpret_cast<uint64_t>(p->src_ip) | reinterpret_cast<uint64_t>(p->dst_ip)) & 3u) != 0)
        return fail(ctx, NEXG_EINVAL, "address arrays must be 4-B aligned%s", nullptr);
    if (p->payload_len && !p->payload) return fail(ctx, NEXG_EINVAL, "NULL payload%s", nullptr);
    if (out_stride < 62u + p->payload_len)
        return fail(ctx, NEXG_EINVAL, "out_stride shorter than a frame%s", nullptr);
    DeviceGuard g(ctx);
    return hip_status(ctx, nexg::launch_build_udp6(*p, out, out_stride, static_cast<hipStream_t>(stream)),
                      NEXG_ELAUNCH);
}

static int check_ip_build(nexg_ctx* ctx, const nexg_ip_build& ip, uint64_t count, const uint8_t* out) {
    if (ip.family != 4 && ip.family != 6) return fail(ctx, NEXG_EINVAL, "IP family must be 4 or 6%s", nullptr);
    if (count && (!ip.src_ip || !ip.dst_ip || !out))
        return fail(ctx, NEXG_EINVAL, "NULL address array or output%s", nullptr);
    if (((reinterpret_cast<uint64_t>(ip.src_ip) | reinterpret_cast<uint64_t>(ip.dst_ip)) & 3u) != 0)
        return fail(ctx, NEXG_EINVAL, "address arrays must be 4-B aligned%s", nullptr);
    return NEXG_OK;
}

int nexg_build_tcp_batch(nexg_ctx* ctx, const nexg_tcp_build* p, uint8_t* out, uint32_t out_stride,
                         void* stream) {
    if (!ctx || !p) return NEXG_EINVAL;
    if (int rc = check_ip_build(ctx, p->ip, p->count, out)) return rc;
    const uint64_t padded = (p->options_len + 3u) & ~3u;
    if (p->options_len > 40u || padded > 40u)  // builder/tcp.rs:128-135
        return fail(ctx, NEXG_ERANGE, "TCP options longer than 40 B%s", nullptr);
    const uint64_t seg = 20u + padded + p->payload_len;
    if (seg > (p->ip.family == 4 ? 65535u - 20u : 65535u))  // builder/tcp.rs:94-99, 146-152
        return fail(ctx, NEXG_ERANGE, "TCP segment length overflow%s", nullptr);
    if (p->payload_len && !p->payload) return fail(ctx, NEXG_EINVAL, "NULL payload%s", nullptr);
    const uint64_t flen = 14u + (p->ip.family == 4 ? 20u : 40u) + seg;
    if (out_stride < flen) return fail(ctx, NEXG_EINVAL, "out_stride shorter than a frame%s", nullptr);
    DeviceGuard g(ctx);
    return hip_status(ctx, nexg::launch_build_tcp(*p, out, out_stride, static_cast<hipStream_t>(stream)),
                      NEXG_ELAUNCH);
}

int nexg_build_icmp_echo_batch(nexg_ctx* ctx, const nexg_icmp_echo_build* p, uint8_t* out,
                               uint32_t out_stride, void* stream) {
    if (!ctx || !p) return NEXG_EINVAL;
    if (int rc = check_ip_build(ctx, p->ip, p->count, out)) return rc;
    const uint64_t len = 8u + (uint64_t)p->payload_len;
    if (len > (p->ip.family == 4 ? 65535u - 20u : 65535u))  // builder/icmp.rs:67-80, icmpv6.rs:72-86
        return fail(ctx, NEXG_ERANGE, "ICMP packet length overflow%s", nullptr);
    if (p->payload_len && !p->payload) return fail(ctx, NEXG_EINVAL, "NULL payload%s", nullptr);
    const uint64_t flen = 14u + (p->ip.family == 4 ? 20u : 40u) + len;
    if (out_stride < flen) return fail(ctx, NEXG_EINVAL, "out_stride shorter than a frame%s", nullptr);
    DeviceGuard g(ctx);
    return hip_status(ctx, nexg::launch_build_icmp_echo(*p, out, out_stride, static_cast<hipStream_t>(stream)),
                      NEXG_ELAUNCH);
}

int nexg_build_arp_batch(nexg_ctx* ctx, const nexg_arp_build* p, uint8_t* out, uint32_t out_stride,
                         void* stream) {
    if (!ctx || !p) return NEXG_EINVAL;
    if (p->hw_addr_len != 6)  // builder/arp.rs:101-108 BuildError::InvalidFieldLength
        return fail(ctx, NEXG_EINVAL, "InvalidFieldLength: ARP hardware address (expected 6)%s", nullptr);
    if (p->proto_addr_len != 4)  // builder/arp.rs:109-115
        return fail(ctx, NEXG_EINVAL, "InvalidFieldLength: ARP protocol address (expected 4)%s", nullptr);
    if (p->count && (!p->target_ip || !out)) return fail(ctx, NEXG_EINVAL, "NULL target array or output%s", nullptr);
    if (out_stride < 42u) return fail(ctx, NEXG_EINVAL, "out_stride shorter than a frame%s", nullptr);
    DeviceGuard g(ctx);
    return hip_status(ctx, nexg::launch_build_arp(*p, out, out_stride, static_cast<hipStream_t>(stream)), NEXG_ELAUNCH);
}

int nexg_build_ndp_ns_batch(nexg_ctx* ctx, const nexg_ndp_ns_build* p, uint8_t* out, uint32_t out_stride,
                            void* stream) {
    if (!ctx || !p) return NEXG_EINVAL;
    if (p->ip.family != 6) return fail(ctx, NEXG_EINVAL, "NDP needs IP family 6%s", nullptr);
    if (int rc = check_ip_build(ctx, p->ip, p->count, out)) return rc;
    if (out_stride < 86u) return fail(ctx, NEXG_EINVAL, "out_stride shorter than a frame%s", nullptr);
    DeviceGuard g(ctx);
    return hip_status(ctx, nexg::launch_build_ndp_ns(*p, out, out_stride, static_cast<hipStream_t>(stream)),
                      NEXG_ELAUNCH);
}

int nexg_gen_lengths(nexg_ctx* ctx, int workload, uint64_t seed, uint64_t first_index,
                     uint64_t count, uint32_t* lengths, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (workload != NEXG_WL_UDP64 && workload != NEXG_WL_IMIX) return fail(ctx, NEXG_EINVAL, "workload%s", nullptr);
    if (count && !lengths) return fail(ctx, NEXG_EINVAL, "NULL lengths%s", nullptr);
    DeviceGuard g(ctx);
    return hip_status(ctx, nexg::launch_gen_lengths(workload, seed, first_index, count, lengths,
                                                    static_cast<hipStream_t>(stream)),
                      NEXG_ELAUNCH);
}

int nexg_gen_frames(nexg_ctx* ctx, int workload, uint64_t seed, uint64_t first_index,
                    uint64_t count, uint8_t* data, const uint64_t* offsets, uint32_t stride,
                    void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (workload != NEXG_WL_UDP64 && workload != NEXG_WL_IMIX) return fail(ctx, NEXG_EINVAL, "workload%s", nullptr);
    if (count && !data) return fail(ctx, NEXG_EINVAL, "NULL data%s", nullptr);
    if (!offsets && stride < (workload == NEXG_WL_UDP64 ? 64u : 1500u))
        return fail(ctx, NEXG_EINVAL, "stride shorter than the workload's frames%s", nullptr);
    DeviceGuard g(ctx);
    return hip_status(ctx, nexg::launch_gen_frames(workload, seed, first_index, count, data, offsets,
                                                   stride, static_cast<hipStream_t>(stream)),
                      NEXG_ELAUNCH);
}

int nexg_gen_udp4_params(nexg_ctx* ctx, uint64_t seed, uint64_t first_index, uint64_t count,
                         uint32_t* src_ip, uint32_t* dst_ip, uint16_t* src_port,
                         uint16_t* dst_port, uint16_t* ip_id, void* stream) {
    if (!ctx) return NEXG_EINVAL;
    if (count && (!src_ip || !dst_ip || !src_port || !dst_port || !ip_id))
        return fail(ctx, NEXG_EINVAL, "NULL output array%s", nullptr);
    DeviceGuard g(ctx);
    return hip_status(ctx, nexg::launch_gen_udp4_params(seed, first_index, count, src_ip, dst_ip,
                                                        src_port, dst_port, ip_id,
                                                        static_cast<hipStream_t>(stream)),
                      NEXG_ELAUNCH);
}

}  // extern "C"
