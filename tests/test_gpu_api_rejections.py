"""GPU: what the second-pass entries of the C ABI answer to a bad call.

One literal table: each row is a valid call of one entry with exactly one
defect, the status it must return and the nexg_ctx_last_error text, compared
for equality. Every defect is refused before any launch (nexg_api.hip), so the
order of an entry's checks is free. A second table holds each entry's empty
batch as include/nexg.h documents it: count 0 and every optional pointer NULL
is NEXG_OK, and *out_count, bucket_first and out_offsets[0] come back zero.
The valid call is a batch of 257 frames of 64 B (two tiles, one partial)."""
import ctypes

import pytest

from nex_amd import abi

pytestmark = pytest.mark.gpu

N = 257
BUCKETS = 8
ENTRIES_CAP = 64
E = abi.EINVAL
NULL = "NULL"    # the argument (or frames.data) as a NULL pointer
SHORT = "SHORT"  # workspace_bytes one byte below the entry's nexg_*_workspace
HUGE = 1 << 62   # a workspace_bytes that covers 2^32 frames: the count stays the only defect


def off(k):
    """The pointer moved up by k bytes: one alignment step below its requirement."""
    return ("off", k)


SIGNATURES = {
    "nexg_decap_batch": "ctx frames records option tunnels inner_off inner_len stream",
    "nexg_decap_select": "ctx tunnels inner_off inner_len count inner_mask out_index out_off out_len out_count "
                         "workspace workspace_bytes stream",
    "nexg_dns_batch": "ctx frames records option out tile_first stream",
    "nexg_dns_entries": "ctx frames dns tile_first entries entries_cap stream",
    "nexg_select_batch": "ctx frames records filter out_index out_off out_len out_rule out_count workspace "
                         "workspace_bytes stream",
    "nexg_gather_plan": "ctx frames align out_offsets out_len workspace workspace_bytes stream",
    "nexg_gather_frames": "ctx frames out_offsets out_data out_cap stream",
    "nexg_gather_rows": "ctx rows row_bytes rows_count index n out stream",
    "nexg_flow_batch": "ctx frames records option out stream",
    "nexg_flow_partition": "ctx frames flows buckets out_index out_off out_len bucket_first workspace "
                           "workspace_bytes stream",
    "nexg_flow_sort": "ctx flows count out_index workspace workspace_bytes stream",
    "nexg_flow_groups": "ctx frames records flows option order out groups_cap out_group out_count workspace "
                        "workspace_bytes stream",
}

# frames_valid: the same four defects for every entry that takes a frame table
FRAMES = [
    ({"frames": NULL}, E, "invalid frame batch"),
    ({"frames.data": NULL}, E, "invalid frame batch"),
    ({"frames.data": off(2)}, E, "invalid frame batch"),
    ({"frames.stride": 0}, E, "invalid frame batch"),
]

REJECTIONS = {
    "nexg_decap_batch": [
        ({"ctx": NULL}, E, ""),
        *FRAMES,
        ({"option.reserved": 1}, E, "decap option: reserved must be 0"),
        ({"option.which": 4}, E, "decap option: unknown tunnel kind bits"),
        ({"records": NULL}, E, "NULL records or output"),
        ({"tunnels": NULL}, E, "NULL records or output"),
        ({"inner_off": NULL}, E, "NULL records or output"),
        ({"inner_len": NULL}, E, "NULL records or output"),
        ({"records": off(8)}, E, "misaligned records or output"),
        ({"tunnels": off(8)}, E, "misaligned records or output"),
        ({"inner_off": off(4)}, E, "misaligned records or output"),
        ({"inner_len": off(2)}, E, "misaligned records or output"),
    ],
    "nexg_decap_select": [
        ({"ctx": NULL}, E, ""),
        ({"count": 1 << 32, "workspace_bytes": HUGE}, E, "decap_select: more than 2^32 - 1 frames"),
        ({"out_count": NULL}, E, "NULL out_count"),
        ({"tunnels": NULL}, E, "NULL input, output or workspace"),
        ({"inner_off": NULL}, E, "NULL input, output or workspace"),
        ({"inner_len": NULL}, E, "NULL input, output or workspace"),
        ({"out_index": NULL}, E, "NULL input, output or workspace"),
        ({"out_off": NULL}, E, "NULL input, output or workspace"),
        ({"out_len": NULL}, E, "NULL input, output or workspace"),
        ({"workspace": NULL}, E, "NULL input, output or workspace"),
        ({"workspace_bytes": SHORT}, E, "decap_select: workspace smaller than nexg_decap_select_workspace"),
        ({"tunnels": off(8)}, E, "misaligned input, output or workspace"),
        ({"inner_off": off(4)}, E, "misaligned input, output or workspace"),
        ({"out_off": off(4)}, E, "misaligned input, output or workspace"),
        ({"out_count": off(4)}, E, "misaligned input, output or workspace"),
        ({"inner_len": off(2)}, E, "misaligned input, output or workspace"),
        ({"out_index": off(2)}, E, "misaligned input, output or workspace"),
        ({"out_len": off(2)}, E, "misaligned input, output or workspace"),
        ({"workspace": off(2)}, E, "misaligned input, output or workspace"),
    ],
    "nexg_dns_batch": [
        ({"ctx": NULL}, E, ""),
        *FRAMES,
        ({"option.reserved": 1}, E, "dns option: reserved must be 0"),
        ({"option.flags": 2}, E, "dns option: unknown flag bits"),
        ({"frames.count": 1 << 32}, E, "dns: more than 2^32 - 1 frames"),
        ({"records": NULL}, E, "NULL records or output"),
        ({"out": NULL}, E, "NULL records or output"),
        ({"tile_first": NULL}, E, "NULL records or output"),
        ({"records": off(8)}, E, "misaligned records or output"),
        ({"out": off(8)}, E, "misaligned records or output"),
        ({"tile_first": off(4)}, E, "misaligned records or output"),
    ],
    "nexg_dns_entries": [
        ({"ctx": NULL}, E, ""),
        *FRAMES,
        ({"frames.count": 1 << 32}, E, "dns: more than 2^32 - 1 frames"),
        ({"dns": NULL}, E, "NULL summaries or tile_first"),
        ({"tile_first": NULL}, E, "NULL summaries or tile_first"),
        ({"entries": NULL}, E, "NULL entries with a nonzero capacity"),
        ({"dns": off(8)}, E, "misaligned summaries, tile_first or entries"),
        ({"entries": off(8)}, E, "misaligned summaries, tile_first or entries"),
        ({"tile_first": off(4)}, E, "misaligned summaries, tile_first or entries"),
    ],
    "nexg_select_batch": [
        ({"ctx": NULL}, E, ""),
        *FRAMES,
        ({"filter": NULL}, E, "select: NULL filter"),
        ({"frames.count": 1 << 32, "workspace_bytes": HUGE}, E, "select: more than 2^32 - 1 frames"),
        ({"out_count": NULL}, E, "NULL out_count"),
        ({"records": NULL}, E, "NULL records, output or workspace"),
        ({"out_index": NULL}, E, "NULL records, output or workspace"),
        ({"out_off": NULL}, E, "NULL records, output or workspace"),
        ({"out_len": NULL}, E, "NULL records, output or workspace"),
        ({"workspace": NULL}, E, "NULL records, output or workspace"),
        ({"workspace_bytes": SHORT}, E, "select: workspace smaller than nexg_select_workspace"),
        ({"records": off(8)}, E, "misaligned records, output or workspace"),
        ({"out_off": off(4)}, E, "misaligned records, output or workspace"),
        ({"out_count": off(4)}, E, "misaligned records, output or workspace"),
        ({"out_index": off(2)}, E, "misaligned records, output or workspace"),
        ({"out_len": off(2)}, E, "misaligned records, output or workspace"),
        ({"workspace": off(2)}, E, "misaligned records, output or workspace"),
    ],
    "nexg_gather_plan": [
        ({"ctx": NULL}, E, ""),
        *FRAMES,
        ({"align": 3}, E, "gather_plan: align must be 1, 4, 8 or 16"),
        ({"frames.count": 1 << 32, "workspace_bytes": HUGE}, E, "gather_plan: more than 2^32 - 1 frames"),
        ({"out_offsets": NULL}, E, "NULL out_offsets"),
        ({"workspace": NULL}, E, "NULL workspace"),
        ({"workspace_bytes": SHORT}, E, "gather_plan: workspace smaller than nexg_gather_plan_workspace"),
        ({"out_offsets": off(4)}, E, "misaligned output or workspace"),
        ({"workspace": off(4)}, E, "misaligned output or workspace"),
        ({"out_len": off(2)}, E, "misaligned output or workspace"),
    ],
    "nexg_gather_frames": [
        ({"ctx": NULL}, E, ""),
        *FRAMES,
        ({"frames.count": 1 << 32}, E, "gather_frames: more than 2^32 - 1 frames"),
        ({"out_offsets": NULL}, E, "NULL out_offsets"),
        ({"out_data": NULL}, E, "NULL out_data with a nonzero capacity"),
        ({"out_offsets": off(4)}, E, "misaligned out_offsets or out_data"),
        ({"out_data": off(8)}, E, "misaligned out_offsets or out_data"),
    ],
    "nexg_gather_rows": [
        ({"ctx": NULL}, E, ""),
        ({"row_bytes": 12}, E, "gather_rows: row_bytes must be 4, 8, 16, 32 or 64"),
        ({"n": 1 << 32}, E, "gather_rows: more than 2^32 - 1 rows"),
        ({"rows": NULL}, E, "NULL rows, index or output"),
        ({"index": NULL}, E, "NULL rows, index or output"),
        ({"out": NULL}, E, "NULL rows, index or output"),
        ({"rows": off(8)}, E, "misaligned rows, index or output"),
        ({"out": off(8)}, E, "misaligned rows, index or output"),
        ({"index": off(2)}, E, "misaligned rows, index or output"),
    ],
    "nexg_flow_batch": [
        ({"ctx": NULL}, E, ""),
        *FRAMES,
        ({"option.reserved": 1}, E, "flow option: reserved must be 0"),
        ({"option.flags": 8}, E, "flow option: unknown flag bits"),
        ({"records": NULL}, E, "NULL records or output"),
        ({"out": NULL}, E, "NULL records or output"),
        ({"records": off(8)}, E, "misaligned records or output"),
        ({"out": off(4)}, E, "misaligned records or output"),
    ],
    "nexg_flow_partition": [
        ({"ctx": NULL}, E, ""),
        *FRAMES,
        ({"buckets": 0}, E, "flow_partition: buckets must be 1..256"),
        ({"buckets": 257, "workspace_bytes": HUGE}, E, "flow_partition: buckets must be 1..256"),
        ({"frames.count": 1 << 32, "workspace_bytes": HUGE}, E, "flow_partition: more than 2^32 - 1 frames"),
        ({"bucket_first": NULL}, E, "NULL bucket_first"),
        ({"out_len": NULL}, E, "flow_partition: out_off and out_len go together"),
        ({"out_off": NULL}, E, "flow_partition: out_off and out_len go together"),
        ({"flows": NULL}, E, "NULL flows, output or workspace"),
        ({"out_index": NULL}, E, "NULL flows, output or workspace"),
        ({"workspace": NULL}, E, "NULL flows, output or workspace"),
        ({"workspace_bytes": SHORT}, E, "flow_partition: workspace smaller than nexg_flow_partition_workspace"),
        ({"flows": off(4)}, E, "misaligned flows, output or workspace"),
        ({"out_off": off(4)}, E, "misaligned flows, output or workspace"),
        ({"bucket_first": off(4)}, E, "misaligned flows, output or workspace"),
        ({"workspace": off(4)}, E, "misaligned flows, output or workspace"),
        ({"out_index": off(2)}, E, "misaligned flows, output or workspace"),
        ({"out_len": off(2)}, E, "misaligned flows, output or workspace"),
    ],
    "nexg_flow_sort": [
        ({"ctx": NULL}, E, ""),
        ({"count": 1 << 32, "workspace_bytes": HUGE}, E, "flow_sort: more than 2^32 - 1 frames"),
        ({"flows": NULL}, E, "NULL flows, output or workspace"),
        ({"out_index": NULL}, E, "NULL flows, output or workspace"),
        ({"workspace": NULL}, E, "NULL flows, output or workspace"),
        ({"workspace_bytes": SHORT}, E, "flow_sort: workspace smaller than nexg_flow_sort_workspace"),
        ({"flows": off(4)}, E, "misaligned flows, output or workspace"),
        ({"workspace": off(4)}, E, "misaligned flows, output or workspace"),
        ({"out_index": off(2)}, E, "misaligned flows, output or workspace"),
    ],
    "nexg_flow_groups": [
        ({"ctx": NULL}, E, ""),
        *FRAMES,
        ({"option.reserved": 1}, E, "flow option: reserved must be 0"),
        ({"option.flags": 8}, E, "flow option: unknown flag bits"),
        ({"frames.count": 1 << 32, "workspace_bytes": HUGE}, E, "flow_groups: more than 2^32 - 1 frames"),
        ({"out_count": NULL}, E, "NULL out_count"),
        ({"records": NULL}, E, "NULL records, flows, order, output or workspace"),
        ({"flows": NULL}, E, "NULL records, flows, order, output or workspace"),
        ({"order": NULL}, E, "NULL records, flows, order, output or workspace"),
        ({"out": NULL}, E, "NULL records, flows, order, output or workspace"),
        ({"workspace": NULL}, E, "NULL records, flows, order, output or workspace"),
        ({"workspace_bytes": SHORT}, E, "flow_groups: workspace smaller than nexg_flow_groups_workspace"),
        ({"records": off(8)}, E, "misaligned records, flows, order, output or workspace"),
        ({"out": off(8)}, E, "misaligned records, flows, order, output or workspace"),
        ({"flows": off(4)}, E, "misaligned records, flows, order, output or workspace"),
        ({"out_count": off(4)}, E, "misaligned records, flows, order, output or workspace"),
        ({"workspace": off(4)}, E, "misaligned records, flows, order, output or workspace"),
        ({"order": off(2)}, E, "misaligned records, flows, order, output or workspace"),
        ({"out_group": off(2)}, E, "misaligned records, flows, order, output or workspace"),
    ],
}

# the empty batch: what changes from the valid call, and the u64 words that must come back zero
NO_FRAMES = {"frames.count": 0, "frames.data": NULL, "frames.data_bytes": 0}
EMPTY = {
    "nexg_decap_batch": ({**NO_FRAMES, "records": NULL, "option": NULL, "tunnels": NULL, "inner_off": NULL,
                          "inner_len": NULL}, None, 0),
    "nexg_decap_select": ({"count": 0, "tunnels": NULL, "inner_off": NULL, "inner_len": NULL, "out_index": NULL,
                           "out_off": NULL, "out_len": NULL, "workspace": NULL, "workspace_bytes": 0}, "out_count", 1),
    "nexg_dns_batch": ({**NO_FRAMES, "records": NULL, "option": NULL, "out": NULL, "tile_first": NULL}, None, 0),
    "nexg_dns_entries": ({**NO_FRAMES, "dns": NULL, "tile_first": NULL, "entries": NULL, "entries_cap": 0}, None, 0),
    "nexg_select_batch": ({**NO_FRAMES, "records": NULL, "out_index": NULL, "out_off": NULL, "out_len": NULL,
                           "out_rule": NULL, "workspace": NULL, "workspace_bytes": 0}, "out_count", 1),
    "nexg_gather_plan": ({**NO_FRAMES, "out_len": NULL, "workspace": NULL, "workspace_bytes": 0}, "out_offsets", 1),
    "nexg_gather_frames": ({**NO_FRAMES, "out_offsets": NULL, "out_data": NULL, "out_cap": 0}, None, 0),
    "nexg_gather_rows": ({"rows": NULL, "rows_count": 0, "index": NULL, "n": 0, "out": NULL}, None, 0),
    "nexg_flow_batch": ({**NO_FRAMES, "records": NULL, "option": NULL, "out": NULL}, None, 0),
    "nexg_flow_partition": ({**NO_FRAMES, "flows": NULL, "out_index": NULL, "out_off": NULL, "out_len": NULL,
                             "workspace": NULL, "workspace_bytes": 0}, "bucket_first", BUCKETS + 1),
    "nexg_flow_sort": ({"count": 0, "flows": NULL, "out_index": NULL, "workspace": NULL, "workspace_bytes": 0}, None, 0),
    "nexg_flow_groups": ({**NO_FRAMES, "records": NULL, "flows": NULL, "option": NULL, "order": NULL, "out": NULL,
                          "groups_cap": 0, "out_group": NULL, "workspace": NULL, "workspace_bytes": 0}, "out_count", 1),
}

assert set(REJECTIONS) == set(EMPTY) == set(SIGNATURES)


class Calls:
    """The valid call of every entry: device pointers as c_void_p, structures as
    ctypes objects, the rest as ints. Each output feeds the entries after it, so
    running the valid calls in SIGNATURES' order is one sane pipeline."""

    def __init__(self, engine):
        import torch
        self.engine = engine
        self.keep = []
        batch = engine.gen_batch(abi.WL_UDP64, N)
        records = engine.parse(batch, out_kind=abi.OUT_RECORD)
        self.keep += [batch, records]
        frames = batch.to_c()
        P = ctypes.c_void_p

        def dev(nbytes):  # zeroed, with room for a pointer moved up by one alignment step
            t = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda")
            self.keep.append(t)
            return P(t.data_ptr())

        rec = P(records.data_ptr())
        tunnels, inner_off, inner_len = dev(N * 16), dev(N * 8), dev(N * 4)
        dns, tile_first = dev(N * 32), dev(abi.dns_tile_first_bytes(N))
        sel_index, gather_offsets = dev(N * 4), dev((N + 1) * 8)
        flows, order = dev(N * 8), dev(N * 4)
        flt = abi.FilterC()
        flt.n_rules = 1  # one rule without tests: every frame
        table = lambda: dict(out_index=dev(N * 4), out_off=dev(N * 8), out_len=dev(N * 4))
        ws = lambda nbytes: dict(workspace=dev(nbytes), workspace_bytes=nbytes)
        self.base = {
            "nexg_decap_batch": dict(frames=frames, records=rec, option=abi.DecapOption(3, 0, 0), tunnels=tunnels,
                                     inner_off=inner_off, inner_len=inner_len),
            "nexg_decap_select": dict(tunnels=tunnels, inner_off=inner_off, inner_len=inner_len, count=N, inner_mask=0xE,
                                      **table(), out_count=dev(8), **ws(abi.decap_select_workspace(N))),
            "nexg_dns_batch": dict(frames=frames, records=rec, option=abi.DnsOption(0, 0, 0), out=dns,
                                   tile_first=tile_first),
            "nexg_dns_entries": dict(frames=frames, dns=dns, tile_first=tile_first, entries=dev(ENTRIES_CAP * 16),
                                     entries_cap=ENTRIES_CAP),
            "nexg_select_batch": dict(frames=frames, records=rec, filter=flt, **{**table(), "out_index": sel_index},
                                      out_rule=dev(N), out_count=dev(8), **ws(abi.select_workspace(N))),
            "nexg_gather_plan": dict(frames=frames, align=4, out_offsets=gather_offsets, out_len=dev(N * 4),
                                     **ws(abi.gather_plan_workspace(N))),
            "nexg_gather_frames": dict(frames=frames, out_offsets=gather_offsets, out_data=dev(N * 64), out_cap=N * 64),
            "nexg_gather_rows": dict(rows=rec, row_bytes=64, rows_count=N, index=sel_index, n=N, out=dev(N * 64)),
            "nexg_flow_batch": dict(frames=frames, records=rec, option=abi.FlowOptionC(), out=flows),
            "nexg_flow_partition": dict(frames=frames, flows=flows, buckets=BUCKETS, **table(),
                                        bucket_first=dev((BUCKETS + 1) * 8),
                                        **ws(abi.flow_partition_workspace(N, BUCKETS))),
            "nexg_flow_sort": dict(flows=flows, count=N, out_index=order, **ws(abi.flow_sort_workspace(N))),
            "nexg_flow_groups": dict(frames=frames, records=rec, flows=flows, option=abi.FlowOptionC(), order=order,
                                     out=dev(N * 32), groups_cap=N, out_group=dev(N * 4), out_count=dev(8),
                                     **ws(abi.flow_groups_workspace(N))),
        }

    def call(self, entry, changes):
        """The entry's valid call with `changes` applied: (status, last error
        of the context the call was given)."""
        names = SIGNATURES[entry].split()
        args = dict(self.base[entry], ctx=self.engine.ctx, stream=None)
        assert set(args) == set(names), entry
        for s in [n for n, v in args.items() if isinstance(v, ctypes.Structure)]:
            args[s] = type(args[s]).from_buffer_copy(args[s])  # a row changes its own copy
        for key, v in changes.items():
            holder, _, field = key.partition(".")
            assert holder in args, (entry, key)
            old = getattr(args[holder], field) if field else args[holder]
            if v is NULL:
                v = None
            elif v is SHORT:
                v = old - 1
            elif isinstance(v, tuple):
                v = (old if field else old.value) + v[1]
                v = v if field else ctypes.c_void_p(v)
            if field:
                setattr(args[holder], field, v)
            else:
                args[holder] = v
        lib = self.engine.lib
        argv = [ctypes.byref(args[n]) if isinstance(args[n], ctypes.Structure) else args[n] for n in names]
        rc = getattr(lib, entry)(*argv)
        return rc, lib.nexg_ctx_last_error(args["ctx"]).decode()

    def fill(self, entry, name, words, value):
        import torch
        p = self.base[entry][name].value
        t = next(t for t in self.keep if hasattr(t, "data_ptr") and t.data_ptr() == p)
        t[: words * 8].view(torch.int64).fill_(value)
        return t[: words * 8].view(torch.int64)


@pytest.fixture(scope="module")
def calls(engine):
    return Calls(engine)


def test_valid_calls(calls):
    """The call every row starts from is accepted, entry by entry."""
    import torch
    for entry in SIGNATURES:
        rc, text = calls.call(entry, {})
        assert rc == abi.OK, (entry, rc, text)
    torch.cuda.synchronize()


@pytest.mark.parametrize("entry", list(SIGNATURES))
def test_rejections(calls, entry):
    bad = []
    for changes, status, text in REJECTIONS[entry]:
        got = calls.call(entry, changes)
        if got != (status, text):
            bad.append((changes, got, (status, text)))
    assert not bad, (entry, bad)


@pytest.mark.parametrize("entry", list(SIGNATURES))
def test_empty_batch(calls, entry):
    import torch
    changes, zeroed, words = EMPTY[entry]
    out = calls.fill(entry, zeroed, words, -1) if zeroed else None
    rc, text = calls.call(entry, changes)
    assert rc == abi.OK, (entry, rc, text)
    torch.cuda.synchronize()
    if zeroed:
        assert (out.cpu().numpy() == 0).all(), (entry, zeroed)


# ---- the builders: a batch whose tiles do not fit one grid -------------------
# One workgroup builds a tile of 256 frames and a grid holds 2^32 - 1
# workgroups, so 2^40 + 1 frames cannot be launched: every build entry answers
# NEXG_ELAUNCH ("HIP: invalid argument") and launches nothing. The buffers hold
# 256 frames, so a kernel that ran a truncated grid of one tile would write them
# and nothing else.
BUILD_FRAMES = 256
BUILD_ENTRIES = {  # entry: frame bytes
    "nexg_build_udp4_batch": 42, "nexg_build_udp4_tuples": 42, "nexg_build_udp6_batch": 62, "nexg_build_tcp_batch": 54,
    "nexg_build_icmp_echo_batch": 42, "nexg_build_arp_batch": 42, "nexg_build_ndp_ns_batch": 86,
}


@pytest.mark.parametrize("entry", list(BUILD_ENTRIES))
def test_build_count_beyond_one_grid(engine, entry):
    import torch
    flen = BUILD_ENTRIES[entry]
    a4, a6, b4, b6, tuples = (torch.zeros(BUILD_FRAMES * w, dtype=torch.uint8, device="cuda") for w in (4, 16, 4, 16, 16))
    out = torch.full((BUILD_FRAMES * flen,), 0xA5, dtype=torch.uint8, device="cuda")
    extra = ()
    if entry in ("nexg_build_udp4_batch", "nexg_build_udp4_tuples"):
        p = abi.Udp4Build()
        if entry == "nexg_build_udp4_batch":
            p.dst_ip = a4.data_ptr()
        else:
            extra = (ctypes.c_void_p(tuples.data_ptr()),)
    elif entry == "nexg_build_udp6_batch":
        p = abi.Udp6Build()
        p.src_ip, p.dst_ip = a6.data_ptr(), b6.data_ptr()
    elif entry == "nexg_build_arp_batch":
        p = abi.ArpBuild()
        p.target_ip, p.hw_addr_len, p.proto_addr_len = a4.data_ptr(), 6, 4
    else:
        p = {"nexg_build_tcp_batch": abi.TcpBuild, "nexg_build_icmp_echo_batch": abi.IcmpEchoBuild,
             "nexg_build_ndp_ns_batch": abi.NdpNsBuild}[entry]()
        six = entry == "nexg_build_ndp_ns_batch"
        p.ip.family = 6 if six else 4
        p.ip.src_ip, p.ip.dst_ip = (a6.data_ptr(), b6.data_ptr()) if six else (a4.data_ptr(), b4.data_ptr())
    p.count = (1 << 40) + 1
    rc = getattr(engine.lib, entry)(engine.ctx, ctypes.byref(p), *extra, ctypes.c_void_p(out.data_ptr()), flen, None)
    text = engine.lib.nexg_ctx_last_error(engine.ctx).decode()
    torch.cuda.synchronize()
    assert (rc, text) == (abi.ELAUNCH, "HIP: invalid argument"), (entry, rc, text)
    assert bool((out == 0xA5).all()), entry
