"""CPU: the host contract of the header rewrite (nex_amd/rewrite.py) and the
corpus of tests/rewrite_frames.py.

rewrite_host is pinned by a hand-written truth table (each field with its view
present and absent, rows derived by hand from include/nexg.h) and compared on
the whole corpus with rewrite_ref, which takes its views and its checksums
from the oracle. INCREMENTAL mode is checked three ways: on frames whose
stored checksums the oracle fixed it equals RECOMPUTE, on garbage checksums it
equals the reference's own RFC 1624 arithmetic, and it preserves the error.
ActionSet.to_c raises ValueError exactly where nexg_actions_check returns
NEXG_EINVAL."""
import ctypes
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.frame import ParseOption
from nex_amd.rewrite import Action, ActionSet, rewrite_host
from tests import helpers
from tests import rewrite_frames as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nex_amd", "libnexg.so")
HDR = os.path.join(ROOT, "include", "nexg.h")
NONE = (0, 0, abi.ACTION_NONE, 0, 0)

# ---- the truth table -----------------------------------------------------------------
PAY = bytes(range(0x60, 0x6A))
UDP4 = helpers._eth(helpers._ipv4(helpers._udp(PAY), 17))   # 14 + 20 + 8 + 10
TCP6 = helpers._eth(helpers._ipv6(helpers._tcp(PAY), 6), 0x86DD)
ICMP4 = helpers._eth(helpers._ipv4(bytes([8, 0, 0x11, 0x22, 0, 1, 0, 2]), 1))
ARP = helpers._eth(bytes(28), 0x0806)
MAC = bytes.fromhex("0a0b0c0d0e0f")


def put(frame, at, data):
    return frame[:at] + bytes(data) + frame[at + len(data):]


def one(frame, action, incremental=False, option=ParseOption()):
    out, rows = rewrite_host([frame], ActionSet([action], incremental=incremental), None, option)
    return out[0], rf.row_tuple(rows[0])


def edits(frame, out):
    """{offset: new byte} of every byte that changed."""
    assert len(frame) == len(out)
    return {i: out[i] for i in range(len(frame)) if frame[i] != out[i]}


#: (what, frame, action, option, bytes written as (offset, data) without the checksum fields, applied, fixed)
TABLE = [
    ("eth_dst: Ethernet view", ARP, Action.mac(dst=MAC), ParseOption(), [(0, MAC)], abi.SET_ETH_DST, 0),
    ("eth_src: Ethernet view", UDP4, Action.mac(src=MAC), ParseOption(), [(6, MAC)], abi.SET_ETH_SRC, 0),
    ("eth_dst: 13 bytes, no view", UDP4[:13], Action.mac(dst=MAC), ParseOption(), [], 0, 0),
    ("eth_dst: raw IP, no view", UDP4[14:], Action.mac(dst=MAC), ParseOption(from_ip_packet=True, offset=0), [], 0, 0),
    ("ip_src 4: IPv4 view", UDP4, Action.nat4(src="1.2.3.4"), ParseOption(), [(26, [1, 2, 3, 4])], abi.SET_IP_SRC, 3),
    ("ip_dst 4: IPv4 view, ICMP: no pseudo-header", ICMP4, Action.nat4(dst="1.2.3.4"), ParseOption(), [(30, [1, 2, 3, 4])],
     abi.SET_IP_DST, 1),
    ("ip_src 4 on an IPv6 frame", TCP6, Action.nat4(src="1.2.3.4"), ParseOption(), [], 0, 0),
    ("ip_src 4: header cut short", UDP4[:33], Action.nat4(src="1.2.3.4"), ParseOption(), [], 0, 0),
    ("ip_dst 6: IPv6 view", TCP6, Action.nat6(dst="::5"), ParseOption(), [(38, bytes(15) + b"\x05")], abi.SET_IP_DST, 2),
    ("ip_dst 6 on an IPv4 frame", UDP4, Action.nat6(dst="::5"), ParseOption(), [], 0, 0),
    ("ip_dst 6: 39 bytes of IPv6", TCP6[:53], Action.nat6(dst="::5"), ParseOption(), [], 0, 0),
    ("ports: UDP view", UDP4, Action.ports(src=0x0102, dst=0x0304), ParseOption(), [(34, [1, 2, 3, 4])],
     abi.SET_SRC_PORT | abi.SET_DST_PORT, 2),
    ("src port: TCP view over IPv6", TCP6, Action.ports(src=0x0102), ParseOption(), [(54, [1, 2])], abi.SET_SRC_PORT, 2),
    ("ports: ICMP has none", ICMP4, Action.ports(src=1, dst=2), ParseOption(), [], 0, 0),
    ("ports: UDP header cut short", UDP4[:41], Action.ports(src=1, dst=2), ParseOption(), [], 0, 0),
    ("ports: TCP data offset 4", put(TCP6, 54 + 12, [0x43]), Action.ports(dst=2), ParseOption(), [], 0, 0),
    ("ports: UDP length past the datagram", put(UDP4, 38, [0, 19]), Action.ports(dst=2), ParseOption(), [], 0, 0),
    ("ttl: IPv4 byte 8", UDP4, Action.set_ttl(9), ParseOption(), [(22, [9])], abi.SET_TTL, 1),
    ("hop limit: IPv6 byte 7, nothing dirty", TCP6, Action.set_ttl(9), ParseOption(), [(21, [9])], abi.SET_TTL, 0),
    ("dec_ttl 3 of 64", UDP4, Action.dec_ttl(3), ParseOption(), [(22, [61])], abi.DEC_TTL, 1),
    ("dec_ttl 65 of 64 stops at 0", TCP6, Action.dec_ttl(65), ParseOption(), [(21, [0])], abi.DEC_TTL, 0),
    ("ttl: no IP view", ARP, Action.set_ttl(9), ParseOption(), [], 0, 0),
    ("tos: IPv4 byte 1, masked", put(UDP4, 15, [0xFF]), Action.set_tos(0x28, 0xFC), ParseOption(), [(15, [0x2B])],
     abi.SET_TOS, 1),
    # helpers._ipv6 starts 6a bc: version 6, traffic class 0xab, flow label c....
    ("traffic class: two nibbles", TCP6, Action.set_tos(0x12, 0xFF), ParseOption(), [(14, [0x61, 0x2C])], abi.SET_TOS, 0),
    ("ecn bits of the traffic class", TCP6, Action.set_tos(0x0, 0x03), ParseOption(), [(15, [0x8C])], abi.SET_TOS, 0),
    ("tos: IHL 4, no view", put(UDP4, 14, [0x44]), Action.set_tos(1, 1), ParseOption(), [], 0, 0),
    ("raw IP at offset 3: version nibble picks IPv4", b"\xee" * 3 + UDP4[14:], Action.nat4(src="1.2.3.4") & Action.ports(dst=7),
     ParseOption(from_ip_packet=True, offset=3), [(15, [1, 2, 3, 4]), (25, [0, 7])], abi.SET_IP_SRC | abi.SET_DST_PORT, 3),
    ("raw IP: version 5", put(UDP4[14:], 0, [0x55]), Action.set_ttl(1), ParseOption(from_ip_packet=True, offset=0), [], 0, 0),
]


@pytest.mark.parametrize("what,frame,action,option,writes,applied,fixed", TABLE, ids=[t[0] for t in TABLE])
def test_truth_table(oracle, what, frame, action, option, writes, applied, fixed):
    out, row = one(frame, action, False, option)
    assert row[:3] == (applied, fixed, 0), row
    edited = frame
    for at, data in writes:
        edited = put(edited, at, data)
    want, rep = oracle.recompute_frame(edited, fixed, option.flags(), option.offset)
    assert out == want, (edits(frame, out), edits(frame, want))
    assert row[3:] == (int(rep["ip_csum"]), int(rep["l4_csum"]))
    # no byte outside the named fields and the two checksum fields moved
    allowed = {at + k for at, data in writes for k in range(len(data))}
    L = option.offset if option.from_ip_packet else 14
    if fixed & abi.FIX_IP:
        allowed |= {L + 10, L + 11}
    if fixed & abi.FIX_L4:
        allowed |= {int(rep["l4_off"]) + {17: 6, 6: 16}.get(int(rep["proto"]), 2) + k for k in (0, 1)}
    assert set(edits(frame, out)) <= allowed


def test_index_picks_the_action_and_never_reaches_past_the_set():
    acts = ActionSet([Action.set_ttl(1), Action.set_ttl(2), Action()])
    frames = [UDP4] * 6 + [bytes(70000)]
    out, rows = rewrite_host(frames, acts, [0, 1, 2, 3, abi.ACTION_NONE, 16, 1])
    assert [f[22] for f in out[:6]] == [1, 2, 64, 64, 64, 64]
    assert [rf.row_tuple(r)[:3] for r in rows] == [(abi.SET_TTL, 1, 0), (abi.SET_TTL, 1, 1), (0, 0, 2), NONE[:3], NONE[:3],
                                                    NONE[:3], (0, 0, 1)]
    assert out[3:6] == [UDP4] * 3 and out[6] == frames[6]
    out0, rows0 = rewrite_host(frames[:2], acts)
    assert [f[22] for f in out0] == [1, 1] and list(rows0["action"]) == [0, 0]


def test_builders_compose():
    a = Action.nat4(src="192.0.2.1") & Action.ports(dst=53) & Action.dec_ttl(1) & Action.mac(dst="02:00:00:00:00:01")
    assert a.sets == abi.SET_IP_SRC | abi.SET_DST_PORT | abi.DEC_TTL | abi.SET_ETH_DST
    assert (a.family, a.ttl, a.dst_port, a.src[:4], a.eth_dst) == (4, 1, 53, bytes([192, 0, 2, 1]), bytes([2, 0, 0, 0, 0, 1]))
    with pytest.raises(ValueError):
        Action.nat4(src="1.1.1.1") & Action.nat6(dst="::1")
    with pytest.raises(ValueError):
        Action.set_ttl(1) & Action.set_ttl(2)
    with pytest.raises(ValueError):
        Action.nat4(src="::1")
    c = ActionSet([a], incremental=True).to_c()
    assert (c.n_actions, c.flags, c.actions[0].sets, c.actions[0].family) == (1, abi.REWRITE_INCREMENTAL, a.sets, 4)


# ---- the corpus -------------------------------------------------------------------------

def host_all(frames, incremental, option=ParseOption()):
    res = {}
    for a, act in enumerate(rf.ACTIONS):
        out, rows = rewrite_host(list(frames), rf.to_set([act], incremental), None, option)
        rows = rows.copy()
        rows["action"] = a % 16  # rf.ref_all numbers the actions by their place in their chunk
        res[a] = (tuple(out), rows)
    return res


def assert_same(got, want, frames, what):
    for a in want:
        for i, (g, w) in enumerate(zip(got[a][0], want[a][0])):
            assert g == w, (what, rf.NAMES[a], i, len(frames[i]), edits(frames[i], g), edits(frames[i], w))
        bad = np.nonzero(got[a][1] != want[a][1])[0]
        assert len(bad) == 0, (what, rf.NAMES[a], int(bad[0]), got[a][1][bad[0]], want[a][1][bad[0]])


@pytest.fixture(scope="module")
def corpus(oracle):
    return rf.corpus()


MODES = [(0, 0)] + [(abi.PARSE_FROM_IP, k) for k in rf.RAW_OFFSETS]


def mode_frames(c, flags, k):
    return (c.fixed, c.garbage) if not flags else rf.raw_ip(k)


def option_of(flags, k):
    return ParseOption(from_ip_packet=bool(flags), offset=k)


def test_corpus_reaches_the_edges(corpus):
    """From the reference alone: every field is applied and refused somewhere,
    both checksums get fixed by every action that can dirty them, and the
    planted frames give 0x0000 and 0x0001 in both fields after the NAT."""
    c = corpus
    assert len(c.fixed) == len(c.garbage) >= 200
    assert any(len(f) == 65535 for f in c.fixed)
    ref = rf.ref_all(c.garbage, False)
    for a, act in enumerate(rf.ACTIONS):
        rows = ref[a][1]
        for bit in range(9):
            if act.sets >> bit & 1:
                n = int((rows["applied"] >> bit & 1).sum())
                assert 3 <= n < len(rows), (act.name, bit, n)
        if act.sets & (rf.ADDR | abi.SET_TTL | abi.DEC_TTL | abi.SET_TOS) and act.family != 6:
            assert int((rows["fixed"] & abi.FIX_IP != 0).sum()) >= 20, act.name
        if act.sets & rf.PORTS:
            assert int((rows["fixed"] & abi.FIX_L4 != 0).sum()) >= 20, act.name
    nat = rf.NAMES.index(rf.NAT44.name)
    for half in (c.fixed, c.garbage):
        for incremental in (False, True)[: 1 if half is c.garbage else 2]:
            rows = rf.ref_all(half, incremental)[nat][1][list(c.planted)]
            assert (rows["fixed"] == rf.BOTH).all()
            assert {0, 1} <= set(rows["ip_csum"].tolist()) and {0, 1} <= set(rows["l4_csum"].tolist())
    for k in rf.RAW_OFFSETS:
        rows = rf.ref_all(rf.raw_ip(k)[1], False, abi.PARSE_FROM_IP, k)[nat][1]
        assert int((rows["fixed"] == rf.BOTH).sum()) >= 50, k


@pytest.mark.parametrize("flags,k", MODES)
def test_recompute_equals_the_reference(corpus, flags, k):
    for frames in mode_frames(corpus, flags, k):
        assert_same(host_all(frames, False, option_of(flags, k)), rf.ref_all(frames, False, flags, k), frames,
                    f"recompute flags {flags} offset {k}")


@pytest.mark.parametrize("flags,k", MODES)
def test_incremental_on_fixed_checksums_equals_recompute(corpus, flags, k):
    fixed, _ = mode_frames(corpus, flags, k)
    opt = option_of(flags, k)
    inc, full = host_all(fixed, True, opt), host_all(fixed, False, opt)
    L = k if flags else 14

    def udp4_zero(f):  # UDP over IPv4 with the checksum field 0: "none"
        return len(f) >= L + 28 and (f[L] >> 4 == 4 if flags else f[12:14] == b"\x08\x00") and f[L + 9] == 17 and \
            f[L + (f[L] & 15) * 4 + 6:][:2] == b"\0\0" and (f[L] & 15) >= 5

    def later_fragment(f):  # RECOMPUTE knows nothing of fragments: it rewrites "ports" in payload bytes
        return len(f) >= L + 20 and (f[L] >> 4 == 4 if flags else f[12:14] == b"\x08\x00") and \
            int.from_bytes(f[L + 6:L + 8], "big") & 0x1FFF

    zero = [i for i, f in enumerate(fixed) if udp4_zero(f)]
    frag = [i for i, f in enumerate(fixed) if later_fragment(f)]
    if not flags:
        assert zero == list(corpus.udp4_zero)
    assert 1 <= len(zero) < 0.05 * len(fixed) and 1 <= len(frag) < 0.05 * len(fixed)
    skip = set(zero) | set(frag)
    for a in inc:
        for i, f in enumerate(fixed):
            if i in skip:
                continue
            assert inc[a][0][i] == full[a][0][i], (rf.NAMES[a], i, edits(f, inc[a][0][i]), edits(f, full[a][0][i]))
            assert inc[a][1][i] == full[a][1][i], (rf.NAMES[a], i, inc[a][1][i], full[a][1][i])
        # the stored-zero frames: the UDP checksum stays 0 and is not reported, everything else as RECOMPUTE
        for i in zero:
            g, w, row = inc[a][0][i], full[a][0][i], inc[a][1][i]
            at = L + (fixed[i][L] & 15) * 4 + 6
            assert g[at:at + 2] == b"\0\0" and not int(row["fixed"]) & abi.FIX_L4 and int(row["l4_csum"]) == 0
            assert g[:at] + g[at + 2:] == w[:at] + w[at + 2:]
            assert (int(row["applied"]), int(row["ip_csum"])) == (int(full[a][1][i]["applied"]), int(full[a][1][i]["ip_csum"]))
        # later IPv4 fragments have no L4 view in INCREMENTAL mode only (include/nexg.h, step 2), so the identity
        # holds for them up to the L4 view: everything ahead of the IP payload, and the whole frame and row under an
        # action that needs no L4 view
        for i in frag:
            f, g, w, row, wrow = fixed[i], inc[a][0][i], full[a][0][i], inc[a][1][i], full[a][1][i]
            P = L + (f[L] & 15) * 4
            if not rf.ACTIONS[a].sets & (rf.ADDR | rf.PORTS):
                assert g == w and row == wrow, (rf.NAMES[a], i)
                continue
            assert g[:P] == w[:P] and g[P:] == f[P:], (rf.NAMES[a], i, edits(f, g), edits(f, w))
            assert int(row["applied"]) == int(wrow["applied"]) & ~rf.PORTS and int(row["ip_csum"]) == int(wrow["ip_csum"])
            assert int(row["fixed"]) == int(wrow["fixed"]) & abi.FIX_IP and int(row["l4_csum"]) == 0


@pytest.mark.parametrize("flags,k", MODES)
def test_incremental_on_garbage_checksums(corpus, oracle, flags, k):
    _, garbage = mode_frames(corpus, flags, k)
    got = host_all(garbage, True, option_of(flags, k))
    assert_same(got, rf.ref_all(garbage, True, flags, k), garbage, f"incremental flags {flags} offset {k}")
    # the error is preserved: stored - correct is the same mod 0xFFFF before and after
    checked = 0
    for a in got:
        for f, g, row in zip(garbage, got[a][0], got[a][1]):
            if not int(row["fixed"]):
                continue
            _, before = oracle.recompute_frame(f, rf.BOTH, flags, k)
            _, after = oracle.recompute_frame(g, rf.BOTH, flags, k)
            L = k if flags else 14
            if int(row["fixed"]) & abi.FIX_IP:
                stored0, stored1 = rf._w(f, L + 10), int(row["ip_csum"])
                assert rf._w(g, L + 10) == stored1
                assert (stored0 - int(before["ip_csum"])) % 0xFFFF == (stored1 - int(after["ip_csum"])) % 0xFFFF
                checked += 1
            if int(row["fixed"]) & abi.FIX_L4 and int(after["done"]) & abi.FIX_L4:
                at = int(after["l4_off"]) + {17: 6, 6: 16}.get(int(after["proto"]), 2)
                stored0, stored1 = rf._w(f, at), int(row["l4_csum"])
                assert rf._w(g, at) == stored1
                assert (stored0 - int(before["l4_csum"])) % 0xFFFF == (stored1 - int(after["l4_csum"])) % 0xFFFF
                checked += 1
    assert checked >= 1000


def test_later_fragments_keep_their_l4_bytes_in_incremental_mode(corpus):
    frag = [f for f in corpus.fixed + corpus.garbage
            if len(f) >= 34 and f[12:14] == b"\x08\x00" and int.from_bytes(f[20:22], "big") & 0x1FFF]
    first = [f for f in corpus.fixed if len(f) >= 34 and f[12:14] == b"\x08\x00" and f[20:22] == b"\x20\x00"]
    assert len(frag) >= 8 and len(first) >= 2
    acts = rf.to_set([rf.NAT44], incremental=True)
    out, rows = rewrite_host(frag, acts)
    for f, g, row in zip(frag, out, rows):
        assert g[34:] == f[34:]  # the ports' place and every L4 byte
        assert int(row["applied"]) == rf.ADDR | abi.DEC_TTL and int(row["fixed"]) == abi.FIX_IP
        assert g[26:34] == rf.S4[:4] + rf.D4[:4]
    out, rows = rewrite_host(first, acts)
    assert all(int(r["applied"]) & rf.PORTS == rf.PORTS and int(r["fixed"]) == rf.BOTH for r in rows)
    # RECOMPUTE knows nothing of fragments
    out, rows = rewrite_host(frag, rf.to_set([rf.NAT44]))
    assert all(int(r["applied"]) & rf.PORTS == rf.PORTS for r in rows)


# ---- validation ------------------------------------------------------------------------------

OK_ACTION = Action.nat4(src="1.2.3.4") & Action.set_tos(0x10, 0xFC)


def invalid_sets():
    """name -> ActionSet: everything nexg_actions_check rejects."""
    bad = {
        "unknown sets bits": replace(OK_ACTION, sets=OK_ACTION.sets | 0x200),
        "unknown high sets bit": replace(OK_ACTION, sets=OK_ACTION.sets | 0x80000000),
        "nonzero reserved": replace(OK_ACTION, reserved=bytes(7) + b"\x01"),
        "SET_TTL together with DEC_TTL": Action(sets=abi.SET_TTL | abi.DEC_TTL, ttl=1),
        "DEC_TTL with ttl 0": Action(sets=abi.DEC_TTL, ttl=0),
        "address set with family 0": Action(sets=abi.SET_IP_SRC, family=0),
        "address set with family 5": Action(sets=abi.SET_IP_DST, family=5),
        "family without an address set": Action(sets=abi.SET_TTL, ttl=1, family=4),
        "family 6 with empty sets": Action(family=6),
        "SET_TOS with tos_mask 0": Action(sets=abi.SET_TOS, tos=0, tos_mask=0),
        "SET_TOS with tos outside the mask": Action(sets=abi.SET_TOS, tos=0x04, tos_mask=0x03),
    }
    sets = {name: ActionSet([OK_ACTION, a]) for name, a in bad.items()}
    sets["n_actions 0"] = ActionSet([])
    sets["n_actions 17"] = ActionSet([OK_ACTION] * 17)
    sets["unknown flags"] = ActionSet([OK_ACTION], flags=0x2)
    sets["unknown high flag"] = ActionSet([OK_ACTION], flags=0x80000001)
    return sets


@pytest.fixture(scope="module")
def clib():
    if not os.path.exists(LIB):
        pytest.fail("nex_amd/libnexg.so is not built")
    lib = ctypes.CDLL(LIB)
    lib.nexg_actions_check.restype = ctypes.c_int
    lib.nexg_actions_check.argtypes = [ctypes.POINTER(abi.ActionsC)]
    return lib


@pytest.mark.parametrize("name", sorted(invalid_sets()))
def test_rejections_python_and_c_agree(clib, name):
    s = invalid_sets()[name]
    with pytest.raises(ValueError):
        s.to_c()
    c = s.to_c(validate=False)
    if name == "n_actions 17":
        c.n_actions = 17
    assert clib.nexg_actions_check(ctypes.byref(c)) == abi.EINVAL


def test_valid_sets_pass(clib):
    valid = [ActionSet([Action()]), ActionSet([OK_ACTION] * 16, incremental=True),
             ActionSet([Action.dec_ttl(255)]), ActionSet([Action.set_ttl(0)]), ActionSet([Action.set_tos(0, 0xFF)])]
    valid += [rf.to_set(acts, inc) for _, acts in rf.action_chunks() for inc in (False, True)]
    for s in valid:
        assert clib.nexg_actions_check(ctypes.byref(s.to_c())) == abi.OK
    assert clib.nexg_actions_check(None) == abi.EINVAL
    c = ActionSet([OK_ACTION]).to_c()
    c.actions[1].sets = 0xFFFF  # an action past n_actions is not looked at
    assert clib.nexg_actions_check(ctypes.byref(c)) == abi.OK
    c.n_actions = 2
    assert clib.nexg_actions_check(ctypes.byref(c)) == abi.EINVAL


def test_struct_layouts_match_c(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', 'int main(void){',
             'printf("%zu %zu %zu\\n", sizeof(nexg_action), sizeof(nexg_actions), sizeof(nexg_rewritten));']
    lines += [f'printf("%zu\\n", offsetof(nexg_action, {f}));' for f, _ in abi.ActionC._fields_]
    lines += [f'printf("%zu\\n", offsetof(nexg_rewritten, {f}));' for f in abi.REWRITTEN_DTYPE.names]
    names = ("SET_ETH_DST", "SET_ETH_SRC", "SET_IP_SRC", "SET_IP_DST", "SET_SRC_PORT", "SET_DST_PORT", "SET_TTL", "DEC_TTL",
             "SET_TOS", "SET_ALL", "REWRITE_INCREMENTAL", "REWRITE_MAX_ACTIONS", "ACTION_NONE")
    lines += [f'printf("%u\\n", (unsigned)(NEXG_{m}));' for m in names]
    lines.append("return 0;}")
    src = tmp_path / "probe_rewrite.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe_rewrite"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    out = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert out[:3] == [64, 1032, 8] == [ctypes.sizeof(abi.ActionC), ctypes.sizeof(abi.ActionsC), abi.REWRITTEN_DTYPE.itemsize]
    k = 3 + len(abi.ActionC._fields_)
    assert out[3:k] == [getattr(abi.ActionC, f).offset for f, _ in abi.ActionC._fields_]
    assert out[k:k + 5] == [abi.REWRITTEN_DTYPE.fields[f][1] for f in abi.REWRITTEN_DTYPE.names]
    assert out[k + 5:] == [getattr(abi, m) for m in names]


def test_header_declares_what_the_library_exports():
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    want = {"nexg_actions_check", "nexg_rewrite_batch"}
    assert want <= exported and want <= set(abi.EXPORTED_SYMBOLS)
    text = open(HDR).read()
    for name in want:
        assert f"int {name}(" in text
