"""What the per-flow counter tests share (nexg_flow_sort / nexg_flow_groups,
include/nexg.h): the pinned 32-bit hash collision, and an independent
reference for the groups (a dict group-by over the hash with a set of keys per
group, on the hash and address code of tests/second_pass_ref.py, not
nex_amd.flow.flow_key)."""
import numpy as np

from nex_amd import abi
from tests import flow_frames as ff
from tests import second_pass_ref as ref

#: with the default key both address pairs hash to COLLISION_HASH (and, the
#: hash being linear, to one value with equal ports appended)
COLLISION_A = ("10.0.0.1", "10.0.0.2")
COLLISION_B = ("231.24.44.220", "10.0.0.2")
COLLISION_HASH = 0x02B7C9B1
COLLISION_PORTS = (1111, 2222)


def collision_frames(pattern="ABAAB"):
    """UDP frames of the two colliding address pairs, with equal ports."""
    sp, dp = COLLISION_PORTS
    a = ff._tuple("udp", *COLLISION_A, sp, dp, "collision A").frame
    b = ff._tuple("udp", *COLLISION_B, sp, dp, "collision B").frame
    return [a if c == "A" else b for c in pattern]


def ref_key(frame, rec, length, symmetric, ports):
    """(kind, proto, key bytes) from the text of include/nexg.h, on
    second_pass_ref's address code; None for a frame without a flow."""
    fl = int(rec["flags"])
    a = None
    if fl & abi.L_IPV4:
        a, v6 = ref.frame_addresses(frame, rec, length, 4), False
    elif fl & abi.L_IPV6:
        a, v6 = ref.frame_addresses(frame, rec, length, 6), True
    if a is None:
        return None
    with_ports = ports and fl & (abi.L_TCP | abi.L_UDP) != 0
    if not v6 and (int(rec["ip_word"]) >> 13 & 1 or int(rec["ip_word"]) & 0x1FFF):
        with_ports = False
    one = a[0] + (int(rec["src_port"]).to_bytes(2, "big") if with_ports else b"")
    two = a[1] + (int(rec["dst_port"]).to_bytes(2, "big") if with_ports else b"")
    if symmetric and one > two:
        one, two = two, one
    n = 16 if v6 else 4
    kind = (abi.FLOW_IPV6 if v6 else abi.FLOW_IPV4) + (1 if with_ports else 0)
    return kind, int(rec["ip_proto"]), one[:n] + two[:n] + one[n:] + two[n:]


def ref_groups(frames, recs, lengths, flows, symmetric, ports):
    """hash -> dict(members (frame numbers, ascending), keys (the set of their
    keys), bytes, row (the flow row of the earliest member)): a group-by that
    knows nothing of sorting, runs or prefix sums. A frame is None (its extent
    is outside the data) or longer than 65535: it adds no bytes."""
    groups = {}
    for i, f in enumerate(frames):
        h = int(flows["hash"][i])
        g = groups.setdefault(h, dict(members=[], keys=set(), bytes=0, row=flows[i], runs=0, last=()))
        key = ref_key(f, recs[i], int(lengths[i]), symmetric, ports)
        g["members"].append(i)
        g["keys"].add(key)
        if g["last"] != () and g["last"] != key:
            g["runs"] += 1  # the members are visited in frame order, which is the sorted order inside a group
        g["last"] = key
        if f is not None and int(lengths[i]) <= 65535:
            g["bytes"] += int(lengths[i])
    return groups


def check_against_ref(groups, group_of, n_groups, order, want, count):
    """groups_host's (or the device's) result against ref_groups'."""
    assert n_groups == len(groups) == len(want)
    order = np.asarray(order)
    assert sorted(order.tolist()) == list(range(count))
    first = 0
    for g, h in zip(groups, sorted(want)):
        w = want[h]
        members = order[first: first + len(w["members"])].tolist()
        assert int(g["hash"]) == h and int(g["first"]) == first and int(g["packets"]) == len(members), (h, g)
        assert members == w["members"] and int(g["first_index"]) == members[0], (h, g)
        assert (int(g["kind"]), int(g["proto"])) == (int(w["row"]["kind"]), int(w["row"]["proto"])), (h, g)
        assert int(g["bytes"]) == w["bytes"] and int(g["reserved"]) == 0, (h, g, w["bytes"])
        assert int(g["mixed"]) == w["runs"] and (int(g["mixed"]) == 0) == (len(w["keys"]) == 1), (h, g, w["keys"])
        assert int(g["flags8"]) == (abi.FLOW_GROUP_MIXED if w["runs"] else 0), (h, g)
        first += len(members)
    assert first == count
    want_of = np.zeros(count, np.uint32)
    for gi, h in enumerate(sorted(want)):
        want_of[want[h]["members"]] = gi
    assert (np.asarray(group_of) == want_of).all()
