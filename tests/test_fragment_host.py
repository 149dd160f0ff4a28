"""CPU: nex_amd.fragment.fragment_host, the plain-Python statement of
include/nexg.h's fragmentation rule that the device output is tested against,
pinned from outside: RFC 791's own worked example, the properties every
fragment train has, the oracle's parse of every piece, and the independent
reassembly of tests/fragment_frames.py."""
import numpy as np
import pytest

from nex_amd import abi
from nex_amd.fragment import FragOption, fragment_host, plan_host
from tests import fragment_frames as ff
from tests.helpers import rfc1071


def test_rfc791_appendix_a_example_2():
    """A datagram of 452 data octets behind a 20-octet header (total length
    472) over a network that carries 280 octets: 256 data octets with MF at
    offset 0, then 196 without MF at offset 32."""
    frame = ff.ipv4(452, ident=111, tos=0, ttl=123, proto=1)
    assert int.from_bytes(frame[16:18], "big") == 472
    pieces, src, rows = fragment_host([frame], 280)
    assert [(int.from_bytes(p[16:18], "big"), int.from_bytes(p[20:22], "big")) for p in pieces] == [(276, 0x2000), (216, 32)]
    assert pieces[0][34:] == frame[34:34 + 256] and pieces[1][34:] == frame[34 + 256:]
    assert [p[18:20] for p in pieces] == [frame[18:20]] * 2 and all(rfc1071(p[14:34]) == 0 for p in pieces)
    assert list(src) == [0, 0]
    assert tuple(rows[0]) == (abi.FRAME_OK, abi.FRAG_SPLIT, 20, 0, 2, 256, 0, 0)


@pytest.fixture(scope="module")
def verdict_of_input(oracle):
    """Per corpus frame: does the oracle's parse give the frame itself an OK
    IPv4 header checksum? ipv4::checksum runs over the header as the reference
    re-serialises it, and an option list that does not re-serialise to its own
    bytes (bytes behind an End of List, a malformed length) fails that verdict
    whatever checksum the header carries: the oracle cannot judge such a
    header's pieces either, and rfc1071 over the bytes does."""
    out = []
    for name, f in ff.corpus():
        ok = False
        if f is not None and len(f) >= 34:
            flags = int(oracle.parse_frame(f)["flags"])
            ok = bool(flags & abi.C_IP_OK)
        out.append(ok)
    exempt = {name for (name, f), ok in zip(ff.corpus(), out)
              if not ok and f is not None and fragment_host([f], 68, True)[2]["kind"][0] == abi.FRAG_SPLIT}
    assert exempt == {"options: eol in the middle", "options: length 0", "options: length 1", "options: length overruns",
                      "options: type in the last byte", "options: forty bytes", "options: forty bytes, splits at 9000",
                      "hl 60 proto 17", "hl 60 proto 6", "Ethernet padding, 60 bytes of options", "65535 bytes, hl 60",
                      "mtu 68 hl 60: D 9", "mtu 68 hl 60: D 16", "mtu 68 hl 60: D 17"}, sorted(exempt)
    # the longest header is judged by the oracle all the same: 40 option bytes that re-serialise to themselves
    judged = {name for (name, f), ok in zip(ff.corpus(), out) if ok and f[14] & 15 == 15}
    assert judged >= {"options: forty bytes that re-serialise to themselves", "mtu 68 hl 60, options that re-serialise: D 17",
                      "hl 60, options that re-serialise, splits at 9000"}, sorted(judged)
    return out


@pytest.mark.parametrize("ignore_df", (False, True), ids=("df kept", "df ignored"))
@pytest.mark.parametrize("mtu", ff.MTUS)
def test_every_train_fits_parses_and_reassembles(oracle, verdict_of_input, mtu, ignore_df):
    frames = ff.frames()
    pieces, src, rows = fragment_host(frames, mtu, ignore_df)
    assert len(src) == len(pieces) == int(rows["pieces"].sum())
    assert (rows["first"] == np.concatenate([[0], np.cumsum(rows["pieces"])[:-1]])).all()
    kinds = set()
    for i, ((name, f), row) in enumerate(zip(ff.corpus(), rows)):
        mine = pieces[int(row["first"]): int(row["first"]) + int(row["pieces"])]
        assert (src[int(row["first"]): int(row["first"]) + int(row["pieces"])] == i).all(), name
        kinds.add((int(row["kind"]), int(row["status"])))
        if row["kind"] == abi.FRAG_PASS:
            assert mine == [f] and row["status"] == abi.FRAME_OK and (row["hdr_len"], row["piece_data"]) == (0, 0), name
            continue
        if row["kind"] != abi.FRAG_SPLIT:
            assert mine == [] and (row["hdr_len"], row["piece_data"]) == (0, 0), name
            assert (row["status"] == abi.FRAME_OK) == (row["kind"] == abi.FRAG_TOO_BIG), name
            continue
        hl, word = 4 * (f[14] & 15), int.from_bytes(f[20:22], "big")
        assert row["status"] == abi.FRAME_OK and row["hdr_len"] == hl and row["piece_data"] == (mtu - hl) & ~7, name
        assert len(mine) >= 2, name
        for k, p in enumerate(mine):
            assert int.from_bytes(p[16:18], "big") <= mtu and len(p) == 14 + int.from_bytes(p[16:18], "big"), (name, k)
            assert (len(p) - 14 - hl) % 8 == 0 or k == len(mine) - 1, (name, k)
            assert len(p) - 14 - hl == row["piece_data"] or k == len(mine) - 1, (name, k)
            rec = oracle.parse_frame(p)
            assert rec["flags"] & abi.L_IPV4, (name, k)
            if verdict_of_input[i]:
                assert rec["flags"] & abi.C_IP_CHECKED and rec["flags"] & abi.C_IP_OK, (name, k)
        back = ff.reassemble(mine[::-1], first_offset=word & 0x1FFF, last_more=bool(word & 0x2000))
        assert back == ff.datagram(f, clear_df=ignore_df), name
    want = {(abi.FRAG_PASS, abi.FRAME_OK), (abi.FRAG_NONE, abi.ERR_BAD_EXTENT), (abi.FRAG_TOO_BIG, abi.FRAME_OK)}
    if mtu < 9000:
        want |= {(abi.FRAG_SPLIT, abi.FRAME_OK), (abi.FRAG_NONE, abi.ERR_INVALID_LENGTH)}
    assert want <= kinds, want - kinds


def test_df_and_ipv6_are_reported_not_cut():
    by_name = dict(ff.corpus())
    for name, mtu, ignore, kind, n in (("DF set", 1500, False, abi.FRAG_TOO_BIG, 0), ("DF set", 1500, True, abi.FRAG_SPLIT, 2),
                                       ("DF set", 9000, False, abi.FRAG_PASS, 1),
                                       ("DF set and it fits everywhere", 68, False, abi.FRAG_PASS, 1),
                                       ("IPv6 at 68 exactly", 68, True, abi.FRAG_PASS, 1),
                                       ("IPv6 one over 68", 68, True, abi.FRAG_TOO_BIG, 0),
                                       ("IPv6 over 1500", 1500, False, abi.FRAG_TOO_BIG, 0),
                                       ("IPv6 over 1500", 9000, False, abi.FRAG_PASS, 1),
                                       ("IPv6 payload length past the frame", 68, False, abi.FRAG_PASS, 1),
                                       ("VLAN-tagged IPv4", 68, False, abi.FRAG_PASS, 1)):
        pieces, _, rows = fragment_host([by_name[name]], mtu, ignore)
        assert (int(rows["kind"][0]), len(pieces)) == (kind, n), (name, mtu, ignore)
    pieces, _, _ = fragment_host([by_name["DF set"]], 1500, True)
    assert all(not p[20] & 0x40 for p in pieces)
    pieces, _, _ = fragment_host([by_name["reserved bit, DF and MF set"]], 576, True)
    assert all(p[20] & 0xC0 == 0x80 and p[20] & 0x20 for p in pieces)  # reserved kept, DF cleared, MF0 on the last too


def test_the_offset_field_has_13_bits():
    by_name = dict(ff.corpus())
    pieces, _, rows = fragment_host([by_name["offset ends at 8191 exactly at mtu 576"]], 576)
    assert rows["kind"][0] == abi.FRAG_SPLIT and int.from_bytes(pieces[-1][20:22], "big") & 0x1FFF == 8191
    pieces, _, rows = fragment_host([by_name["offset overflows by one at mtu 576"]], 576)
    assert pieces == [] and (rows["status"][0], rows["kind"][0]) == (abi.ERR_INVALID_LENGTH, abi.FRAG_NONE)


def test_the_most_pieces_a_frame_gives():
    """hl 60 at mtu 68 leaves 8 data bytes per piece. A table holds frames of at
    most 65535 bytes, so TL <= 65521 and D <= 65461: 8183 pieces. (A total
    length of 65535 would give 8185, but needs a frame of 65549 bytes, which
    rule 1 refuses as a bad extent.)"""
    by_name = dict(ff.corpus())
    pieces, _, rows = fragment_host([by_name["65535 bytes, hl 60"]], 68)
    assert len(pieces) == rows["pieces"][0] == 8183
    assert int.from_bytes(pieces[-1][20:22], "big") == 8182 and len(pieces[-1]) == 14 + 60 + 5
    too_long = ff.ipv4(65535 - 60, ff.OPTIONS["forty bytes"])
    assert int.from_bytes(too_long[16:18], "big") == 65535 and len(too_long) == 65549
    pieces, _, rows = fragment_host([too_long], 68)
    assert pieces == [] and (rows["status"][0], rows["kind"][0]) == (abi.ERR_BAD_EXTENT, abi.FRAG_NONE)
    for mtu in ff.MTUS:  # no frame of the corpus gives more
        _, _, rows = fragment_host(ff.frames(), mtu)
        assert int(rows["pieces"].max()) <= 8183


def test_option_validation_matches_the_c_check():
    FragOption(68).validate()
    FragOption(65535, abi.FRAG_IGNORE_DF, 16).validate()
    for bad in (FragOption(67), FragOption(65536), FragOption(1500, 2), FragOption(1500, 0, 2), FragOption(1500, 0, 32),
                FragOption(1500, 0, 0), FragOption(1500, 0, 1, 1)):
        with pytest.raises(ValueError):
            bad.validate()
    with pytest.raises(ValueError):
        fragment_host([b""], 67)
    assert list(plan_host([0, 1, 16, 17], 16)) == [0, 0, 16, 32, 64]


def test_header_declares_and_library_exports():
    import ctypes
    import os
    import re
    from nex_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "nexg.h")).read()
    for fn in ("nexg_fragment_plan", "nexg_fragment_frames"):
        assert re.search(r"^int " + fn + r"\(nexg_ctx\* ctx,", text, re.M), fn
        assert fn in abi.EXPORTED_SYMBOLS
    assert "nexg_frag_option_check" in abi.EXPORTED_SYMBOLS and "nexg_fragment_plan_workspace" in abi.HEADER_INLINE
    lib = _lib.load()
    assert lib.nexg_fragment_plan(None, None, None, None, None, None, None, 0, None) == abi.EINVAL
    assert lib.nexg_fragment_frames(None, None, None, None, None, 0, None, None, None, None, 0, None) == abi.EINVAL
    good = abi.FragOptionC(mtu=1500, flags=0, align=1, reserved=0)
    assert lib.nexg_frag_option_check(ctypes.byref(good)) == abi.OK and lib.nexg_frag_option_check(None) == abi.EINVAL
    for field, v in (("mtu", 67), ("mtu", 65536), ("flags", 2), ("align", 3), ("align", 0), ("reserved", 1)):
        bad = abi.FragOptionC(mtu=1500, flags=0, align=1, reserved=0)
        setattr(bad, field, v)
        assert lib.nexg_frag_option_check(ctypes.byref(bad)) == abi.EINVAL, (field, v)
    for n in (0, 1, 256, 257, 65536, 65537, 1 << 24):
        tiles = (n + 255) // 256
        assert abi.fragment_plan_workspace(n) >= 16 * tiles + 8 and abi.fragment_plan_workspace(n) % 8 == 0
