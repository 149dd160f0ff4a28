"""CPU: the strength of the fuzz corpus of tests/second_pass_fuzz.py, as a
permanent test. Every GPU test of the DNS, decap, select and flow passes
asserts device == host contract on some corpus, so a one-token fault in a
contract that a corpus does not notice would not be noticed in the kernel
either. For each entry of MUTANTS the contract function's source is taken, the
old text replaced by the new one, the variant built in a scratch namespace,
and the fuzz corpus must hold an input on which the variant differs from the
original (or raises).

SURVIVED_THE_HAND_CORPORA lists the faults the hand corpora (dns_frames.py,
select_frames.py, flow_frames.py as the suite had them before the fuzz corpus)
do not notice; that is asserted too, and is why this test exists. If a later
change to a hand corpus kills one of them, drop it from that list only.

Two faults of the list cannot be killed by any input, and are asserted as such
(EQUIVALENT): the variant is the same function.
  - dns_host, `n - pos < ln` made `<=`: the two differ only when a label takes
    exactly the bytes that are left; the original then goes on to read the next
    length byte at pos == n and fails there, with the same MALFORMED summary
    (so does dns.rs:765 and then :756).
  - gre_fields, `0xC000` made `0x8000`: the two differ only for R set without
    C, and every header with R set is refused in the end whether or not its
    checksum + offset word was consumed (gre.rs:57-63, 79-82).
For these the test asserts that the corpus holds the inputs at the boundary
(a label ending on the last message byte; R-only headers with fewer than,
exactly and more than 4 bytes after the first word) and that the variant gives
the original's result on all of them."""
import inspect

import pytest

from nex_amd import abi
from nex_amd import dns as hostdns
from nex_amd import flow as hostflow
from nex_amd import select as hostselect
from nex_amd import tunnel as hosttunnel
from tests import dns_frames as df
from tests import flow_frames as ff
from tests import second_pass_fuzz as fz
from tests import second_pass_ref as ref
from tests import select_frames as sf

#: (name, function, old text, new text, which occurrence of the old text)
MUTANTS = [
    # ---- dns_host
    ("dns label <=", hostdns.dns_host, "if n - pos < ln:", "if n - pos <= ln:", 0),
    ("dns section short: answers only", hostdns.dns_host, "if got < declared:",
     "if got < declared and sec == abi.DNS_ANSWER:", 0),
    ("dns type+class <= 4", hostdns.dns_host, "n - pos < 4", "n - pos <= 4", 0),
    ("dns type+class < 3", hostdns.dns_host, "n - pos < 4", "n - pos < 3", 0),
    ("dns record > 12", hostdns.dns_host, "n - pos >= 12", "n - pos > 12", 0),
    ("dns record >= 11", hostdns.dns_host, "n - pos >= 12", "n - pos >= 11", 0),
    ("dns data cut >=", hostdns.dns_host, "if dl > room", "if dl >= room", 0),
    ("dns advance by data_len", hostdns.dns_host, "min(dl, room)", "dl", 0),
    ("dns length byte at pos > n", hostdns.dns_host, "if pos >= n:", "if pos > n:", 0),
    ("dns header <= 12", hostdns.dns_host, "if n < 12:", "if n <= 12:", 0),
    # ---- rule_matches
    ("rule any-addr: destination with src_bits - 1", hostselect.rule_matches, "_prefix(d, r.src, r.src_bits))",
     "_prefix(d, r.src, max(r.src_bits - 1, 0)))", 0),
    ("rule tcp flags under 0x3F", hostselect.rule_matches, "& r.tcp_mask == r.tcp_value",
     "& r.tcp_mask & 0x3F == r.tcp_value & 0x3F", 0),
    ("rule ipv6 header < length", hostselect.rule_matches, "l3 + 40 <= length", "l3 + 40 < length", 0),
    ("rule sport low end", hostselect.rule_matches, "l4 and r.sport_lo <= sport <=", "l4 and r.sport_lo < sport <=", 0),
    ("rule sport high end", hostselect.rule_matches, "<= sport <= r.sport_hi)", "<= sport < r.sport_hi)", 0),
    ("rule dport low end", hostselect.rule_matches, "r.dport_lo <= dport", "r.dport_lo < dport", 0),
    ("rule dport high end", hostselect.rule_matches, "dport <= r.dport_hi", "dport < r.dport_hi", 0),
    ("rule any-port: dport high end", hostselect.rule_matches, "<= dport <= r.sport_hi", "<= dport < r.sport_hi", 0),
    ("rule length low end", hostselect.rule_matches, "r.len_lo <= length", "r.len_lo < length", 0),
    ("rule length high end", hostselect.rule_matches, "length <= r.len_hi", "length < r.len_hi", 0),
    ("rule src prefix one bit short", hostselect.rule_matches, "not _prefix(s, r.src, r.src_bits):",
     "not _prefix(s, r.src, max(r.src_bits - 1, 0)):", 0),
    ("rule dst prefix one bit short", hostselect.rule_matches, "not _prefix(d, r.dst, r.dst_bits):",
     "not _prefix(d, r.dst, max(r.dst_bits - 1, 0)):", 0),
    # ---- flow_key
    ("flow fragment test 0x1FFF", hostflow.flow_key, "& 0x3FFF", "& 0x1FFF", 0),
    ("flow fragment test 0x2000", hostflow.flow_key, "& 0x3FFF", "& 0x2000", 0),
    ("flow ipv6 header >= length", hostflow.flow_key, "l3 + 40 > length", "l3 + 40 >= length", 0),
    ("flow symmetric compare without ports", hostflow.flow_key, "src + sp > dst + dp", "src > dst", 0),
    ("flow symmetric compare >=", hostflow.flow_key, "src + sp > dst + dp", "src + sp >= dst + dp", 0),
    # ---- gre_fields
    ("gre base header <= 4", hosttunnel.gre_fields, "< 4:", "<= 4:", 0),
    ("gre checksum word <= 4", hosttunnel.gre_fields, "< 4:", "<= 4:", 1),
    ("gre key <= 4", hosttunnel.gre_fields, "< 4:", "<= 4:", 2),
    ("gre sequence <= 4", hosttunnel.gre_fields, "< 4:", "<= 4:", 3),
    ("gre key and sequence swapped", hosttunnel.gre_fields, "key, seq)", "seq, key)", 0),
    ("gre routing test dropped", hosttunnel.gre_fields, "if flags & 0x4000:", "if False:", 0),
    ("gre checksum word for C only", hosttunnel.gre_fields, "0xC000", "0x8000", 0),
    # ---- vxlan_fields
    ("vxlan <= 8", hosttunnel.vxlan_fields, "< 8:", "<= 8:", 0),
    ("vxlan vni from bytes 5..8", hosttunnel.vxlan_fields, "payload[4:7]", "payload[5:8]", 0),
]
EQUIVALENT = {"dns label <=", "gre checksum word for C only"}
SURVIVED_THE_HAND_CORPORA = {
    "dns label <=", "dns section short: answers only", "rule any-addr: destination with src_bits - 1",
    "rule tcp flags under 0x3F", "flow fragment test 0x1FFF", "flow fragment test 0x2000", "flow ipv6 header >= length",
    "rule ipv6 header < length"}
OPTIONS = [hostflow.FlowOption(symmetric=s, ports=p) for s in (False, True) for p in (True, False)]


def variant(fn, old, new, nth):
    """`fn` with the nth occurrence of `old` in its source replaced by `new`,
    built in a copy of its module's namespace."""
    src = inspect.getsource(fn)
    parts = src.split(old)
    assert len(parts) > nth + 1, (fn.__name__, old, "is not in the source")
    src = old.join(parts[: nth + 1]) + new + old.join(parts[nth + 1:])
    space = dict(inspect.getmodule(fn).__dict__)
    exec(compile(src, f"<variant of {fn.__name__}>", "exec"), space)
    return space[fn.__name__]


def differs(a, b, inputs):
    """The first input on which the two functions differ (the variant raising counts), or None."""
    for x in inputs:
        want = a(*x)
        try:
            got = b(*x)
        except Exception:  # noqa: BLE001 - a variant that indexes past the message is a detected fault
            return x
        if got != want:
            return x
    return None


class Inputs:
    """Per contract function, the argument tuples a corpus gives it."""

    def __init__(self, messages, gre_payloads, vxlan_payloads, sel_frames, sel_recs, rules, flow_frames, flow_recs):
        self.by_fn = {
            "dns_host": [(m,) for m in messages],
            "gre_fields": [(p,) for p in gre_payloads],
            "vxlan_fields": [(p,) for p in vxlan_payloads],
            "rule_matches": lambda: ((f, r, len(f), rule) for rule in rules for f, r in zip(sel_frames, sel_recs)),
            "flow_key": lambda: ((f, r, len(f), o) for o in OPTIONS for f, r in zip(flow_frames, flow_recs)),
        }

    def of(self, fn):
        x = self.by_fn[fn.__name__]
        return x() if callable(x) else x


@pytest.fixture(scope="module")
def fuzz_inputs(oracle):
    c = fz.corpora(oracle)
    messages = {ref.udp_payload(f, r) for f, r in zip(c.dns, c.dns_recs)} - {None}
    gre, vxlan = set(), set()
    for f, r in zip(c.tun, c.tun_recs):  # a parser sees the payloads of its own candidates
        kind = ref.tunnel_candidate(f, r)
        if kind != abi.TUN_NONE:
            p = bytes(f[int(r["payload_off"]): int(r["payload_off"]) + int(r["payload_len"])])
            (gre if kind == abi.TUN_GRE else vxlan).add(p)
    rules = [r for flt in c.filters for r in flt.rules]
    return Inputs(sorted(messages), sorted(gre), sorted(vxlan), c.sel, c.sel_recs, rules, c.flow, c.flow_recs)


@pytest.fixture(scope="module")
def hand_inputs(oracle):
    """The hand corpora: the DNS case list's messages, the select corpus with
    its table rules and filters, the flow corpus."""
    messages = [c.msg for c in df.cases() if c.msg is not None]
    sel = [x.frame for x in sf.corpus()]
    sel_recs = oracle.parse_frames(sel, sf.PARSE_FLAGS)
    rules = [r for _, flt in sf.all_filters() for r in flt.rules]
    flow = [x.frame for x in ff.corpus()]
    flow_recs = oracle.parse_frames(flow, ff.PARSE_FLAGS)
    return Inputs(messages, [], [], sel, sel_recs, rules, flow, flow_recs)


def test_the_list():
    names = [m[0] for m in MUTANTS]
    assert len(set(names)) == len(names) >= 30
    assert EQUIVALENT <= set(names) and SURVIVED_THE_HAND_CORPORA <= set(names)


@pytest.mark.parametrize("name,fn,old,new,nth", [m for m in MUTANTS if m[0] not in EQUIVALENT],
                         ids=[m[0] for m in MUTANTS if m[0] not in EQUIVALENT])
def test_fuzz_corpus_kills(fuzz_inputs, name, fn, old, new, nth):
    hit = differs(fn, variant(fn, old, new, nth), fuzz_inputs.of(fn))
    assert hit is not None, f"{name}: no input of the fuzz corpus tells `{new}` from `{old}` in {fn.__name__}"


@pytest.mark.parametrize("name,fn,old,new,nth", [m for m in MUTANTS if m[0] in SURVIVED_THE_HAND_CORPORA],
                         ids=[m[0] for m in MUTANTS if m[0] in SURVIVED_THE_HAND_CORPORA])
def test_hand_corpora_do_not(hand_inputs, name, fn, old, new, nth):
    hit = differs(fn, variant(fn, old, new, nth), hand_inputs.of(fn))
    assert hit is None, f"{name}: a hand corpus now kills it ({hit!r}); drop it from SURVIVED_THE_HAND_CORPORA"


def test_equivalent_variants_are_the_same_function(fuzz_inputs):
    """See the module docstring: no input exists; the boundary inputs are in the corpus and agree."""
    by_name = {m[0]: m for m in MUTANTS}
    _, fn, old, new, nth = by_name["dns label <="]
    at_boundary = [x for x in fuzz_inputs.of(fn) if ref.qname_label_ends_message(x[0])]
    assert len(at_boundary) >= 20
    assert differs(fn, variant(fn, old, new, nth), fuzz_inputs.of(fn)) is None
    _, fn, old, new, nth = by_name["gre checksum word for C only"]
    r_only = [x for x in fuzz_inputs.of(fn) if len(x[0]) >= 4 and x[0][0] & 0xC0 == 0x40]
    assert {min(len(x[0]) - 4, 5) for x in r_only} == {0, 1, 2, 3, 4, 5}
    assert differs(fn, variant(fn, old, new, nth), fuzz_inputs.of(fn)) is None
    assert all(fn(*x) is None for x in r_only)
