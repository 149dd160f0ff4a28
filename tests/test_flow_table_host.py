"""CPU: the host contract of the flow table across batches
(nex_amd.flow.merge_host restates nexg_flow_table_merge of include/nexg.h).

- merge_host chained over the batch sequences of tests/flow_table_ref.py (the
  corpus cut into batches, the pinned collision pair in one batch and across
  batches, a real flow under hash 0, keys that differ in kind or in protocol
  alone, expiry at, below and above min_epoch, empty batches, bad extents)
  against RefTable, the independent per-hash dictionary fed frame by frame,
  under the four symmetric x ports options: the table after every batch, and
  every frame's entry through slot and group_of;
- what the sequences must show, stated on its own: where MIXED appears and
  where it does not, what expires, that nothing is lost at min_epoch = 0;
- seeded faults in merge_host that the sequences must notice, in the way of
  tests/test_second_pass_mutants.py."""
import numpy as np
import pytest

from nex_amd import abi
from nex_amd.flow import merge_host
from tests import flow_table_ref as tr
from tests.test_second_pass_mutants import variant


@pytest.fixture(scope="module")
def seqs(oracle):
    return tr.sequences(oracle)


@pytest.mark.parametrize("symmetric,ports", tr.OPTIONS)
def test_merge_host_against_the_reference(seqs, symmetric, ports):
    for name, batches in seqs.items():
        want, fed = tr.run_reference(batches, symmetric, ports)
        got = tr.run_host(merge_host, batches, symmetric, ports)
        for k, ((table, row), (want_table, want_row)) in enumerate(zip(got, want)):
            tr.entries_equal(table, want_table, (name, k))
            assert (row == want_row).all(), (name, k)
            assert (np.diff(table["hash"].astype(np.int64)) > 0).all(), (name, k)
        if all(b.min_epoch == 0 for b in batches):
            assert int(got[-1][0]["packets"].sum()) == fed == sum(len(b.frames) for b in batches), name


def last_table(seqs, name, symmetric=False, ports=True):
    return [t for t, _ in tr.run_host(merge_host, seqs[name], symmetric, ports)]


def entry(table, h):
    rows = table[table["hash"] == h]
    assert len(rows) == 1, (h, len(rows))
    return rows[0]


def test_mixed_appears_at_the_merge_and_only_there(seqs):
    first, second = last_table(seqs, "collision: A then B")
    a = [e for e in first if int(e["kind"]) == abi.FLOW_IPV4_L4 and bytes(e["key"][:4]) == bytes([10, 0, 0, 1])]
    assert len(a) == 1 and int(a[0]["flags8"]) == 0
    h = int(a[0]["hash"])
    e = entry(second, h)
    assert int(e["flags8"]) == abi.FLOW_ENTRY_MIXED and int(e["packets"]) == 2 and int(e["last_epoch"]) == 2
    assert bytes(e["key"]) == bytes(a[0]["key"])  # the first key stays
    assert int(second["flags8"].sum()) == 1 and len(second) == 2
    first, second = last_table(seqs, "collision: A then A")
    assert int(entry(second, h)["flags8"]) == 0 and int(entry(second, h)["packets"]) == 3
    tables = last_table(seqs, "collision: A, B, then A again")
    assert [int(entry(t, h)["flags8"]) for t in tables] == [0, 1, 1]
    tables = last_table(seqs, "collision inside a batch, then carried")
    assert [int(entry(t, h)["flags8"]) for t in tables] == [1, 1, 1]
    assert [int(entry(t, h)["last_epoch"]) for t in tables] == [1, 1, 3]


def test_the_no_flow_group_is_an_entry_like_any_other(seqs):
    first, second = last_table(seqs, "no flow, then a real flow under hash 0")
    e = entry(first, 0)
    assert (int(e["kind"]), int(e["proto"]), int(e["flags8"]), int(e["packets"])) == (abi.FLOW_NONE, 0, 0, 1)
    assert not e["key"].any()
    e = entry(second, 0)
    assert (int(e["kind"]), int(e["flags8"]), int(e["packets"])) == (abi.FLOW_NONE, abi.FLOW_ENTRY_MIXED, 2)
    first, second = last_table(seqs, "a real flow under hash 0, then no flow")
    assert (int(entry(first, 0)["kind"]), int(entry(first, 0)["flags8"])) == (abi.FLOW_IPV4_L4, 0)
    assert (int(entry(second, 0)["kind"]), int(entry(second, 0)["flags8"])) == (abi.FLOW_IPV4_L4, abi.FLOW_ENTRY_MIXED)


def test_kind_and_proto_are_part_of_the_key(seqs):
    for name in ("same key bytes, another protocol", "same padded key bytes, another kind"):
        first, second = last_table(seqs, name)
        shared = set(first["hash"].tolist()) & set(seqs[name][1].flows(False, True)["hash"].tolist())
        assert len(shared) == 1, name
        h = shared.pop()
        assert bytes(entry(first, h)["key"]) == bytes(entry(second, h)["key"]), name
        assert (int(entry(first, h)["flags8"]), int(entry(second, h)["flags8"])) == (0, abi.FLOW_ENTRY_MIXED), name


def test_expiry(seqs):
    tables = last_table(seqs, "expiry: equal is kept, one below is dropped")
    assert [len(t) for t in tables] == [1, 2, 3, 3]
    assert sorted(tables[3]["last_epoch"].tolist()) == [6, 7, 8]  # epoch 5 went, epoch 6 == min_epoch stayed
    tables = last_table(seqs, "expiry: an old entry that is matched stays")
    assert [len(t) for t in tables] == [1, 2, 3, 3]
    assert sorted(tables[3]["last_epoch"].tolist()) == [7, 8, 8]  # epoch 6 went; the entry of epoch 5 was matched
    old = entry(tables[3], int(tables[0]["hash"][0]))
    assert (int(old["packets"]), int(old["last_epoch"])) == (2, 8)
    tables = last_table(seqs, "expiry: everything old goes, the batch's own flows stay")
    assert (tables[2]["last_epoch"] == 9).all() and 0 < len(tables[2]) < len(tables[1])
    tables = last_table(seqs, "an empty batch expires")
    assert (tables[2]["last_epoch"] == 2).all() and 0 < len(tables[2]) < len(tables[1])
    assert [len(t) for t in last_table(seqs, "an empty batch into an empty table")] == [0]


# ---- seeded faults ---------------------------------------------------------------------------------

#: (name, old text, new text) in merge_host's source
MUTANTS = [
    ("group before table on ties", '<= int(groups[j]["hash"])', '< int(groups[j]["hash"])'),
    ("> instead of >= in the expiry", 'int(e["last_epoch"]) >= min_epoch', 'int(e["last_epoch"]) > min_epoch'),
    ("MIXED not OR-ed with the old flag", 'mixed = bool(int(e["flags8"]) & abi.FLOW_ENTRY_MIXED) or', 'mixed ='),
    ("the key compare ignores kind", 'differs = kind != int(e["kind"]) or', 'differs ='),
    ("the key compare ignores proto", 'proto != int(e["proto"]) or', ''),
    ("last_epoch not updated on a match", 'e["last_epoch"] = epoch\n', 'pass\n'),
    ("dropped entries still counted in slot", 'n_out += 1 if keep else 0', 'n_out += 1'),
]


def result(merge, batches, symmetric, ports):
    return [(t.tobytes(), r.tobytes()) for t, r in tr.run_host(merge, batches, symmetric, ports)]


@pytest.mark.parametrize("name,old,new", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_the_sequences_notice(seqs, name, old, new):
    bad = variant(merge_host, old, new, 0)
    for batches in seqs.values():
        try:
            if result(bad, batches, False, True) != result(merge_host, batches, False, True):
                return
        except Exception:  # noqa: BLE001 - a variant that raises is a detected fault
            return
    pytest.fail(f"{name}: no sequence tells `{new}` from `{old}` in merge_host")
