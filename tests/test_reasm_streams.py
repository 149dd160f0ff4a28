"""CPU: the stream contract of nex_amd.reassemble.Reassembler, under the
recording rig of tests/test_engine_streams.py (a stand-in for libnexg and a
proxy of torch whose streams are plain objects): run and push given stream=S
enqueue every kernel on S and do their host work (outputs, workspaces, the
read-backs, the gathers of the held frames) with S current; the current stream
is used as it stands; a rejected argument leaves the caller's stream current."""
import pytest
import torch

from nex_amd.engine import FrameBatch
from nex_amd.reassemble import Reassembler
from tests.test_engine_streams import N, FakeStream, Rig, check_all_on, events


def seeded(rig):
    """A Reassembler that already holds two frames, so that push takes the path that puts them in front."""
    rs = Reassembler(rig.eng, max_held_bytes=1 << 20)
    rs._held = FrameBatch(data=torch.zeros(128, dtype=torch.uint8), count=2, offsets=torch.tensor([0, 64, 128]))
    rs._epochs = torch.zeros(2, dtype=torch.int32)
    return rs


CASES = {
    "run": (lambda r, s: Reassembler(r.eng).run(r.table, align=16, stream=s),
            lambda r, s: Reassembler(r.eng).run(r.table, align=3, stream=s)),
    "push": (lambda r, s: seeded(r).push(r.table, 7, stream=s),
             lambda r, s: seeded(r).push(r.table, 1 << 32, stream=s)),
    "push, nothing held": (lambda r, s: Reassembler(r.eng).push(r.batch, 7, min_epoch=3, stream=s), None),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_explicit_stream_carries_the_host_side(monkeypatch, name):
    d, s = FakeStream("D", 0xD0), FakeStream("S", 0x50)
    rig = Rig(monkeypatch, d)
    out, src, rows, (hidx, held) = CASES[name][0](rig, s)
    check_all_on(rig.log, s)
    assert rig.torch.cuda.current is d
    assert len(events(rig.log, "enter")) == len(events(rig.log, "exit")) >= 1
    names = [e[1] for e in events(rig.log, "lib")]
    assert [n for n in names if n.startswith("nexg_reasm")] == ["nexg_reasm_plan", "nexg_reasm_frames", "nexg_reasm_held"]
    assert ("nexg_gather_frames" in names) == name.startswith("push")
    assert rows.numel() == 16 * (N + 2 if name == "push" else N) and out.count == 0 and held.count == 0


@pytest.mark.parametrize("name", sorted(k for k, (_, bad) in CASES.items() if bad))
def test_rejected_arguments_restore_the_stream(monkeypatch, name):
    d, s = FakeStream("D", 0xD0), FakeStream("S", 0x50)
    rig = Rig(monkeypatch, d)
    with pytest.raises(ValueError):
        CASES[name][1](rig, s)
    assert rig.torch.cuda.current is d
    assert not events(rig.log, "lib")
    for _, op, current in events(rig.log, "torch"):
        assert current is s, f"torch.{op} ran with {current} current, not {s}"


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("explicit", [False, True], ids=["stream=None", "stream=current"])
def test_current_stream_is_used_as_it_stands(monkeypatch, name, explicit):
    s = FakeStream("S", 0x50)
    rig = Rig(monkeypatch, s)
    CASES[name][0](rig, s if explicit else None)
    check_all_on(rig.log, s)
    assert rig.torch.cuda.current is s
    assert not events(rig.log, "enter")


def test_the_reassembler_is_no_engine_method():
    """The pass has state of its own, and tests/test_engine_streams.py's case table names every public Engine and
    FlowTable method that takes a stream."""
    from nex_amd.engine import Engine, FlowTable
    assert not any("reas" in n for cls in (Engine, FlowTable) for n in dir(cls))
