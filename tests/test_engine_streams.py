"""CPU: the stream contract of every Engine pass and of FlowTable.update.

A pass given `stream=S` enqueues its kernels on S, and everything its host
side does through torch (outputs, workspaces, count cells, cumsum, the
read-backs that size the second kernel) has to be in S's order as well: torch
issues those on the *current* stream and from its allocator pool, so the body
has to run under torch.cuda.stream(S). Nothing here needs a GPU or the
library: the engine gets a recording stand-in for libnexg and a thin proxy of
torch whose streams are plain objects, and the log says on which stream each
library call, allocation and reduction happened. torch.empty is served as
zeros, so every read-back is 0 and every method runs to its end.

The case table has one entry per public method with a `stream` parameter; the
completeness test holds it against inspect.signature, so a pass added without
a case fails here."""
import contextlib
import inspect

import pytest
import torch

from nex_amd import abi
from nex_amd import engine as engine_mod
from nex_amd.encap import Tunnel, TunnelSet
from nex_amd.engine import Engine, FlowTable, FrameBatch
from nex_amd.flow import FlowOption
from nex_amd.match import Pattern, PatternSet
from nex_amd.rewrite import Action, ActionSet
from nex_amd.select import Filter, Rule

N = 5  # frames of every input batch


class FakeStream:
    def __init__(self, name, handle):
        self.name, self.cuda_stream = name, handle

    def __repr__(self):
        return f"<stream {self.name}>"


class FakeCuda:
    def __init__(self, log, current):
        self.log, self.current = log, current

    def current_stream(self, device=None):
        return self.current

    @contextlib.contextmanager
    def stream(self, s):
        before = self.current
        self.log.append(("enter", s))
        self.current = s
        try:
            yield
        finally:
            self.current = before
            self.log.append(("exit", s))

    def synchronize(self, device=None):
        pass


class FakeTorch:
    """torch, with streams that are plain objects and a log of what allocates
    or reduces: (op, current stream)."""
    LOGGED = ("empty", "zeros", "stack", "cumsum", "full")

    def __init__(self, log, current):
        self.log = log
        self.cuda = FakeCuda(log, current)

    def __getattr__(self, name):
        real = getattr(torch, "zeros" if name == "empty" else name)
        if name not in self.LOGGED:
            return real

        def logged(*args, **kwargs):
            self.log.append(("torch", name, self.cuda.current))
            return real(*args, **kwargs)
        return logged


class FakeLib:
    """libnexg: every nexg_* entry logs (name, its last argument, the current
    stream) and reports success."""

    def __init__(self, log, cuda):
        self._log, self._cuda = log, cuda

    def nexg_ctx_last_error(self, ctx):
        return b"no error"

    def nexg_strerror(self, rc):
        return b"no error"

    def __getattr__(self, name):
        if not name.startswith("nexg_"):
            raise AttributeError(name)

        def call(*args):
            last = args[-1]
            self._log.append(("lib", name, getattr(last, "value", last), self._cuda.current))
            return abi.OK
        return call


class Rig:
    """An Engine over the stand-ins, and the inputs of every case."""

    def __init__(self, monkeypatch, current):
        self.log = []
        self.torch = FakeTorch(self.log, current)
        monkeypatch.setattr(engine_mod, "_torch", lambda: self.torch)
        eng = Engine.__new__(Engine)
        eng.lib = FakeLib(self.log, self.torch.cuda)
        eng.ctx = object()
        eng.device = 0
        eng.torch_device = torch.device("cpu")
        self.eng = eng
        u8 = lambda n: torch.zeros(n, dtype=torch.uint8)  # noqa: E731
        self.batch = FrameBatch(data=u8(N * 64), count=N, stride=64)
        self.table = FrameBatch(data=u8(N * 64), count=N, offsets=torch.arange(N, dtype=torch.int64) * 64,
                                lengths=torch.full((N,), 64, dtype=torch.int32))
        self.records, self.rows8, self.tunnels = u8(N * 64), u8(N * 8), u8(N * 16)
        self.index = torch.zeros(N, dtype=torch.int32)
        self.i32 = torch.zeros(N, dtype=torch.int32)
        self.ip4, self.ip6, self.mac = u8(N * 4).view(N, 4), u8(N * 16).view(N, 16), u8(N * 6).view(N, 6)
        self.tuples = torch.zeros((N, 4), dtype=torch.int32)
        self.big = u8(16384)
        self.actions = ActionSet([Action(sets=abi.SET_TTL, ttl=7)])
        self.tunnel_set = TunnelSet((Tunnel.vxlan(vni=5001, src="192.0.2.1", dst="198.51.100.7"),))
        self.filter = Filter([Rule.udp() & Rule.port(53)])
        self.patterns = PatternSet([Pattern(b"Host: ", nocase=True)])
        self.flow_option = FlowOption(symmetric=True)
        self.flow_table = FlowTable(eng, self.flow_option, capacity=4)
        self.flow_table._next = u8(0)  # too small: update has to allocate it again
        self.log.clear()


# name -> (call, invalid): call(rig, stream) makes the call, invalid(rig, stream) (or None) makes one
# that the method's own argument validation rejects with ValueError
CASES = {
    "Engine.parse": (lambda r, s: r.eng.parse(r.batch, out_kind=abi.OUT_RECORD, stream=s),
                     lambda r, s: r.eng.parse(r.batch, out=r.rows8[:1], stream=s)),
    "Engine.sparse_expand": (lambda r, s: r.eng.sparse_expand(r.batch, r.records, stream=s), None),
    "Engine.recompute_checksums": (lambda r, s: r.eng.recompute_checksums(r.batch, stream=s), None),
    "Engine.rewrite": (lambda r, s: r.eng.rewrite(r.batch, r.actions, stream=s),
                       lambda r, s: r.eng.rewrite(r.batch, ActionSet([]), stream=s)),
    "Engine.decode_options": (lambda r, s: r.eng.decode_options(r.batch, r.records, stream=s), None),
    "Engine.decap": (lambda r, s: r.eng.decap(r.batch, r.records, stream=s), None),
    "Engine.decap_select": (lambda r, s: r.eng.decap_select(r.tunnels, r.table, {abi.INNER_ETHERNET}, stream=s), None),
    "Engine.select": (lambda r, s: r.eng.select(r.batch, r.records, r.filter, want_rule=True, stream=s),
                      lambda r, s: r.eng.select(r.batch, r.records, Filter([]), stream=s)),
    "Engine.match": (lambda r, s: r.eng.match(r.batch, r.records, r.patterns, stream=s),
                     lambda r, s: r.eng.match(r.batch, r.records, PatternSet([]), stream=s)),
    "Engine.match_select": (lambda r, s: r.eng.match_select(r.batch, r.rows8, any=1, stream=s),
                            lambda r, s: r.eng.match_select(r.batch, r.rows8, any=-1, stream=s)),
    "Engine.gather": (lambda r, s: r.eng.gather(r.table, align=16, stream=s),
                      lambda r, s: r.eng.gather(r.table, align=3, stream=s)),
    "Engine.encap": (lambda r, s: r.eng.encap(r.batch, r.tunnel_set, stream=s),
                     lambda r, s: r.eng.encap(r.batch, r.tunnel_set, align=3, stream=s)),
    "Engine.fragment": (lambda r, s: r.eng.fragment(r.batch, 576, align=4, stream=s),
                        lambda r, s: r.eng.fragment(r.batch, 10, stream=s)),
    "Engine.gather_rows": (lambda r, s: r.eng.gather_rows(r.records, 64, r.index, stream=s),
                           lambda r, s: r.eng.gather_rows(r.records, 5, r.index, stream=s)),
    "Engine.flow": (lambda r, s: r.eng.flow(r.batch, r.records, r.flow_option, stream=s),
                    lambda r, s: r.eng.flow(r.batch, r.records, FlowOption(reserved=1), stream=s)),
    "Engine.flow_partition": (lambda r, s: r.eng.flow_partition(r.batch, r.rows8, 8, stream=s),
                              lambda r, s: r.eng.flow_partition(r.batch, r.rows8, 0, stream=s)),
    "Engine.flow_sort": (lambda r, s: r.eng.flow_sort(r.rows8, stream=s), None),
    "Engine.flow_groups": (lambda r, s: r.eng.flow_groups(r.batch, r.records, r.rows8, r.flow_option, stream=s),
                           lambda r, s: r.eng.flow_groups(r.batch, r.records, r.rows8, FlowOption(reserved=1), stream=s)),
    "Engine.flow_table_merge": (lambda r, s: r.eng.flow_table_merge(r.batch, r.records, r.rows8[:32], stream=s),
                                lambda r, s: r.eng.flow_table_merge(r.batch, r.records, r.rows8[:32], table_cap=2,
                                                                    out=r.rows8, stream=s)),
    "Engine.dns": (lambda r, s: r.eng.dns(r.batch, r.records, stream=s), None),
    "Engine.probe_stream": (lambda r, s: r.eng.probe_stream(r.big, 8, stream=s), None),
    "Engine.probe_write": (lambda r, s: r.eng.probe_write(r.big, stream=s), None),
    "Engine.probe_span_clock": (lambda r, s: r.eng.probe_span_clock(r.table, stream=s), None),
    "Engine.probe_latency": (lambda r, s: r.eng.probe_latency(r.big, stream=s), None),
    "Engine.checksum": (lambda r, s: r.eng.checksum(r.batch, 0, stream=s), None),
    "Engine.build_udp4": (lambda r, s: r.eng.build_udp4(r.i32, r.i32, stream=s),
                          lambda r, s: r.eng.build_udp4(r.i32[:1], r.i32, stream=s)),
    "Engine.build_udp4_tuples": (lambda r, s: r.eng.build_udp4_tuples(r.tuples, stream=s),
                                 lambda r, s: r.eng.build_udp4_tuples(r.tuples, out=r.rows8, stream=s)),
    "Engine.build_udp6": (lambda r, s: r.eng.build_udp6(r.ip6, r.ip6, stream=s),
                          lambda r, s: r.eng.build_udp6(r.ip6[:2], r.ip6, stream=s)),
    "Engine.build_tcp": (lambda r, s: r.eng.build_tcp(4, r.ip4, r.ip4, stream=s),
                         lambda r, s: r.eng.build_tcp(4, r.ip4[:2], r.ip4, stream=s)),
    "Engine.build_icmp_echo": (lambda r, s: r.eng.build_icmp_echo(6, r.ip6, r.ip6, stream=s),
                               lambda r, s: r.eng.build_icmp_echo(6, r.ip6[:2], r.ip6, stream=s)),
    "Engine.build_arp": (lambda r, s: r.eng.build_arp(r.ip4, stream=s), None),
    "Engine.build_ndp_ns": (lambda r, s: r.eng.build_ndp_ns(r.ip6, r.ip6, stream=s), None),
    "Engine.gen_batch": (lambda r, s: r.eng.gen_batch(abi.WL_IMIX, N, record_gap=16, stream=s), None),
    "Engine.gen_udp4_params": (lambda r, s: r.eng.gen_udp4_params(N, stream=s), None),
    "FlowTable.update": (lambda r, s: r.flow_table.update(r.batch, r.records, 1, stream=s), None),
}
INVALID = sorted(k for k, (_, bad) in CASES.items() if bad is not None)


def test_case_table_is_complete():
    """Every public method of Engine and FlowTable that takes `stream`."""
    have = {f"{cls.__name__}.{name}" for cls in (Engine, FlowTable) for name, fn in inspect.getmembers(cls, callable)
            if not name.startswith("_") and "stream" in inspect.signature(fn).parameters}
    assert have == set(CASES)
    assert len(have) >= 35


def events(log, kind):
    return [e for e in log if e[0] == kind]


def check_all_on(log, s):
    calls = events(log, "lib")
    assert calls, "no library call was made"
    for _, name, handle, current in calls:
        assert handle == s.cuda_stream, f"{name} was given stream {handle:#x}, not {s}"
        assert current is s, f"{name} was called with {current} current, not {s}"
    for _, op, current in events(log, "torch"):
        assert current is s, f"torch.{op} ran with {current} current, not {s}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_explicit_stream_carries_the_host_side(monkeypatch, name):
    """stream=S while D is current: the library gets S, every allocation and
    reduction happens with S current, and D is current again on return."""
    d, s = FakeStream("D", 0xD0), FakeStream("S", 0x50)
    rig = Rig(monkeypatch, d)
    CASES[name][0](rig, s)
    check_all_on(rig.log, s)
    assert rig.torch.cuda.current is d
    assert len(events(rig.log, "enter")) == len(events(rig.log, "exit")) >= 1


@pytest.mark.parametrize("name", INVALID)
def test_rejected_arguments_restore_the_stream(monkeypatch, name):
    d, s = FakeStream("D", 0xD0), FakeStream("S", 0x50)
    rig = Rig(monkeypatch, d)
    with pytest.raises(ValueError):
        CASES[name][1](rig, s)
    assert rig.torch.cuda.current is d
    for _, op, current in events(rig.log, "torch"):
        assert current is s, f"torch.{op} ran with {current} current, not {s}"


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("explicit", [False, True], ids=["stream=None", "stream=current"])
def test_current_stream_is_used_as_it_stands(monkeypatch, name, explicit):
    """stream=None (or the current stream itself) while S is current: the
    library gets S, and torch.cuda.stream is never entered, so the default
    path does the host work it always did."""
    s = FakeStream("S", 0x50)
    rig = Rig(monkeypatch, s)
    CASES[name][0](rig, s if explicit else None)
    check_all_on(rig.log, s)
    assert rig.torch.cuda.current is s
    assert not events(rig.log, "enter")
