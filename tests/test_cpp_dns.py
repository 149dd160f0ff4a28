"""The C++ host API's DNS message pass (include/nexg.hpp Engine::dns,
dns_entries, dns_bufs, nexg::decode_dns_name; tests/native/cpp_dns_test.cpp).
CPU: the wrappers compile with -Wall -Werror and link against libnexg.so, and
decode_dns_name reproduces the reference's name vectors and error kinds. GPU:
the case list gives the same summaries, entry rows and decoded names as the
generator implies."""
import subprocess

import pytest

from nex_amd import abi

from tests.helpers import build_native_test  # __graft_entry__.build() makes it too


def test_cpp_dns_compiles_and_links():
    exe = build_native_test("cpp_dns_test")
    r = subprocess.run([exe, "--link"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["link", "ok", "3", "10", str(abi.dns_tile_first_bytes(65537)),
                                str(abi.dns_tile_first_bytes(0))]


@pytest.mark.gpu
def test_cpp_dns_gpu(tmp_path):
    from tests import dns_frames as df
    exe = build_native_test("cpp_dns_test")
    cs = df.cycled(df.cases(), 65)
    frames = [c.frame for c in cs]
    p = tmp_path / "frames.txt"
    p.write_text("".join((f.hex() or "-") + "\n" for f in frames))
    r = subprocess.run([exe, "--gpu", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split(" ", 2) for l in r.stdout.splitlines()]
    row = 0
    it = iter(lines)
    nxt = next(it, None)
    for i, c in enumerate(cs):
        want, wentries = c.expect()
        assert nxt is not None and nxt[0] == "D", (i, c.what)
        got = df.summary_array([want])
        raw = bytes.fromhex(nxt[1])
        assert raw[:28] == got.tobytes()[:28], (i, c.what)
        assert int(nxt[2]) == row, (i, c.what)
        names = iter(c.names)
        nxt = next(it, None)
        for e in wentries:
            assert nxt is not None and nxt[0] == "E", (i, c.what)
            assert bytes.fromhex(nxt[1]) == df.entry_array([e]).tobytes(), (i, c.what, e)
            if e["section"] == 0:
                assert nxt[2] == "=" + next(names), (i, c.what)
            nxt = next(it, None)
        row += len(wentries)
    assert nxt is None and row == sum(len(c.entries) for c in cs if c.candidate() and c.status == 0) > 50
