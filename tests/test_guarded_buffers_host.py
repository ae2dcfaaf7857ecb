"""The guarded arena of tests/guarded_buffers.py on a CPU arena: planted out-of-bounds torch writes are reported by buffer name and
byte offset, writes inside a buffer are not, a modified input is caught - the harness fails when it should, without any kernel
misbehaving."""
import pytest
import torch

from tests.guarded_buffers import ALIGN, GUARD_MIN, Arena, trailing_guard_bytes

B, NB = 5, 3


def _arena(fill=0xFF, reverse=False):
    g = torch.Generator().manual_seed(0)
    ar = Arena(B, "cpu", fill=fill, reverse=reverse)
    ar.add("v", torch.float32, (B, NB, 3), data=torch.randn(B, NB, 3, generator=g))
    ar.add("count", torch.int32, (B,), data=torch.arange(B, dtype=torch.int32))
    ar.add("jrot1", torch.float64, (B, 2), role="inout", data=torch.randn(B, 2, generator=g, dtype=torch.float64))
    ar.add("v_new", torch.float32, (B, NB, 3))
    ar.add("status", torch.int32, (B,))
    ar.add("p_out", torch.float64, (B, NB, 3))
    ar.add("ws", torch.uint8, (B * 1000 + 512,), role="ws")
    return ar.build()


@pytest.mark.parametrize("fill,reverse", [(0xFF, False), (0x00, True)])
def test_layout_alignment_fill_and_guards(fill, reverse):
    ar = _arena(fill, reverse)
    starts = [ar.span(n)[0] for n in ar.order()]
    for n in ar.names():
        start, nbytes, before, after = ar.span(n)
        assert ar.ptr(n).value % ALIGN == 0, n
        assert before[1] - before[0] >= GUARD_MIN and before[1] == start
        assert after[0] == start + nbytes
        assert after[1] - after[0] >= trailing_guard_bytes(nbytes, B) >= max(GUARD_MIN, 4 * (nbytes // B))
    assert starts == sorted(starts, reverse=reverse)
    spans = sorted(ar.span(n) for n in ar.names())
    assert spans[0][2][0] == 0 and spans[-1][3][1] == ar.mem.numel()          # a guard at both ends of the arena
    # the guards, the buffers and nothing else tile the arena
    covered = torch.zeros(ar.mem.numel(), dtype=torch.int32)
    for start, nbytes, before, after in spans:
        for lo, hi in (before, (start, start + nbytes), after):
            covered[lo:hi] += 1
    assert bool((covered == 1).all())
    assert bool(torch.isnan(ar["v_new"]).all()) and bool(torch.isnan(ar["p_out"]).all()) and bool((ar["status"] == -1).all())
    assert bool((ar.bytes_of("ws") == fill).all())
    assert ar["count"].tolist() == list(range(B))
    assert ar.check() == []
    assert ar.ptr(None) is None and ar.ptr("absent") is None


def test_a_write_inside_reports_nothing():
    ar = _arena()
    snap = ar.snapshot_inputs()
    ar["v_new"].fill_(1.5)
    ar["status"].zero_()
    ar["p_out"][B - 1, NB - 1, 2] = 2.0
    ar.bytes_of("ws").fill_(7)
    ar["jrot1"].add_(1.0)                                    # in-out: not part of the default snapshot
    assert ar.check() == []
    assert ar.inputs_unchanged(snap) == []


@pytest.mark.parametrize("reverse", [False, True])
def test_one_element_past_and_one_before_are_reported_by_name_and_offset(reverse):
    ar = _arena(reverse=reverse)
    n = B * NB * 3
    vs = ar.span("v_new")[0]
    flat = ar.mem[vs:].view(torch.float32)                                   # the buffer and what follows it, as floats
    flat[n] = 1.0                                                            # v_new[B, 0, 0]: one element past the end
    assert ar.check() == [("v_new", "after", 4 * n, 4 * n + 3)]
    ar.mem[vs + 4 * n:vs + 4 * n + 4] = 0xFF
    assert ar.check() == []
    st = ar.span("status")[0]
    ar.mem[st - 4:st].view(torch.int32)[0] = 0                               # status[-1]
    assert ar.check() == [("status", "before", -4, -1)]
    ar.mem[st - 4:st] = 0xFF
    # a scene block past the workspace, and a store for a scene that does not exist (B = 5 packed four to a wave: scenes 5 .. 7)
    ws, wn = ar.span("ws")[:2]
    ar.mem[ws + wn:ws + wn + 1000] = 3
    per = NB * 3 * 8
    po = ar.span("p_out")[0]
    ar.mem[po + 7 * per:po + 8 * per] = 0
    got = ar.check()
    assert ("ws", "after", wn, wn + 999) in got
    assert ("p_out", "after", 7 * per, 8 * per - 1) in got
    assert len(got) == 2


def test_zero_filled_guards_report_a_nonzero_write():
    ar = _arena(fill=0x00, reverse=True)
    c, cn = ar.span("count")[:2]
    ar.mem[c + cn:c + cn + 4].view(torch.int32)[0] = -1
    assert ar.check() == [("count", "after", cn, cn + 3)]


def test_a_modified_input_is_caught():
    ar = _arena()
    snap = ar.snapshot_inputs()
    assert sorted(snap) == ["count", "v"]
    ar["v"][2, 1, 0] += 1.0
    got = ar.inputs_unchanged(snap)
    assert len(got) == 1 and got[0][0] == "v"
    off = (2 * NB * 3 + 3) * 4
    assert off <= got[0][1] <= got[0][2] < off + 4
    assert ar.inputs_unchanged(snap, exempt=("v",)) == []
    # named snapshots: an in-out buffer that a particular call must leave alone
    snap = ar.snapshot_inputs(["jrot1", "count"])
    ar["jrot1"][0, 0] = 0.25
    assert [g[0] for g in ar.inputs_unchanged(snap)] == ["jrot1"]
    assert ar.inputs_unchanged(snap, exempt=("jrot1",)) == []


def test_roles_are_checked():
    ar = Arena(2)
    with pytest.raises(ValueError):
        ar.add("x", torch.float32, (2,), role="in")
    with pytest.raises(ValueError):
        ar.add("x", torch.float32, (2,), role="out", data=torch.zeros(2))
    ar.add("x", torch.float32, (2,))
    with pytest.raises(ValueError):
        ar.add("x", torch.float32, (2,))
