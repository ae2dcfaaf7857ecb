"""GPU: the buffer contract (tests/test_hip_buffer_contract.py, on tests/guarded_buffers.py) of lcp_move_find_contacts_bp_f64 - guard
bands around every buffer, const inputs bitwise unchanged, padded contact slots zero, independence of buffer neighbourhood - once with
every optional pointer set and once with every optional pointer NULL (v, c_pen, p_out, max_pen, dt_used, t, trials, no_contact,
dt_scene, candidates), at nb = 7 / capacity 8 and nb = 40 / capacity 16."""
import pytest
import torch

from tests.test_hip_buffer_contract import F32, F64, I32, U8, Call, Case, R, _absmax, _check, _geometry, _narrow_scenes, _pad_slots, _wide_scenes

pytestmark = pytest.mark.gpu
DT = 1.0 / 30
OPTIONAL_OUT = ("c_pen", "p_out", "max_pen", "dt_used", "t", "trials", "candidates")


def _bp_case(scenes_, maxc, nvcap, full):
    kind, radius, verts, nverts, pose, totals = _geometry(scenes_, nvcap)
    B, nb = pose.shape[0], pose.shape[1]
    svm = max(totals)
    bufs = [("kind", I32, (B, nb), "in", kind), ("radius", F64, (B, nb), "in", radius), ("verts_local", F64, (B, nb, nvcap, 2), "in", verts),
            ("nverts", I32, (B, nb), "in", nverts), ("p_start", F64, (B, nb, 3), "in", pose)]
    det = [("c_n", F32, (B, maxc, 2)), ("c_p1", F32, (B, maxc, 2)), ("c_p2", F32, (B, maxc, 2)), ("c_i1", I32, (B, maxc)), ("c_i2", I32, (B, maxc)),
           ("count", I32, (B,))]
    t0 = 0.5 + torch.arange(B, dtype=F64)
    k_done = B // 2
    if full:
        v = torch.zeros(B, nb, 3)
        v[:, 1:, 2] = 40.0 + 10.0 * torch.arange(B).reshape(B, 1)
        dts = DT / (1 + torch.arange(B, dtype=F64))
        dts[k_done] = 0.0                                        # a finished scene among the live ones
        mask = torch.zeros(B, nb, nb, dtype=U8)
        mask[B - 1, 0, 1] = mask[B - 1, 1, 0] = 1
        bufs += [("v", F32, (B, nb, 3), "in", v), ("dt_scene", F64, (B,), "in", dts), ("no_contact", U8, (B, nb, nb), "in", mask)]
        det += [("p_out", F64, (B, nb, 3)), ("c_pen", F64, (B, maxc)), ("max_pen", F64, (B,)), ("dt_used", F64, (B,)), ("trials", I32, (B,)),
                ("candidates", I32, (B,))]
    bufs += [(n, d, s, "out", None) for n, d, s in det]
    if full:
        bufs.append(("t", F64, (B,), "inout", t0))
    writes = [n for n, _, _ in det] + (["t"] if full else [])
    steps = [Call("lcp_move_find_contacts_bp_f64",
                  [B, nb, maxc, nvcap, svm, R("kind"), R("radius"), R("verts_local"), R("nverts"), R("no_contact"), R("p_start"), R("v"), DT, DT / 4,
                   1, 16 if full else 1, 0.1, 1e-6] +
                  [R(n) for n in ("p_out", "c_n", "c_p1", "c_p2", "c_pen", "c_i1", "c_i2", "count", "max_pen", "dt_used", "t", "trials", "dt_scene",
                                  "candidates")], writes)]

    def post(outs):
        cnt = outs["count"]
        assert bool((cnt >= 0).all())
        pad = _pad_slots(cnt, maxc)
        for n in ("c_n", "c_p1", "c_p2", "c_pen", "c_i1", "c_i2"):
            if n in outs:
                assert _absmax(outs[n][pad]) == 0.0, (n, "padded records are not zero")
        if full:
            k = k_done
            assert float(outs["dt_used"][k]) == 0.0 and float(outs["t"][k]) == float(t0[k]) and int(outs["trials"][k]) == 1
            assert torch.equal(outs["p_out"][k], pose[k])
            live = torch.arange(B) != k
            assert bool((outs["dt_used"][live] > 0).all()) and torch.equal(outs["t"][live], t0[live] + outs["dt_used"][live])
            assert bool((outs["candidates"] >= 0).all()) and bool((outs["candidates"] <= nb * (nb - 1) // 2).all())

    # (with everything set: the optional OUTPUTS left out change nothing else)
    return Case(B, bufs, steps, nulls=[set(OPTIONAL_OUT)] if full else [], post=post)


@pytest.mark.parametrize("full", [True, False], ids=["all-set", "all-null"])
def test_bp_detection_7_bodies_capacity_8(full):
    outs = _check(_bp_case(_narrow_scenes(7, 3, 9), maxc=32, nvcap=8, full=full))
    assert int(outs["count"].max()) > 0


@pytest.mark.parametrize("full", [True, False], ids=["all-set", "all-null"])
def test_bp_detection_40_bodies_capacity_16(full):
    outs = _check(_bp_case(_wide_scenes(40, 3, 2064, (9, 17)), maxc=128, nvcap=16, full=full))
    assert int(outs["count"].min()) > 0
    if full:
        assert int(outs["candidates"].min()) > 0
