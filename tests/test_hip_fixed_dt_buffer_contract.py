"""GPU: the buffer contract (tests/test_hip_buffer_contract.py, on tests/guarded_buffers.py) of the three entry points of the
fixed-interval stepping: lcp_move_find_contacts_dts_f64, lcp_substep_begin_f64, lcp_substep_commit_f32 - guard bands around every
buffer, const inputs bitwise unchanged, optional outputs NULL, padded contact slots zero, independence of buffer neighbourhood."""
import pytest
import torch

from tests.test_hip_buffer_contract import (F32, F64, I32, QUAD_B, Call, Case, R, _absmax, _check, _geometry, _narrow_scenes, _pad_slots, _randn,
                                            _wide_scenes)

pytestmark = pytest.mark.gpu
DT = 1.0 / 30


def _dts_case(scenes_, maxc, nvcap=8, svm=None):
    kind, radius, verts, nverts, pose, totals = _geometry(scenes_, nvcap)
    B, nb = pose.shape[0], pose.shape[1]
    svm = max(totals) if svm is None else svm
    v = torch.zeros(B, nb, 3)
    v[:, 1:, 2] = 40.0 + 10.0 * torch.arange(B).reshape(B, 1)
    dts = DT / (1 + torch.arange(B, dtype=F64))
    dts[B // 2] = 0.0                                            # a finished scene among the live ones
    t0 = 0.5 + torch.arange(B, dtype=F64)
    bufs = [("kind", I32, (B, nb), "in", kind), ("radius", F64, (B, nb), "in", radius), ("verts_local", F64, (B, nb, nvcap, 2), "in", verts),
            ("nverts", I32, (B, nb), "in", nverts), ("p_start", F64, (B, nb, 3), "in", pose), ("v", F32, (B, nb, 3), "in", v),
            ("dt_scene", F64, (B,), "in", dts)]
    det = [("p_out", F64, (B, nb, 3)), ("c_n", F32, (B, maxc, 2)), ("c_p1", F32, (B, maxc, 2)), ("c_p2", F32, (B, maxc, 2)),
           ("c_pen", F64, (B, maxc)), ("c_i1", I32, (B, maxc)), ("c_i2", I32, (B, maxc)), ("count", I32, (B,)), ("max_pen", F64, (B,)),
           ("dt_used", F64, (B,)), ("trials", I32, (B,))]
    bufs += [(n, d, s, "out", None) for n, d, s in det] + [("t", F64, (B,), "inout", t0)]
    steps = [Call("lcp_move_find_contacts_dts_f64",
                  [B, nb, maxc, nvcap, svm, R("kind"), R("radius"), R("verts_local"), R("nverts"), None, R("p_start"), R("v"), DT, DT / 4, 1, 16,
                   0.1, 1e-6] + [R(n) for n in ("p_out", "c_n", "c_p1", "c_p2", "c_pen", "c_i1", "c_i2", "count", "max_pen", "dt_used", "t",
                                                "trials", "dt_scene")],
                  [n for n, _, _ in det] + ["t"])]

    def post(outs):
        pad = _pad_slots(outs["count"].clamp(min=0), maxc)
        for n in ("c_n", "c_p1", "c_p2", "c_pen", "c_i1", "c_i2"):
            assert _absmax(outs[n][pad]) == 0.0, (n, "padded records are not zero")
        k = B // 2
        assert float(outs["dt_used"][k]) == 0.0 and float(outs["t"][k]) == float(t0[k]) and int(outs["trials"][k]) == 1
        assert torch.equal(outs["p_out"][k], pose[k])
        live = torch.arange(B) != k
        assert bool((outs["dt_used"][live] > 0).all()) and torch.equal(outs["t"][live], t0[live] + outs["dt_used"][live])

    return Case(B, bufs, steps, nulls=[{"c_pen", "max_pen", "dt_used", "t", "trials"}], post=post)


@pytest.mark.parametrize("B", QUAD_B)
def test_dts_detection_narrow_3_bodies(B):
    """Four scenes per wave (B = 1: the scene is the finished one; B = 5: a tail row)."""
    outs = _check(_dts_case(_narrow_scenes(3, B, 7), maxc=16))
    assert B == 1 or int(outs["count"].max()) > 0


def test_dts_detection_narrow_7_bodies():
    outs = _check(_dts_case(_narrow_scenes(7, 3, 9), maxc=32))
    assert int(outs["count"].max()) > 0


def test_dts_detection_wide_33_bodies_capacity_16():
    outs = _check(_dts_case(_wide_scenes(33, 3, 2064, (9, 17)), maxc=128, nvcap=16))
    assert int(outs["count"].min()) > 0


@pytest.mark.parametrize("B", [1, 5, 257])
def test_substep_begin_and_commit(B):
    """Both element-wise kernels: every output element written, nothing else (a block of 256 threads ends inside the guards at these
    sizes), inputs const; `v_new` is in-out and only the finished scenes' rows change."""
    nb = 3
    t = 0.5 + _randn(1, B, dtype=F64).abs()
    end_t = t + DT * (torch.arange(B, dtype=F64) % 3)            # every third scene is finished
    count = (torch.arange(B) % 5).to(I32)
    v_new0 = _randn(4, B, nb, 3)
    bufs = [("t", F64, (B,), "in", t), ("end_t", F64, (B,), "in", end_t), ("f", F32, (B, nb, 3), "in", 100 * _randn(2, B, nb, 3)),
            ("count", I32, (B,), "in", count), ("dt_k", F64, (B,), "out", None), ("active", I32, (B,), "out", None),
            ("count_eff", I32, (B,), "out", None), ("f_eff", F32, (B, nb, 3), "out", None),
            ("v_old", F32, (B, nb, 3), "in", _randn(3, B, nb, 3)), ("v_new", F32, (B, nb, 3), "inout", v_new0)]
    steps = [Call("lcp_substep_begin_f64", [B, nb] + [R(n) for n in ("t", "end_t", "f", "count", "dt_k", "active", "count_eff", "f_eff")],
                  ["dt_k", "active", "count_eff", "f_eff"]),
             Call("lcp_substep_commit_f32", [B, nb, R("active"), R("v_old"), R("v_new")], ["v_new"])]

    def post(outs):
        on = (torch.arange(B) % 3) != 0
        assert outs["active"].tolist() == on.to(I32).tolist()
        assert torch.equal(outs["v_new"][on], v_new0[on]) and (B < 2 or not torch.equal(outs["v_new"], v_new0))

    _check(Case(B, bufs, steps, post=post))


def test_required_pointers_are_checked_before_any_launch():
    """A NULL where the header requires a buffer: LCP_E_BADARG and nothing written."""
    B, nb = 3, 3
    bufs = [("t", F64, (B,), "in", torch.zeros(B, dtype=F64)), ("end_t", F64, (B,), "in", torch.ones(B, dtype=F64)),
            ("f", F32, (B, nb, 3), "in", _randn(2, B, nb, 3)), ("count", I32, (B,), "in", torch.ones(B, dtype=I32)),
            ("dt_k", F64, (B,), "out", None), ("active", I32, (B,), "out", None), ("count_eff", I32, (B,), "out", None),
            ("v_old", F32, (B, nb, 3), "in", _randn(3, B, nb, 3)), ("v_new", F32, (B, nb, 3), "out", None)]
    steps = [Call("lcp_substep_begin_f64", [B, nb] + [R(n) for n in ("t", "end_t", "f", "count", "dt_k", "active", "count_eff", "f_eff")],
                  ["dt_k", "active", "count_eff"], rc=-1),                                     # (f_eff was not carved: NULL)
             Call("lcp_substep_commit_f32", [B, nb, R("active_missing"), R("v_old"), R("v_new")], ["v_new"], rc=-1),
             Call("lcp_substep_commit_f32", [0, nb, R("active"), R("v_old"), R("v_new")], ["v_new"], rc=-1)]
    from tests.test_hip_buffer_contract import _run
    _run(Case(B, bufs, steps))
