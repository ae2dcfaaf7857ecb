"""CPU: the float64 mirror of the contact report (tests/contact_report_host.py) against the oracle's assembled G and A, against its own
pair part, and the identity M (v_new - v) - dt f = G^T z + Je^T y on the oracle's own fp64 solves."""
import numpy as np
import pytest
import torch

from oracle import pdipm_oracle as O
from tests import contact_report_host as RH

F64 = torch.float64


def _oracle_sums(c):
    """G^T z and A^T y per body coordinate, and the sums of the magnitudes of their terms, with G = [Jc; Jf; 0] as the oracle assembles
    it (pdipm_oracle.contact_jacobians: world.py:172-211).  Rows the report does not read (beyond the count, inactive scenes) enter
    with z = 0; a record index outside [0, nb) is given a phantom body of its own (bodies -1 and nb of nb + 2), dropped afterwards."""
    B, nb, maxc, e, _ = RH.dims(c)
    live = RH.record_impulses(c)[4]
    z = c["z"].to(F64).clone()
    lv = live.to(F64)
    z[:, :maxc] *= lv
    z[:, maxc:3 * maxc] *= lv.repeat_interleave(2, dim=1)
    Jc, Jf = O.contact_jacobians(c["c_n"].to(F64), c["c_p1"].to(F64), c["c_p2"].to(F64), c["c_i1"].long() + 1, c["c_i2"].long() + 1, nb + 2)
    G = torch.cat([Jc, Jf], 1)                                                # (the gamma rows of G are zero: engines.py:67-68)
    terms = G * z[:, :3 * maxc].unsqueeze(-1)
    keep = lambda t: t.reshape(B, nb + 2, 3)[:, 1:nb + 1]
    got = {"contact": keep(terms.sum(1)), "S_contact": keep(terms.abs().sum(1))}
    if e:
        jt = c["Je"].to(F64) * c["y"].to(F64).unsqueeze(-1)
        if c["active"] is not None:
            jt = jt * (c["active"] != 0).to(F64).reshape(B, 1, 1)
        got["joint"], got["S_joint"] = jt.sum(1).reshape(B, nb, 3), jt.abs().sum(1).reshape(B, nb, 3)
    return got


@pytest.mark.parametrize("name", RH.CASE_NAMES)
def test_mirror_body_sums_are_the_oracles_GTz_and_ATy(name):
    c, ref = RH.case(name), RH.reference(name)
    want = _oracle_sums(c)
    err = (ref["body_impulse"] - want["contact"]).abs()
    assert float(want["S_contact"].max()) > 0.0
    assert bool((err <= 1e-12 * want["S_contact"]).all()), float((err / want["S_contact"].clamp(min=1e-300)).max())
    # and the mirror's S is the sum of |G[r, k] z[r]| over the rows of G: the two friction multipliers of a record count separately
    assert bool(((ref["S_body_impulse"] - want["S_contact"]).abs() <= 1e-12 * want["S_contact"]).all())
    if "joint" in want:
        err = (ref["joint_impulse"] - want["joint"]).abs()
        assert bool((err <= 1e-12 * want["S_joint"]).all())
    else:
        assert float(ref["joint_impulse"].abs().max()) == 0.0


def test_the_named_cases_cover_what_they_are_named_for():
    rag, inv = RH.case("ragged"), RH.case("invalid")
    assert int(rag["count"].max()) > 12 and int(rag["count"].min()) == 0 and int((rag["active"] == 0).sum()) >= 2
    ref = RH.reference("ragged")
    for n in RH.OUTPUTS:
        assert float(ref[n][rag["active"] == 0].abs().max()) == 0.0, n                     # an inactive scene: all zeros
    assert float(ref["body_impulse"][0].abs().max()) == 0.0                                # count 0: no record
    ref = RH.reference("invalid")
    assert float(ref["pair_impulse"][:, :5].abs().max()) == 0.0 and int(ref["pair_contacts"][:, :5].abs().max()) == 0
    assert float(ref["pair_normal"][:, 5:].min()) > 0.0
    assert torch.equal(ref["pair_impulse"][:, 5, 1:], -ref["pair_impulse"][:, 6, 1:])      # (0, 1) against (1, 0): opposite forces
    assert RH.dims(RH.case("nojoints"))[3] == 0 and RH.dims(RH.case("nopairs"))[4] == 0
    assert RH.dims(RH.case("full")) == (2, 64, 1024, 24, 1024)
    for name in RH.CASE_NAMES:                                                             # the threshold test has something to count
        thr = RH.some_zn(name)
        hi = RH.report_host(RH.case(name), thr)
        assert 0 < int(hi["body_touching"].sum()) < int(RH.reference(name)["body_touching"].sum()), name


@pytest.mark.parametrize("name", ["small", "edge65", "ragged", "nojoints"])
def test_with_all_pairs_a_bodys_force_is_its_pairs_as_first_minus_as_second(name):
    from lcp_physics_amd.physics.proximity import PairSet
    c = dict(RH.case(name))
    B, nb = RH.dims(c)[:2]
    pairs = PairSet.all_pairs(nb, B)
    c["first"], c["second"] = pairs.first, pairs.second
    ref = RH.report_host(c)
    total, S = torch.zeros(B, nb, 2, dtype=F64), torch.zeros(B, nb, 2, dtype=F64)
    for q in range(pairs.P):
        f, s = int(pairs.first[0, q]), int(pairs.second[0, q])
        total[:, f] += ref["pair_impulse"][:, q, 1:]
        total[:, s] -= ref["pair_impulse"][:, q, 1:]
        S[:, f] += ref["S_pair_impulse"][:, q, 1:]
        S[:, s] += ref["S_pair_impulse"][:, q, 1:]
    assert float(S.max()) > 0.0
    assert bool(((total - ref["body_impulse"][..., 1:]).abs() <= 1e-12 * S).all())
    assert torch.equal(S > 0, ref["S_body_impulse"][..., 1:] > 0)


# ------------------------------------------------------------------------------------------------------------- the identity
def _identity_ratio(Mdiag, v, f, dt, v_new, c):
    """max over coordinates of |M (v_new - v) - dt f - body_impulse - joint_impulse| / S, S the sum of the magnitudes of every term."""
    ref = RH.report_host(c)
    M, v, f, v_new = (t.to(F64) for t in (Mdiag, v, f, v_new))
    res = M * v_new - M * v - dt * f - ref["body_impulse"] - ref["joint_impulse"]
    S = (M * v_new).abs() + (M * v).abs() + (dt * f).abs() + ref["S_body_impulse"] + ref["S_joint_impulse"]
    assert float(S.min()) >= 0.0
    return float((res.abs() / S.clamp(min=1e-300)).max())


def _solved_case(sc):
    """The oracle's fp64 solve of a scene batch (every record used) as a case of the mirror."""
    args = [t.to(F64) if isinstance(t, torch.Tensor) and t.is_floating_point() else t for t in sc.assembly_args()]
    v_new, sol, _ = O.solve_dynamics(*args)
    e = sc.Je.shape[1]
    assert float(sol.resid.max()) < 1e-9, ("the oracle did not converge on this scene", sol.resid.tolist())
    c = {"nb": sc.nb, "c_n": sc.c_n, "c_p1": sc.c_p1, "c_p2": sc.c_p2, "c_i1": sc.c_i1, "c_i2": sc.c_i2, "z": sol.z, "count": None,
         "active": None, "y": sol.y if e else None, "Je": sc.Je if e else None, "first": None, "second": None}
    return v_new, c


def test_the_identity_holds_on_the_oracles_fp64_solves():
    """|M (v_new - v) - dt f - G^T z - Je^T y| < 2^-24 S per coordinate on the oracle's own float64 solves - the largest ratios measured
    here: a pinned four-box stack 3.1e-16, a jointed chain in contact 1.9e-16, joints without contact below 1e-16.  The GPU test of the
    identity on worlds (tests/test_hip_contact_report.py) counts the fp64 solve's own residual as below one float32 rounding of S; this
    is where that is checked."""
    from lcp_physics_amd import scenes
    from tests.test_hip_primal import _with_joint_rows
    bound = 2.0 ** -24
    stack = scenes.make_stack_scenes(B=3, nbox=4, pts_per_interface=4, seed=11, dtype=F64)
    v_new, c = _solved_case(stack)
    r_stack = _identity_ratio(stack.Mdiag, stack.v, stack.f, stack.dt, v_new, c)
    # (the identity is a statement about a SOLUTION: with more welded rows than this the oracle's PDIPM stalls on these stacks - final
    # residual of order 10 - and the multipliers it returns satisfy nothing; e = 4 couples the top box's rotation to the floor's)
    chain = _with_joint_rows(scenes.make_stack_scenes(B=3, nbox=4, pts_per_interface=2, seed=12, dtype=F64), 4)
    v_new, c = _solved_case(chain)
    assert float(c["y"].abs().max()) > 0.0 and float(c["z"].abs().max()) > 0.0
    r_chain = _identity_ratio(chain.Mdiag, chain.v, chain.f, chain.dt, v_new, c)
    # joints, no contact: engines.py:36-49 as oracle/world_oracle.py:55-63 solves it, [[M, -Je^T], [Je, 0]] (x; y) = (u; 0) per scene
    free = _with_joint_rows(scenes.make_stack_scenes(B=3, nbox=4, pts_per_interface=2, seed=13, dtype=F64), 9)
    nz, e = 3 * free.nb, free.Je.shape[1]
    xs, ys = [], []
    for b in range(free.B):
        Md, Jm = free.Mdiag[b].reshape(-1).numpy(), free.Je[b].numpy()
        u = Md * free.v[b].reshape(-1).numpy() + free.dt * free.f[b].reshape(-1).numpy()
        P = np.block([[np.diag(Md), -Jm.T], [Jm, np.zeros((e, e))]])
        sol = np.linalg.solve(P, np.concatenate([u, np.zeros(e)]))
        xs.append(sol[:nz])
        ys.append(sol[nz:])
    v_new = torch.tensor(np.stack(xs)).reshape(free.B, free.nb, 3)
    c = {"nb": free.nb, "c_n": free.c_n, "c_p1": free.c_p1, "c_p2": free.c_p2, "c_i1": free.c_i1, "c_i2": free.c_i2,
         "z": torch.zeros(free.B, 4 * free.nc, dtype=F64), "count": torch.zeros(free.B, dtype=torch.int32), "active": None,
         "y": torch.tensor(np.stack(ys)), "Je": free.Je, "first": None, "second": None}
    assert float(c["y"].abs().max()) > 0.0
    r_free = _identity_ratio(free.Mdiag, free.v, free.f, free.dt, v_new, c)
    print("identity residual / S: stack %.3g   chain %.3g   joints, no contact %.3g   (bound %.3g)" % (r_stack, r_chain, r_free, bound))
    assert r_stack < bound and r_chain < bound and r_free < bound
