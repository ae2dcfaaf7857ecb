"""CPU: the mirror of the time-of-impact query (tests/toi_host.py) against closed forms, against brute force (the distance on a grid
of 4000 times plus bisection) and against central differences of its own advancement."""
import math

import pytest
import torch

from tests import toi_host as TH

F64 = torch.float64


def _one(bodies, vel, pairs, horizon, **kw):
    return TH._finish(TH._assemble([bodies], 8), [vel], [pairs], horizon, **kw)


def test_circle_circle_head_on_is_the_closed_form():
    """(|q| - r1 - r2 - margin) / closing speed: the advancement is exact after one step."""
    c = _one([("circle", (0.0, 1.0, 2.0), 3.0), ("circle", (0.0, 31.0, 42.0), 4.0)], [(0.3, 3.0, 4.0), (-2.0, -1.5, -2.0)],
             [(0, 1, 0.0), (1, 0, 0.25)], 10.0)
    for r, mg in ((0, 0.0), (1, 0.25)):
        a = TH.advance(c, 0, r)
        want = (50.0 - 7.0 - mg) / 7.5
        print("head-on circles: toi %.15g, closed form %.15g, %d evaluations" % (a["toi"], want, a["iters"]))
        assert a["status"] == TH.HIT and abs(a["toi"] - want) <= 1e-6 / 7.5 + 1e-12 and a["iters"] == 2
    n = TH.advance(c, 0, 0)["normal"]
    assert float((n - torch.tensor([0.6, 0.8], dtype=F64)).abs().max()) <= 1e-12


def test_circle_against_a_rect_face_is_the_closed_form():
    """A ball against the face of a wall that does not turn: (gap - margin) / speed.  The bullet of the issue: in one dt it would land
    beyond the wall."""
    c, ref = TH.case("bullet"), TH.reference("bullet")
    for r, mg in ((0, 0.0), (1, 0.0), (2, 0.05)):
        want = (44.0 - mg) / 1800.0
        print("bullet pair %d: toi %.15g, closed form %.15g, %d evaluations" % (r, float(ref["toi"][0, r]), want, int(ref["iters"][0, r])))
        assert int(ref["status"][0, r]) == TH.HIT and abs(float(ref["toi"][0, r]) - want) <= 1e-6 / 1800.0 + 1e-12
        assert int(ref["iters"][0, r]) == 2
    assert float(c["p"][0, 0, 1] + c["v"][0, 0, 1].double() * c["horizon"][0]) > 56.0    # ... where the end pose overlaps nothing
    assert torch.equal(ref["normal"][0, 0], torch.tensor([1.0, 0.0], dtype=F64)) and float(ref["normal"][0, 1, 0]) == -1.0


def test_the_six_cases_end_as_they_were_built_to():
    want = {"bullet": TH.HIT, "rod": TH.HIT, "boxes": TH.HIT, "glance": TH.HIT, "separating": TH.MISS, "spin": TH.UNCONVERGED}
    for name in TH.SIX:
        ref = TH.reference(name)
        print(name, "status", ref["status"].tolist(), "toi", ref["toi"].tolist(), "evaluations", ref["iters"].tolist(), "first touch",
              ref["root"].tolist())
        assert bool((ref["status"] == want[name]).all()), name
    assert bool((TH.reference("separating")["toi"] == TH.case("separating")["horizon"][0]).all())
    spin = TH.reference("spin")
    assert float(spin["toi"][0, 0]) < float(spin["root"][0, 0]) < TH.INF                  # a true lower bound of a touch that exists


@pytest.mark.parametrize("name", TH.SIX + ("mixed",))
def test_hits_agree_with_brute_force_and_no_iterate_passes_the_first_touch(name):
    c, ref = TH.case(name), TH.reference(name)
    B, P = c["pair_first"].shape
    assert int(ref["excluded"].sum()) <= 0.02 * B * P
    worst = 0.0
    for b in range(B):
        hz = float(c["horizon"][b])
        for r in range(P):
            root = float(ref["root"][b, r])
            for t in ref["times"][(b, r)]:                                               # every t_k, whatever the status
                assert t <= root + 1e-9 * hz, (name, b, r, t, root)
            if bool(ref["excluded"][b, r]):
                continue
            st = int(ref["status"][b, r])
            if st == TH.HIT:
                bound = 2 * c["tol"] / abs(float(ref["ddot"][b, r])) + 1e-9 * hz
                err = abs(float(ref["toi"][b, r]) - root)
                worst = max(worst, err / bound)
                assert err <= bound, (name, b, r, err, bound)
            elif st == TH.MISS and ref["times"][(b, r)]:
                assert root == TH.INF or root >= hz * (1 - 1e-9), (name, b, r, root)      # no touch before the horizon
    print("%s: %d pairs, status counts %s, |toi - brute| at most %.3g of its bound, excluded %d" % (
        name, B * P, torch.bincount(ref["status"].flatten().long(), minlength=4).tolist(), worst, int(ref["excluded"].sum())))


def test_mixed_has_hits_and_misses_of_every_kind_of_pair():
    ref = TH.reference("mixed")
    assert int((ref["status"] == TH.HIT).sum()) >= 6 and int((ref["status"] == TH.MISS).sum()) >= 3


@pytest.mark.parametrize("name", TH.EDGES + ("notqueried",))
def test_the_edge_cases_exclude_at_most_two_percent(name):
    c, ref = TH.case(name), TH.reference(name)
    assert int(ref["excluded"].sum()) <= 0.02 * ref["excluded"].numel()
    if name == "notqueried":
        assert bool((ref["status"][:2] == TH.MISS).all()) and bool((ref["toi"][0] == 2.0).all()) and bool((ref["toi"][1] == 0.0).all())
        assert int((ref["status"][2] == TH.HIT).sum()) > 0
    else:
        first = c["pair_first"][0]
        bad = (first == c["pair_second"][0]) | (first < 0) | (first >= 5) | (c["pair_second"][0] >= 5)
        assert bool((ref["status"][:, bad] == TH.MISS).all()) and bool((ref["toi"][:, bad] == 2.0).all())


@pytest.mark.parametrize("name", ["rod", "boxes", "glance", "mixed"])
def test_the_implicit_gradient_against_central_differences_of_the_advancement(name):
    """The advancement at tol = 1e-12 is a function of the inputs; its central differences (step 1e-6 on coordinates of order 10 to
    100) resolve 6 to 7 digits.  The implicit gradient agrees to 1e-5 of the largest entry."""
    c, ref = TH.case(name), TH.reference(name)
    B, P = c["pair_first"].shape
    pick = [(b, r) for b in range(B) for r in range(P) if int(ref["status"][b, r]) == TH.HIT and not bool(ref["excluded"][b, r])][:3]
    assert pick
    worst = 0.0
    for b, r in pick:
        fine = TH.advance(c, b, r, tol=1e-12, max_iter=1024)
        assert fine["status"] == TH.HIT
        ddot, (gp, gv, gr, gvl), _ = TH.pair_gradient(c, b, r, fine["toi"])
        assert ddot < 0.0
        k = [int(c["pair_first"][b, r]), int(c["pair_second"][b, r])]
        big = max(float(g.abs().max()) for g in (gp, gv, gr, gvl))
        h = 1e-6

        def fd(key, idx):
            vals = []
            for s in (+1, -1):
                d = dict(c)
                d[key] = c[key].clone().double()
                d[key][idx] += s * h
                vals.append(TH.advance(d, b, r, tol=1e-12, max_iter=1024)["toi"])
            return (vals[0] - vals[1]) / (2 * h)

        errs = []
        for s in range(2):
            for q in range(3):
                errs.append(abs(fd("p", (b, k[s], q)) - float(gp[s, q])))
                errs.append(abs(fd("v", (b, k[s], q)) - float(gv[s, q])))
            if int(c["kind"][b, k[s]]) == 0:
                errs.append(abs(fd("radius", (b, k[s])) - float(gr[s])))
            else:
                for j in range(min(int(c["nverts"][b, k[s]]), 4)):
                    for q in range(2):
                        errs.append(abs(fd("verts_local", (b, k[s], j, q)) - float(gvl[s, j, q])))
        mg = abs(fd("margin", (b, r)) - 1.0 / ddot)
        worst = max(worst, max(errs + [mg]) / big)
        print("%s scene %d pair %d: |implicit - central difference| %.3g of %.3g" % (name, b, r, max(errs + [mg]), big))
        assert max(errs + [mg]) <= 1e-5 * big
    print("%s: worst relative difference %.3g" % (name, worst))
