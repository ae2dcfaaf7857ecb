"""CPU: the host mirror of the proximity query (tests/proximity_host.py) against answers known by hand, the edge rules of the header
(include/lcp_hip.h, "proximity queries"), central differences of itself, the reference's own penetrations
(tests/golden/contacts_pairs.npz), and the condition the GPU comparison puts on its cases: at most 2 % of a case's pairs are ones the
mirror cannot decide."""
import math

import pytest
import torch

from tests import proximity_host as PH
from tests.render_host import _rect

F64 = torch.float64
INF = float("inf")
ATOL_PEN = 1e-9                                                                           # (tests/test_hip_contacts.py)


def _query(bodies, pairs, cap=8, **kw):
    c = PH._assemble([bodies], cap)
    c.update(PH._pairs([pairs]))
    out = PH.pairs_host(c, **kw)
    return out["dist"][0], out["normal"][0], out["w1"][0], out["w2"][0]


def _close(a, b, tol=1e-13):
    return float((a - torch.tensor(b, dtype=F64)).abs().max()) <= tol


# ------------------------------------------------------------------------------------------------------------- known answers
def test_two_circles_apart_touching_overlapping_and_coincident():
    a, b = ("circle", (0.0, 0.0, 0.0), 2.0), ("circle", (0.7, 10.0, 0.0), 3.0)
    d, n, w1, w2 = _query([a, b, ("circle", (0.0, 4.0, 0.0), 3.0), ("circle", (0.0, 0.0, 0.0), 1.0)],
                          [(0, 1, INF), (1, 0, INF), (0, 2, INF), (0, 3, INF)])
    assert d.tolist() == [5.0, 5.0, -1.0, -3.0]
    assert n.tolist() == [[1.0, 0.0], [-1.0, 0.0], [1.0, 0.0], [0.0, 0.0]]
    assert w1.tolist() == [[2.0, 0.0], [7.0, 0.0], [2.0, 0.0], [0.0, 0.0]] and w2.tolist() == [[7.0, 0.0], [2.0, 0.0], [1.0, 0.0], [0.0, 0.0]]


def test_a_circle_against_a_rect_face_corner_and_inside():
    rect = ("hull", (0.0, 10.0, 0.0), _rect(4.0, 6.0))                                  # x in [8, 12], y in [-3, 3]
    left, diag, inner = ("circle", (0.0, 3.0, 1.0), 2.0), ("circle", (0.0, 15.0, 7.0), 1.0), ("circle", (0.0, 11.5, 0.5), 0.25)
    d, n, w1, w2 = _query([left, diag, inner, rect], [(0, 3, INF), (3, 0, INF), (1, 3, INF), (2, 3, INF), (3, 2, INF)])
    assert _close(d, [3.0, 3.0, 4.0, -0.75, -0.75])                                      # 5 - 2; |(3, 4)| - 1; -0.5 - 0.25
    assert _close(n, [[1.0, 0.0], [-1.0, 0.0], [-0.6, -0.8], [-1.0, 0.0], [1.0, 0.0]])
    assert _close(w1, [[5.0, 1.0], [8.0, 1.0], [14.4, 6.2], [11.25, 0.5], [12.0, 0.5]])
    assert _close(w2, [[8.0, 1.0], [5.0, 1.0], [12.0, 3.0], [12.0, 0.5], [11.25, 0.5]])
    for k in range(5):
        assert abs(float((n[k] * (w2[k] - w1[k])).sum() - d[k])) < 1e-13


def test_two_rects_apart_vertex_to_face_and_overlapping():
    """A square turned by 45 degrees, its corner (10 - sqrt 2, 0) pointing at the right face x = 2 of an axis-aligned box; then the
    same square pushed 0.5 into the face."""
    r2 = math.sqrt(2.0)
    box = ("hull", (0.0, 0.0, 0.0), _rect(4.0, 6.0))
    far, deep = ("hull", (math.pi / 4, 10.0, 0.5), _rect(2.0, 2.0)), ("hull", (math.pi / 4, 1.5 + r2, 0.5), _rect(2.0, 2.0))
    d, n, w1, w2 = _query([box, far, deep], [(0, 1, INF), (1, 0, INF), (0, 2, INF), (2, 0, INF)])
    assert _close(d, [8.0 - r2, 8.0 - r2, -0.5, -0.5], 1e-12)
    assert _close(n, [[1.0, 0.0], [-1.0, 0.0], [1.0, 0.0], [-1.0, 0.0]], 1e-12)
    assert _close(w1, [[2.0, 0.5], [10.0 - r2, 0.5], [2.0, 0.5], [1.5, 0.5]], 1e-12)
    assert _close(w2, [[10.0 - r2, 0.5], [2.0, 0.5], [1.5, 0.5], [2.0, 0.5]], 1e-12)


def test_two_rects_corner_to_corner():
    a, b = ("hull", (0.0, 0.0, 0.0), _rect(2.0, 2.0)), ("hull", (0.0, 5.0, 6.0), _rect(2.0, 2.0))
    d, n, w1, w2 = _query([a, b], [(0, 1, INF)])
    assert _close(d, [5.0]) and _close(n, [[0.6, 0.8]]) and _close(w1, [[1.0, 1.0]]) and _close(w2, [[4.0, 5.0]])


# ------------------------------------------------------------------------------------------------------------- edge rules
def test_invalid_pairs_and_the_clamp_return_max_dist_and_zeros():
    a, b = ("circle", (0.0, 0.0, 0.0), 2.0), ("circle", (0.0, 10.0, 0.0), 3.0)
    stick = ("hull", (0.0, 5.0, 0.0), [[0.0, -3.0], [0.0, 3.0]])
    pairs = [(0, 0, 7.0), (-1, 1, 7.0), (0, 3, INF), (0, 2, 9.0), (2, 1, 4.0), (0, 1, 5.0), (0, 1, 4.5), (0, 1, 5.5)]
    d, n, w1, w2 = _query([a, b, stick], pairs)
    assert d.tolist() == [7.0, 7.0, INF, 9.0, 4.0, 5.0, 4.5, 5.0]                        # (dist >= max_dist clamps: 5 at 5 does)
    assert float(n[:7].abs().max()) == 0.0 and float(w1[:7].abs().max()) == 0.0 and float(w2[:7].abs().max()) == 0.0
    assert n[7].tolist() == [1.0, 0.0]


def test_a_scene_over_the_vertex_limit_is_not_queried():
    bodies = [("hull", (0.0, 10.0, 0.0), _rect(4.0, 6.0)), ("circle", (0.0, 0.0, 0.0), 1.0)]
    assert _close(_query(bodies, [(0, 1, 50.0)], scene_verts_max=4)[0], [7.0])
    assert _query(bodies, [(0, 1, 50.0)], scene_verts_max=3)[0].tolist() == [50.0]


def test_swapping_the_pair_flips_the_normal_and_swaps_the_witnesses():
    c = PH.case("small")
    ref = PH.reference("small")
    f, s = c["pair_first"], c["pair_second"]
    seen = 0
    for b in range(f.shape[0]):
        for r in range(0, 40, 4):                                                         # (a, c, inf) and (c, a, inf) follow each other
            assert (int(f[b, r]), int(s[b, r])) == (int(s[b, r + 1]), int(f[b, r + 1]))
            assert abs(float(ref["dist"][b, r] - ref["dist"][b, r + 1])) < 1e-12
            assert float((ref["normal"][b, r] + ref["normal"][b, r + 1]).abs().max()) < 1e-12
            assert float((ref["w1"][b, r] - ref["w2"][b, r + 1]).abs().max()) < 1e-9
            seen += 1
    assert seen == 30


# ------------------------------------------------------------------------------------------------------------- the reference
def test_dist_is_the_references_penetration_on_the_pair_fixture():
    """600 DiffContactHandler pairs: dist = -max_k pen on the 543 with a record (172 circle-circle, 262 circle-hull, 109 hull-hull),
    dist > eps = 0.1 on the 57 without."""
    c, has, pen = PH.fixture_case()
    out = PH.pairs_host(c)
    d = out["dist"][:, 0]
    kinds = (c["kind"][has] != 0).sum(1)
    assert int(has.sum()) == 543 and [int((kinds == k).sum()) for k in range(3)] == [172, 262, 109]
    err = float((d + pen)[has].abs().max())
    print("|dist + max pen| %.3g   smallest dist without a record %.4g" % (err, float(d[~has].min())))
    assert err <= ATOL_PEN
    assert float(d[~has].min()) > 0.1


# ------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", PH.CASE_NAMES)
def test_at_most_two_percent_of_a_case_are_pairs_the_mirror_cannot_decide(name):
    ref, c = PH.reference(name), PH.case(name)
    ex = ref["excluded"]
    assert bool(torch.isfinite(ref["dist"][ref["live"]]).all())
    assert torch.equal(ref["dist"][~ref["live"]], c["pair_max_dist"][~ref["live"]])
    for k, g in ref["grads"].items():
        assert bool(torch.isfinite(g).all()), k
    if name in PH.GENERIC:
        assert int(ex.sum()) <= 0.02 * ex.numel(), (int(ex.sum()), ex.numel())
    err = ((ref["normal"] * (ref["w2"] - ref["w1"])).sum(-1) - ref["dist"])[ref["live"]].abs().max()
    assert float(err) < 1e-10                                                             # dist = n . (w2 - w1), in every case
    if name == "stack":
        assert int(ex.sum()) >= 6                                                         # parallel faces: the deliberate exception


def test_small_holds_every_kind_of_pair_in_every_state():
    c, ref = PH.case("small"), PH.reference("small")
    assert c["pair_first"].shape == (3, 70) and c["kind"].shape[1] == 6
    kinds = c["kind"].long()
    f, s, md = c["pair_first"].long(), c["pair_second"].long(), c["pair_max_dist"]
    real = (f >= 0) & (f < 5) & (s >= 0) & (s < 5) & (f != s)
    hulls = torch.gather(kinds, 1, f.clamp(0, 5)) + torch.gather(kinds, 1, s.clamp(0, 5))
    for nh in range(3):                                                                   # circle-circle, circle-hull, hull-hull
        sel = real & (hulls == nh)
        assert int((sel & ref["live"] & (ref["dist"] > 0)).sum()) > 0, nh
        assert int((sel & ~ref["live"] & torch.isfinite(md)).sum()) > 0, nh               # beyond a finite max_dist
        if nh > 0:
            assert int((sel & ref["live"] & (ref["dist"] < 0)).sum()) > 0, nh
    assert int((~real).sum()) == 3 * 17 and not bool(ref["live"][~real].any())            # self, -1, nb and beyond, the two-vertex hull
    inside = (f == 1) & (s == 4) & torch.isinf(md)                                        # circle 1's centre lies inside the pentagon
    r1 = c["radius"][:, 1].unsqueeze(1).expand_as(md)
    assert int(inside.sum()) > 0 and bool((ref["dist"][inside] < -r1[inside]).all())


def test_wide_and_big_hulls_are_at_the_limits():
    c, ref = PH.case("wide"), PH.reference("wide")
    assert int(c["nverts"].sum(1).max()) == 1024 and c["pair_first"].shape == (2, 1024)
    assert int((ref["dist"] < 0).sum()) > 20 and int((~ref["live"]).sum()) > 100 and int(ref["live"].sum()) > 1000
    c, ref = PH.case("big_hulls"), PH.reference("big_hulls")
    assert c["verts_local"].shape[2] == 64 and c["nverts"].tolist() == [[64, 64, 64]]
    assert int((ref["dist"] < 0).sum()) == 2 and int((ref["dist"] > 0).sum()) == 4


def test_stack_ties_leave_dist_normal_force_and_torque_alone():
    """Resting and side-by-side boxes: dist and normal by hand; whichever tied feature is taken, each body's force is -+g n and the pair's
    total torque about the origin vanishes (dist = n . (w2 - w1), so the two arms differ by a multiple of n)."""
    c, ref = PH.case("stack"), PH.reference("stack")
    want = {(0, 1): (0.0, (0.0, -1.0)), (1, 2): (-0.02, (0.0, -1.0)), (1, 3): (2.0, (1.0, 0.0))}
    for b, pr in enumerate(PH.STACK_PAIRS):
        key, sg = (pr, 1.0) if pr in want else ((pr[1], pr[0]), -1.0)
        if key in want:
            assert abs(float(ref["dist"][b, 0]) - want[key][0]) < 1e-12, pr
            assert _close(ref["normal"][b, 0], [sg * v for v in want[key][1]], 1e-12), pr
        g, gp = ref["g_dist"][b, 0], ref["grads"]["p"][b]
        assert float((gp[pr[1], 1:] - g * ref["normal"][b, 0]).abs().max()) < 1e-12
        assert float((gp[pr[0], 1:] + g * ref["normal"][b, 0]).abs().max()) < 1e-12
        torque = gp[:, 0] + c["p"][b, :, 1] * gp[:, 2] - c["p"][b, :, 2] * gp[:, 1]
        assert abs(float(torque.sum())) < 1e-9 * float((c["p"][b, :, 1:].abs().max() * g.abs())), pr


# ------------------------------------------------------------------------------------------------------------- gradient
@pytest.mark.parametrize("name", ["small", "tiny", "big_hulls"])
@pytest.mark.parametrize("leaf", PH.LEAVES)
def test_autograd_of_the_mirror_equals_its_central_differences(name, leaf):
    """Directional: sum_r g_r (dist_r(x + h d) - dist_r(x - h d)) / 2h against <autograd's gradient, d> for random directions d of
    one input array at a time and the reference's cotangent g, zeroed on the pairs within 1e-3 of a change of branch (finite
    differences do not cross one).  h = 1e-6, 1e-6 relative to sum_r |g_r| |d dist_r|: a second-order scheme on a smooth function of
    order-100 coordinates."""
    ref, c = PH.reference(name), PH.case(name)
    g = torch.where((ref["gap"] < 1e-3) | ~ref["live"], torch.zeros_like(ref["g_dist"]), ref["g_dist"])
    cl = PH.leaves(c)
    grad = torch.autograd.grad(PH.pairs_host(cl)["dist"], cl[leaf], g, allow_unused=True)[0]
    if leaf == "radius" and not bool((c["kind"] == 0).any()):                             # no circle in the case: no radius is read
        assert grad is None
        return
    assert grad is not None and float(grad.abs().max()) > 0
    h = 1e-6
    for seed in range(3):
        d = torch.randn(c[leaf].shape, generator=torch.Generator().manual_seed(seed), dtype=F64)
        with torch.no_grad():
            hi = PH.pairs_host(dict(c, **{leaf: c[leaf] + h * d}))
            lo = PH.pairs_host(dict(c, **{leaf: c[leaf] - h * d}))
        fd = torch.where(g != 0, (hi["dist"] - lo["dist"]) / (2 * h), torch.zeros_like(g))
        scale = float((g.abs() * fd.abs()).sum())
        assert abs(float((g * fd).sum()) - float((grad * d).sum())) <= 1e-6 * scale, (leaf, seed)
