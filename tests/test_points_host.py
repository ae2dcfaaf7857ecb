"""CPU: the host mirror of the point probe (tests/points_host.py) against answers known by hand, the edge rules of the header
(include/lcp_hip.h, "point probes"), central differences of itself, the mirror of the proximity query (a circle of radius rho at the
point), and the condition the GPU comparison puts on its cases: at most 2 % of a case's points are ones the mirror cannot decide.
Then the host side of `physics.points.PointSet`, which needs no GPU."""
import math

import pytest
import torch

from tests import points_host as PH
from tests import proximity_host as XH
from tests.render_host import _rect, pixel_centres

F64 = torch.float64
INF = float("inf")


def _probe(bodies, points, cap=8, **kw):
    c = PH._assemble([bodies], cap)
    c.update(PH._points([points]))
    out = PH.points_host(c, **kw)
    return out["dist"][0], out["body"][0], out["normal"][0]


def _close(a, b, tol=1e-13):
    return float((a - torch.tensor(b, dtype=F64)).abs().max()) <= tol


# ------------------------------------------------------------------------------------------------------------- known answers
def test_a_point_against_a_circle_outside_inside_and_at_its_centre():
    d, k, n = _probe([("circle", (0.7, 10.0, 0.0), 3.0)], [(-1, (2.0, 0.0), -1, INF), (-1, (10.0, 2.0), -1, INF), (-1, (10.0, 0.0), -1, INF)])
    assert d.tolist() == [5.0, -1.0, -3.0] and k.tolist() == [0, 0, 0]
    assert n.tolist() == [[-1.0, 0.0], [0.0, 1.0], [0.0, 0.0]]                            # (u is exactly 0 at the centre)


def test_a_point_against_a_rect_face_corner_inside_and_on_the_face():
    rect = ("hull", (0.0, 10.0, 0.0), _rect(4.0, 6.0))                                  # x in [8, 12], y in [-3, 3]
    d, k, n = _probe([rect], [(-1, (3.0, 1.0), -1, INF), (-1, (15.0, 7.0), -1, INF), (-1, (11.5, 0.5), -1, INF), (-1, (12.0, 1.0), -1, INF)])
    assert _close(d, [5.0, 5.0, -0.5, 0.0]) and k.tolist() == [0, 0, 0, 0]              # the face; |(3, 4)|; the right face; on it
    assert _close(n, [[-1.0, 0.0], [0.6, 0.8], [1.0, 0.0], [1.0, 0.0]])


def test_a_mounted_point_moves_with_its_body_and_never_tests_it():
    bodies = [("circle", (math.pi / 2, 0.0, 0.0), 5.0), ("circle", (0.0, 0.0, 20.0), 2.0)]
    # mounted on body 0 (turned by 90 degrees): (1, 0) -> world (0, 1): body 1 at 20 - 2 - 1; in the world frame body 0 is nearer
    d, k, n = _probe(bodies, [(0, (1.0, 0.0), -1, INF), (-1, (0.0, 1.0), -1, INF), (0, (1.0, 0.0), 0, INF), (2, (0.0, 1.0), -1, INF),
                              (-2, (0.0, 1.0), -1, 9.0), (-1, (0.0, 1.0), 1, INF), (-1, (0.0, 1.0), 2, 7.0), (-1, (0.0, 1.0), -2, 7.0)])
    assert _close(d[:2], [17.0, -4.0]) and k.tolist() == [1, 0, -1, -1, -1, 1, -1, -1]
    assert d[2:].tolist() == [INF, INF, 9.0, 17.0, 7.0, 7.0]                              # void: max_dist itself
    assert _close(n[0], [0.0, -1.0]) and float(n[[2, 3, 4, 6, 7]].abs().max()) == 0.0


def test_the_cutoff_voids_at_equality_and_the_smaller_index_wins_a_tie():
    twin = ("circle", (0.0, 10.0, 0.0), 2.0)
    stick = ("hull", (0.0, 5.0, 0.0), [[0.0, -3.0], [0.0, 3.0]])                         # two vertices: never a candidate
    d, k, n = _probe([stick, twin, twin], [(-1, (0.0, 0.0), -1, INF), (-1, (0.0, 0.0), -1, 8.0), (-1, (0.0, 0.0), -1, 8.5),
                                           (-1, (0.0, 0.0), 0, 50.0)])
    assert d.tolist() == [8.0, 8.0, 8.0, 50.0] and k.tolist() == [1, -1, 1, -1]


def test_a_scene_over_the_vertex_limit_is_not_probed():
    c = PH._assemble([[("hull", (0.0, 10.0, 0.0), _rect(4.0, 6.0))]], 8)
    c.update(PH._points([[(-1, (0.0, 0.0), -1, 100.0)]]))
    assert PH.points_host(c, scene_verts_max=4)["body"].tolist() == [[0]]
    out = PH.points_host(c, scene_verts_max=3)
    assert out["body"].tolist() == [[-1]] and out["dist"].tolist() == [[100.0]]


# ------------------------------------------------------------------------------------------------------------- the cases
def test_the_named_points_of_small_are_what_they_are_called():
    c, ref = PH.case("small"), PH.reference("small")
    nm, d, k, n, ex = c["names"], ref["dist"], ref["body"], ref["normal"], ref["excluded"]
    assert c["pt_body"].shape == (3, 70) and c["kind"].shape == (3, 6)
    assert k[:, nm["centre"]].tolist() == [0] * 3 and torch.equal(d[:, nm["centre"]], -c["radius"][:, 0])
    assert float(n[:, nm["centre"]].abs().max()) == 0.0 and not bool(ex[:, nm["centre"]].any())
    assert d[:, nm["on_face"]].tolist() == [0.0, 0.5, 0.5] and ex[:, nm["on_face"]].tolist() == [True, False, False]
    assert d[:, nm["inside_rect"]].tolist() == [-9.0] * 3 and k[:, nm["inside_rect"]].tolist() == [2] * 3
    assert torch.equal(n[:, nm["inside_rect"]], torch.tensor([[0.0, 1.0]] * 3, dtype=F64))
    assert k[:, nm["inside_vertex"]].tolist() == [4] * 3 and float(d[:, nm["inside_vertex"]].max()) < 0.0
    assert k[:, nm["vertex_outer"]].tolist() == [4] * 3
    assert float((d[:, nm["vertex_outer"]] - math.hypot(4.0, 0.2)).abs().max()) < 1e-12     # the distance from the vertex itself
    assert d[:, nm["beyond"]].tolist() == [5.0] * 3 and k[:, nm["beyond"]].tolist() == [-1] * 3
    assert d[:, nm["at_cutoff"]].tolist() == [8.0] * 3 and k[:, nm["at_cutoff"]].tolist() == [-1, 2, 2]      # d == max_dist: void
    assert ex[:, nm["at_cutoff"]].tolist() == [True, False, False]
    assert c["pt_body"][:, nm["mounted"]].tolist() == [3] * 3 and bool(ref["live"][:, nm["mounted"]].all())
    assert k[:, nm["far_target"]].tolist() == [4] * 3 and float(d[:, nm["far_target"]].min()) > 50.0          # circle 0 is 8 away
    for name in ("own_mount", "bad_mount", "stick_alone"):
        assert k[:, nm[name]].tolist() == [-1] * 3 and d[:, nm[name]].tolist() == [INF] * 3, name
    assert int((k[:, nm["stick"]] == 5).sum()) == 0 and bool(ref["live"][:, nm["stick"]].all())
    assert int((k == 5).sum()) == 0                                                       # the two-vertex hull is never selected
    assert all(int((k == b).sum()) > 0 for b in range(5)) and int((k == -1).sum()) > 0
    mounted = c["pt_body"][:, len(nm):] >= 0
    assert 0.2 < float(mounted.double().mean()) < 0.5                                     # a third of the random points


@pytest.mark.parametrize("name", PH.CASE_NAMES + ("check",))
def test_at_most_two_percent_of_a_case_are_points_the_mirror_cannot_decide(name):
    ref = PH.reference(name)
    ex = ref["excluded"]
    assert int(ex.sum()) <= 0.02 * ex.numel(), (int(ex.sum()), ex.numel())
    assert not bool(torch.isnan(ref["dist"]).any())
    for k, g in ref["grads"].items():
        assert bool(torch.isfinite(g).all()), k
    c = PH.case(name)
    if name == "check":                                                                   # gradcheck's inputs: every point live and clean
        assert c["pt_body"].shape == (2, 6) and c["kind"].shape == (2, 3)
        assert int(ex.sum()) == 0 and bool(ref["live"].all()) and float(ref["gap"].min()) > 0.1
        assert int((ref["dist"] < 0).sum()) == 2
    if name == "wide":
        assert int(c["nverts"].sum(1).max()) == 1024 and c["pt_body"].shape == (2, 1024)
        finite = torch.isfinite(c["pt_max_dist"])
        assert int(finite.sum()) == 1024 and int((ref["live"] & finite).sum()) > 300 and int((~ref["live"] & finite).sum()) > 100
        assert int((c["pt_body"] >= 0).sum()) > 300 and int((c["pt_target"] >= 0).sum()) > 300
    if name == "tiny_mounted":
        assert c["pt_body"].shape == (7, 1) and not bool(ref["live"].any())
    if name == "tiny_world":
        assert c["pt_body"].shape == (7, 1) and int(ref["live"].sum()) >= 4 and int((~ref["live"]).sum()) >= 1


@pytest.mark.parametrize("name", ["small", "wide", "tiny_world"])
def test_the_normal_is_a_unit_vector_on_live_points_off_a_centre(name):
    ref = PH.reference(name)
    ln = ref["normal"].norm(dim=-1)
    centre = ref["live"] & (ln == 0)
    assert int(centre.sum()) == (3 if name == "small" else 0)                             # the named point of `small`
    assert float((ln[ref["live"] & ~centre] - 1.0).abs().max()) < 1e-12
    assert float(ln[~ref["live"]].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------- gradient
@pytest.mark.parametrize("name", ["small", "check", "tiny_world"])
@pytest.mark.parametrize("leaf", PH.LEAVES)
def test_autograd_of_the_mirror_equals_its_central_differences(name, leaf):
    """Directional: sum_r g_r (dist_r(x + h d) - dist_r(x - h d)) / 2h against <autograd's gradient, d> for random directions d of
    one input array at a time and the reference's cotangent g, zeroed on the points within 1e-3 of a change of branch (finite
    differences do not cross one).  h = 1e-6, 1e-6 relative to sum_r |g_r| |d dist_r|: a second-order scheme on a smooth function of
    order-100 coordinates."""
    ref, c = PH.reference(name), PH.case(name)
    g = torch.where((ref["gap"] < 1e-3) | ~ref["live"], torch.zeros_like(ref["g_dist"]), ref["g_dist"])
    cl = PH.leaves(c)
    grad = torch.autograd.grad(PH.points_host(cl)["dist"], cl[leaf], g, allow_unused=True)[0]
    if name == "tiny_world" and leaf == "verts_local":                                    # (one circle: no vertex has a gradient)
        assert grad is None or float(grad.abs().max()) == 0.0
        return
    assert grad is not None and float(grad.abs().max()) > 0
    h = 1e-6
    for seed in range(3):
        d = torch.randn(c[leaf].shape, generator=torch.Generator().manual_seed(seed), dtype=F64)
        with torch.no_grad():
            hi = PH.points_host(dict(c, **{leaf: c[leaf] + h * d}))
            lo = PH.points_host(dict(c, **{leaf: c[leaf] - h * d}))
        moved = hi["body"] != lo["body"]
        assert not bool(moved.any()) or bool((g[moved] == 0).all())
        fd = torch.where(g == 0, torch.zeros_like(g), (hi["dist"] - lo["dist"]) / (2 * h))      # (void: inf - inf)
        scale = float((g.abs() * fd.abs()).sum())
        assert abs(float((g * fd).sum()) - float((grad * d).sum())) <= 1e-6 * scale, (leaf, seed)


# ------------------------------------------------------------------------------------------------------------- the proximity query
def test_a_circle_at_the_point_is_the_proximity_query_of_the_same_rule():
    """A circle body of radius rho placed at a world point: pair dist = point dist(target = k) - rho, for every body of `small` - the
    two mirrors were written apart, from the same paragraph of the header."""
    c = PH.case("small")
    xy = torch.tensor(PH.np.random.default_rng(11).uniform(40.0, 260.0, (3, 9, 2)), dtype=F64)
    xy[:, 0] = c["p"][:, 4, 1:3] + 1.5                                                    # one inside the pentagon
    rho = 2.5
    pc, qc = PH.probe_circles(c, xy, rho)
    pair, point = XH.pairs_host(pc), PH.points_host(qc)
    real = (qc["pt_target"] != 5)                                                         # the two-vertex hull: invalid / void
    assert bool(torch.isfinite(pair["dist"][real]).all()) and bool(torch.isfinite(point["dist"][real]).all())
    assert bool(torch.isinf(pair["dist"][~real]).all()) and bool(torch.isinf(point["dist"][~real]).all())
    assert float((pair["dist"] - (point["dist"] - rho))[real].abs().max()) < 1e-12
    assert int((point["dist"][real] < 0).sum()) > 0
    # the normal from the circle (body 1 of the pair) towards body k is -u
    keep = real & ~pair["excluded"] & ~point["excluded"]
    assert float((pair["normal"] + point["normal"])[keep].abs().max()) < 1e-9


# ------------------------------------------------------------------------------------------------------------- PointSet (host side)
def test_point_set_checks_shapes_the_point_limit_and_max_dist():
    from lcp_physics_amd.physics.points import PointSet
    c = PH.case("small")
    ps = PointSet(c["pt_body"], c["pt_xy"], c["pt_target"], c["pt_max_dist"])
    assert (ps.B, ps.N) == (3, 70)
    with pytest.raises(ValueError, match="points.xy"):
        PointSet(c["pt_body"], c["pt_xy"][:, :69], c["pt_target"], c["pt_max_dist"])
    with pytest.raises(ValueError, match="points.target"):
        PointSet(c["pt_body"], c["pt_xy"], c["pt_target"][:2], c["pt_max_dist"])
    with pytest.raises(ValueError, match="points.max_dist"):
        PointSet(c["pt_body"], c["pt_xy"], c["pt_target"], c["pt_max_dist"].reshape(3, 70, 1))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="positive"):
            PointSet(c["pt_body"], c["pt_xy"], c["pt_target"], c["pt_max_dist"].clone().index_fill_(1, torch.tensor([3]), bad))
    z = lambda n, *s, dt_=F64: torch.ones(2, n, *s, dtype=dt_)
    assert PointSet(z(1024, dt_=torch.int32), z(1024, 2), z(1024, dt_=torch.int32), z(1024)).N == 1024
    for n in (0, 1025):
        with pytest.raises(ValueError, match="1 to 1024 points"):
            PointSet(z(n, dt_=torch.int32), z(n, 2), z(n, dt_=torch.int32), z(n))


def test_point_set_builders():
    from lcp_physics_amd.physics.points import PointSet
    ps = PointSet.on_body(3, [(1.0, 2.0), (3.0, 4.0), (5.0, 6.0)], B=4, target=2, max_dist=50.0)
    assert (ps.B, ps.N) == (4, 3) and ps.body.dtype == torch.int32 and ps.target.dtype == torch.int32 and ps.xy.dtype == F64
    assert ps.body.unique().tolist() == [3] and ps.target.unique().tolist() == [2] and ps.max_dist.unique().tolist() == [50.0]
    assert ps.xy[2].tolist() == [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]
    pw = PointSet.world([(7.0, 8.0)], B=2)
    assert pw.body.tolist() == [[-1], [-1]] and pw.target.tolist() == [[-1], [-1]] and bool(torch.isinf(pw.max_dist).all())
    with pytest.raises(ValueError, match="positive"):
        PointSet.world([(7.0, 8.0)], B=2, max_dist=0.0)
    moved = pw.to("cpu")
    assert torch.equal(moved.xy, pw.xy) and moved.xy.is_contiguous()


def test_point_set_grid_is_the_cameras_pixel_centres():
    from lcp_physics_amd.physics.points import PointSet
    from lcp_physics_amd.physics.render import Camera
    cam = Camera(24, 40, origin=(420.0, 400.5), pixels_per_meter=0.3)
    ps = PointSet.grid(cam, B=3, max_dist=60.0)
    X, Y = pixel_centres(24, 40, 420.0, 400.5, 0.3)                                       # (x0 + (j + 1/2) / ppm, y0 + (i + 1/2) / ppm)
    assert (ps.B, ps.N) == (3, 960) and ps.body.unique().tolist() == [-1]
    assert torch.equal(ps.xy.reshape(3, 24, 40, 2)[1], torch.stack([X, Y], -1))
    sub = PointSet.grid(cam, 8, 16, B=1)                                                   # the top-left 8 x 16 pixels
    assert torch.equal(sub.xy.reshape(8, 16, 2), torch.stack([X, Y], -1)[:8, :16])
    ext = PointSet.grid((0.0, 10.0, 8.0, 16.0), 3, 4, B=2)                                 # cells of 2 x 2
    assert ext.xy[0, :5].tolist() == [[1.0, 11.0], [3.0, 11.0], [5.0, 11.0], [7.0, 11.0], [1.0, 13.0]]
    with pytest.raises(ValueError, match="1 to 1024 points"):
        PointSet.grid(Camera(33, 32), B=1)
    with pytest.raises(ValueError, match="needs h and w"):
        PointSet.grid((0.0, 0.0, 1.0, 1.0), B=1)
