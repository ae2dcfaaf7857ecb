"""GPU: the point probe of lcp_points.hip (lcp_point_distance_f64, lcp_point_distance_backward_f64; physics/points.py) against the
host mirror tests/points_host.py, which tests/test_points_host.py checks on the CPU.

`dist` is compared everywhere, within 1e-9.  `body` (equal) and `normal` (within 1e-9) are compared on the points the mirror itself
can decide (`excluded` marks the others: a second body or feature within 1e-9, max h or d - max_dist within 1e-9 of 0, or a unit
vector formed from a length below 1e-3; at most 2 % of a case, asserted on the CPU).  The tolerance: fp64 rounding on coordinates up
to 1e3 is about 1e-13 after a handful of operations; the quotient by a length of at least 1e-3 grows that to 1e-10, and 1e-9 leaves
a decade.  The backward takes the reference's cotangent, which is zero on the excluded points, so that they reach no gradient on either
side: every gradient within 1e-8 of the mirror's autograd, relative to the array's largest entry (the gate of the range sensors and
the proximity queries)."""
import pytest
import torch

from tests import points_host as PH

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, I32 = torch.float64, torch.int32
INF = float("inf")
SCENE = ("kind", "radius", "verts_local", "nverts", "p")
POINTS = ("pt_body", "pt_xy", "pt_target", "pt_max_dist")


def _lib():
    from lcp_physics_amd import _lib as L
    return L


def _absmax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _sizes(c, svm=None):
    B, nb, cap = c["verts_local"].shape[:3]
    nv = torch.where(c["kind"] != 0, c["nverts"].clamp(0, cap), torch.zeros_like(c["nverts"]))
    return [B, nb, cap, int(nv.sum(1).max()) if svm is None else svm, c["pt_body"].shape[1]]


def _inputs(c, svm=None):
    d = {k: c[k].to(DEV).contiguous() for k in SCENE + POINTS}
    return d, _sizes(c, svm) + [_lib().ptr(d[k]) for k in SCENE + POINTS]


def _forward(c, svm=None):
    """The raw entry into outputs pre-filled with NaN / -7: dist, body, normal (CPU)."""
    L = _lib()
    d, args = _inputs(c, svm)
    B, N = c["pt_body"].shape
    dist = torch.full((B, N), float("nan"), dtype=F64, device=DEV)
    body = torch.full((B, N), -7, dtype=I32, device=DEV)
    normal = torch.full((B, N, 2), float("nan"), dtype=F64, device=DEV)
    rc = L.load().lcp_point_distance_f64(*args, L.ptr(dist), L.ptr(body), L.ptr(normal), L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    return dist.cpu(), body.cpu(), normal.cpu()


def _backward(c, g_dist, svm=None):
    """The raw entry into outputs pre-filled with NaN: the four gradients (CPU), keyed as points_host.LEAVES."""
    L = _lib()
    d, args = _inputs(c, svm)
    g = g_dist.to(DEV).contiguous()
    outs = [torch.full(c[k].shape, float("nan"), dtype=F64, device=DEV) for k in PH.LEAVES]
    rc = L.load().lcp_point_distance_backward_f64(*args, L.ptr(g), *[L.ptr(o) for o in outs], L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    return {k: o.cpu() for k, o in zip(PH.LEAVES, outs)}


_FWD = {}


def _fwd(name):
    if name not in _FWD:
        _FWD[name] = _forward(PH.case(name))
    return _FWD[name]


@pytest.mark.parametrize("name", PH.CASE_NAMES)
def test_forward_matches_the_mirror(name):
    ref, c = PH.reference(name), PH.case(name)
    dist, body, normal = _fwd(name)
    keep = ~ref["excluded"]
    assert int((~keep).sum()) <= 0.02 * keep.numel()                                      # (the mirror alone: test_points_host.py too)
    assert not bool(torch.isnan(dist).any()) and bool(torch.isfinite(normal).all()) and int(body.min()) >= -1    # written, everywhere
    both = torch.isfinite(dist) & torch.isfinite(ref["dist"])
    assert torch.equal(torch.isfinite(dist), torch.isfinite(ref["dist"]))                 # (+inf: a void point without a cutoff)
    ed = _absmax((dist - ref["dist"])[both])
    en = _absmax((normal - ref["normal"])[keep])
    print("%s: |dist - mirror| %.3g  |normal - mirror| %.3g  body mismatches %d  excluded %d of %d" % (
        name, ed, en, int((body != ref["body"])[keep].sum()), int((~keep).sum()), keep.numel()))
    assert ed <= 1e-9 and en <= 1e-9 and torch.equal(body[keep], ref["body"][keep])
    # a void point is max_dist itself, -1 and no normal, exactly
    void = body < 0
    assert torch.equal(dist[void], c["pt_max_dist"][void]) and _absmax(normal[void]) == 0.0
    assert bool((dist[~void] < c["pt_max_dist"][~void]).all())


def test_the_named_points_of_small():
    """`on_face` and `at_cutoff` of scene 0 are points the mirror leaves out by its own rule; at representable coordinates they are
    decided exactly, and are compared here."""
    ref, c = PH.reference("small"), PH.case("small")
    nm = c["names"]
    dist, body, normal = _fwd("small")
    for name, r in nm.items():
        assert _absmax((dist[:, r] - ref["dist"][:, r])[torch.isfinite(ref["dist"][:, r])]) <= 1e-9, name
        if name not in ("on_face", "at_cutoff"):
            assert torch.equal(body[:, r], ref["body"][:, r]) and _absmax(normal[:, r] - ref["normal"][:, r]) <= 1e-9, name
    assert torch.equal(dist[:, nm["centre"]], -c["radius"][:, 0]) and _absmax(normal[:, nm["centre"]]) == 0.0
    assert body[:, nm["centre"]].tolist() == [0] * 3
    assert float(dist[0, nm["on_face"]]) == 0.0 and body[:, nm["on_face"]].tolist() == [2] * 3
    assert _absmax(normal[0, nm["on_face"]] - torch.tensor([1.0, 0.0], dtype=F64)) <= 1e-15      # (|e| / |e| through 1 / |e|: an ulp)
    assert _absmax(normal[:, nm["inside_rect"]] - torch.tensor([[0.0, 1.0]] * 3, dtype=F64)) <= 1e-15
    assert _absmax(dist[:, nm["inside_rect"]] + 9.0) <= 1e-14
    assert body[:, nm["inside_vertex"]].tolist() == [4] * 3 and float(dist[:, nm["inside_vertex"]].max()) < 0.0
    assert body[:, nm["vertex_outer"]].tolist() == [4] * 3
    assert dist[:, nm["beyond"]].tolist() == [5.0] * 3 and body[:, nm["beyond"]].tolist() == [-1] * 3
    assert dist[:, nm["at_cutoff"]].tolist() == [8.0] * 3 and body[:, nm["at_cutoff"]].tolist() == [-1, 2, 2]      # d == max_dist: void
    assert body[:, nm["far_target"]].tolist() == [4] * 3
    for name in ("own_mount", "bad_mount", "stick_alone"):
        assert body[:, nm[name]].tolist() == [-1] * 3 and dist[:, nm[name]].tolist() == [INF] * 3, name
    assert int((body == 5).sum()) == 0                                                    # the two-vertex hull


@pytest.mark.parametrize("name", PH.CASE_NAMES)
def test_backward_matches_the_mirrors_autograd(name):
    ref, c = PH.reference(name), PH.case(name)
    got = _backward(c, ref["g_dist"])
    for k in PH.LEAVES:
        want = ref["grads"][k]
        assert bool(torch.isfinite(got[k]).all()), k                                      # written, everywhere
        err, scale = float((got[k] - want).abs().max()), float(want.abs().max())
        print("%s %s: |difference| %.3g of %.3g" % (name, k, err, scale))
        assert err <= 1e-8 * scale, k                                                     # (no gradient in the mirror: exactly 0)
    if name in ("small", "wide"):
        assert all(_absmax(ref["grads"][k]) > 0 for k in ("p", "verts_local", "pt_xy"))
    still = ~ref["live"] & ~ref["excluded"]                                             # void points
    if int(still.sum()):
        assert _absmax(got["pt_xy"][still]) == 0.0
    hull = c["kind"] != 0
    cap = c["verts_local"].shape[2]
    pad = torch.arange(cap).reshape(1, 1, cap) >= (c["nverts"] * hull).unsqueeze(2)
    assert _absmax(got["radius"][hull]) == 0.0 and _absmax(got["verts_local"][pad]) == 0.0


@pytest.mark.parametrize("name", ["small", "wide"])
def test_two_runs_of_the_backward_give_the_same_bits(name):
    c, g = PH.case(name), PH.reference(name)["g_dist"]
    a, b = _backward(c, g), _backward(c, g)
    for k in a:
        assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)), k


def test_a_finite_cutoff_leaves_the_bits_of_every_live_point():
    """`wide` with every max_dist = +inf against `wide` as it is (finite cutoffs on half): the wavefront's skip of bodies beyond the
    cutoff changes no bit of a point that is live under the cutoff."""
    c = PH.case("wide")
    free = dict(c, pt_max_dist=torch.full_like(c["pt_max_dist"], INF))
    cut, far = _fwd("wide"), _forward(free)
    live = cut[1] >= 0
    finite = torch.isfinite(c["pt_max_dist"])
    assert int((live & finite).sum()) > 300 and int((~live & finite).sum()) > 100
    assert torch.equal(cut[0][live].view(torch.int64), far[0][live].view(torch.int64)) and torch.equal(cut[1][live], far[1][live])
    assert torch.equal(cut[2][live].view(torch.int64), far[2][live].view(torch.int64))


def test_a_circle_at_the_point_is_the_shipped_pair_distance():
    """Circles of radius rho appended to `small` at world points, through lcp_pair_distance_f64: pair dist + rho = point dist."""
    L = _lib()
    c = PH.case("small")
    xy = torch.tensor(PH.np.random.default_rng(11).uniform(40.0, 260.0, (3, 9, 2)), dtype=F64)
    xy[:, 0] = c["p"][:, 4, 1:3] + 1.5                                                    # one inside the pentagon
    rho = 2.5
    pc, qc = PH.probe_circles(c, xy, rho)
    point = _forward(qc)[0]
    names = SCENE + ("pair_first", "pair_second", "pair_max_dist")
    d = {k: pc[k].to(DEV).contiguous() for k in names}
    B, P = pc["pair_first"].shape
    pair = torch.full((B, P), float("nan"), dtype=F64, device=DEV)
    sizes = _sizes(dict(pc, pt_body=pc["pair_first"]))
    rc = L.load().lcp_pair_distance_f64(*sizes, *[L.ptr(d[k]) for k in names], L.ptr(pair), None, None, None, L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    pair = pair.cpu()
    real = qc["pt_target"] != 5                                                           # the two-vertex hull: invalid / void
    assert bool(torch.isinf(pair[~real]).all()) and bool(torch.isinf(point[~real]).all())
    err = _absmax((pair + rho - point)[real])
    print("|pair dist + rho - point dist| %.3g over %d queries, %d inside" % (err, int(real.sum()), int((point[real] < 0).sum())))
    assert err <= 1e-9 and int((point[real] < 0).sum()) > 0


def test_a_scene_over_the_vertex_limit_is_all_void():
    c = PH.case("wide")
    dist, body, normal = _forward(c, svm=1023)
    assert torch.equal(dist, c["pt_max_dist"]) and int((body != -1).sum()) == 0 and _absmax(normal) == 0.0
    for k, g in _backward(c, PH.reference("wide")["g_dist"], svm=1023).items():
        assert _absmax(g) == 0.0, k


# ------------------------------------------------------------------------------------------------------------- the autograd surface
def _geom(c, leaves=False):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.points import PointSet
    t = lambda k: c[k].to(DEV).contiguous()
    lf = (lambda k: t(k).requires_grad_(True)) if leaves else t
    geom = GeometryBatch(t("kind"), lf("radius"), lf("verts_local"), t("nverts"), None, _sizes(c)[3])
    points = PointSet(t("pt_body"), lf("pt_xy"), t("pt_target"), t("pt_max_dist"))
    return geom, lf("p"), points


def test_point_distances_returns_the_entrys_bits_and_its_backward_the_entrys_gradients():
    from lcp_physics_amd.physics.points import point_distances
    c, ref = PH.case("small"), PH.reference("small")
    geom, p, points = _geom(c, leaves=True)
    dist, body, normal = point_distances(geom, p, points, normals=True)
    want = _fwd("small")
    assert torch.equal(dist.detach().cpu(), want[0]) and torch.equal(body.cpu(), want[1]) and torch.equal(normal.cpu(), want[2])
    assert dist.requires_grad and not body.requires_grad and not normal.requires_grad
    assert dist.dtype == F64 and body.dtype == I32 and len(point_distances(geom, p, points)) == 2
    dist.backward(ref["g_dist"].to(DEV))
    raw = _backward(c, ref["g_dist"])
    for k, t in zip(PH.LEAVES, (p, geom.radius, geom.verts_local, points.xy)):
        assert torch.equal(t.grad.cpu(), raw[k]), k
    # only what requires grad is asked for
    geom2, p2, points2 = _geom(c)
    p2.requires_grad_(True)
    point_distances(geom2, p2, points2)[0].backward(ref["g_dist"].to(DEV))
    assert torch.equal(p2.grad.cpu(), raw["p"]) and points2.xy.grad is None


def test_gradcheck_at_six_points_and_three_bodies():
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.points import PointSet, point_distances
    c = PH.case("check")                                                                  # every point live, far from a branch
    assert c["pt_body"].shape[1] == 6 and c["kind"].shape[1] == 3
    t = lambda k: c[k].to(DEV).contiguous()
    ins = [t(k).requires_grad_(True) for k in PH.LEAVES]

    def fn(p, radius, verts_local, xy):
        geom = GeometryBatch(t("kind"), radius, verts_local, t("nverts"), None, _sizes(c)[3])
        return point_distances(geom, p, PointSet(t("pt_body"), xy, t("pt_target"), t("pt_max_dist")))[0]

    assert torch.autograd.gradcheck(fn, ins, eps=1e-6, atol=1e-6, rtol=1e-6, nondet_tol=0.0)


def test_world_probe_reaches_v0_through_differentiable_steps():
    """A ball over a floor (the scene of tests/test_hip_render.py::_world): after two differentiable steps the distance from points
    mounted on the ball to the floor is part of the roll-out's graph, and its value is the mirror's at `world.p`."""
    import numpy as np
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.points import PointSet, point_distances
    from tests.test_hip_bodies import _rollout_bodies, _rollout_fixture
    d, B = _rollout_fixture(), 4
    t64 = lambda a: torch.tensor(a, dtype=F64)
    bb = _rollout_bodies(d, B, t64(float(d["ball_rad"])), t64(d["box_verts_raw"]), t64(float(d["mass"][0])), t64(float(d["mass"][1])))
    v0 = bb.v0.detach().clone().requires_grad_(True)
    f = bb.f_gravity.clone()
    f[:, 0] = 0.0                                                                         # the floor is held by Je and carries no gravity
    Je = torch.tensor(np.repeat(d["Je"][:1], B, axis=0), dtype=torch.float32, device=DEV)
    world = ContactWorld(bb.geom, bb.p0.detach().clone(), v0, bb.Mdiag, f, bb.rest, bb.fric, Je=Je, dt=float(d["dt"]), maxc=8)
    tips = PointSet.on_body(1, [(0.0, 0.0), (3.0, 1.0), (-2.0, 4.0)], B, max_dist=5000.0).to(DEV)
    free = PointSet.world([(float(d["ball_pos"].reshape(-1)[-2]), float(d["ball_pos"].reshape(-1)[-1])), (0.0, 0.0)], B).to(DEV)
    for a, b in zip(world.probe(free, normals=True), point_distances(world.geom, world.p, free, normals=True)):     # a plain world
        assert torch.equal(a, b)
    for _ in range(2):
        world.step(differentiable=True)
    dist, body = world.probe(tips)
    assert dist.requires_grad and body.cpu().tolist() == [[0] * 3] * B                    # the floor: the only other body
    g = world.geom
    host = dict(kind=g.kind.cpu(), radius=g.radius.detach().cpu(), verts_local=g.verts_local.detach().cpu(), nverts=g.nverts.cpu(),
                p=world.p.detach().cpu(), pt_body=tips.body.cpu(), pt_xy=tips.xy.cpu(), pt_target=tips.target.cpu(), pt_max_dist=tips.max_dist.cpu())
    ref = PH.points_host(host)
    assert torch.equal(body.cpu(), ref["body"]) and _absmax(dist.detach().cpu() - ref["dist"]) <= 1e-9
    dist.sum().backward()
    gv = v0.grad.cpu()
    print("d sum(dist) / d v0", gv[0].tolist())
    assert bool(torch.isfinite(gv).all()) and float(gv[:, 1].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_are_refused_before_any_launch():
    L = _lib()
    lib, c = L.load(), PH.case("small")
    d, args = _inputs(c)
    B, N = c["pt_body"].shape
    dist = torch.full((B, N), float("nan"), dtype=F64, device=DEV)
    g = torch.zeros(B, N, dtype=F64, device=DEV)
    g_p = torch.full(c["p"].shape, float("nan"), dtype=F64, device=DEV)
    stream = L.stream_ptr(torch.device(DEV))
    fwd = lambda a, out=True: lib.lcp_point_distance_f64(*a, L.ptr(dist) if out else None, None, None, stream)
    bwd = lambda a, out=True: lib.lcp_point_distance_backward_f64(*a, L.ptr(g), L.ptr(g_p) if out else None, None, None, None, stream)
    with_size = lambda k, v: args[:k] + [v] + args[k + 1:]
    bad = [with_size(4, 0), with_size(4, 1025), with_size(1, 65), with_size(1, 0), with_size(2, 7), with_size(3, 1025), with_size(0, -1),
           with_size(9, None), with_size(10, None), with_size(11, None), with_size(12, None), with_size(13, None)]
    for a in bad:                                                                         # sizes out of range; p or a point array NULL
        assert fwd(a) == -1 and bwd(a) == -1
    assert fwd(args, out=False) == -1 and bwd(args, out=False) == -1                      # no output
    assert lib.lcp_point_distance_backward_f64(*args, None, L.ptr(g_p), None, None, None, stream) == -1          # g_dist = NULL
    assert fwd(with_size(0, 0)) == 0 and bwd(with_size(0, 0)) == 0                        # B = 0: success, no launch
    torch.cuda.synchronize()
    assert bool(torch.isnan(dist).all()) and bool(torch.isnan(g_p).all())                 # nothing was written
    assert fwd(args) == 0 and bwd(args) == 0


def test_host_side_refusals():
    from lcp_physics_amd.physics.points import PointSet, point_distances
    c = PH.case("small")
    geom, p, points = _geom(c)
    with pytest.raises(ValueError, match="positive"):
        PointSet(points.body, points.xy, points.target, points.max_dist.clone().index_fill_(1, torch.tensor([3], device=DEV), 0.0))
    cpu = lambda s: PointSet(s.body.cpu(), s.xy.cpu(), s.target.cpu(), s.max_dist.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        point_distances(geom, p.cpu(), points)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        point_distances(geom, p, cpu(points))
    with pytest.raises(ValueError, match="scenes"):
        point_distances(geom, p, PointSet.world([(0.0, 0.0)], B=2).to(DEV))
    with pytest.raises(RuntimeError, match="must be"):
        point_distances(geom, p, PointSet(points.body.long(), points.xy, points.target, points.max_dist))
