"""GPU: the overlap query of lcp_overlap.hip (lcp_pair_overlap_f64, lcp_pair_overlap_backward_f64; physics/overlap.py) against the host
mirror tests/overlap_host.py, which tests/test_overlap_host.py checks on the CPU, and against the clip yardstick directly.

Tolerances: `area` within 1e-9 of the mirror on EVERY pair (the project's tolerance for these queries: the same fp64 arithmetic on
coordinates of order 100 to 1000, areas up to a few thousand; the area is continuous, so the mirror has no undecided pairs); invalid
and culled pairs exactly 0.  Against the clip: 1e-10 R^2, plus the inscribed 4096-gon's deficit where a circle takes part.  The
backward takes the reference's cotangent, which is zero on the pairs where the area has a kink (`shared`, `rotated`: a piece of one
boundary lies in the other's, no gradient exists): every gradient within 1e-8 of the mirror's autograd, relative to the leaf's largest
reference entry."""
import pytest
import torch

from tests import overlap_host as OH

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, I32 = torch.float64, torch.int32
SCENE = ("kind", "radius", "verts_local", "nverts", "p")
PAIRS = ("pair_first", "pair_second")
NAN = float("nan")


def _lib():
    from lcp_physics_amd import _lib as L
    return L


def _absmax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _sizes(c, svm=None):
    B, nb, cap = c["verts_local"].shape[:3]
    nv = torch.where(c["kind"] != 0, c["nverts"].clamp(0, cap), torch.zeros_like(c["nverts"]))
    return [B, nb, cap, int(nv.sum(1).max()) if svm is None else svm, c["pair_first"].shape[1]]


def _inputs(c, svm=None):
    d = {k: c[k].detach().to(DEV).contiguous() for k in SCENE + PAIRS}
    return d, _sizes(c, svm) + [_lib().ptr(d[k]) for k in SCENE + PAIRS]


def _forward(c, svm=None):
    """The raw entry into an output pre-filled with NaN: area (CPU)."""
    L = _lib()
    d, args = _inputs(c, svm)
    area = torch.full(tuple(c["pair_first"].shape), NAN, dtype=F64, device=DEV)
    rc = L.load().lcp_pair_overlap_f64(*args, L.ptr(area), L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    return area.cpu()


def _backward(c, g_area, svm=None):
    """The raw entry into outputs pre-filled with NaN: the three gradients (CPU), keyed as overlap_host.LEAVES."""
    L = _lib()
    d, args = _inputs(c, svm)
    g = g_area.to(DEV).contiguous()
    outs = [torch.full(c[k].shape, NAN, dtype=F64, device=DEV) for k in OH.LEAVES]
    rc = L.load().lcp_pair_overlap_backward_f64(*args, L.ptr(g), *[L.ptr(o) for o in outs], L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    return {k: o.cpu() for k, o in zip(OH.LEAVES, outs)}


_FWD = {}


def _fwd(name):
    if name not in _FWD:
        _FWD[name] = _forward(OH.case(name))
    return _FWD[name]


def _classes(c):
    """invalid [B,P]: no pair at all; far [B,P]: the bounding circles are at least 1e-3 apart (culled by any rounding of the bound)."""
    B, P = c["pair_first"].shape
    nb = c["kind"].shape[1]
    invalid, far = torch.zeros(B, P, dtype=torch.bool), torch.zeros(B, P, dtype=torch.bool)
    for b in range(B):
        for r in range(P):
            k1, k2 = int(c["pair_first"][b, r]), int(c["pair_second"][b, r])
            ok = k1 != k2 and 0 <= k1 < nb and 0 <= k2 < nb
            ok = ok and all(int(c["kind"][b, k]) == 0 or int(c["nverts"][b, k]) >= 3 for k in (k1, k2))
            invalid[b, r] = not ok
            if ok:
                gap = float((c["p"][b, k1, 1:] - c["p"][b, k2, 1:]).norm()) - OH.bounding_radius(c, b, k1) - OH.bounding_radius(c, b, k2)
                far[b, r] = gap > 1e-3
    return invalid, far


# ------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("name", OH.CASE_NAMES)
def test_forward_matches_the_mirror(name):
    ref, c = OH.reference(name), OH.case(name)
    area = _fwd(name)
    invalid, far = _classes(c)
    assert not bool(torch.isnan(area).any()) and bool((area >= 0).all())                   # written, everywhere
    assert _absmax(area[invalid]) == 0.0 and _absmax(area[far]) == 0.0                    # exactly 0
    err = _absmax(area - ref["area"])                                                     # every pair
    print("%s: |area - mirror| %.3g at areas up to %.4g   invalid %d, culled %d, overlapping %d of %d" % (
        name, err, float(ref["area"].max()), int(invalid.sum()), int(far.sum()), int((area > 0).sum()), area.numel()))
    assert err <= 1e-9
    assert torch.equal(area > 0, ref["area"] > 0) or name in ("shared", "rotated")
    if name == "rotated":                                                                 # touching from outside at a generic rotation
        assert _absmax(area[torch.arange(48) % 4 != 2]) <= 1e-12 * 60.0 ** 2 and float(area[2::4].min()) > 10.0
    if name == "invalid":
        assert int(invalid.sum()) == 10 and float(area[0, -1]) > 0.0
    if name == "wide":
        assert int(far.sum()) > 0 and int((area[:, 256:] > 0).sum()) > 0                  # both sides of the 256-pair chunk edge


def test_shared_boundaries_count_once():
    area = _fwd("shared")[0]
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.overlap import body_areas
    c = OH.case("shared")
    own = float(body_areas(GeometryBatch(c["kind"], c["radius"], c["verts_local"], c["nverts"], None, None))[0, 4])
    want = torch.tensor([own if w is None else w for w in OH.SHARED_WANT], dtype=F64)
    print("shared:", area.tolist(), "want", want.tolist())
    assert _absmax(area - want) <= 1e-9 and float(area[0]) == 0.0 and float(area[1]) == 0.0


@pytest.mark.parametrize("name", ["small", "big_hulls", "rotated", "near"])
def test_forward_against_the_clip(name):
    c, area = OH.case(name), _fwd(name)
    B, P = area.shape
    worst = 0.0
    for b in range(B):
        for r in range(P):
            k1, k2 = int(c["pair_first"][b, r]), int(c["pair_second"][b, r])
            want, slack = OH.clip_pair(c, b, k1, k2)
            R2 = max(OH.bounding_radius(c, b, k1), OH.bounding_radius(c, b, k2)) ** 2
            err = abs(float(area[b, r]) - want)
            assert err <= slack + 1e-10 * R2, (b, r, float(area[b, r]), want)
            if slack == 0.0:
                worst = max(worst, err / R2)
    print("%s: |area - clip| / R^2 over the hull pairs %.3g" % (name, worst))


def test_the_pair_fixture_as_one_batch_of_600_scenes():
    """tests/golden/contacts_pairs.npz: area > 0 exactly where the pair's signed distance is negative (pairs within 1e-9 of touching
    left out: at most 1 % of the 600), and no more than the smaller body's own area."""
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.overlap import body_areas
    from lcp_physics_amd.physics.proximity import PairSet, pair_distances
    from tests.proximity_host import fixture_case
    c, _, _ = fixture_case()
    area = _forward(c)[:, 0]
    t = lambda k: c[k].to(DEV).contiguous()
    geom = GeometryBatch(t("kind"), t("radius"), t("verts_local"), t("nverts"), None, _sizes(c)[3])
    dist = pair_distances(geom, t("p"), PairSet(t("pair_first"), t("pair_second"), t("pair_max_dist")))[:, 0].cpu()
    own = body_areas(GeometryBatch(c["kind"], c["radius"], c["verts_local"], c["nverts"], None, None))
    decided = dist.abs() > 1e-9
    print("fixture: %d of 600 overlap, %d undecided, largest area %.4g, area - min own %.3g" % (
        int((area > 0).sum()), int((~decided).sum()), float(area.max()), float((area - own.min(1).values).max())))
    assert area.shape == (600,) and int((~decided).sum()) <= 6
    assert torch.equal((area > 0)[decided], (dist < 0)[decided]) and int((area > 0).sum()) > 100
    assert bool((area <= own.min(1).values + 1e-9).all())


# ------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("name", OH.CASE_NAMES)
def test_backward_matches_the_mirrors_autograd(name):
    ref, c = OH.reference(name), OH.case(name)
    got = _backward(c, ref["g_area"])
    for k in OH.LEAVES:
        assert bool(torch.isfinite(got[k]).all()), k                                      # written, everywhere
    hull = c["kind"] != 0
    cap = c["verts_local"].shape[2]
    pad = torch.arange(cap).reshape(1, 1, cap) >= (c["nverts"] * hull).unsqueeze(2)
    assert _absmax(got["radius"][hull]) == 0.0 and _absmax(got["verts_local"][pad]) == 0.0
    assert int(ref["kink"].sum()) == (ref["kink"].numel() if name in ("shared", "rotated") else 0)
    for k in OH.LEAVES:
        want = ref["grads"][k]
        err, scale = float((got[k] - want).abs().max()), float(want.abs().max())
        print("%s %s: |difference| %.3g of %.3g" % (name, k, err, scale))
        assert err <= 1e-8 * scale, k
        # (shared: every pair has a kink and a zero cotangent; big_hulls and shared have no circle)
        assert scale > 0 or name in ("shared", "rotated") or (k == "radius" and not bool((c["kind"] == 0).any())), k


def test_a_pair_of_area_0_has_zero_gradient_and_a_kink_a_finite_one():
    c = OH.case("small")
    area = _fwd("small")
    g = torch.where(area > 0, torch.zeros_like(area), torch.ones_like(area))              # a cotangent on the pairs that are apart only
    assert int((g > 0).sum()) >= 3
    for k, t in _backward(c, g).items():
        assert _absmax(t) == 0.0, k
    got = _backward(OH.case("shared"), torch.ones(1, 6, dtype=F64))
    assert all(bool(torch.isfinite(t).all()) for t in got.values())


@pytest.mark.parametrize("name", ["small", "wide", "big_hulls"])
def test_two_runs_of_the_backward_give_the_same_bits(name):
    c, g = OH.case(name), OH.reference(name)["g_area"]
    a, b = _backward(c, g), _backward(c, g)
    for k in a:
        assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)), k


# ------------------------------------------------------------------------------------------------------------- independence
def test_the_area_does_not_depend_on_the_cull():
    """The bounding data cannot be inflated from outside (a hull's comes from its staged vertices), so: scene 0 of `small`, whose three
    pairs all overlap, next to a copy whose bodies stand 1000 apart.  The copy's pairs are exactly 0; the original's have the bits
    they have inside `small`, where other scenes' pairs are culled around them."""
    c = OH.case("small")
    two = {k: c[k][:1].repeat(2, *[1] * (c[k].dim() - 1)).clone() for k in SCENE + PAIRS}
    two["p"][1, :, 1] += 1000.0 * torch.arange(3, dtype=F64)
    area = _forward(two)
    assert torch.equal(area[0].view(torch.int64), _fwd("small")[0].view(torch.int64)) and bool((area[0] > 0).all())
    assert _absmax(area[1]) == 0.0
    for k, t in _backward(two, torch.ones(2, 3, dtype=F64)).items():
        assert _absmax(t[1]) == 0.0 and (k == "radius" or _absmax(t[0]) > 0.0), k


def test_a_scene_over_the_vertex_limit_returns_zeros():
    c = OH.case("wide")
    nv = torch.where(c["kind"] != 0, c["nverts"], torch.zeros_like(c["nverts"])).sum(1)
    big, less = int(nv.argmax()), int(nv.argmin())
    assert int(nv[big]) > int(nv[less])
    area = _forward(c, svm=int(nv[big]) - 1)
    assert _absmax(area[big]) == 0.0 and torch.equal(area[less], _fwd("wide")[less])
    got = _backward(c, OH.reference("wide")["g_area"], svm=int(nv[big]) - 1)
    full = _backward(c, OH.reference("wide")["g_area"])
    for k in got:
        assert _absmax(got[k][big]) == 0.0 and torch.equal(got[k][less], full[k][less]), k


# ------------------------------------------------------------------------------------------------------------- the autograd surface
def _geom(c, leaves=False):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.proximity import PairSet
    t = lambda k: c[k].to(DEV).contiguous()
    lf = (lambda k: t(k).requires_grad_(True)) if leaves else t
    geom = GeometryBatch(t("kind"), lf("radius"), lf("verts_local"), t("nverts"), None, _sizes(c)[3])
    return geom, lf("p"), PairSet(t("pair_first"), t("pair_second"), t("pair_max_dist"))


def test_pair_overlaps_returns_the_entrys_bits_and_its_backward_the_entrys_gradients():
    from lcp_physics_amd.physics.overlap import body_areas, pair_overlaps
    c, ref = OH.case("small"), OH.reference("small")
    geom, p, pairs = _geom(c, leaves=True)
    area = pair_overlaps(geom, p, pairs)
    assert isinstance(area, torch.Tensor) and area.requires_grad and torch.equal(area.detach().cpu(), _fwd("small"))
    area.backward(ref["g_area"].to(DEV))
    raw = _backward(c, ref["g_area"])
    for k, t in zip(OH.LEAVES, (p, geom.radius, geom.verts_local)):
        assert torch.equal(t.grad.cpu(), raw[k]), k
    # only what requires grad is asked for
    geom2, p2, pairs2 = _geom(c)
    p2.requires_grad_(True)
    pair_overlaps(geom2, p2, pairs2).backward(ref["g_area"].to(DEV))
    assert torch.equal(p2.grad.cpu(), raw["p"]) and geom2.radius.grad is None and geom2.verts_local.grad is None
    # iou: the union from body_areas
    a, iou = pair_overlaps(geom2, p2.detach(), pairs2, iou=True)
    own = body_areas(geom2)
    f, s = pairs2.first.long(), pairs2.second.long()
    want = a / (torch.gather(own, 1, f) + torch.gather(own, 1, s) - a)
    assert torch.equal(a.cpu(), _fwd("small")) and _absmax(iou - want) <= 1e-15 and 0.0 < float(iou.max()) <= 1.0
    inv = OH.case("invalid")
    geom3, p3, pairs3 = _geom(inv)
    a3, iou3 = pair_overlaps(geom3, p3, pairs3, iou=True)
    assert _absmax(iou3[0, :-1]) == 0.0 and float(iou3[0, -1]) > 0.0 and bool(torch.isfinite(iou3).all())


def _gradcheck_case():
    """Three bodies (a circle, a rect, a pentagon) and three pairs, each overlapping partially and far from every tie."""
    import numpy as np
    rng = np.random.default_rng(5)
    c = OH._assemble([[("circle", (0.2, 100.0, 92.0), 14.0), ("hull", (0.35, 122.0, 100.0), OH._rect(40.0, 30.0)),
                       ("hull", (0.8, 108.0, 112.0), OH._hull(rng, 5, 22.0, 20.0))]], 8)
    c.update(OH._pairs([[(0, 1, OH.INF), (2, 0, OH.INF), (1, 2, OH.INF)]]))
    return c


def test_gradcheck_at_three_bodies_and_three_pairs():
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.overlap import pair_overlaps
    from lcp_physics_amd.physics.proximity import PairSet
    c = _gradcheck_case()
    out = OH.overlaps_host(c)
    assert float(out["area"].min()) > 20.0 and not bool(out["kink"].any())
    t = lambda k: c[k].to(DEV).contiguous()
    ins = [t(k).requires_grad_(True) for k in OH.LEAVES]

    def fn(p, radius, verts_local):
        geom = GeometryBatch(t("kind"), radius, verts_local, t("nverts"), None, _sizes(c)[3])
        return pair_overlaps(geom, p, PairSet(t("pair_first"), t("pair_second"), t("pair_max_dist")))

    assert torch.autograd.gradcheck(fn, ins, eps=1e-6, atol=1e-6, rtol=1e-6, nondet_tol=0.0)


def _zone_world(v0):
    """A ball (body 0) in free flight towards a goal zone (body 1, a rect that `no_contact` keeps out of collisions); dt = 2^-5 and
    velocities of a few bits, so that the float32 state adds into the float64 pose without rounding."""
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.contacts import GeometryBatch
    B = 2
    geom = GeometryBatch.from_shapes([("circle", 10.0), ("rect", (60.0, 40.0))], B)
    geom.no_contact = (torch.ones(B, 2, 2, dtype=torch.uint8) - torch.eye(2, dtype=torch.uint8)).contiguous()
    p0 = torch.tensor([[0.0, 100.0, 100.0], [0.3, 134.0, 104.0]], dtype=F64, device=DEV).repeat(B, 1, 1)
    p0[1, 0, 2] += 6.0                                                                     # (the scenes differ)
    Mdiag = torch.tensor([[50.0, 1.0, 1.0], [80.0, 2.0, 2.0]], dtype=torch.float32, device=DEV).repeat(B, 1, 1)
    zeros = torch.zeros(B, 2, dtype=torch.float32, device=DEV)
    return ContactWorld(geom.to(DEV), p0, v0, Mdiag, torch.zeros(B, 2, 3, device=DEV), zeros + 0.5, zeros + 0.5, Je=None, dt=2.0 ** -5, maxc=4)


def test_world_overlap_reaches_v0_through_differentiable_steps():
    """After three differentiable steps the ball has drifted 3 dt v0 into the zone: d(area)/d(v0) of the ball is non-zero, points along
    the approach (+x), and agrees within 1e-6 relative with a central difference over two re-run roll-outs at v0x -+ 2^-4 (the step in
    the pose, 3 dt 2^-4 = 0.006, leaves a truncation of that squared times the third derivative, about 1 / r^2, over 6: 1e-7 relative)."""
    from lcp_physics_amd.physics.overlap import pair_overlaps
    from lcp_physics_amd.physics.proximity import PairSet
    base = torch.tensor([[0.0, 16.0, 2.0], [0.0, 0.0, 0.0]], dtype=torch.float32, device=DEV).repeat(2, 1, 1)
    pairs = PairSet.all_pairs(2, 2).to(DEV)

    def rollout(v0, differentiable):
        world = _zone_world(v0)
        if not differentiable:
            assert torch.equal(world.overlap(pairs), pair_overlaps(world.geom, world.p, pairs))        # a plain world
        for _ in range(3):
            world.step(differentiable=differentiable)
        assert int(world.contacts.count.sum()) == 0                                       # the zone collides with nothing
        return world.overlap(pairs)

    v0 = base.clone().requires_grad_(True)
    area = rollout(v0, True)
    assert area.requires_grad and float(area.detach().min()) > 1.0
    area.sum().backward()
    g = v0.grad.double().cpu()
    h = 2.0 ** -4
    up, dn = base.clone(), base.clone()
    up[:, 0, 1] += h
    dn[:, 0, 1] -= h
    with torch.no_grad():
        fd = ((rollout(up, False) - rollout(dn, False)).sum(1) / (2 * h)).cpu()
    print("d area / d v0 of the ball", g[:, 0].tolist(), " central difference in x", fd.tolist())
    assert bool(torch.isfinite(g).all()) and bool((g[:, 0, 1] > 0).all())                 # non-zero, along the approach
    assert float(((g[:, 0, 1] - fd).abs() / fd.abs()).max()) <= 1e-6


# ------------------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_are_refused_before_any_launch():
    L = _lib()
    lib, c = L.load(), OH.case("small")
    d, args = _inputs(c)
    B, P = c["pair_first"].shape
    area = torch.full((B, P), NAN, dtype=F64, device=DEV)
    g = torch.zeros(B, P, dtype=F64, device=DEV)
    g_p = torch.full(c["p"].shape, NAN, dtype=F64, device=DEV)
    stream = L.stream_ptr(torch.device(DEV))
    fwd = lambda a, out=True: lib.lcp_pair_overlap_f64(*a, L.ptr(area) if out else None, stream)
    bwd = lambda a, out=True: lib.lcp_pair_overlap_backward_f64(*a, L.ptr(g), L.ptr(g_p) if out else None, None, None, stream)
    with_size = lambda k, v: args[:k] + [v] + args[k + 1:]
    bad = [with_size(0, -1), with_size(4, 0), with_size(4, 1025), with_size(1, 0), with_size(1, 65), with_size(2, 7), with_size(2, 65),
           with_size(3, -1), with_size(3, 1025)] + [with_size(k, None) for k in range(5, 12)]     # sizes; every array NULL in turn
    for a in bad:
        assert fwd(a) == -1 and bwd(a) == -1
    assert fwd(args, out=False) == -1 and bwd(args, out=False) == -1                      # no output
    assert lib.lcp_pair_overlap_backward_f64(*args, None, L.ptr(g_p), None, None, stream) == -1        # g_area = NULL
    assert fwd(with_size(0, 0)) == 0 and bwd(with_size(0, 0)) == 0                        # B = 0: success, no launch
    torch.cuda.synchronize()
    assert bool(torch.isnan(area).all()) and bool(torch.isnan(g_p).all())                 # nothing was written
    assert fwd(args) == 0 and bwd(args) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(area).any()) and not bool(torch.isnan(g_p).any())


def test_host_side_refusals():
    from lcp_physics_amd.physics.overlap import pair_overlaps
    from lcp_physics_amd.physics.proximity import PairSet
    c = OH.case("small")
    geom, p, pairs = _geom(c)
    cpu = lambda q: PairSet(q.first.cpu(), q.second.cpu(), q.max_dist.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pair_overlaps(geom, p.cpu(), pairs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pair_overlaps(geom, p, cpu(pairs))
    with pytest.raises(ValueError, match="scenes"):
        pair_overlaps(geom, p, PairSet(pairs.first[:2], pairs.second[:2], pairs.max_dist[:2]))
    with pytest.raises(ValueError, match="must be"):
        pair_overlaps(geom, p[:, :2].contiguous(), pairs)
    with pytest.raises(RuntimeError, match="must be"):
        pair_overlaps(geom, p.float(), pairs)
