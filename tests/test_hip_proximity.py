"""GPU: the proximity query of lcp_proximity.hip (lcp_pair_distance_f64, lcp_pair_distance_backward_f64; physics/proximity.py) against
the host mirror tests/proximity_host.py, which tests/test_proximity_host.py checks on the CPU.

Tolerances are those of tests/test_hip_sensors.py for the matching quantities (the same fp64 arithmetic on the same coordinates of
order 100 to 1000): `dist` within 1e-9 on every pair, `normal` within 1e-9 and the witness points (coordinates, like a distance) within
1e-9 on the pairs the mirror can decide; clamped and invalid pairs exactly `max_dist` and zeros.  The comparison of witnesses and
gradients leaves out the pairs the mirror itself cannot decide (`excluded`: a second candidate feature within 1e-9, or max(sep_A, sep_B)
within 1e-9 of 0; at most 2 % of a case, asserted on the CPU) - except in `stack`, where parallel faces tie on purpose and only what
every tied feature shares is compared.  The backward takes the reference's cotangent, which is zero on the excluded pairs: every
gradient within 1e-8 of the mirror's autograd, relative to the array's largest entry."""
import pytest
import torch

from tests import proximity_host as PH

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, I32 = torch.float64, torch.int32
SCENE = ("kind", "radius", "verts_local", "nverts", "p")
PAIRS = ("pair_first", "pair_second", "pair_max_dist")
INF = float("inf")


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
    d = {k: c[k].to(DEV).contiguous() for k in SCENE + PAIRS}
    return d, _sizes(c, svm) + [_lib().ptr(d[k]) for k in SCENE + PAIRS]


def _forward(c, svm=None, only_dist=False):
    """The raw entry into outputs pre-filled with NaN: dist, normal, w1, w2 (CPU); `only_dist`: the other three NULL."""
    L = _lib()
    d, args = _inputs(c, svm)
    B, P = c["pair_first"].shape
    outs = [torch.full((B, P) + ((2,) if k else ()), float("nan"), dtype=F64, device=DEV) for k in range(4)]
    ptrs = [L.ptr(o) if (k == 0 or not only_dist) else None for k, o in enumerate(outs)]
    rc = L.load().lcp_pair_distance_f64(*args, *ptrs, L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    return tuple(o.cpu() for o in outs)


def _backward(c, g_dist, svm=None):
    """The raw entry into outputs pre-filled with NaN: the three gradients (CPU), keyed as proximity_host.LEAVES."""
    L = _lib()
    d, args = _inputs(c, svm)
    g = g_dist.to(DEV).contiguous()
    outs = [torch.full(c[k].shape, float("nan"), dtype=F64, device=DEV) for k in PH.LEAVES]
    rc = L.load().lcp_pair_distance_backward_f64(*args, L.ptr(g), *[L.ptr(o) for o in outs], L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    return {k: o.cpu() for k, o in zip(PH.LEAVES, outs)}


_FWD = {}


def _fwd(name):
    if name not in _FWD:
        _FWD[name] = _forward(PH.case(name))
    return _FWD[name]


# ------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("name", PH.CASE_NAMES)
def test_forward_matches_the_mirror(name):
    ref, c = PH.reference(name), PH.case(name)
    dist, normal, w1, w2 = _fwd(name)
    live, md = ref["live"], c["pair_max_dist"]
    keep = live & ~ref["excluded"]
    if name in PH.GENERIC:
        assert int(ref["excluded"].sum()) <= 0.02 * keep.numel()                          # (the mirror alone: test_proximity_host.py too)
    assert not bool(torch.isnan(dist).any()) and all(bool(torch.isfinite(t).all()) for t in (normal, w1, w2))       # written, everywhere
    # clamped and invalid pairs: exactly max_dist and zeros
    assert torch.equal(dist[~live], md[~live])
    assert _absmax(normal[~live]) == 0.0 and _absmax(w1[~live]) == 0.0 and _absmax(w2[~live]) == 0.0
    assert bool((dist[live] < md[live]).all())
    ed = _absmax((dist - ref["dist"])[live])                                              # (every pair, the undecided ones too)
    en = _absmax((normal - ref["normal"])[live if name == "stack" else keep])             # (stack: every tied feature has this normal)
    ew = max(_absmax((w1 - ref["w1"])[keep]), _absmax((w2 - ref["w2"])[keep]))
    ec = _absmax(((normal * (w2 - w1)).sum(-1) - dist)[live])
    print("%s: |dist - mirror| %.3g  |normal - mirror| %.3g  |witness - mirror| %.3g  |n . (w2 - w1) - dist| %.3g  excluded %d of %d" % (
        name, ed, en, ew, ec, int(ref["excluded"].sum()), keep.numel()))
    assert ed <= 1e-9 and en <= 1e-9 and ew <= 1e-9 and ec <= 1e-9


def test_the_pair_fixture_as_one_batch_of_600_scenes():
    """tests/golden/contacts_pairs.npz: dist = -max_k pen within the project's ATOL_PEN on the 543 pairs with a record, dist > eps = 0.1
    on the 57 without."""
    c, has, pen = PH.fixture_case()
    dist = _forward(c, only_dist=True)[0][:, 0]
    err = _absmax((dist + pen)[has])
    print("|dist + max pen| %.3g   smallest dist without a record %.4g" % (err, float(dist[~has].min())))
    assert int(has.sum()) == 543 and err <= 1e-9
    assert float(dist[~has].min()) > 0.1


# ------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("name", PH.CASE_NAMES)
def test_backward_matches_the_mirrors_autograd(name):
    ref, c = PH.reference(name), PH.case(name)
    got = _backward(c, ref["g_dist"])
    for k in PH.LEAVES:
        assert bool(torch.isfinite(got[k]).all()), k                                      # written, everywhere
    hull = c["kind"] != 0
    cap = c["verts_local"].shape[2]
    pad = torch.arange(cap).reshape(1, 1, cap) >= (c["nverts"] * hull).unsqueeze(2)
    assert _absmax(got["radius"][hull]) == 0.0 and _absmax(got["verts_local"][pad]) == 0.0
    if name == "stack":
        # parallel faces tie: the force on either body and the pair's total torque about the origin are the same for every tied feature
        want, gp, pose = ref["grads"]["p"], got["p"], c["p"]
        scale = float(want.abs().max())
        ef = _absmax((gp - want)[..., 1:])
        torque = lambda g: (g[..., 0] + pose[..., 1] * g[..., 2] - pose[..., 2] * g[..., 1]).sum(1)
        arm = float((pose[..., 1:].abs().max() * ref["g_dist"].abs().max()))             # the size of the terms that cancel
        et = _absmax(torque(gp) - torque(want))
        print("stack: |force difference| %.3g of %.3g   |torque difference| %.3g of %.3g" % (ef, scale, et, arm))
        assert ef <= 1e-8 * scale and et <= 1e-8 * arm
        return
    for k in PH.LEAVES:
        want = ref["grads"][k]
        err, scale = float((got[k] - want).abs().max()), float(want.abs().max())
        print("%s %s: |difference| %.3g of %.3g" % (name, k, err, scale))
        assert err <= 1e-8 * scale, k                                                     # (no circle in the case: radius exactly 0)
        assert scale > 0 or (k == "radius" and not bool((c["kind"] == 0).any())), k


@pytest.mark.parametrize("name", ["small", "wide", "big_hulls"])
def test_two_runs_of_the_backward_give_the_same_bits(name):
    c, g = PH.case(name), PH.reference(name)["g_dist"]
    a, b = _backward(c, g), _backward(c, g)
    for k in a:
        assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)), k


# ------------------------------------------------------------------------------------------------------------- independence
@pytest.mark.parametrize("name", ["small", "wide"])
def test_dist_does_not_depend_on_the_optional_outputs_or_on_the_cull(name):
    c = PH.case(name)
    dist = _fwd(name)[0]
    alone = _forward(c, only_dist=True)[0]
    assert torch.equal(alone.view(torch.int64), dist.view(torch.int64))
    # no cutoff at all: every pair that a finite max_dist left below it has the same bits
    free = _forward(dict(c, pair_max_dist=torch.full_like(c["pair_max_dist"], INF)), only_dist=True)[0]
    below = dist < c["pair_max_dist"]
    assert int((below & torch.isfinite(c["pair_max_dist"])).sum()) > 0
    assert torch.equal(free[below].view(torch.int64), dist[below].view(torch.int64))
    # and a cutoff that culls most pairs leaves the survivors alone
    cut = torch.full_like(c["pair_max_dist"], 20.0)
    tight = _forward(dict(c, pair_max_dist=cut), only_dist=True)[0]
    valid = torch.isfinite(free)                                                          # (an invalid pair returns its max_dist: inf)
    kept = valid & (free < 20.0)
    assert int(kept.sum()) > 0 and int((valid & ~kept).sum()) > 0
    assert torch.equal(tight[kept].view(torch.int64), free[kept].view(torch.int64)) and bool((tight[~kept] == 20.0).all())


def test_a_scene_over_the_vertex_limit_is_not_queried():
    c = PH.case("wide")
    dist, normal, w1, w2 = _forward(c, svm=1023)
    assert torch.equal(dist, c["pair_max_dist"]) and max(_absmax(normal), _absmax(w1), _absmax(w2)) == 0.0
    for k, g in _backward(c, PH.reference("wide")["g_dist"], svm=1023).items():
        assert float(g.abs().max()) == 0.0, k


# ------------------------------------------------------------------------------------------------------------- the autograd surface
def _geom(c, leaves=False):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.proximity import PairSet
    t = lambda k: c[k].to(DEV).contiguous()
    lf = (lambda k: t(k).requires_grad_(True)) if leaves else t
    geom = GeometryBatch(t("kind"), lf("radius"), lf("verts_local"), t("nverts"), None, _sizes(c)[3])
    return geom, lf("p"), PairSet(t("pair_first"), t("pair_second"), t("pair_max_dist"))


def test_pair_distances_returns_the_entrys_bits_and_its_backward_the_entrys_gradients():
    from lcp_physics_amd.physics.proximity import pair_distances
    c, ref = PH.case("small"), PH.reference("small")
    geom, p, pairs = _geom(c, leaves=True)
    out = pair_distances(geom, p, pairs, witnesses=True)
    want = _fwd("small")
    assert len(out) == 4 and all(torch.equal(a.detach().cpu(), b) for a, b in zip(out, want))
    assert out[0].requires_grad and not any(t.requires_grad for t in out[1:])
    alone = pair_distances(geom, p, pairs)
    assert isinstance(alone, torch.Tensor) and torch.equal(alone.detach().cpu(), want[0])
    out[0].backward(ref["g_dist"].to(DEV))
    raw = _backward(c, ref["g_dist"])
    for k, t in zip(PH.LEAVES, (p, geom.radius, geom.verts_local)):
        assert torch.equal(t.grad.cpu(), raw[k]), k
    # only what requires grad is asked for
    geom2, p2, pairs2 = _geom(c)
    p2.requires_grad_(True)
    pair_distances(geom2, p2, pairs2).backward(ref["g_dist"].to(DEV))
    assert torch.equal(p2.grad.cpu(), raw["p"]) and geom2.radius.grad is None and geom2.verts_local.grad is None


def _gradcheck_case():
    """Three bodies (a circle, a rect, a pentagon) and six pairs, every one decided by a wide margin: the circle apart from both hulls,
    the hulls overlapping, in both orders."""
    import numpy as np
    rng = np.random.default_rng(5)
    c = PH._assemble([[("circle", (0.2, 100.0, 92.0), 12.0), ("hull", (0.35, 150.0, 108.0), PH._rect(40.0, 30.0)),
                       ("hull", (0.8, 176.0, 128.0), PH._hull(rng, 5, 22.0, 20.0))]], 8)
    c.update(PH._pairs([[(0, 1, INF), (1, 0, INF), (0, 2, INF), (2, 0, 500.0), (1, 2, INF), (2, 1, INF)]]))
    return c


def test_gradcheck_at_three_bodies_and_six_pairs():
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.proximity import PairSet, pair_distances
    c = _gradcheck_case()
    out = PH.pairs_host(c)
    assert bool(out["live"].all()) and float(out["gap"].min()) > 0.5 and int((out["dist"] < 0).sum()) == 2     # far from every branch
    t = lambda k: c[k].to(DEV).contiguous()
    ins = [t(k).requires_grad_(True) for k in PH.LEAVES]

    def fn(p, radius, verts_local):
        geom = GeometryBatch(t("kind"), radius, verts_local, t("nverts"), None, _sizes(c)[3])
        return pair_distances(geom, p, PairSet(t("pair_first"), t("pair_second"), t("pair_max_dist")))

    assert torch.autograd.gradcheck(fn, ins, eps=1e-6, atol=1e-6, rtol=1e-6, nondet_tol=0.0)


def test_world_clearance_reaches_v0_through_differentiable_steps():
    """Two bodies in free flight (no forces, no joints, no contact): after five differentiable steps p = p0 + 5 dt v0, so the clearance's
    gradient with respect to the linear velocities is -+ 5 dt n.  The step's state is float32 (`v`) added into a float64 pose: five
    chained float32 updates and their backward carry a few float32 roundings (6e-8 each) on a value of 5 dt, hence 1e-5 relative."""
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.proximity import PairSet, pair_distances
    B, dt = 4, 1.0 / 30
    geom = GeometryBatch.from_shapes([("circle", 10.0), ("rect", (30.0, 20.0))], B).to(DEV)
    p0 = torch.tensor([[0.0, 100.0, 100.0], [0.4, 170.0, 130.0]], dtype=F64, device=DEV).repeat(B, 1, 1)
    p0[:, 1, 1] += torch.arange(B, dtype=F64, device=DEV) * 3.0
    v0 = torch.tensor([[0.1, 3.0, -2.0], [-0.2, -4.0, 1.0]], dtype=torch.float32, device=DEV).repeat(B, 1, 1).requires_grad_(True)
    Mdiag = torch.tensor([[50.0, 1.0, 1.0], [80.0, 2.0, 2.0]], dtype=torch.float32, device=DEV).repeat(B, 1, 1)
    zeros = torch.zeros(B, 2, dtype=torch.float32, device=DEV)
    world = ContactWorld(geom, p0, v0, Mdiag, torch.zeros(B, 2, 3, device=DEV), zeros + 0.5, zeros + 0.5, Je=None, dt=dt, maxc=4)
    pairs = PairSet.all_pairs(2, B).to(DEV)
    for a, b in zip(world.clearance(pairs, witnesses=True), pair_distances(world.geom, world.p, pairs, witnesses=True)):   # a plain world
        assert torch.equal(a, b)
    for _ in range(5):
        world.step(differentiable=True)
    dist, normal, _, _ = world.clearance(pairs, witnesses=True)
    assert dist.requires_grad and int(world.contacts.count.sum()) == 0 and float(dist.detach().min()) > 20.0
    dist.sum().backward()
    g, n = v0.grad.double().cpu(), normal[:, 0].cpu()
    want = 5 * dt * torch.stack([-n, n], 1)                                               # body 1 (first): -n, body 2: +n
    err = float((g[..., 1:] - want).abs().max())
    print("d dist / d v0", g[0].tolist(), " |linear - (-+ 5 dt n)| %.3g of %.3g" % (err, 5 * dt))
    assert bool(torch.isfinite(g).all()) and err <= 1e-5 * 5 * dt
    assert float(g[:, 1, 0].abs().max()) > 0.0                                            # the rect's turn moves its witness


# ------------------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_are_refused_before_any_launch():
    L = _lib()
    lib, c = L.load(), PH.case("small")
    d, args = _inputs(c)
    B, P = c["pair_first"].shape
    dist = torch.full((B, P), float("nan"), dtype=F64, device=DEV)
    g = torch.zeros(B, P, dtype=F64, device=DEV)
    g_p = torch.full(c["p"].shape, float("nan"), dtype=F64, device=DEV)
    stream = L.stream_ptr(torch.device(DEV))
    fwd = lambda a, out=True: lib.lcp_pair_distance_f64(*a, L.ptr(dist) if out else None, None, None, None, stream)
    bwd = lambda a, out=True: lib.lcp_pair_distance_backward_f64(*a, L.ptr(g), L.ptr(g_p) if out else None, None, None, stream)
    with_size = lambda k, v: args[:k] + [v] + args[k + 1:]
    bad = [with_size(0, -1), with_size(4, 0), with_size(4, 1025), with_size(1, 0), with_size(1, 65), with_size(2, 7), with_size(2, 65),
           with_size(3, -1), with_size(3, 1025)] + [with_size(k, None) for k in range(5, 13)]     # sizes; every array NULL in turn
    for a in bad:
        assert fwd(a) == -1 and bwd(a) == -1
    assert fwd(args, out=False) == -1 and bwd(args, out=False) == -1                      # no output
    assert lib.lcp_pair_distance_backward_f64(*args, None, L.ptr(g_p), None, None, stream) == -1       # g_dist = NULL
    assert fwd(with_size(0, 0)) == 0 and bwd(with_size(0, 0)) == 0                        # B = 0: success, no launch
    torch.cuda.synchronize()
    assert bool(torch.isnan(dist).all()) and bool(torch.isnan(g_p).all())                 # nothing was written
    assert fwd(args) == 0 and bwd(args) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dist).any()) and not bool(torch.isnan(g_p).any())


def test_host_side_refusals():
    from lcp_physics_amd.physics.proximity import PairSet, pair_distances
    c = PH.case("small")
    f, s, md = c["pair_first"], c["pair_second"], c["pair_max_dist"]
    with pytest.raises(ValueError, match="positive"):
        PairSet(f, s, md.clone().index_fill_(1, torch.tensor([3]), 0.0))
    with pytest.raises(ValueError, match="positive"):
        PairSet.all_pairs(4, 2, max_dist=-5.0)
    with pytest.raises(ValueError, match="positive"):
        PairSet(f, s, md.clone().index_fill_(1, torch.tensor([3]), float("nan")))
    with pytest.raises(ValueError, match="must be"):
        PairSet(f, s[:, :5], md)
    with pytest.raises(ValueError, match="1 to 1024"):
        PairSet(f[:, :0], s[:, :0], md[:, :0])
    with pytest.raises(ValueError, match="1024"):
        PairSet.all_pairs(46, 1)                                                          # 1035 pairs (45 bodies: 990)
    with pytest.raises(ValueError, match="1024"):
        PairSet.between(range(33), range(32), 1)
    geom, p, pairs = _geom(c)
    cpu = lambda q: PairSet(q.first.cpu(), q.second.cpu(), q.max_dist.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pair_distances(geom, p.cpu(), pairs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pair_distances(geom, p, cpu(pairs))
    with pytest.raises(ValueError, match="scenes"):
        pair_distances(geom, p, PairSet(pairs.first[:2], pairs.second[:2], pairs.max_dist[:2]))


def test_the_pair_sets():
    from lcp_physics_amd.physics.proximity import PairSet
    ap = PairSet.all_pairs(4, 3, max_dist=7.0)
    assert ap.first.tolist() == [[0, 0, 0, 1, 1, 2]] * 3 and ap.second.tolist() == [[1, 2, 3, 2, 3, 3]] * 3      # the contact list's order
    assert ap.first.dtype == I32 and ap.max_dist.dtype == F64 and ap.max_dist.tolist() == [[7.0] * 6] * 3 and (ap.B, ap.P) == (3, 6)
    assert PairSet.all_pairs(45, 1).P == 990 and bool(torch.isinf(PairSet.all_pairs(3, 1).max_dist).all())
    bt = PairSet.between([0, 5], [1, 2, 3], 2)
    assert bt.first.tolist() == [[0, 0, 0, 5, 5, 5]] * 2 and bt.second.tolist() == [[1, 2, 3, 1, 2, 3]] * 2
    on = ap.to(DEV)
    assert on.first.is_cuda and on.second.is_cuda and on.max_dist.is_cuda and on.first.is_contiguous()
