"""GPU: the ray caster of lcp_sensors.hip (lcp_cast_rays_f64, lcp_cast_rays_backward_f64; physics/sensors.py) against the host mirror
tests/sensors_host.py, which tests/test_sensors_host.py checks on the CPU.

The comparison leaves out the rays the mirror itself cannot decide (`excluded`: |n . u| < 0.05 at the hit, or two nearest candidate
distances within 1e-9; at most 2 % of a case, asserted on the CPU).  On the others: `dist` within 1e-9 (fp64 rounding of about 1e-16
on coordinates up to 1e3, amplified by 1 / |n . u| <= 20 over a handful of operations, is about 1e-11; 1e-9 leaves two orders),
`hit` equal, `normal` within 1e-9.  The backward takes the reference's cotangent, which is zero on the excluded rays, so that they
reach no gradient on either side: every gradient within 1e-8 of the mirror's autograd, relative to the array's largest entry."""
import pytest
import torch

from tests import sensors_host as SH

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, I32 = torch.float64, torch.int32
SCENE = ("kind", "radius", "verts_local", "nverts", "p")
RAYS = ("ray_body", "ray_origin", "ray_angle", "ray_range")


def _lib():
    from lcp_physics_amd import _lib as L
    return L


def _absmax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _sizes(c, svm=None):
    B, nb, cap = c["verts_local"].shape[:3]
    nv = torch.where(c["kind"] != 0, c["nverts"].clamp(0, cap), torch.zeros_like(c["nverts"]))
    return [B, nb, cap, int(nv.sum(1).max()) if svm is None else svm, c["ray_body"].shape[1]]


def _inputs(c, svm=None):
    d = {k: c[k].to(DEV).contiguous() for k in SCENE + RAYS}
    return d, _sizes(c, svm) + [_lib().ptr(d[k]) for k in SCENE + RAYS]


def _forward(c, svm=None):
    """The raw entry into outputs pre-filled with NaN / -7: dist, hit, normal (CPU)."""
    L = _lib()
    d, args = _inputs(c, svm)
    B, R = c["ray_body"].shape
    dist = torch.full((B, R), float("nan"), dtype=F64, device=DEV)
    hit = torch.full((B, R), -7, dtype=I32, device=DEV)
    normal = torch.full((B, R, 2), float("nan"), dtype=F64, device=DEV)
    rc = L.load().lcp_cast_rays_f64(*args, L.ptr(dist), L.ptr(hit), L.ptr(normal), L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    return dist.cpu(), hit.cpu(), normal.cpu()


def _backward(c, g_dist, svm=None):
    """The raw entry into outputs pre-filled with NaN: the five gradients (CPU), keyed as sensors_host.LEAVES."""
    L = _lib()
    d, args = _inputs(c, svm)
    g = g_dist.to(DEV).contiguous()
    outs = [torch.full(c[k].shape, float("nan"), dtype=F64, device=DEV) for k in SH.LEAVES]
    rc = L.load().lcp_cast_rays_backward_f64(*args, L.ptr(g), *[L.ptr(o) for o in outs], L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    return {k: o.cpu() for k, o in zip(SH.LEAVES, outs)}


_FWD = {}


def _fwd(name):
    if name not in _FWD:
        _FWD[name] = _forward(SH.case(name))
    return _FWD[name]


@pytest.mark.parametrize("name", SH.CASE_NAMES)
def test_forward_matches_the_mirror(name):
    ref = SH.reference(name)
    dist, hit, normal = _fwd(name)
    keep = ~ref["excluded"]
    assert int((~keep).sum()) <= 0.02 * keep.numel()                                      # (the mirror alone: test_sensors_host.py too)
    assert bool(torch.isfinite(dist).all()) and bool(torch.isfinite(normal).all()) and int(hit.min()) >= -1      # written, everywhere
    ed = float((dist - ref["dist"]).abs()[keep].max())
    en = float((normal - ref["normal"]).abs()[keep].max())
    print("%s: |dist - mirror| %.3g  |normal - mirror| %.3g  hit mismatches %d  excluded %d of %d" % (
        name, ed, en, int((hit != ref["hit"])[keep].sum()), int((~keep).sum()), keep.numel()))
    assert ed <= 1e-9 and en <= 1e-9 and torch.equal(hit[keep], ref["hit"][keep])
    # a miss is the range itself and no normal; an origin inside is 0 and no normal
    rng = SH.case(name)["ray_range"]
    assert torch.equal(dist[hit < 0], rng[hit < 0]) and float(normal[(hit < 0) | (dist == 0)].abs().max()) == 0.0


def test_the_named_rays_of_small():
    """The vertex ray is one the mirror cannot decide (two entering edges tie: which normal is rounding); its distance and its body are
    decided, and are compared here."""
    ref, nm = SH.reference("small"), SH.case("small")["names"]
    dist, hit, normal = _fwd("small")
    for r in nm.values():
        assert torch.equal(hit[:, r], ref["hit"][:, r]) and float((dist[:, r] - ref["dist"][:, r]).abs().max()) <= 1e-9, r
    assert hit[:, nm["parallel_outside"]].tolist() == [-1] * 3 and hit[:, nm["parallel_between"]].tolist() == [1] * 3
    assert torch.equal(normal[:, nm["parallel_between"]], torch.tensor([[-1.0, 0.0]] * 3, dtype=F64))
    assert int((hit == 4).sum()) == 0                                                     # the two-vertex hull


@pytest.mark.parametrize("name", SH.CASE_NAMES)
def test_backward_matches_the_mirrors_autograd(name):
    ref, c = SH.reference(name), SH.case(name)
    got = _backward(c, ref["g_dist"])
    for k in SH.LEAVES:
        want = ref["grads"][k]
        assert bool(torch.isfinite(got[k]).all()), k                                      # written, everywhere
        err, scale = float((got[k] - want).abs().max()), float(want.abs().max())
        print("%s %s: |difference| %.3g of %.3g" % (name, k, err, scale))
        assert err <= 1e-8 * scale, k                                                     # (no circle in the case: radius exactly 0)
        assert scale > 0 or (k == "radius" and not bool((c["kind"] == 0).any())), k
    still = ((ref["hit"] < 0) | (ref["dist"] == 0)) & ~ref["excluded"]                  # misses, clamped rays, origins inside
    assert int(still.sum()) > 0
    assert float(got["ray_origin"][still].abs().max()) == 0.0 and float(got["ray_angle"][still].abs().max()) == 0.0
    hull = c["kind"] != 0
    cap = c["verts_local"].shape[2]
    pad = torch.arange(cap).reshape(1, 1, cap) >= (c["nverts"] * hull).unsqueeze(2)
    assert _absmax(got["radius"][hull]) == 0.0 and _absmax(got["verts_local"][pad]) == 0.0


def test_a_scene_over_the_vertex_limit_is_not_sensed():
    c = SH.case("wide")
    dist, hit, normal = _forward(c, svm=1023)
    assert torch.equal(dist, c["ray_range"]) and int((hit != -1).sum()) == 0 and float(normal.abs().max()) == 0.0
    for k, g in _backward(c, SH.reference("wide")["g_dist"], svm=1023).items():
        assert float(g.abs().max()) == 0.0, k


@pytest.mark.parametrize("name", SH.CASE_NAMES)
def test_two_runs_of_the_backward_give_the_same_bits(name):
    c, g = SH.case(name), SH.reference(name)["g_dist"]
    a, b = _backward(c, g), _backward(c, g)
    for k in a:
        assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)), k


# ------------------------------------------------------------------------------------------------------------- the autograd surface
def _geom(c, leaves=False):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.sensors import RaySet
    t = lambda k: c[k].to(DEV).contiguous()
    lf = (lambda k: t(k).requires_grad_(True)) if leaves else t
    geom = GeometryBatch(t("kind"), lf("radius"), lf("verts_local"), t("nverts"), None, _sizes(c)[3])
    rays = RaySet(t("ray_body"), lf("ray_origin"), lf("ray_angle"), t("ray_range"))
    return geom, lf("p"), rays


def test_cast_rays_returns_the_entrys_bits_and_its_backward_the_entrys_gradients():
    from lcp_physics_amd.physics.sensors import cast_rays
    c, ref = SH.case("small"), SH.reference("small")
    geom, p, rays = _geom(c, leaves=True)
    dist, hit, normal = cast_rays(geom, p, rays, normals=True)
    want = _fwd("small")
    assert torch.equal(dist.detach().cpu(), want[0]) and torch.equal(hit.cpu(), want[1]) and torch.equal(normal.cpu(), want[2])
    assert dist.requires_grad and not hit.requires_grad and not normal.requires_grad
    assert len(cast_rays(geom, p, rays)) == 2
    dist.backward(ref["g_dist"].to(DEV))
    raw = _backward(c, ref["g_dist"])
    for k, t in zip(SH.LEAVES, (p, geom.radius, geom.verts_local, rays.origin, rays.angle)):
        assert torch.equal(t.grad.cpu(), raw[k]), k
    # only what requires grad is asked for
    geom2, p2, rays2 = _geom(c)
    p2.requires_grad_(True)
    cast_rays(geom2, p2, rays2)[0].backward(ref["g_dist"].to(DEV))
    assert torch.equal(p2.grad.cpu(), raw["p"]) and rays2.origin.grad is None


def test_gradcheck_at_six_rays_and_three_bodies():
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.sensors import RaySet, cast_rays
    c = SH.case("tiny")                                                                   # every ray a clean hit, far from a branch
    assert c["ray_body"].shape[1] == 6 and c["kind"].shape[1] == 3
    t = lambda k: c[k].to(DEV).contiguous()
    ins = [t(k).requires_grad_(True) for k in SH.LEAVES]

    def fn(p, radius, verts_local, origin, angle):
        geom = GeometryBatch(t("kind"), radius, verts_local, t("nverts"), None, _sizes(c)[3])
        return cast_rays(geom, p, RaySet(t("ray_body"), origin, angle, t("ray_range")))[0]

    assert torch.autograd.gradcheck(fn, ins, eps=1e-6, atol=1e-6, rtol=1e-6, nondet_tol=0.0)


def test_world_sense_reaches_v0_through_differentiable_steps():
    """A ball over a floor (the scene of tests/test_hip_render.py::_world): after two differentiable steps the readings of a fan
    mounted on the ball are part of the roll-out's graph."""
    import numpy as np
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.sensors import RaySet, cast_rays
    from tests.test_hip_bodies import _rollout_bodies, _rollout_fixture
    d, B = _rollout_fixture(), 4
    t64 = lambda a: torch.tensor(a, dtype=F64)
    bb = _rollout_bodies(d, B, t64(float(d["ball_rad"])), t64(d["box_verts_raw"]), t64(float(d["mass"][0])), t64(float(d["mass"][1])))
    v0 = bb.v0.detach().clone().requires_grad_(True)
    f = bb.f_gravity.clone()
    f[:, 0] = 0.0                                                                         # the floor is held by Je and carries no gravity
    Je = torch.tensor(np.repeat(d["Je"][:1], B, axis=0), dtype=torch.float32, device=DEV)
    world = ContactWorld(bb.geom, bb.p0.detach().clone(), v0, bb.Mdiag, f, bb.rest, bb.fric, Je=Je, dt=float(d["dt"]), maxc=8)
    rays = RaySet.fan(1, 16, 6.0, 2000.0, B).to(DEV)
    free = RaySet.fan(-1, 16, 6.0, 2000.0, B, origin=(float(d["ball_pos"].reshape(-1)[-2]), float(d["ball_pos"].reshape(-1)[-1]))).to(DEV)
    for a, b in zip(world.sense(free, normals=True), cast_rays(world.geom, world.p, free, normals=True)):      # a plain world
        assert torch.equal(a, b)
    for _ in range(2):
        world.step(differentiable=True)
    dist, hit = world.sense(rays)
    assert dist.requires_grad and int((hit == 0).sum()) > 0                               # the floor is seen
    dist.sum().backward()
    g = v0.grad.cpu()
    print("d sum(dist) / d v0", g[0].tolist())
    assert bool(torch.isfinite(g).all()) and float(g[:, 1].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_are_refused_before_any_launch():
    L = _lib()
    lib, c = L.load(), SH.case("small")
    d, args = _inputs(c)
    B, R = c["ray_body"].shape
    dist = torch.full((B, R), float("nan"), dtype=F64, device=DEV)
    g = torch.zeros(B, R, dtype=F64, device=DEV)
    g_p = torch.full(c["p"].shape, float("nan"), dtype=F64, device=DEV)
    stream = L.stream_ptr(torch.device(DEV))
    fwd = lambda a, out=True: lib.lcp_cast_rays_f64(*a, L.ptr(dist) if out else None, None, None, stream)
    bwd = lambda a, out=True: lib.lcp_cast_rays_backward_f64(*a, L.ptr(g), L.ptr(g_p) if out else None, None, None, None, None, stream)
    with_size = lambda k, v: args[:k] + [v] + args[k + 1:]
    bad = [with_size(4, 0), with_size(4, 1025), with_size(1, 65), with_size(9, None)]     # R = 0, R = 1025, nb = 65, p = NULL
    for a in bad:
        assert fwd(a) == -1 and bwd(a) == -1
    assert fwd(args, out=False) == -1 and bwd(args, out=False) == -1                      # no output
    assert lib.lcp_cast_rays_backward_f64(*args, None, L.ptr(g_p), None, None, None, None, stream) == -1      # g_dist = NULL
    assert fwd(with_size(0, 0)) == 0 and bwd(with_size(0, 0)) == 0                        # B = 0: success, no launch
    torch.cuda.synchronize()
    assert bool(torch.isnan(dist).all()) and bool(torch.isnan(g_p).all())                 # nothing was written
    assert fwd(args) == 0 and bwd(args) == 0


def test_host_side_refusals():
    from lcp_physics_amd.physics.sensors import RaySet, cast_rays
    c = SH.case("small")
    with pytest.raises(ValueError, match="positive"):
        RaySet(c["ray_body"], c["ray_origin"], c["ray_angle"], c["ray_range"].clone().index_fill_(1, torch.tensor([3]), 0.0))
    with pytest.raises(ValueError, match="positive"):
        RaySet.fan(-1, 4, 1.0, -5.0, 2)
    geom, p, rays = _geom(c)
    cpu = lambda r: RaySet(r.body.cpu(), r.origin.cpu(), r.angle.cpu(), r.range.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cast_rays(geom, p.cpu(), rays)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cast_rays(geom, p, cpu(rays))
