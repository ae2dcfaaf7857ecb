"""GPU: the mechanism links of lcp_links.hip (lcp_link_jacobian_f64, lcp_link_jacobian_backward_f64; physics/links.py;
`ContactWorld(links=...)`) against the host mirror tests/links_host.py, which tests/test_links_host.py checks on the CPU, and against
worlds held by the code that was there before: a constant `Je` and a `JointSet`.

Forward: every entry of Je is the float32 rounding of the mirror's float64 value to within one float32 ulp, structural zeros are exact
zeros, base rows are Je_base's bits.  Backward: see `BACKWARD_GATE`.  Worlds: see the tests' docstrings; every margin there is measured
in the test itself on the code from before (a one-ulp perturbation of a `JointSet` world's Je, that world's own equality residual)."""
import math

import pytest
import torch

from tests import links_host as LH

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32, I32 = torch.float64, torch.float32, torch.int32
NAN = float("nan")
BASES = ("none", "floor", "joint")
# The backward against the mirror's autograd, |got - want| relative to the largest gradient entry of the case, over all cases and bases.
# Measured once on an MI355X: the largest is 3.45e-16 (see test_backward_matches_the_mirrors_autograd); the gate is 8 times that.
BACKWARD_GATE = 8 * 3.45e-16


def _lib():
    from lcp_physics_amd import _lib as L
    return L


def _absmax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _one_ulp(got, want64):
    """`got` (float32) is the float32 rounding of `want64` or one of its two float32 neighbours."""
    w = want64.to(F32)
    inf = torch.full_like(w, float("inf"))
    return (got == w) | (got == torch.nextafter(w, inf)) | (got == torch.nextafter(w, -inf))


_BASE_CACHE = {}


def _base(name, how):
    """The rows above the links' (GPU, float32) and their random cotangent: none, three constant rows that pin body 0 (the floor of
    the demo worlds), or the two rows of a `JointSet` with one revolute joint at the case's pose."""
    key = (name, how)
    if key not in _BASE_CACHE:
        c = LH.case(name)
        B, nb = c["p"].shape[:2]
        if how == "none":
            base = None
        elif how == "floor":
            base = torch.zeros(B, 3, 3 * nb, dtype=F32)
            base[:, :, :3] = torch.eye(3)
            base = base.to(DEV)
        else:
            from lcp_physics_amd.physics.joints import JointSet
            js = JointSet.from_list([("joint", 0, None, (1.5, -2.5))], c["p"]).to(DEV)
            base = js.jacobian(c["p"].to(DEV).contiguous())
            assert base.shape == (B, 2, 3 * nb)
        e0 = 0 if base is None else base.shape[1]
        g0 = torch.randn(B, e0, 3 * nb, generator=torch.Generator().manual_seed(3), dtype=F64).to(F32)
        _BASE_CACHE[key] = (base, g0)
    return _BASE_CACHE[key]


def _inputs(c, e0):
    d = {k: c[k].to(DEV).contiguous() for k in LH.LINK_ARRAYS + ("p",)}
    B, nb = c["p"].shape[:2]
    return d, [B, nb, c["kind"].shape[1], e0, LH.el_of(c["kind"])] + [_lib().ptr(d[k]) for k in LH.LINK_ARRAYS + ("p",)]


def _forward(name, how="none"):
    """The raw entry into a matrix pre-filled with NaN: Je (CPU) and the base it was given (CPU, or None)."""
    L = _lib()
    c = LH.case(name)
    base, _ = _base(name, how)
    e0 = 0 if base is None else base.shape[1]
    d, args = _inputs(c, e0)
    out = torch.full((args[0], e0 + args[4], 3 * args[1]), NAN, dtype=F32, device=DEV)
    rc = L.load().lcp_link_jacobian_f64(*args, L.ptr(base), L.ptr(out), L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    return out.cpu(), None if base is None else base.cpu()


def _backward(name, how="none", absent=()):
    """The raw entry into outputs pre-filled with NaN: the four gradients (CPU) keyed as links_host.LEAVES; `absent`: NULL."""
    L = _lib()
    c = LH.case(name)
    base, g0 = _base(name, how)
    d, args = _inputs(c, g0.shape[1])
    gJe = torch.cat([g0, c["g_Je"]], 1).to(DEV).contiguous()
    outs = {n: (None if n in absent else torch.full(c[n].shape, NAN, dtype=F64, device=DEV)) for n in LH.LEAVES}
    rc = L.load().lcp_link_jacobian_backward_f64(*args, L.ptr(gJe), *[L.ptr(outs[n]) for n in LH.LEAVES], L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    return {n: o.cpu() for n, o in outs.items() if o is not None}


# ------------------------------------------------------------------------------------------------------------- the entries
@pytest.mark.parametrize("how", BASES)
@pytest.mark.parametrize("name", LH.CASE_NAMES)
def test_forward_matches_the_mirror(name, how):
    ref = LH.reference(name)
    out, base = _forward(name, how)
    assert bool(torch.isfinite(out).all())                                                 # written, everywhere
    e0 = 0 if base is None else base.shape[1]
    if e0:
        assert _bits(out[:, :e0], base)                                                    # base rows: Je_base's bits
    rows = out[:, e0:]
    ok = _one_ulp(rows, ref["Je"])
    assert bool(ok.all()), (int((~ok).sum()), "entries off by more than one float32 ulp; first", (~ok).nonzero()[0].tolist())
    assert bool((rows[~ref["struct"]].view(I32) == 0).all())                               # structural zeros: +0.0
    assert bool((rows[~ref["live"]].view(I32) == 0).all())                                 # dead links keep their rows, all zero
    assert _absmax(rows) > 0.5
    assert _bits(_forward(name, how)[0], out)


@pytest.mark.parametrize("how", BASES)
@pytest.mark.parametrize("name", LH.CASE_NAMES)
def test_backward_matches_the_mirrors_autograd(name, how):
    """Every output against the mirror's autograd through its autograd Jacobian, |got - want| relative to the largest entry of the
    case's four gradients - one scale per case, because they are derivatives of one scalar built from the same products, and an output
    that is zero by the formulas (a slot's g_a2, a rod's g_phi) is 1e-17 of rounding in the mirror and exactly 0 in the kernel.
    Measured on an MI355X over the 7 cases x 3 bases (the base rows' cotangent must not leak into the links'): between 1.2e-16
    ("many_scenes") and 3.45e-16 ("one_slot"), the float64 roundings of a dozen products; the same figure with each base.
    `BACKWARD_GATE` is 8 times the largest, far below the 1e-9 at which the difference would be a defect of the formulas."""
    c, ref = LH.case(name), LH.reference(name)
    got = _backward(name, how)
    worst = 0.0
    line = []
    scale = max(_absmax(ref["grads"][n]) for n in LH.LEAVES)
    for n in LH.LEAVES:
        assert bool(torch.isfinite(got[n]).all()), n                                       # written, everywhere
        err = _absmax(got[n] - ref["grads"][n])
        worst = max(worst, err / scale)
        line.append("%s %.2g of %.3g" % (n, err, _absmax(ref["grads"][n])))
    print("%s / %s: |got - want| of max |want|:  %s   largest / %.3g = %.3g" % (name, how, "   ".join(line), scale, worst))
    assert BACKWARD_GATE <= 1e-9 and worst <= BACKWARD_GATE
    # bodies no live link names: exact zeros; links that wrote zeros or nothing: exact zeros
    B, nb = c["p"].shape[:2]
    named = ref["struct"].reshape(B, -1, nb, 3).any(dim=(1, 3))
    assert _absmax(got["p"][~named]) == 0.0
    if name == "mixed":
        assert not bool(named[:, 4].any())
    if name == "invalid":
        assert not bool(named[:, 2].any())
        dead = torch.tensor([1, 2, 3, 4, 5, 6, 7])
        assert all(_absmax(got[n][:, dead]) == 0.0 for n in ("a1", "a2", "phi")) and _absmax(got["a1"][:, 0]) > 0.0


@pytest.mark.parametrize("name", ["mixed", "many_scenes", "many_links"])
def test_two_runs_give_the_same_bits_whichever_outputs_are_asked_for(name):
    first, again = _backward(name, "floor"), _backward(name, "floor")
    for n in LH.LEAVES:
        assert _bits(first[n], again[n]), n
    for gone in LH.LEAVES:
        part = _backward(name, "floor", absent=(gone,))
        assert gone not in part
        for n in part:
            assert _bits(first[n], part[n]), (n, "without", gone)
    only_p = _backward(name, "floor", absent=("a1", "a2", "phi"))
    assert _bits(first["p"], only_p["p"])


def _case_set(name):
    from lcp_physics_amd.physics.links import LinkSet
    c = LH.case(name)
    el = LH.el_of(c["kind"])
    d = {k: c[k].to(DEV).contiguous() for k in LH.LINK_ARRAYS + ("p",)}
    return LinkSet(*[d[k] for k in LH.LINK_ARRAYS], torch.zeros(c["p"].shape[0], el, dtype=F64, device=DEV), el), d


def test_the_autograd_surface_returns_the_entrys_bits_and_asks_only_for_required_gradients(monkeypatch):
    from lcp_physics_amd.physics.links import LinkSet, link_jacobian
    L = _lib()
    lib = L.load()
    ls, d = _case_set("mixed")
    base, g0 = _base("mixed", "joint")
    raw_f, _ = _forward("mixed", "joint")
    raw_g = _backward("mixed", "joint")
    gJe = torch.cat([g0, LH.case("mixed")["g_Je"]], 1).to(DEV)
    assert _bits(ls.jacobian(d["p"], Je_base=base).cpu(), raw_f)
    calls = []
    real = lib.lcp_link_jacobian_backward_f64

    def spy(*args):
        calls.append([a is not None for a in args[13:17]])
        return real(*args)

    monkeypatch.setattr(lib, "lcp_link_jacobian_backward_f64", spy, raising=False)

    def run(required):
        t = {n: d[n].clone().requires_grad_(n in required) for n in LH.LEAVES}
        b = base.clone().requires_grad_("base" in required)
        fs = LinkSet(ls.kind, ls.first, ls.second, t["a1"], t["a2"], t["phi"], ls.rest, ls.e)
        Je = link_jacobian(fs, t["p"], Je_base=b)
        assert Je.dtype == F32 and _bits(Je.detach().cpu(), raw_f)
        if required:
            Je.backward(gJe)
        return t, b

    t, b = run(LH.LEAVES + ("base",))
    assert calls == [[True] * 4]
    for n in LH.LEAVES:
        assert t[n].grad.dtype == F64 and _bits(t[n].grad.cpu(), raw_g[n]), n
    assert _bits(b.grad.cpu(), g0)                                                         # the base rows' cotangent, handed on
    t, b = run(("p", "phi"))
    assert calls[1] == [True, False, False, True] and b.grad is None and t["a1"].grad is None
    assert _bits(t["p"].grad.cpu(), raw_g["p"]) and _bits(t["phi"].grad.cpu(), raw_g["phi"])
    t, b = run(("base",))                                                                  # nothing of the kernel's: no launch
    assert len(calls) == 2 and _bits(b.grad.cpu(), g0)
    out = torch.full(raw_f.shape, NAN, dtype=F32, device=DEV)                              # the plain route: into the caller's buffer
    assert ls.jacobian(d["p"], Je_base=base, out=out) is out and _bits(out.cpu(), raw_f)


def test_bad_arguments_are_refused_before_any_launch():
    from lcp_physics_amd.physics.links import LinkSet
    L = _lib()
    lib = L.load()
    ls, d = _case_set("mixed")
    c = LH.case("mixed")
    _, args = _inputs(c, 0)
    args[5:] = [L.ptr(d[k]) for k in LH.LINK_ARRAYS + ("p",)]
    stream = L.stream_ptr(torch.device(DEV))
    B, nb, nl, _, el = args[:5]
    out = torch.full((B, el, 3 * nb), NAN, dtype=F32, device=DEV)
    g_p = torch.full((B, nb, 3), NAN, dtype=F64, device=DEV)
    gJe = c["g_Je"].to(DEV)
    fwd = lambda a, o=True, b=None: lib.lcp_link_jacobian_f64(*a, b, L.ptr(out) if o else None, stream)
    bwd = lambda a, g=True, o=True: lib.lcp_link_jacobian_backward_f64(*a, L.ptr(gJe) if g else None, L.ptr(g_p) if o else None,
                                                                       None, None, None, stream)
    with_arg = lambda k, v: args[:k] + [v] + args[k + 1:]
    for a in [with_arg(0, -1), with_arg(1, 0), with_arg(2, 0), with_arg(3, -1), with_arg(4, -1), with_arg(4, 2 * nl + 1)] + \
            [with_arg(k, None) for k in range(5, 12)]:
        assert fwd(a) == -1 and bwd(a) == -1
    for a in (with_arg(2, 257), with_arg(1, 65)):                                          # LCP_E_TOOLARGE: L > 256, nb > 64
        assert fwd(a) == -2 and bwd(a) == -2
    assert fwd(args, o=False) == -1 and fwd(with_arg(3, 2)) == -1 and bwd(args, g=False) == -1 and bwd(args, o=False) == -1
    assert fwd(with_arg(0, 0)) == 0 and bwd(with_arg(0, 0)) == 0                           # B == 0: accepted, nothing launched
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(g_p).all())
    assert fwd(args) == 0 and bwd(args) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g_p).all())
    # the host layer: more than 256 links, a wrong dtype, a wrong device, a non-contiguous input, a base of another shape
    many = lambda t: t[:, :1].repeat(1, 257, *([1] * (t.dim() - 2)))
    with pytest.raises(ValueError, match="256"):
        LinkSet(*[many(getattr(ls, n)) for n in LH.LINK_ARRAYS], torch.zeros(B, 257, dtype=F64, device=DEV), 257)
    with pytest.raises(RuntimeError):
        ls.jacobian(d["p"].float())
    with pytest.raises(RuntimeError):
        ls.jacobian(d["p"].cpu())
    with pytest.raises(RuntimeError):
        ls.jacobian(d["p"].transpose(0, 1).contiguous().transpose(0, 1))
    with pytest.raises(RuntimeError):
        LinkSet(ls.kind, ls.first, ls.second, ls.a1.transpose(0, 1).contiguous().transpose(0, 1), ls.a2, ls.phi, ls.rest, ls.e).jacobian(d["p"])
    with pytest.raises(ValueError):
        ls.jacobian(d["p"][:2])
    with pytest.raises(ValueError):
        ls.jacobian(d["p"], Je_base=torch.zeros(B, 3, 3 * nb + 3, dtype=F32, device=DEV))
    with pytest.raises(RuntimeError):
        ls.jacobian(d["p"], Je_base=torch.zeros(B, 3, 3 * nb, dtype=F64, device=DEV))


# ------------------------------------------------------------------------------------------------------------- worlds
DT = 1.0 / 30
PIN = (300.0, 30.0)
BOX = (20.0, 60.0)


def _world_parts(shapes, p0, mass, B):
    """Geometry, Mdiag and gravity of circles (radius 10) and boxes (20 x 60) at poses p0 [B,nb,3], masses [B,nb]."""
    from lcp_physics_amd import scenes
    from lcp_physics_amd.physics.contacts import GeometryBatch
    nb = len(shapes)
    inertia = torch.stack([mass[:, k] * (100.0 / 2 if s[0] == "circle" else (BOX[0] ** 2 + BOX[1] ** 2) / 12.0) for k, s in enumerate(shapes)], 1)
    Mdiag = torch.stack([inertia, mass, mass], -1)
    f = torch.zeros(B, nb, 3, dtype=F64)
    f[:, :, 2] = mass * scenes.GRAVITY
    geom = GeometryBatch.from_shapes(shapes, B)
    geom.no_contact = (torch.ones(B, nb, nb, dtype=torch.uint8) - torch.eye(nb, dtype=torch.uint8)).contiguous()
    half = torch.full((B, nb), 0.5, dtype=F32, device=DEV)
    return geom.to(DEV), Mdiag.to(F32).to(DEV), f.to(F32).to(DEV), half


def _pendulum(route, B=8, grad=False, **kw):
    """A box hung from the world point PIN, 40 below its pin at rest, every scene released at another angle and with another mass:
    `route` "joint" - a `JointSet` revolute joint (the code from before); "slots" - two world slots with t = (1, 0) and t = (0, 1)
    (tests/test_links_host.py::test_two_world_slots_are_the_revolute_joint_to_the_world).  Returns (world, leaves {p0, Mdiag})."""
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.joints import JointSet
    from lcp_physics_amd.physics.links import LinkSet
    th = torch.linspace(0.2, 1.2, B, dtype=F64)
    pin = torch.tensor(PIN, dtype=F64)
    centre = pin + 40.0 * torch.stack([torch.sin(th), torch.cos(th)], -1)
    p0 = torch.cat([(0.5 * th).unsqueeze(-1), centre], -1).unsqueeze(1)                    # [B,1,3]
    mass = (0.5 + torch.arange(B, dtype=F64) / (2 * B)).unsqueeze(1)
    geom, Mdiag, f, half = _world_parts([("rect", BOX)], p0, mass, B)
    leaves = {"p0": p0.to(DEV).clone(), "Mdiag": Mdiag.clone()}
    if grad:
        for t in leaves.values():
            t.requires_grad_(True)
    # both mechanisms are built from the leaf p0, so that in both the pin stays at PIN when p0 moves: the JointSet keeps the graph of
    # its polar anchor (constraints.py:21-23), the slots' body-frame anchor is R(rot)^T (PIN - c) of the same leaf
    q0 = leaves["p0"]
    if route == "joint":
        kw["joints"] = JointSet.from_list([("joint", 0, None, PIN)], q0, B)
    else:
        rot = q0[:, 0, 0]
        dx, dy = PIN[0] - q0[:, 0, 1], PIN[1] - q0[:, 0, 2]
        arm = torch.stack([torch.cos(rot) * dx + torch.sin(rot) * dy, -torch.sin(rot) * dx + torch.cos(rot) * dy], -1)
        kw["links"] = LinkSet.from_list([("slot", 0, None, arm, PIN, -math.pi / 2), ("slot", 0, None, arm, PIN, 0.0)], q0, B)
    world = ContactWorld(geom, leaves["p0"], torch.zeros(B, 1, 3, dtype=F32, device=DEV), leaves["Mdiag"], f, half, half, dt=DT, maxc=4,
                         **kw)
    return world, leaves


def _rod_world(B=2, hinged=False, as_constant=False, **kw):
    """`hinged=False`: a circle on a rod of length 40 to the world point PIN, released 0.5 rad (and, per scene, a little more) from the
    vertical.  `hinged=True`: the box of `_pendulum` on its `JointSet` joint, and the circle on a rod from the box's lower end to its
    own centre - a double pendulum held by a JointSet and a link together.  `as_constant`: the world is given the links' rows at the
    starting pose as a constant `Je` instead.  Returns (world, p0 on the device, the LinkSet)."""
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.joints import JointSet
    from lcp_physics_amd.physics.links import LinkSet
    th = 0.5 + 0.1 * torch.arange(B, dtype=F64)
    pin = torch.tensor(PIN, dtype=F64)
    mass = 0.8 + 0.3 * torch.arange(B, dtype=F64).unsqueeze(1)
    if not hinged:
        centre = pin + 40.0 * torch.stack([torch.sin(th), torch.cos(th)], -1)
        p0 = torch.cat([torch.zeros(B, 1, dtype=F64), centre], -1).unsqueeze(1)
        shapes = [("circle", 10.0)]
        ls = LinkSet.from_list([("distance", 0, None, (0.0, 0.0), PIN)], p0, B).to(DEV)
    else:
        box_c = pin + torch.tensor([0.0, 30.0], dtype=F64)                                 # the box hangs straight, pinned at its upper end
        low = box_c + torch.tensor([0.0, 30.0], dtype=F64)
        centre = low + 40.0 * torch.stack([torch.sin(th), torch.cos(th)], -1)
        p0 = torch.stack([torch.cat([torch.zeros(B, 1, dtype=F64), box_c.expand(B, 2)], -1),
                          torch.cat([torch.zeros(B, 1, dtype=F64), centre], -1)], 1)
        shapes = [("rect", BOX), ("circle", 10.0)]
        mass = mass.expand(B, 2).contiguous()
        ls = LinkSet.from_list([("distance", 1, 0, (0.0, 0.0), (0.0, 30.0))], p0, B).to(DEV)
        kw["joints"] = JointSet.from_list([("joint", 0, None, PIN)], p0, B).to(DEV)
    geom, Mdiag, f, half = _world_parts(shapes, p0, mass, B)
    p0 = p0.to(DEV)
    if as_constant:
        kw["Je"] = ls.jacobian(p0.contiguous())
    else:
        kw["links"] = ls
    world = ContactWorld(geom, p0.clone(), torch.zeros(B, len(shapes), 3, dtype=F32, device=DEV), Mdiag, f, half, half, dt=DT, maxc=4, **kw)
    return world, p0, ls


def test_a_plain_step_equals_the_step_of_a_world_given_the_same_rows_as_a_constant():
    """`ContactWorld(links=ls)` against `ContactWorld(Je=ls.jacobian(p0))`: the same solver sees the same matrix, so `v_new` and `p`
    are bit-identical after one step (not after two: the constant rows stay behind)."""
    (wl, p0, ls), (wc, _, _) = _rod_world(), _rod_world(as_constant=True)
    assert wl.e == wc.e == 1 and _bits(wl.Je.cpu(), wc.Je.cpu()) and not wl._pinned and not wc._pinned
    rl, rc = wl.step(), wc.step()
    assert _bits(rl["v_new"].cpu(), rc["v_new"].cpu()) and _bits(wl.p.cpu(), wc.p.cpu()) and _absmax(wl.v) > 0.5
    assert not _bits(wl.Je.cpu(), wc.Je.cpu()) and _bits(wl.Je.cpu(), ls.jacobian(wl.p).cpu())      # rebuilt at the new pose


def _je_residual(Je, v):
    return _absmax(torch.einsum("bez,bz->be", Je.double(), v.double().reshape(v.shape[0], -1)))


def _run_pendulum(route, steps, bump=False, differentiable=False, grad=False):
    """`steps` steps of `_pendulum(route)`: (the world, the Je every solve consumed, the largest |Je v_new| over the solves, leaves).
    `bump`: one float32 ulp on the entry -pos1_y of every scene's Je before the first step."""
    world, leaves = _pendulum(route, grad=grad)
    if bump:
        with torch.no_grad():
            world.Je[:, 0, 0] = torch.nextafter(world.Je[:, 0, 0], torch.full_like(world.Je[:, 0, 0], float("inf")))
    used, worst = [], 0.0
    for _ in range(steps):
        Je = world.Je.detach().clone()
        world.step(differentiable=differentiable)
        used.append(Je.cpu())
        worst = max(worst, _je_residual(Je, world.v.detach()))
    return world, used, worst, leaves


def _pendulum_yardsticks():
    """Measured on the `JointSet` pendulum - code from before the links: its own equality residual over 10 steps, and how far 10 steps
    move when ONE float32 ulp is added to one entry of every scene's Je before the first."""
    if "y" not in _BASE_CACHE:
        wj, used, worst, _ = _run_pendulum("joint", 10)
        wb, _, _, _ = _run_pendulum("joint", 10, bump=True)
        _BASE_CACHE["y"] = dict(p=wj.p.cpu(), v=wj.v.cpu(), used=used, residual=worst, ulp_dev=_absmax(wj.p.cpu() - wb.p.cpu()))
    return _BASE_CACHE["y"]


def test_a_pendulum_on_two_world_slots_is_the_pendulum_on_a_revolute_joint():
    """B = 8 starting angles, 10 plain steps.  Je of the two worlds agrees to one float32 ulp at every step; an entry whose two values
    are both below 2^-24 of the row's largest counts as equal (the slots' directions carry cos(pi / 2) = 6.1e-17 where the joint's rows
    have 0: below half an ulp of the 1 next to it in every sum the solvers form).  `p` agrees within 4 times the largest deviation of
    the JointSet world from ITSELF when one entry of its Je is moved by one float32 ulp before the first step - measured here, every run.
    Measured on an MI355X: the perturbed JointSet world deviates by 1.5e-07 (positions of order 39); |p(slots) - p(joint)| is 0 - every
    float32 entry of Je came out the same at all ten steps, so the two worlds ran the same solves."""
    y = _pendulum_yardsticks()
    ws, used, _, _ = _run_pendulum("slots", 10)
    for k, (a, b) in enumerate(zip(used, y["used"])):
        tiny = torch.maximum(a.abs(), b.abs()) <= 2.0 ** -24 * torch.maximum(a.abs(), b.abs()).amax(dim=2, keepdim=True)
        ok = _one_ulp(a, b.double()) | tiny
        assert bool(ok.all()), ("step", k, a[~ok].tolist(), b[~ok].tolist())
    dev = _absmax(ws.p.cpu() - y["p"])
    swing = _absmax(y["p"][:, 0, 1:] - torch.tensor(PIN, dtype=F64))
    print("pendulum: |p(slots) - p(joint)| %.3g   one-ulp deviation of the JointSet world %.3g   (positions of order %.3g)" % (dev, y["ulp_dev"], swing))
    assert y["ulp_dev"] > 0.0 and dev <= 4.0 * y["ulp_dev"]
    assert _absmax(ws.links.residual(ws.p)) < 0.5                                          # the anchor is still near both lines


def test_pendulum_gradients_through_five_recorded_steps_agree_with_the_revolute_joints():
    """d(sum p_final^2) / d(p0, Mdiag) through 5 differentiable steps - the links' autograd path (`_LinkJacobianFn` on the dynamics
    node, dL/dJe from lcp_step_backward_je_f32) against the JointSet's.  The margin is measured the same way: 4 times the change of the
    JointSet world's own gradients when one entry of its Je is moved by one float32 ulp before the first step.
    Both mechanisms are built from the leaf p0 (`_pendulum`), so both keep the pin at PIN when p0 moves.
    Measured on an MI355X: d/dp0 (entries up to 679) |slots - joint| 1.6e-13 where the one-ulp change is 8.1e-07; d/dMdiag (up to 336)
    0 where it is 3.1e-05."""
    grads = {}
    for key, route, bump in (("joint", "joint", False), ("bumped", "joint", True), ("slots", "slots", False)):
        world, _, _, leaves = _run_pendulum(route, 5, bump=bump, differentiable=True, grad=True)
        (world.p ** 2).sum().backward()
        grads[key] = {n: t.grad.detach().cpu() for n, t in leaves.items()}
        assert all(bool(torch.isfinite(g).all()) and _absmax(g) > 0.0 for g in grads[key].values()), key
    ok = []
    for n in ("p0", "Mdiag"):
        margin, dev = _absmax(grads["bumped"][n] - grads["joint"][n]), _absmax(grads["slots"][n] - grads["joint"][n])
        print("pendulum d loss / d %s: |slots - joint| %.3g   one-ulp change of the JointSet world %.3g   (of %.3g)"
              % (n, dev, margin, _absmax(grads["joint"][n])))
        ok.append(margin > 0.0 and dev <= 4.0 * margin)
    assert all(ok)


def test_a_rod_holds_its_row_as_well_as_the_revolute_joint_holds_its_rows():
    """A circle on a rod to a world point, under gravity, 30 steps: after every solve max |Je v_new| is at most twice the same quantity
    of the JointSet pendulum (the solver's own equality residual, measured here).  The rod's length drifts, as a revolute joint's
    anchor does - `LinkSet.residual` stays finite and is printed, not gated.
    Measured on an MI355X: rod 7.0e-07, JointSet pendulum 1.46e-06; the length of 40 drifts by 0.29 over the 30 steps."""
    y = _pendulum_yardsticks()
    world, p0, ls = _rod_world()
    worst, drift = 0.0, 0.0
    for _ in range(30):
        Je = world.Je.clone()
        world.step()
        worst = max(worst, _je_residual(Je, world.v))
        res = ls.residual(world.p)
        assert bool(torch.isfinite(res).all())
        drift = max(drift, _absmax(res))
    print("rod: largest |Je v_new| %.3g   JointSet pendulum %.3g   largest |length - 40| %.3g" % (worst, y["residual"], drift))
    assert _absmax(world.p - p0) > 5.0 and worst <= 2.0 * y["residual"]


GRAPH_WORLDS = {"links alone": dict(), "links with a JointSet": dict(hinged=True), "post_stab": dict(hinged=True, post_stab=True)}


@pytest.mark.parametrize("name", sorted(GRAPH_WORLDS))
def test_a_captured_run_equals_ten_eager_steps_bit_for_bit(name):
    (wg, _, _), (we, p0, ls) = _rod_world(**GRAPH_WORLDS[name]), _rod_world(**GRAPH_WORLDS[name])
    wg.run(10, graph=True)
    for _ in range(10):
        we.step()
    torch.cuda.synchronize()
    assert _bits(wg.p.cpu(), we.p.cpu()) and _bits(wg.v.cpu(), we.v.cpu()) and torch.equal(wg.t, we.t) and _bits(wg.Je.cpu(), we.Je.cpu())
    assert _absmax(we.p - p0) > 1.0 and we.e == ls.e + (2 if we.joints is not None else 0)
    assert _bits(we.Je.cpu(), ls.jacobian(we.p, Je_base=we._Je_base).cpu())


def test_a_captured_fixed_interval_run_leaves_finished_scenes_rows_at_their_pose():
    """`run(10, graph=True, fixed_dt=True, max_substeps=4)`: every scene finishes its interval in the first sub-step, the other three
    find it finished - and its rows are rebuilt at the pose it kept."""
    (wg, _, _), (we, p0, ls) = _rod_world(hinged=True), _rod_world(hinged=True)
    wg.run(10, graph=True, fixed_dt=True, max_substeps=4)
    for _ in range(10):
        we.step(fixed_dt=True, max_substeps=4)
    torch.cuda.synchronize()
    assert we.substeps.tolist() == [1, 1] and not bool(we.behind.any())
    assert _bits(wg.p.cpu(), we.p.cpu()) and _bits(wg.v.cpu(), we.v.cpu()) and torch.equal(wg.t, we.t) and _bits(wg.Je.cpu(), we.Je.cpu())
    assert _bits(we.Je[:, 2:].cpu(), ls.jacobian(we.p).cpu())                              # the links' rows: a function of the pose alone
    plain, _, _ = _rod_world(hinged=True)
    for _ in range(10):
        plain.step()
    assert _bits(plain.p.cpu(), we.p.cpu())                                                # one sub-step of dt is the plain step


def test_restart_report_elements_and_ccd_see_the_combined_rows():
    from lcp_physics_amd.physics.force_elements import ForceSet
    els = ForceSet.from_list([("drag", 1, {"lin": 0.05, "ang": 0.5})], 2).to(DEV)
    world, p0, ls = _rod_world(hinged=True, report=True, ccd=True, elements=els)
    Je0 = world.Je.clone()
    assert world.e == 3 and tuple(Je0.shape) == (2, 3, 6)
    for _ in range(3):
        Je = world.Je.clone()
        out = world.step()
        want = torch.einsum("bez,be->bz", Je.double(), out["y"].double()).reshape(2, 2, 3)    # Je^T y, rows in order
        assert bool(_one_ulp(world.report.joint_impulse.cpu(), want.cpu()).all())
        assert _absmax(world.report.joint_impulse) > 0.0 and _je_residual(Je, world.v) < 1e-3
    assert not _bits(world.Je.cpu(), Je0.cpu())
    world.restart(p0)
    assert _bits(world.Je.cpu(), Je0.cpu()) and _absmax(world.v) == 0.0
    rec = world.step(differentiable=True)                                                  # and a recorded step after plain ones
    assert bool(torch.isfinite(rec["v_new"]).all()) and tuple(world.Je.shape) == (2, 3, 6)
    world.step()


def test_a_world_without_links_is_the_world_from_before():
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.links import LinkSet
    (wj, _), (ws, _) = _pendulum("joint"), _pendulum("slots")
    assert wj.links is None and wj._Je_base is None and wj.e == 2 and _bits(wj.Je.cpu(), wj.joints.jacobian(wj.p).cpu())
    wc, p0, ls = _rod_world(as_constant=True)
    assert wc.links is None and wc.e == 1 and wc.Je.shape == (2, 1, 3)
    free = ContactWorld(wc.geom, p0.clone(), wc.v.clone(), wc.Mdiag, wc.f, wc.rest, wc.fric, dt=DT, maxc=4)
    assert free.links is None and free.Je is None and free.e == 0 and free._pinned
    assert ws.e == 2 and ws.joints is None and not ws._pinned
    with pytest.raises(ValueError, match="scenes"):                                        # B mismatch with the world
        ContactWorld(wc.geom, p0.clone(), wc.v.clone(), wc.Mdiag, wc.f, wc.rest, wc.fric, dt=DT, maxc=4,
                     links=LinkSet.from_list([("distance", 0, None, (0.0, 0.0), PIN)], p0[0].cpu(), 3).to(DEV))
