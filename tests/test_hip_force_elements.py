"""GPU: the force elements of lcp_forces.hip (lcp_force_elements_f64, lcp_force_elements_backward_f64; physics/force_elements.py;
`ContactWorld(elements=...)`) against the host mirror tests/force_elements_host.py, which tests/test_force_elements_host.py checks on
the CPU.

Forward: |f_out - f64| <= 2^-24 |f64| + 1e-12 S per entry - one float32 rounding of the sum, plus the float64 bound (2 E + 1) 2^-53 S of
a sum of E terms at E = 1024 with a factor 4 for the library functions.  Backward: every output within 1e-8 of the mirror's autograd,
relative to the output's largest entry (the rule of the sensors' and the proximity backward).  Worlds: the kernel route against a
`force_fn` closure over the mirror's formulas on the device, within 1e-5 of the motion's (or the gradient's) scale - chained float32
updates, the precedent of tests/test_hip_proximity.py::test_world_clearance_reaches_v0_through_differentiable_steps."""
import pytest
import torch

from tests import force_elements_host as FH

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32, I32 = torch.float64, torch.float32, torch.int32
NAN = float("nan")


def _lib():
    from lcp_physics_amd import _lib as L
    return L


def _absmax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _inputs(c):
    """The case on the device and the arguments both entries share."""
    d = {k: c[k].to(DEV).contiguous() for k in FH.ELEMENT_ARRAYS + ("p", "v", "f_base", "g_f")}
    B, nb = c["p"].shape[:2]
    return d, [B, nb, c["kind"].shape[1]] + [_lib().ptr(d[k]) for k in FH.ELEMENT_ARRAYS + ("p", "v")]


def _forward(c, base="given"):
    """The raw entry: f_out (CPU).  `base`: "given" (the case's f_base, f_out pre-filled with NaN), "null", "zeros" or "alias" (f_out is
    f_base's own buffer)."""
    L = _lib()
    d, args = _inputs(c)
    fb = {"given": d["f_base"], "null": None, "zeros": torch.zeros_like(d["f_base"]), "alias": d["f_base"].clone()}[base]
    out = fb if base == "alias" else torch.full(c["p"].shape, NAN, dtype=F32, device=DEV)
    rc = L.load().lcp_force_elements_f64(*args, L.ptr(fb), L.ptr(out), L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    return out.cpu()


def _backward(c, absent=()):
    """The raw entry into outputs pre-filled with NaN: the eight gradients (CPU) keyed as force_elements_host.LEAVES; `absent`: NULL."""
    L = _lib()
    d, args = _inputs(c)
    shapes = {n: (c["p"].shape if n in ("p", "v") else c[n].shape) for n in FH.LEAVES}
    outs = {n: (None if n in absent else torch.full(shapes[n], NAN, dtype=F64, device=DEV)) for n in FH.LEAVES}
    rc = L.load().lcp_force_elements_backward_f64(*args, L.ptr(d["g_f"]), *[L.ptr(outs[n]) for n in FH.LEAVES], L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    return {n: o.cpu() for n, o in outs.items() if o is not None}


# ------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("name", FH.CASE_NAMES)
def test_forward_matches_the_mirror(name):
    c, ref = FH.case(name), FH.reference(name)
    out = _forward(c)
    assert bool(torch.isfinite(out).all())                                                 # written, everywhere
    err = (out.double() - ref["f64"]).abs()
    bound = 2.0 ** -24 * ref["f64"].abs() + 1e-12 * ref["S"]
    worst = float((err / bound.clamp(min=1e-300)).max())
    print("%s: largest |f_out - f64| / (2^-24 |f64| + 1e-12 S) = %.3f   largest |f| %.3g" % (name, worst, _absmax(ref["f64"])))
    assert bool((err <= bound).all())
    # bodies no element touches - every body of a scene without a valid element - carry f_base's bits
    un = ~ref["touched"]
    assert _bits(out[un], c["f_base"][un])
    if name == "invalid":
        assert not bool(ref["valid"][2].any()) and _bits(out[2], c["f_base"][2])
    if name == "untouched":
        assert int(un.sum()) >= 15
    # f_base = NULL is a base of zeros, and f_out may be f_base itself
    assert _bits(_forward(c, "null"), _forward(c, "zeros"))
    assert _bits(_forward(c, "alias"), out)


# ------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("name", FH.CASE_NAMES)
def test_backward_matches_the_mirrors_autograd(name):
    c, ref = FH.case(name), FH.reference(name)
    got = _backward(c)
    dead = ~ref["valid"] | ref["sat"] | (ref["gap"]["L"] == 0.0)
    line = []
    for n in FH.LEAVES:
        assert bool(torch.isfinite(got[n]).all()), n                                       # written, everywhere
        want = ref["grads"][n]
        err, scale = _absmax(got[n] - want), _absmax(want)
        line.append("%s %.2g of %.3g" % (n, err, scale))
        assert err <= 1e-8 * scale, (n, err, scale)
        if n not in ("p", "v"):
            assert _absmax(got[n][dead]) == 0.0, n                                         # invalid, saturated, L == 0: exactly zero
    print(name + ": |got - want| of max |want|:  " + "   ".join(line))
    if name in ("saturated", "invalid"):
        assert int(dead.sum()) > 0 and int((~dead).sum()) > 0


@pytest.mark.parametrize("name", ["small", "edge65", "full"])
def test_two_runs_give_the_same_bits_whichever_outputs_are_asked_for(name):
    c = FH.case(name)
    first, again = _backward(c), _backward(c)
    fwd = _forward(c)
    for n in FH.LEAVES:
        assert _bits(first[n], again[n]), n
    for gone in FH.LEAVES:
        part = _backward(c, absent=(gone,))
        assert gone not in part
        for n in part:
            assert _bits(first[n], part[n]), (n, "without", gone)
    only_p = _backward(c, absent=tuple(n for n in FH.LEAVES if n != "p"))
    assert _bits(first["p"], only_p["p"])
    assert _bits(_forward(c), fwd)                                                         # and the forward's bits after all of that


# ------------------------------------------------------------------------------------------------------------- autograd surface
def _gradcheck_set():
    """nb 3, E 4: a world spring, a body-to-body spring, a motor and a drag, far from saturation (no limit) and from L = 0."""
    from lcp_physics_amd.physics.force_elements import ForceSet
    els = ForceSet.from_list([("spring", -1, 0, (2.0, 7.0), (0.3, -0.2), {"k": 3.0, "c": 0.4, "rest": 1.5}),
                              ("spring", 0, 1, (0.5, 0.1), (-0.4, 0.2), {"k": 2.0, "c": 0.3, "rest": 2.0}),
                              ("motor", 1, 2, {"kp": 1.5, "kd": 0.2, "target": 0.7, "rate": -0.3}),
                              ("drag", 2, {"lin": 0.6, "ang": 0.1})], 2).to(DEV)
    g = torch.Generator().manual_seed(5)
    p = torch.cat([torch.rand(2, 3, 1, generator=g, dtype=F64) - 0.5, 6.0 * torch.rand(2, 3, 2, generator=g, dtype=F64)], -1).to(DEV)
    v = torch.randn(2, 3, 3, generator=g, dtype=F64).to(DEV)
    return els, p, v


def test_gradcheck_of_element_forces():
    """torch.autograd.gradcheck on `element_forces` with eps = 1e-6 and tolerances 1e-6 at nb 3, E 4.

    `f` is float32 by the entry's contract, so a central difference of `f` itself over 2e-6 is quantised in steps of ulp(f) / 2e-6 -
    measured on an MI355X: every entry of the numerical Jacobian a multiple of 0.0596 (|f| < 1) to 0.24 (|f| < 4), against analytical
    entries of order 1, and gradcheck refuses it whatever the backward returns.  The entry accumulates in float64 on top of `f_base`
    and rounds once, so TWO calls give the sum to about 2^-48: hi = element_forces(...), lo = element_forces(..., f_base=-hi) is the
    float32 rounding of (sum - hi), and hi + lo in float64 is what gradcheck differentiates here - the same public call, the same
    backward (it runs for both), eps and tolerances unchanged.  `v` is float32 at the entry and cannot be stepped by 1e-6; it is
    held fixed here and its gradient is compared with float64 autograd in test_backward_matches_the_mirrors_autograd (1e-8)."""
    from lcp_physics_amd.physics.force_elements import ForceSet, element_forces
    els, p, v = _gradcheck_set()
    v = v.to(F32)
    names = ("k", "c", "x0", "w0", "a1", "a2")
    leaves = [p.clone().requires_grad_(True)] + [getattr(els, n).clone().requires_grad_(True) for n in names]

    def fn(p_, *params):
        fs = ForceSet(els.kind, els.b1, els.b2, params[4], params[5], params[0], params[1], params[2], params[3], els.limit)
        hi = element_forces(fs, p_, v)
        lo = element_forces(fs, p_, v, f_base=-hi)
        return hi.double() + lo.double()

    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-6, rtol=1e-6)


def test_element_forces_returns_the_entrys_bits_and_asks_only_for_required_gradients(monkeypatch):
    from lcp_physics_amd.physics.force_elements import ForceSet, element_forces
    L = _lib()
    lib, c = L.load(), FH.case("small")
    d, _ = _inputs(c)
    raw_f, raw_g = _forward(c), _backward(c)
    calls = []
    real = lib.lcp_force_elements_backward_f64

    def spy(*args):
        calls.append([a is not None for a in args[16:24]])
        return real(*args)

    monkeypatch.setattr(lib, "lcp_force_elements_backward_f64", spy, raising=False)

    def run(required):
        leaf = lambda n: d[n].clone().requires_grad_(n in required)
        t = {n: leaf(n) for n in FH.LEAVES + ("f_base",)}
        fs = ForceSet(d["kind"], d["b1"], d["b2"], t["a1"], t["a2"], t["k"], t["c"], t["x0"], t["w0"], d["limit"])
        f = element_forces(fs, t["p"], t["v"], f_base=t["f_base"])
        assert f.dtype == F32 and _bits(f.detach().cpu(), raw_f)
        if required:
            f.backward(d["g_f"])
        return t

    t = run(FH.LEAVES + ("f_base",))
    assert calls == [[True] * 8]
    for n in FH.LEAVES:
        want = raw_g[n].to(F32) if n == "v" else raw_g[n]                                  # g_v: cast to v's dtype
        assert t[n].grad.dtype == d[n].dtype and _bits(t[n].grad.cpu(), want), n
    assert _bits(t["f_base"].grad.cpu(), c["g_f"])                                         # g_f_base = g_f
    t = run(("k", "p"))
    assert calls[1] == [n in ("k", "p") for n in FH.LEAVES]
    assert _bits(t["k"].grad.cpu(), raw_g["k"]) and _bits(t["p"].grad.cpu(), raw_g["p"]) and t["v"].grad is None and t["a1"].grad is None
    t = run(("f_base",))                                                                   # nothing of the kernel's: no launch
    assert len(calls) == 2 and _bits(t["f_base"].grad.cpu(), c["g_f"])
    out = torch.full(c["p"].shape, NAN, dtype=F32, device=DEV)                             # the plain route: into the caller's buffer
    fs = ForceSet(*[d[n] for n in FH.ELEMENT_ARRAYS])
    assert element_forces(fs, d["p"], d["v"], f_base=d["f_base"], out=out) is out and _bits(out.cpu(), raw_f)


def test_bad_arguments_are_refused_before_any_launch():
    L = _lib()
    lib, c = L.load(), FH.case("small")
    d, args = _inputs(c)
    stream = L.stream_ptr(torch.device(DEV))
    out = torch.full(c["p"].shape, NAN, dtype=F32, device=DEV)
    g_p = torch.full(c["p"].shape, NAN, dtype=F64, device=DEV)
    fwd = lambda a, o=True: lib.lcp_force_elements_f64(*a, L.ptr(d["f_base"]), L.ptr(out) if o else None, stream)
    bwd = lambda a, g=True, o=True: lib.lcp_force_elements_backward_f64(*a, L.ptr(d["g_f"]) if g else None, L.ptr(g_p) if o else None,
                                                                        *[None] * 7, stream)
    with_arg = lambda k, v: args[:k] + [v] + args[k + 1:]
    bad = [with_arg(0, -1), with_arg(1, 0), with_arg(1, 65), with_arg(2, 0), with_arg(2, 1025)] + [with_arg(k, None) for k in range(3, 15)]
    for a in bad:
        assert fwd(a) == -1 and bwd(a) == -1
    assert fwd(args, o=False) == -1 and bwd(args, g=False) == -1 and bwd(args, o=False) == -1
    assert fwd(with_arg(0, 0)) == 0 and bwd(with_arg(0, 0)) == 0                           # B == 0: accepted, nothing launched
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(g_p).all())
    assert fwd(args) == 0 and bwd(args) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g_p).all())


# ------------------------------------------------------------------------------------------------------------- worlds
B = 2
DT = 1.0 / 30


def _rep(rows, dtype):
    return torch.tensor(rows, dtype=dtype, device=DEV).repeat(B, 1, 1) if isinstance(rows[0], (list, tuple)) else \
        torch.tensor(rows, dtype=dtype, device=DEV).repeat(B, 1)


def _free_world():
    """(a) Contact-free: three discs far apart, a spring between 0 and 1, a world spring on 2, a motor turning 1 against 0, drag on 2."""
    shapes = [("circle", 5.0)] * 3
    p0 = _rep([[0.1, 100.0, 100.0], [-0.2, 160.0, 110.0], [0.3, 130.0, 190.0]], F64)
    p0[1, :, 1] += 4.0                                                                     # (the scenes differ)
    v0 = _rep([[0.2, 3.0, -2.0], [-0.1, -4.0, 1.0], [0.0, 2.0, 5.0]], F32)
    Mdiag = _rep([[12.0, 1.0, 1.0], [20.0, 2.0, 2.0], [15.0, 1.5, 1.5]], F32)
    elements = [("spring", 0, 1, (2.0, 1.0), (-1.0, 3.0), {"k": 6.0, "c": 0.5, "rest": 50.0}),
                ("spring", -1, 2, (120.0, 150.0), (1.5, -2.0), {"k": 4.0, "c": 0.2, "rest": 30.0, "limit": 500.0}),
                ("motor", 0, 1, {"kp": 40.0, "kd": 3.0, "target": 0.5, "rate": 0.1}),
                ("drag", 2, {"lin": 0.3, "ang": 0.5})]
    return dict(shapes=shapes, p=p0, v=v0, Mdiag=Mdiag, f=torch.zeros(B, 3, 3, dtype=F32, device=DEV),
                rest=torch.full((B, 3), 0.5, dtype=F32, device=DEV), fric=torch.full((B, 3), 0.5, dtype=F32, device=DEV), Je=None,
                maxc=4, elements=elements)


def _pulled_box_world():
    """(b) A box resting on a pinned floor, pulled sideways by a spring to a world point."""
    from lcp_physics_amd import scenes
    w = scenes.make_drop_world(B, nbox=1, gap=(0.01, 0.02))
    w = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in w.items()}
    x, y = float(w["p"][0, 1, 1]), float(w["p"][0, 1, 2])
    w.update(maxc=8, elements=[("spring", -1, 1, (x + 120.0, y + 1.0), (5.0, 2.0), {"k": 3.0, "c": 0.4, "rest": 60.0}),
                               ("drag", 1, {"lin": 0.05, "ang": 2.0})])
    return w


WORLDS = {"free": _free_world, "pulled_box": _pulled_box_world}
EL_LEAVES = ("k", "c", "x0", "a1")


def _build(name, route, grad=False):
    """The world `name` on the kernel route (`elements=`) or on the closure route (`force_fn` over the mirror's formulas on the device);
    `grad`: p0, v0, Mdiag and the elements' k, c, x0, a1 are leaves.  Returns (world, leaves)."""
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.force_elements import ForceSet
    w = WORLDS[name]()
    els = ForceSet.from_list(w["elements"], B).to(DEV)
    leaves = {"p0": w["p"].clone(), "v0": w["v"].clone(), "Mdiag": w["Mdiag"].clone()}
    leaves.update({n: getattr(els, n).clone() for n in EL_LEAVES})
    if grad:
        for t in leaves.values():
            t.requires_grad_(True)
    els = ForceSet(els.kind, els.b1, els.b2, leaves["a1"], els.a2, leaves["k"], leaves["c"], leaves["x0"], els.w0, els.limit)
    geom = GeometryBatch.from_shapes(w["shapes"], B).to(DEV)
    kw = dict(Je=w["Je"], dt=DT, maxc=w["maxc"])
    if route == "kernel":
        world = ContactWorld(geom, leaves["p0"], leaves["v0"], leaves["Mdiag"], w["f"], w["rest"], w["fric"], elements=els, **kw)
    else:
        world = ContactWorld(geom, leaves["p0"], leaves["v0"], leaves["Mdiag"], w["f"], w["rest"], w["fric"], **kw)
        case = {n: getattr(els, n) for n in FH.ELEMENT_ARRAYS}
        world.force_fn = lambda t: FH.forces_host(dict(case, p=world.p, v=world.v, f_base=world.f))["f64"].to(F32)
    return world, leaves


def _margin(what, a, b, scale):
    err = _absmax(a.double() - b.double())
    print("%s: |kernel route - closure route| %.3g of %.3g (%.2g)" % (what, err, scale, err / scale))
    return err <= 1e-5 * scale


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_world_kernel_route_against_closure_route_ten_steps(name):
    (wk, lk), (wc, _) = _build(name, "kernel"), _build(name, "closure")
    start = lk["p0"].clone()                                                               # (plain steps reuse the tensor they were given)
    for _ in range(10):
        wk.step()
        wc.step()
    moved = wk.p - start
    assert _absmax(moved[..., 1:]) > 1.0 and _absmax(wk.v) > 0.5                           # the elements move the bodies
    if name == "pulled_box":
        assert int(wk.contacts.count.min()) >= 1 and torch.equal(wk.contacts.count, wc.contacts.count)
    else:
        assert int(wk.contacts.count.sum()) == 0
    ok_p = _margin(name + " p after 10 steps", wk.p, wc.p, _absmax(moved))
    ok_v = _margin(name + " v after 10 steps", wk.v, wc.v, _absmax(wk.v))
    assert ok_p and ok_v


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_world_kernel_route_against_closure_route_gradients_of_five_recorded_steps(name):
    grads = {}
    for route in ("kernel", "closure"):
        world, leaves = _build(name, route, grad=True)
        for _ in range(5):
            world.step(differentiable=True)
        weight = torch.tensor([30.0, 1.0, -0.5], dtype=F64, device=DEV)
        (world.p * weight).sum().backward()
        grads[route] = {n: t.grad for n, t in leaves.items()}
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads[route].values()), route
    ok = [_margin("%s d loss / d %s" % (name, n), grads["kernel"][n], grads["closure"][n], _absmax(grads["closure"][n])) for n in grads["kernel"]]
    assert all(_absmax(g) > 0.0 for g in grads["closure"].values())
    assert all(ok)


def test_a_captured_run_equals_ten_eager_steps_bit_for_bit():
    (wg, _), (we, _) = _build("pulled_box", "kernel"), _build("pulled_box", "kernel")
    wg.run(10, graph=True)
    for _ in range(10):
        we.step()
    torch.cuda.synchronize()
    assert _bits(wg.p.cpu(), we.p.cpu()) and _bits(wg.v.cpu(), we.v.cpu()) and torch.equal(wg.t, we.t)
    assert _absmax(we.v) > 0.5


def test_a_fixed_interval_step_agrees_with_the_closure_route_and_leaves_a_finished_scene_alone():
    (wk, lk), (wc, _) = _build("free", "kernel"), _build("free", "closure")
    start = lk["p0"].clone()
    wk.step(fixed_dt=True)
    wc.step(fixed_dt=True)
    assert wk.substeps.tolist() == [1] * B and torch.equal(wk.t, wc.t)
    moved = wk.p - start
    assert _margin("fixed_dt p", wk.p, wc.p, _absmax(moved)) and _margin("fixed_dt v", wk.v, wc.v, _absmax(wk.v))
    # a second sub-step finds every scene at its end_t: the elements' force is not zero there, and nothing moves
    w2, _ = _build("free", "kernel")
    w2.step(fixed_dt=True, max_substeps=2)
    assert w2.substeps.tolist() == [1] * B and not bool(w2.behind.any())
    assert _absmax(w2._forces()) > 1.0
    assert _bits(w2.p.cpu(), wk.p.cpu()) and _bits(w2.v.cpu(), wk.v.cpu()) and torch.equal(w2.t, wk.t)


def test_a_world_without_elements_returns_its_own_force_tensor():
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.contacts import GeometryBatch
    w = _free_world()
    world = ContactWorld(GeometryBatch.from_shapes(w["shapes"], B).to(DEV), w["p"], w["v"], w["Mdiag"], w["f"], w["rest"], w["fric"],
                         Je=None, dt=DT, maxc=4)
    assert world.elements is None and world._forces() is world.f and world._forces(differentiable=True) is world.f
    with pytest.raises(ValueError):
        from lcp_physics_amd.physics.force_elements import ForceSet
        ContactWorld(world.geom, w["p"], w["v"], w["Mdiag"], w["f"], w["rest"], w["fric"], Je=None, dt=DT, maxc=4,
                     elements=ForceSet.from_list(w["elements"], B + 1).to(DEV))
