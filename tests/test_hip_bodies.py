"""GPU: bodies constructed on the device (lcp_bodies.hip: `lcp_body_properties_f64`, `lcp_body_properties_backward_f64`, and
`physics.bodies.BodyBatch` on top of them) against what the unmodified reference's `Circle` / `Rect` / `Hull` constructors and its
autograd give (tests/golden/bodies.npz, tools/gen_bodies_golden.py; pinned on the CPU by tests/test_bodies_fixture.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REP = 3
GATE = 1e-12                   # x the quantity's scale over the fixture: the gate of tests/test_hip_shape_grad.py:61-62 (fp64 on both sides)
FP32_EPS = 2.0 ** -24
_CACHE = {}


def _fixture():
    if "d" not in _CACHE:
        _CACHE["d"] = np.load(os.path.join(GOLDEN, "bodies.npz"))
    return _CACHE["d"]


def _scale(ref):
    return max(1.0, float(np.abs(ref).max()))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _mixed_order(d, cap):
    """The fixture's bodies with at most `cap` vertices, circles, rects and hulls interleaved (a fixed permutation)."""
    idx = np.nonzero(d["m_nverts"] <= cap)[0]
    return idx[np.random.default_rng(7).permutation(len(idx))]


def _run(d, idx, nb, cap, rep=REP, backward=True):
    """Bodies `idx` laid out as scenes of `nb` bodies (the last scene filled up from the front) at capacity `cap`, every scene `rep`
    times; returns per body of `idx` the outputs of replica 0 and whether all replicas have the same bits."""
    from lcp_physics_amd.physics import bodies as bd
    n = len(idx)
    S = (n + nb - 1) // nb
    full = np.concatenate([idx, idx[:S * nb - n]])
    T = lambda a, dt_: torch.tensor(np.repeat(a[full].reshape((S, nb) + a.shape[1:]), rep, axis=0), dtype=dt_, device=DEV).contiguous()
    kind = T((d["m_kind"] != 0).astype(np.int32), torch.int32)
    ins = (kind, T(d["m_radius"], torch.float64), T(d["m_verts_raw"][:, :cap], torch.float64), T(d["m_nverts"], torch.int32),
           T(d["m_mass"], torch.float64))
    g = float(d["m_g"])
    out = bd.body_properties(ins[0], ins[1], ins[2], ins[3], ins[4], g)
    if backward:
        grads = bd.body_properties_backward(ins[0], ins[1], ins[2], ins[3], ins[4], g, T(d["m_g_centroid"], torch.float64),
                                            T(d["m_g_verts"][:, :cap], torch.float64), T(d["m_g_inertia"], torch.float64),
                                            T(d["m_g_Mdiag"], torch.float32), T(d["m_g_f"], torch.float32))
        out.update({"d_" + k: v for k, v in grads.items()})
    torch.cuda.synchronize()
    res, same = {}, True
    for k, v in out.items():
        a = v.cpu().numpy()
        a = a.reshape((S, rep, nb) + a.shape[2:])
        same = same and all(np.array_equal(_bits(a[:, 0]), _bits(a[:, r])) for r in range(1, rep))
        res[k] = a[:, 0].reshape((S * nb,) + a.shape[3:])[:n]
    return res, same


def _all64():
    if "all64" not in _CACHE:
        d = _fixture()
        _CACHE["all64"] = _run(d, np.arange(len(d["m_kind"])), 5, 64)
    return _CACHE["all64"]


def test_forward_matches_the_reference_constructors_on_every_case():
    """All 120 bodies (circles, rects, hulls of 3 .. 64 vertices, half of them offset from the reference point by up to 300), five per
    scene at capacity 64: centroid, recentred vertices and inertia within 1e-12 x scale of the reference's values; Mdiag and the
    gravity force within one fp32 ulp of float32(reference); no status bit."""
    d = _fixture()
    got, same = _all64()
    assert same
    for key, ref in (("centroid", d["m_centroid"]), ("verts_local", d["m_verts"]), ("inertia", d["m_inertia"])):
        err = float(np.abs(got[key] - ref).max()) / _scale(ref)
        print("forward %s: worst |difference| / scale %.2g" % (key, err))
        assert err <= GATE, (key, err)
    for key, ref in (("Mdiag", d["m_Mdiag"]), ("f_gravity", d["m_f"])):
        r32 = ref.astype(np.float32)
        assert got[key].dtype == np.float32 and (np.abs(got[key] - r32) <= np.spacing(np.abs(r32))).all(), key
    assert (got["status"] == 0).all()
    nv = d["m_nverts"]
    assert np.abs(got["verts_local"] * (np.arange(64)[None, :] >= nv[:, None])[..., None]).max() == 0.0


def test_backward_matches_the_reference_autograd_with_the_recorded_cotangents():
    """d(sum cot . outputs)/d(raw vertices, radius, mass) from ONE backward launch against the reference's autograd through
    `Hull.__init__` / `_get_centroid` / `_get_ang_inertia` / `M` / `Gravity`: 1e-12 x scale; and d/d(dims) of the rects through
    `BodyBatch.from_list`'s torch construction of the four vertices (bodies.py:260-262), same gate."""
    from lcp_physics_amd.physics.bodies import BodyBatch
    d = _fixture()
    got, same = _all64()
    assert same
    hull, circ = d["m_kind"] == 2, d["m_kind"] == 0
    for name, g, ref in (("raw vertices", got["d_verts_raw"][hull], d["m_d_verts_raw"][hull]),
                         ("radius", got["d_radius"][circ], d["m_d_radius"][circ]), ("mass", got["d_mass"], d["m_d_mass"])):
        err = float(np.abs(g - ref).max()) / _scale(ref)
        print("backward %s: worst |difference| / scale %.2g (scale %.3g)" % (name, err, _scale(ref)))
        assert np.abs(ref).max() > 0.1 and err <= GATE, (name, err)
    assert np.abs(got["d_radius"][~circ]).max() == 0.0 and np.abs(got["d_verts_raw"][circ]).max() == 0.0
    assert np.abs(got["d_verts_raw"] * (np.arange(64)[None, :] >= d["m_nverts"][:, None])[..., None]).max() == 0.0
    # the rects through from_list: dims and mass are leaves, the cotangents go to replica 0
    rects = np.nonzero(d["m_kind"] == 1)[0]
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    dims = [t64(d["m_dims"][i]).requires_grad_(True) for i in rects]
    mass = [t64(d["m_mass"][i]).requires_grad_(True) for i in rects]
    bb = BodyBatch.from_list([("rect", d["m_ref"][i].tolist(), dm, {"mass": m}) for i, dm, m in zip(rects, dims, mass)], REP,
                             g=float(d["m_g"]))
    c = lambda k, dt_=torch.float64: torch.tensor(d[k][rects], dtype=dt_, device=DEV)
    loss = ((bb.centroid[0] * c("m_g_centroid")).sum() + (bb.geom.verts_local[0] * c("m_g_verts")[:, :8]).sum()
            + (bb.inertia[0] * c("m_g_inertia")).sum() + (bb.Mdiag[0] * c("m_g_Mdiag", torch.float32)).sum().double()
            + (bb.f_gravity[0] * c("m_g_f", torch.float32)).sum().double())
    loss.backward()
    gd, gm = np.stack([x.grad.numpy() for x in dims]), np.array([float(x.grad) for x in mass])
    err_d = float(np.abs(gd - d["m_d_dims"][rects]).max()) / _scale(d["m_d_dims"])
    err_m = float(np.abs(gm - d["m_d_mass"][rects]).max()) / _scale(d["m_d_mass"])
    print("backward dims: %.2g, mass through from_list: %.2g" % (err_d, err_m))
    assert err_d <= GATE and err_m <= GATE
    assert np.abs((bb.p0[0, :, 1:] - bb.centroid[0]).detach().cpu().numpy() - d["m_ref"][rects]).max() <= 1e-12 * 900


@pytest.mark.parametrize("cap", [8, 16, 64])
def test_layouts_give_identical_bits_and_capacities_agree(cap):
    """The same bodies (circles, rects and hulls mixed in every scene) as scenes of 1, 5 and 33 bodies - at 8 bodies per wavefront a
    tail wavefront, and more than one wavefront per scene - at capacity `cap`: replicas and the same body at another place of the
    batch have identical bits in every output of both launches; against capacity 64 the results agree within 1e-12 x scale."""
    d = _fixture()
    idx = _mixed_order(d, cap)
    nv, kinds = d["m_nverts"][idx], d["m_kind"][idx]
    assert 3 in nv and cap in nv and (kinds == 0).sum() >= 10 and (cap != 64 or 33 in nv)
    hulls5 = (kinds[:len(idx) // 5 * 5] != 0).reshape(-1, 5)
    assert (hulls5.any(axis=1) & ~hulls5.all(axis=1)).sum() >= 5                         # circles and hulls share scenes (and wavefronts)
    base = None
    for nb in (1, 5, 33):
        got, same = _run(d, idx, nb, cap)
        assert same, nb
        assert (got["status"] == 0).all()
        if base is None:
            base = got
            continue
        for k in base:
            assert np.array_equal(_bits(base[k]), _bits(got[k])), (k, nb)
    ref, _ = _all64()
    for k in ("centroid", "verts_local", "inertia", "d_verts_raw", "d_radius", "d_mass"):
        a, b = base[k], ref[k][idx]
        b = b[:, :cap] if b.ndim == 3 else b
        assert float(np.abs(a - b).max()) <= GATE * _scale(ref[k]), k
    for k in ("Mdiag", "f_gravity"):
        assert (np.abs(base[k] - ref[k][idx]) <= np.spacing(np.abs(ref[k][idx]))).all(), k


def _bad_scene(d):
    """Five bodies that share one wavefront at capacity 8: a reversed hull, a non-convex one, one with two vertices, one without
    area, and an untouched hull of the fixture."""
    five = int(np.nonzero((d["m_kind"] == 2) & (d["m_nverts"] == 5))[0][0])
    good = int(np.nonzero((d["m_kind"] == 2) & (d["m_nverts"] == 6))[0][0])
    pent = d["m_verts_raw"][five, :5]
    dart = np.array([[20.0, 0.0], [0.0, 20.0], [5.0, 0.0], [0.0, -20.0]])                 # the fixture's orientation, a reflex vertex at (5, 0)
    line = np.array([[0.0, 0.0], [10.0, 0.0], [20.0, 0.0], [30.0, 0.0]])
    return [pent[::-1].copy(), dart, pent[:2].copy(), line, d["m_verts_raw"][good, :6].copy()], good


def test_status_bits_and_the_check_of_from_list():
    from lcp_physics_amd import _lib
    from lcp_physics_amd.physics import bodies as bd
    d = _fixture()
    polys, good = _bad_scene(d)
    verts = np.zeros((1, 5, 8, 2))
    for i, p in enumerate(polys):
        verts[0, i, :len(p)] = p
    T = lambda a, dt_: torch.tensor(np.repeat(a, REP, axis=0), dtype=dt_, device=DEV)
    mass = np.full((1, 5), float(d["m_mass"][good]))
    out = bd.body_properties(T(np.ones((1, 5), np.int32), torch.int32), T(np.zeros((1, 5)), torch.float64), T(verts, torch.float64),
                             T(np.array([[len(p) for p in polys]], np.int32), torch.int32), T(mass, torch.float64), float(d["m_g"]))
    torch.cuda.synchronize()
    want = [_lib.BODY_ST_ORIENTATION, _lib.BODY_ST_NONCONVEX, _lib.BODY_ST_COUNT, _lib.BODY_ST_DEGENERATE, 0]
    assert out["status"].cpu().tolist() == [want] * REP
    # the good neighbour in the same wavefront has its fixture values
    for key, ref in (("centroid", "m_centroid"), ("verts_local", "m_verts"), ("inertia", "m_inertia")):
        a, b = out[key][0, 4].cpu().numpy(), d[ref][good]
        b = b[:8] if b.ndim == 2 else b
        assert float(np.abs(a - b).max()) <= GATE * _scale(d[ref]), key
    assert float(out["verts_local"][:, 2, 2:].abs().max()) == 0.0                        # slots >= nv of a flagged body are still zero
    # a circle with a non-finite radius
    c = bd.body_properties(torch.zeros(1, 2, dtype=torch.int32, device=DEV), torch.tensor([[float("nan"), 2.0]], dtype=torch.float64, device=DEV),
                           torch.zeros(1, 2, 8, 2, dtype=torch.float64, device=DEV), torch.zeros(1, 2, dtype=torch.int32, device=DEV),
                           torch.ones(1, 2, dtype=torch.float64, device=DEV))
    assert c["status"].cpu().tolist() == [[_lib.BODY_ST_DEGENERATE, 0]] and float(c["inertia"][0, 1]) == 2.0
    # from_list names the first bad body; check=False reads nothing back
    bodies = [("circle", [0.0, 0.0], 5.0), ("hull", [50.0, 0.0], polys[4].tolist()), ("hull", [100.0, 0.0], polys[0].tolist())]
    with pytest.raises(ValueError, match="body 2 of scene 0.*order"):
        bd.BodyBatch.from_list(bodies, REP)
    with pytest.raises(ValueError, match="body 1 of scene 0.*convex"):
        bd.BodyBatch.from_list([bodies[0], ("hull", [9.0, 9.0], polys[1].tolist())], REP)
    raw = {k: v.to(DEV) for k, v in bd.BodyBatch.raw_inputs(bodies, REP).items()}
    torch.cuda.synchronize()
    calls = []
    real = bd.BodyBatch.raise_on_status
    bd.BodyBatch.raise_on_status = staticmethod(lambda st: calls.append(1))
    torch.cuda.set_sync_debug_mode("error")
    try:
        bb = bd.BodyBatch.from_raw(raw, g=10.0, check=False, scene_verts_max=11)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        bd.BodyBatch.raise_on_status = real
    assert not calls and bb.status.cpu().tolist() == [[0, 0, _lib.BODY_ST_ORIENTATION]] * REP
    assert bd.BodyBatch.from_list(bodies[:2], REP, g=10.0).f_gravity[0].cpu().tolist() == [[0.0, 0.0, 10.0]] * 2


def test_no_backward_node_without_a_learnable_input():
    """The rule of test_constant_geometry_launches_no_shape_kernel...: constant shapes and masses launch no backward kernel - the
    outputs carry no graph at all; one learnable mass and they do."""
    from lcp_physics_amd.physics.bodies import BodyBatch
    bodies = [("circle", [0.0, 0.0], 5.0), ("rect", [50.0, 0.0], [4.0, 2.0])]
    bb = BodyBatch.from_list(bodies, REP, g=10.0)
    for t in (bb.geom.radius, bb.geom.verts_local, bb.p0, bb.Mdiag, bb.f_gravity, bb.inertia):
        assert not t.requires_grad and t.grad_fn is None
    m = torch.tensor(2.0, dtype=torch.float64, requires_grad=True)
    bb = BodyBatch.from_list([bodies[0], ("rect", [50.0, 0.0], [4.0, 2.0], {"mass": m})], REP, g=10.0)
    assert bb.Mdiag.grad_fn is not None and bb.f_gravity.requires_grad
    (bb.Mdiag.sum() + bb.f_gravity.sum()).backward()
    assert abs(float(m.grad) - REP * ((16.0 + 4.0) / 12 + 2 + 10.0)) < 1e-12


# ---- roll-out --------------------------------------------------------------------------------------------------------------
def _rel(got, ref):
    """tests/test_hip_shape_grad.py `_rel`: per scene max |got - ref| / max |ref|; a scene whose reference gradient lies below fp32
    rounding of the set's largest gradient is measured against that largest gradient."""
    den, top = np.abs(ref).max(axis=1), np.abs(ref).max()
    return np.abs(got - ref).max(axis=1) / np.where(den > FP32_EPS * top, den, top)


def _rollout_fixture():
    d0 = _fixture()
    return {k[2:]: d0[k] for k in d0.files if k.startswith("r_")}


def _rollout_bodies(d, B, rad, verts, m_ball, m_box, check=True):
    from lcp_physics_amd.physics.bodies import BodyBatch
    return BodyBatch.from_list([("rect", d["floor_pos"].tolist(), d["floor_dims"].tolist(), {"restitution": float(d["rest"][0]), "fric_coeff": float(d["fric"][0])}),
                                ("circle", d["ball_pos"].tolist(), rad, {"mass": m_ball, "restitution": float(d["rest"][1]), "fric_coeff": float(d["fric"][1])}),
                                ("hull", d["box_ref"].tolist(), verts, {"mass": m_box, "restitution": float(d["rest"][2]), "fric_coeff": float(d["fric"][2])})],
                               B, g=float(d["g"]), check=check)


def _forces(d, rep):
    """(f, force_fn): the constant that takes gravity off the floor again (the fixture attaches `Gravity` to the ball and the box
    only) and the pushes of the first `t_push` seconds."""
    n = d["force_ball"].shape[0]
    B = n * rep
    rp = lambda a: torch.tensor(np.repeat(a, rep, axis=0), dtype=torch.float32, device=DEV)
    fb, fx = rp(d["force_ball"]), rp(d["force_box"])
    mult, t_push = float(d["mult"]), float(d["t_push"])
    f = torch.zeros(B, 3, 3, dtype=torch.float32, device=DEV)
    f[:, 0, 2] = -float(d["g"])                                                        # (the floor's mass is the default, 1)
    z = torch.zeros(B, 1, 3, dtype=torch.float32, device=DEV)

    def force_fn(t):
        on = (t < t_push).to(torch.float32).unsqueeze(1)
        return torch.cat([z, (fb * mult * on).unsqueeze(1), (fx * mult * on).unsqueeze(1)], dim=1)

    return f, force_fn


def test_rollout_gradient_of_raw_vertices_radius_and_masses_matches_the_reference_autograd():
    """The ball / box / floor scene with the bodies built by `BodyBatch.from_list(...).world(...)` from leaves set BEFORE construction:
    the box's raw vertices (relative to a reference point that is not its centroid), the ball's radius, both masses; `Gravity` on
    both (fixture `r_*`, six scenes, 40 steps, loss = |ball - box|).  d(loss)/d(leaf) now has the reference's three paths - contact
    frame, mass matrix / gravity, initial position.  Trajectory rule and gates of
    test_rollout_shape_gradient_through_hull_contacts_matches_the_reference_autograd: a scene counts if its clock (1e-12) and its
    contact count at every step are the fixture's, at most one of the six may fall off; p_final 5e-4; gradients 1e-5 relative per
    scene (`_rel`; radius and raw vertices as one row as there, the two masses as another); replicas bitwise equal."""
    d = _rollout_fixture()
    n, rep = d["force_ball"].shape[0], 16
    B = n * rep
    t64 = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    rad, verts, m_ball, m_box = t64(float(d["ball_rad"])), t64(d["box_verts_raw"]), t64(float(d["mass"][0])), t64(float(d["mass"][1]))
    bb = _rollout_bodies(d, B, rad, verts, m_ball, m_box)
    for k in ("radius", "verts_raw", "mass"):                                           # per-scene gradients of the shared leaves
        bb.raw[k].retain_grad()
    f, force_fn = _forces(d, rep)
    world = bb.world(f=f, force_fn=force_fn, Je=torch.tensor(np.repeat(d["Je"], rep, axis=0), dtype=torch.float32, device=DEV),
                     dt=float(d["dt"]), maxc=8)
    assert np.abs(world.p.detach().cpu().numpy()[::rep] - d["p0"]).max() <= 1e-11
    ncs = []
    for _ in range(int(d["nsteps"])):
        world.step(differentiable=True)
        ncs.append(world.contacts.count.clone())
    pos = world.p[:, :, 1:]
    loss = (pos[:, 1] - pos[:, 2]).norm(dim=1)
    loss.sum().backward()
    torch.cuda.synchronize()
    t_ok = np.abs(world.t.cpu().numpy()[::rep] - d["t"][:, -1]) < 1e-12
    n_ok = (torch.stack(ncs, 1).cpu().numpy()[::rep] == d["ncontacts"]).all(axis=1)
    same = t_ok & n_ok
    print("scenes on the reference's trajectory:", same.tolist())
    assert same.sum() >= n - 1
    pf = world.p.detach().cpu().numpy()[::rep]
    print("p_final: worst |difference| %.3g" % np.abs(pf - d["p_final"])[same].max())
    assert np.abs(pf - d["p_final"])[same].max() <= 5e-4
    gr, gv, gm = (bb.raw[k].grad.cpu().numpy() for k in ("radius", "verts_raw", "mass"))
    for g in (gr, gv, gm):                                                              # replicas are bitwise replicas
        assert np.abs(g.reshape((n, rep) + g.shape[1:]) - g[::rep][:, None]).max() == 0.0
    assert np.abs(gr[:, [0, 2]]).max() == 0.0 and np.abs(gv[:, 1]).max() == 0.0 and np.abs(gv[:, 2, 4:]).max() == 0.0
    got = np.concatenate([gr[::rep, 1:2], gv[::rep, 2, :4].reshape(n, 8)], axis=1)
    ref = np.concatenate([d["grad_rad"][:, None], d["grad_verts"].reshape(n, 8)], axis=1)
    err, err_m = _rel(got, ref), _rel(gm[::rep, 1:], d["grad_mass"])
    print("roll-out, d(loss)/d(ball radius, box raw vertices): relative error per scene", np.array2string(err, precision=2))
    print("roll-out, d(loss)/d(ball mass, box mass): relative error per scene", np.array2string(err_m, precision=2))
    print(np.array2string(got, precision=5)); print(np.array2string(ref, precision=5))
    print(np.array2string(gm[::rep, 1:], precision=5)); print(np.array2string(d["grad_mass"], precision=5))
    assert err[same].max() <= 1e-5, err
    assert err_m[same].max() <= 1e-5, err_m
    # the leaves themselves hold the sum over the scenes
    assert abs(float(rad.grad) - gr[:, 1].sum()) <= 1e-9 * np.abs(gr).sum() and np.abs(verts.grad.numpy() - gv[:, 2, :4].sum(axis=0)).max() <= 1e-9 * np.abs(gv).sum()
    assert abs(float(m_box.grad) - gm[:, 2].sum()) <= 1e-9 * np.abs(gm).sum()


def test_construction_rollout_and_backward_captured_in_a_hip_graph_equal_the_eager_run():
    """The property launches, `restart`, the steps, the loss and the backward (with lcp_body_properties_backward_f64 at its end) in
    one HIP graph, as in test_differentiable_rollout_with_a_learnable_radius_captured_in_a_hip_graph_equals_the_eager_run: replayed
    with new parameter values it returns the eager run's loss and gradients bit for bit."""
    from lcp_physics_amd.physics.bodies import BodyBatch
    d = _rollout_fixture()
    n, rep, steps = d["force_ball"].shape[0], 2, 14                                     # (first contacts at step 2 or 3)
    B = n * rep
    f, push = _forces(d, rep)
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    bb0 = _rollout_bodies(d, B, t64(float(d["ball_rad"])), t64(d["box_verts_raw"]), t64(1.0), t64(1.0))
    world = bb0.world(f=f, force_fn=push, Je=torch.tensor(np.repeat(d["Je"], rep, axis=0), dtype=torch.float32, device=DEV),
                      dt=float(d["dt"]), maxc=8)
    const = {k: v.detach() for k, v in bb0.raw.items()}
    sel = lambda i, shape: (torch.arange(3, device=DEV) == i).to(torch.float64).reshape(shape)

    def loss_of(rad, verts, mass):
        raw = dict(const)                                                               # device tensors only: capturable
        raw["radius"] = (sel(1, (1, 3)) * rad).expand(B, 3).contiguous()
        pad = torch.cat([verts, verts.new_zeros(4, 2)]).reshape(1, 1, 8, 2)
        raw["verts_raw"] = (const["verts_raw"] * (1.0 - sel(2, (1, 3, 1, 1))) + sel(2, (1, 3, 1, 1)) * pad).contiguous()
        raw["mass"] = (sel(0, (1, 3)) + sel(1, (1, 3)) * mass[0] + sel(2, (1, 3)) * mass[1]).expand(B, 3).contiguous()
        bb = BodyBatch.from_raw(raw, g=float(d["g"]), check=False, scene_verts_max=8)
        world.geom, world.Mdiag = bb.geom, bb.Mdiag
        total = bb.f_gravity + f
        world.force_fn = lambda t: total + push(t)
        world.restart(bb.p0, bb.v0)
        for _ in range(steps):
            world.step(differentiable=True)
        pos = world.p[:, :, 1:]
        return (pos[:, 1] - pos[:, 2]).norm(dim=1)

    dev = lambda a: torch.tensor(a, dtype=torch.float64, device=DEV, requires_grad=True)
    rad, verts, mass = dev(float(d["ball_rad"])), dev(d["box_verts_raw"]), dev([1.0, 1.0])
    if hasattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch"):
        torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            rad.grad = verts.grad = mass.grad = None
            loss_of(rad, verts, mass).sum().backward()
    torch.cuda.current_stream().wait_stream(side)
    rad.grad = verts.grad = mass.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss_g = loss_of(rad, verts, mass)
        loss_g.sum().backward()
    with torch.no_grad():                                                               # new parameter values in the captured tensors
        rad.mul_(1.01); mass.mul_(1.1); verts.add_(0.25)
    g.replay()
    torch.cuda.synchronize()
    got = (loss_g.clone(), rad.grad.clone(), verts.grad.clone(), mass.grad.clone())
    r2, v2, m2 = [t.detach().clone().requires_grad_(True) for t in (rad, verts, mass)]
    loss_e = loss_of(r2, v2, m2)
    loss_e.sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(got[0], loss_e.detach()) and torch.equal(got[1], r2.grad) and torch.equal(got[2], v2.grad) and torch.equal(got[3], m2.grad)
    assert float(v2.grad.abs().max()) > 0.0 and float(m2.grad.abs().max()) > 0.0
