"""GPU: the backward of the contact frame with respect to the SHAPE of the bodies (lcp_contacts_shape.hip:
`lcp_contact_frame_backward_shape_f64`) - radii and body-frame hull vertices - against what the unmodified reference's autograd
gives `Circle.rad` / `Hull.verts` (tests/golden/shape_grad.npz, tools/gen_shape_grad_golden.py; pinned on the CPU by
tests/test_shape_grad_fixture.py), at the frame level and through `ContactWorld.step(differentiable=True)`."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture():
    return np.load(os.path.join(GOLDEN, "shape_grad.npz"))


def _frame_batch(d, sel, cap, rep=2):
    """The frame-level configurations `sel` as scenes of two bodies, each `rep` times, at vertex capacity `cap`."""
    from lcp_physics_amd.physics.contacts import GeometryBatch
    r = lambda a, dt_: torch.tensor(np.repeat(a[sel], rep, axis=0), dtype=dt_).contiguous()
    geom = GeometryBatch(r(d["f_kind"], torch.int32), r(d["f_rad"], torch.float64), r(d["f_verts_local"][:, :, :cap], torch.float64),
                         r(d["f_nverts"], torch.int32), None, None).to(DEV)
    gs = [r(d[k], torch.float32).to(DEV) for k in ("f_g_n", "f_g_p1", "f_g_p2")]
    return geom, r(d["f_pose"], torch.float64).to(DEV), gs


def _frame_grads(d, sel, cap, rep=2):
    from lcp_physics_amd.physics import contacts as ct
    geom, p, gs = _frame_batch(d, sel, cap, rep)
    cb = ct.find_contacts(geom, p, maxc=2, eps=float(d["f_eps"]))
    d_rad, d_verts = ct.contact_frame_backward_shape(geom, p, cb, *gs, eps=float(d["f_eps"]))
    torch.cuda.synchronize()
    return cb, d_rad.cpu().numpy(), d_verts.cpu().numpy()


def test_frame_level_shape_gradients_match_the_reference_autograd():
    """Every configuration of the fixture (232: circle / circle, circle / hull in either order by GJK vertex region, GJK edge region
    and deep SAT, hull / hull with either body as the reference and one or two clipped points, hulls of 3 .. 16 vertices), none
    excluded: the records `find_contacts` detects are the fixture's, and d(sum g . (n, p1, p2))/d(radius, verts_local) agrees with the
    reference's autograd to 1e-12 x max(1, largest |gradient|) - the gate of the pose derivative in
    test_contact_frame_backward_matches_autograd_of_the_circle_record (both sides are fp64 autodiff of the same expressions)."""
    d = _fixture()
    n, rep = d["f_count"].shape[0], 2
    cb, d_rad, d_verts = _frame_grads(d, np.arange(n), 16, rep)
    assert (cb.count.cpu().numpy()[::rep] == d["f_count"]).all()
    live = (np.arange(2)[None, :] < d["f_count"][:, None])[..., None]
    for key, ref, tol in (("c_n", "f_normal", 1e-6), ("c_p1", "f_p1", 1e-5), ("c_p2", "f_p2", 1e-5)):
        assert np.abs((getattr(cb, key).cpu().numpy()[::rep] - d[ref]) * live).max() <= tol, key
    assert np.abs((cb.c_pen.cpu().numpy()[::rep] - d["f_pen"]) * live[..., 0]).max() <= 1e-9
    for got in (d_rad, d_verts):                                            # replicas are bitwise replicas
        assert np.array_equal(got[0::rep], got[1::rep])
    er, ev = np.abs(d_rad[::rep] - d["f_d_rad"]), np.abs(d_verts[::rep] - d["f_d_verts"])
    sr, sv = max(1.0, np.abs(d["f_d_rad"]).max()), max(1.0, np.abs(d["f_d_verts"]).max())
    per_type = [max(er[d["f_rtype"] == t].max() / sr, ev[d["f_rtype"] == t].max() / sv) for t in range(len(d["f_type_names"]))]
    print("shape gradient against the reference's autograd, worst |difference| / scale per record type:",
          dict(zip(d["f_type_names"].tolist(), ["%.2g" % e for e in per_type])))
    assert np.abs(d["f_d_rad"]).max() > 0.1 and np.abs(d["f_d_verts"]).max() > 0.1
    assert er.max() <= 1e-12 * sr, er.max() / sr
    assert ev.max() <= 1e-12 * sv, ev.max() / sv
    # circles have no vertex gradient, hulls no radius gradient, vertex slots beyond nverts are zero
    kind, nv = d["f_kind"], d["f_nverts"]
    assert np.abs(d_rad[::rep][kind == 1]).max() == 0.0 and np.abs(d_verts[::rep][kind == 0]).max() == 0.0
    assert np.abs(d_verts[::rep] * (np.arange(16)[None, None, :] >= nv[..., None])[..., None]).max() == 0.0


def test_narrow_and_wide_layouts_give_the_same_bits():
    """The configurations whose hulls have at most 8 vertices through the layout of the lcp_contacts.hip entries (capacity 8) and
    through a wide layout (capacity 16): one kernel, the same gradients bit for bit."""
    d = _fixture()
    sel = np.nonzero(d["f_nverts"].max(axis=1) <= 8)[0]
    assert len(sel) >= 100
    cb8, r8, v8 = _frame_grads(d, sel, 8)
    cb16, r16, v16 = _frame_grads(d, sel, 16)
    assert torch.equal(cb8.count, cb16.count) and torch.equal(cb8.c_n, cb16.c_n)
    assert np.array_equal(r8, r16) and np.array_equal(v8, v16[:, :, :8]) and np.abs(v16[:, :, 8:]).max() == 0.0
    assert np.abs(v8).max() > 0.1


def test_outputs_are_optional_written_not_accumulated_and_zero_beyond_scene_verts_max():
    from lcp_physics_amd.physics import contacts as ct
    d = _fixture()
    sel = np.arange(d["f_count"].shape[0])
    geom, p, gs = _frame_batch(d, sel, 16, 1)
    cb = ct.find_contacts(geom, p, maxc=2, eps=float(d["f_eps"]))
    both = ct.contact_frame_backward_shape(geom, p, cb, *gs, eps=float(d["f_eps"]))
    again = ct.contact_frame_backward_shape(geom, p, cb, *gs, eps=float(d["f_eps"]))
    only_r = ct.contact_frame_backward_shape(geom, p, cb, *gs, eps=float(d["f_eps"]), want_verts=False)
    only_v = ct.contact_frame_backward_shape(geom, p, cb, *gs, eps=float(d["f_eps"]), want_radius=False)
    assert only_r[1] is None and only_v[0] is None
    assert torch.equal(both[0], again[0]) and torch.equal(both[1], again[1])
    assert torch.equal(both[0], only_r[0]) and torch.equal(both[1], only_v[1])
    # a bound on the scene's vertices that the two 16-gons exceed: those scenes get zeros, the others their gradient
    small = ct.GeometryBatch(geom.kind, geom.radius, geom.verts_local, geom.nverts, None, 20)
    z = ct.contact_frame_backward_shape(small, p, cb, *gs, eps=float(d["f_eps"]))
    over = torch.tensor(d["f_nverts"].sum(axis=1) > 20, device=DEV)
    assert bool(over.any()) and float(z[1][over].abs().max()) == 0.0 and float(z[0][over].abs().max()) == 0.0
    assert torch.equal(z[1][~over], both[1][~over]) and torch.equal(z[0][~over], both[0][~over])


def _learnable(geom, radius=True, verts=False):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    rad = geom.radius.detach().clone().requires_grad_(radius)
    vl = geom.verts_local.detach().clone().requires_grad_(verts)
    return GeometryBatch(geom.kind, rad, vl, geom.nverts, geom.no_contact, geom.scene_verts_max), rad, vl


FP32_EPS = 2.0 ** -24


def _rel(got, ref):
    """Per scene: max |got - ref| / max |ref| - the measure of the force-gradient roll-out tests.  The cotangents that reach the
    contact frame are fp32 (lcp_step_backward_f32), so a scene whose reference gradient lies below fp32 rounding of the scene set's
    largest gradient - zero by symmetry: exactly 0, or the 1e-16 .. 1e-18 that fp64 cancellation left in the reference - has no
    resolvable scale of its own and is measured against the set's largest gradient instead."""
    den, top = np.abs(ref).max(axis=1), np.abs(ref).max()
    return np.abs(got - ref).max(axis=1) / np.where(den > FP32_EPS * top, den, top)


def test_rollout_radius_gradient_of_the_three_balls_matches_the_reference_autograd():
    """The batched `grad_demo` of test_rollout_gradient_matches_the_reference_autograd with the balls' radii as leaves: 36
    differentiable steps, loss = |target - ball|, d(loss)/d(radius of each ball) against the reference's autograd on the eight scenes
    (fixture `b_*`).  Same trajectory checks; the gradient gate is that test's, 1e-4 relative per scene (`_rel`: five scenes have
    no spin anywhere, the arms' dependence on the radii reaches nothing and the reference's gradient is exactly zero)."""
    from tests.test_hip_contacts import _rollout_world
    d0 = _fixture()
    d = {k[2:]: d0[k] for k in d0.files if k.startswith("b_")}
    d.update(mult=d0["mult"], t_push=d0["t_push"], dt=d0["dt"])
    rep = 16
    world, _ = _rollout_world(d, rep, requires_grad=False)
    world.geom, rad, _ = _learnable(world.geom)
    ncs = []
    for _ in range(int(d["nsteps"])):
        world.step(differentiable=True)
        ncs.append(world.contacts.count.clone())
    a, b = [int(i) for i in d["loss_bodies"]]
    pos = world.p[:, :, 1:]
    loss = (pos[:, a] - pos[:, b]).norm(dim=1)
    loss.sum().backward()
    torch.cuda.synchronize()
    assert np.abs(world.t.cpu().numpy()[::rep] - d["t"][:, -1]).max() < 1e-12
    assert (torch.stack(ncs, 1).cpu().numpy()[::rep] == d["ncontacts"]).all()
    assert np.abs(world.p.detach().cpu().numpy()[::rep] - d["p_final"]).max() <= 1e-4
    assert np.abs(loss.detach().cpu().numpy()[::rep] - d["loss"]).max() <= 1e-5 * np.abs(d["loss"]).max()
    gr = rad.grad.cpu().numpy()
    assert np.abs(gr.reshape(-1, rep, 3) - gr[::rep][:, None]).max() == 0.0          # replicas are bitwise replicas
    ref = d["grad_rad"]
    assert np.abs(ref).max() > 1e-4
    err = _rel(gr[::rep], ref)
    print("ball roll-out, d(loss)/d(radius): relative error per scene", np.array2string(err, precision=2))
    print(np.array2string(gr[::rep], precision=6)); print(np.array2string(ref, precision=6))
    assert err.max() <= 1e-4, err


def _box_world(d, rep, post=None):
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.contacts import GeometryBatch
    nv = d["force_ball"].shape[0]
    B = nv * rep
    rp = lambda a, dt_: torch.tensor(np.repeat(a, rep, axis=0), dtype=dt_, device=DEV)
    shapes = [("rect", tuple(d["floor_dims"][0])), ("circle", float(d["ball_rad"][0])), ("hull", d["box_verts"][0])]
    geom, rad, vl = _learnable(GeometryBatch.from_shapes(shapes, B).to(DEV), True, True)
    grav = rp(d["gravity"], torch.float32)
    fb, fx = rp(d["force_ball"], torch.float32), rp(d["force_box"], torch.float32)
    mult, t_push = float(d["mult"]), float(d["t_push"])

    def force_fn(t):
        on = (t < t_push).to(torch.float32).unsqueeze(1)
        z = torch.zeros(B, 1, 3, dtype=torch.float32, device=DEV)
        return grav + torch.cat([z, (fb * mult * on).unsqueeze(1), (fx * mult * on).unsqueeze(1)], dim=1)

    world = ContactWorld(geom, rp(d["p0"], torch.float64), rp(d["v0"], torch.float32), rp(d["Mdiag"], torch.float32),
                         torch.zeros(B, 3, 3, device=DEV), rp(d["rest"], torch.float32), rp(d["fric"], torch.float32),
                         Je=rp(d["Je"], torch.float32), dt=float(d["dt"]), maxc=8, force_fn=force_fn)
    return world, rad, vl


def test_rollout_shape_gradient_through_hull_contacts_matches_the_reference_autograd():
    """The ball / box / floor scene of test_rollout_gradient_through_hull_contacts_matches_the_reference_autograd with the box a
    `Hull` whose four vertices are leaves and the ball's radius a leaf (fixture `x_*`, six scenes, 40 steps, loss = |ball - box|):
    d(loss)/d(ball radius, box vertices) through circle / hull and hull / hull records against the reference's autograd.  Scenes
    whose every dt-halving and contact-count decision matched the reference's are compared, at most one may fall off; the gradient
    gate is that test's: 1e-5 relative per scene (`_rel`: in two scenes the box is never turned and the reference's gradient is what
    fp64 cancellation left of zero, 1e-16 .. 1e-18)."""
    d0 = _fixture()
    d = {k[2:]: d0[k] for k in d0.files if k.startswith("x_")}
    d.update(mult=d0["mult"], t_push=d0["t_push"], dt=d0["dt"])
    nv, rep = d["force_ball"].shape[0], 16
    world, rad, vl = _box_world(d, rep)
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
    assert same.sum() >= nv - 1
    pf = world.p.detach().cpu().numpy()[::rep]
    assert np.abs(pf - d["p_final"])[same].max() <= 5e-4, np.abs(pf - d["p_final"])[same].max()
    gr, gv = rad.grad.cpu().numpy(), vl.grad.cpu().numpy()
    for g in (gr, gv):                                                               # replicas are bitwise replicas
        assert np.abs(g.reshape((nv, rep) + g.shape[1:]) - g[::rep][:, None]).max() == 0.0
    assert np.abs(gr[:, [0, 2]]).max() == 0.0 and np.abs(gv[:, 1]).max() == 0.0 and np.abs(gv[:, :, 4:]).max() == 0.0
    got = np.concatenate([gr[::rep, 1:2], gv[::rep, 2, :4].reshape(nv, 8)], axis=1)
    ref = np.concatenate([d["grad_rad"][:, None], d["grad_verts"].reshape(nv, 8)], axis=1)
    err = _rel(got, ref)
    print("hull roll-out, d(loss)/d(ball radius, box vertices): relative error per scene", np.array2string(err, precision=2))
    print(np.array2string(got, precision=5)); print(np.array2string(ref, precision=5))
    assert err[same].max() <= 1e-5, err


def _chain_shape_grad(post_stab, steps=30):
    from lcp_physics_amd import scenes
    B = 8
    chains = scenes.ChainWorlds(B, links=4, device=DEV, post_stab=post_stab)
    chains.geom, rad, vl = _learnable(chains.geom, True, True)
    target = chains.p0 + torch.tensor([0.2, 20.0, -5.0], dtype=torch.float64, device=DEV)
    world = chains.world(torch.linspace(0.5, 1.6, B, device=DEV),
                         torch.tensor([0.0, 1.0, 0.05], device=DEV) * torch.linspace(0.8, 1.3, B, device=DEV).unsqueeze(1))
    for _ in range(steps):
        world.step(differentiable=True)
    ((world.p - target) ** 2).mean(dim=(1, 2)).sum().backward()
    torch.cuda.synchronize()
    return rad.grad, vl.grad


def test_shape_gradient_with_post_stabilisation_has_the_second_frame_nodes_share():
    """The jointed chain hit by a projectile (scenes.ChainWorlds, the scene of the post-stabilisation fixtures): with post_stab the
    step has a second frame node (world.py:109-121) that takes the shape as an input too; the gradient of the links' vertices is
    finite, not zero, and not the one of the run without post-stabilisation.  (The projectile's radius has no gradient here, as in
    the reference: n, p1, p2 of a circle / hull record do not depend on it, contacts.py:106-138 - only the penetration does, which
    nothing differentiates.)"""
    r1, v1 = _chain_shape_grad(True)
    r0, v0 = _chain_shape_grad(False)
    for g in (r1, v1, r0, v0):
        assert bool(torch.isfinite(g).all())
    assert float(v1.abs().max()) > 0.0 and float(v0.abs().max()) > 0.0 and not torch.equal(v1, v0)
    assert float(r1.abs().max()) == 0.0 and float(r0.abs().max()) == 0.0


def test_differentiable_rollout_with_a_learnable_radius_captured_in_a_hip_graph_equals_the_eager_run():
    """test_differentiable_rollout_captured_in_a_hip_graph_equals_the_eager_run with `radius` and `verts_local` requiring grad: the roll-out, the loss
    and the backward - now with lcp_contact_frame_backward_shape_f64 at both frame nodes of every step - in one HIP graph; replayed
    with new parameter values it returns the eager run's loss and gradients bit for bit."""
    from lcp_physics_amd import scenes
    B, links, steps = 8, 4, 30                                   # (the projectile reaches the chain after some twenty steps)
    chains = scenes.ChainWorlds(B, links=links, device=DEV)
    base = chains.geom
    target = chains.p0 + torch.tensor([0.2, 20.0, -5.0], dtype=torch.float64, device=DEV)

    def loss_of(mass, push, rad, vl):
        from lcp_physics_amd.physics.contacts import GeometryBatch
        chains.geom = GeometryBatch(base.kind, rad, vl, base.nverts, base.no_contact, base.scene_verts_max)
        world = chains.world(mass, push)
        for _ in range(steps):
            world.step(differentiable=True)
        return ((world.p - target) ** 2).mean(dim=(1, 2))

    mass = torch.linspace(0.5, 1.6, B, device=DEV).requires_grad_(True)
    push = (torch.tensor([0.0, 1.0, 0.05], device=DEV) * torch.linspace(0.8, 1.3, B, device=DEV).unsqueeze(1)).requires_grad_(True)
    rad = base.radius.detach().clone().requires_grad_(True)
    vl = base.verts_local.detach().clone().requires_grad_(True)
    if hasattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch"):
        torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            mass.grad = push.grad = rad.grad = vl.grad = None
            loss_of(mass, push, rad, vl).sum().backward()
    torch.cuda.current_stream().wait_stream(side)
    mass.grad = push.grad = rad.grad = vl.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss_g = loss_of(mass, push, rad, vl)
        loss_g.sum().backward()
    with torch.no_grad():                                        # new parameter values in the captured tensors
        mass.mul_(1.1); push.mul_(0.95); rad.mul_(1.001)
    g.replay()
    torch.cuda.synchronize()
    got = (loss_g.clone(), mass.grad.clone(), push.grad.clone(), rad.grad.clone(), vl.grad.clone())
    m2, p2, r2, v2 = [t.detach().clone().requires_grad_(True) for t in (mass, push, rad, vl)]
    loss_e = loss_of(m2, p2, r2, v2)
    loss_e.sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(got[0], loss_e.detach()) and torch.equal(got[1], m2.grad) and torch.equal(got[2], p2.grad)
    assert torch.equal(got[3], r2.grad) and torch.equal(got[4], v2.grad) and float(v2.grad.abs().max()) > 0.0


def test_constant_geometry_launches_no_shape_kernel_and_keeps_the_pose_gradient(monkeypatch):
    """A world whose geometry does not require grad: no call of `contact_frame_backward_shape`, and the frame node's pose gradient is
    `contact_frame_backward` called directly, bit for bit.  With a learnable radius the same roll-out calls it at every frame node."""
    from lcp_physics_amd.physics import contacts as ct
    calls = []
    real = ct.contact_frame_backward_shape
    monkeypatch.setattr(ct, "contact_frame_backward_shape", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    d = _fixture()
    geom, p, gs = _frame_batch(d, np.arange(d["f_count"].shape[0]), 16, 1)
    cb = ct.find_contacts(geom, p, maxc=2, eps=float(d["f_eps"]))
    pl = p.clone().requires_grad_(True)
    outs = ct.ContactFrameFunction.apply(pl, geom, cb, float(d["f_eps"]))
    sum((o * g).sum() for o, g in zip(outs, gs)).backward()
    direct = ct.contact_frame_backward(geom, p, cb, *gs, eps=float(d["f_eps"]))
    assert not calls and torch.equal(pl.grad, direct) and float(direct.abs().max()) > 0.0
    # the same node with the shape as an input: the pose gradient keeps its bits, the shape gradient is the direct call's
    g2, rad, vl = _learnable(geom, True, True)
    pl2 = p.clone().requires_grad_(True)
    outs = ct.ContactFrameFunction.apply(pl2, g2, cb, float(d["f_eps"]), rad, vl)
    sum((o * g).sum() for o, g in zip(outs, gs)).backward()
    dr, dv = real(geom, p, cb, *gs, eps=float(d["f_eps"]))
    assert len(calls) == 1 and torch.equal(pl2.grad, direct) and torch.equal(rad.grad, dr) and torch.equal(vl.grad, dv)
    # worlds
    d0 = _fixture()
    dx = {k[2:]: d0[k] for k in d0.files if k.startswith("x_")}
    dx.update(mult=d0["mult"], t_push=d0["t_push"], dt=d0["dt"])
    grads = []
    for learn in (False, True):
        del calls[:]
        world, rad, vl = _box_world(dx, 2)
        if not learn:
            world.geom = ct.GeometryBatch(world.geom.kind, rad.detach(), vl.detach(), world.geom.nverts, None, world.geom.scene_verts_max)
        v0 = world.v.clone().requires_grad_(True)
        world.v = v0
        for _ in range(12):
            world.step(differentiable=True)
        world.p[:, 1:, 1:].sum().backward()
        torch.cuda.synchronize()
        grads.append(v0.grad.clone())
        assert (len(calls) > 0) == learn, len(calls)
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0.0
