"""Generate tests/golden/fixed_dt.npz: the UNMODIFIED reference `World` stepped with `world.step(fixed_dt=True)`
(physics/world.py:72-80: `end_t = t + dt; while t < end_t: step_dt(end_t - t)`).  TEST INFRASTRUCTURE ONLY; needs the
reference tree (oracle/ref_shim.py) and runs on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_fixed_dt_golden.py

The sub-steps are recorded by wrapping `step_dt` on the world INSTANCE; no reference file is touched.

(a) `w_*` (one entry per field, the scenes concatenated; tests/fixed_dt_io.py unpacks): the ten scenes of oracle/make_golden_world.py (`_scenes()`: contact creation, dt halving, the non-strict
    floor, revolute and fixed joints, a time-dependent force, post-stabilisation) with the same step counts.  Per step: p, v, t,
    contact count, number of sub-steps; per sub-step (flat, `sub_step` = the step it belongs to): dt asked, t after, f(t) the solve
    saw; and what a ContactWorld needs to rebuild the scene (the fields of world_traj.npz).  The time-dependent forces of these
    scenes switch off at t = 0.1 (forces.py:14-18): `f` / `f_off` / `t_switch` restate that, checked against every recorded f(t).
(b) `g_*`: the eight `grad_demo` scenes of oracle/make_golden_rollout.py (`make_world`, `FORCES`), 36 steps: per-step sub-step
    counts, clocks and contact counts, final poses, loss and d(loss)/d(force) from the reference's autograd through the sub-steps.

The generator asserts that every scene has a step with more than one sub-step, that the eight scenes of (b) do not all take
the same counts, and that a second run reproduces counts and clocks.
"""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import make_golden_rollout as R  # noqa: E402
from oracle import make_golden_world as GW  # noqa: E402
from oracle import ref_shim  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "fixed_dt.npz")
T_SWITCH = 0.1                                     # forces.py:14-18


def spy_on_substeps(world, nb):
    """Wrap `world.step_dt`: every call appends (dt asked, t after, f(t) of its solve) to the list returned."""
    inner = world.step_dt
    subs = []

    def step_dt(dt):
        f = world.apply_forces(world.t).reshape(nb, 3).detach().numpy().copy()
        inner(dt)
        subs.append((float(dt), float(world.t), f))
    world.step_dt = step_dt
    return subs


def record_world(name, make):
    from lcp_physics.physics import constraints as C_
    from lcp_physics.physics.bodies import Circle
    from lcp_physics.physics.world import World
    random.seed(0)
    bodies, joints, nsteps, strict = make()
    post_stab = name.endswith("_poststab")
    world = World(bodies, joints, dt=1.0 / 30, strict_no_penetration=strict, post_stab=post_stab)
    nb = len(bodies)
    f_on = world.apply_forces(0).reshape(nb, 3).numpy().copy()
    f_off = world.apply_forces(1e9).reshape(nb, 3).numpy().copy()
    jt = {C_.Joint: 1, C_.FixedJoint: 2, C_.XConstraint: 3, C_.YConstraint: 4, C_.RotConstraint: 5, C_.TotalConstraint: 6}
    rec = dict(kind=np.array([0 if isinstance(b, Circle) else 1 for b in bodies]),
               size=np.array([[float(b.rad), 0.0] if isinstance(b, Circle) else b.dims.numpy().tolist() for b in bodies]),
               dt=np.float64(world.dt), strict=np.int64(strict), post_stab=np.int64(post_stab), eps=np.float64(float(world.eps)),
               tol=np.float64(float(world.tol)), Mdiag=torch.diagonal(world.M()).reshape(nb, 3).numpy().copy(),
               f=f_on, f_off=f_off, t_switch=np.float64(T_SWITCH),
               rest=np.array([float(b.restitution) for b in bodies]), fric=np.array([float(b.fric_coeff) for b in bodies]),
               Je=world.Je().numpy().copy(),
               jtype=np.array([jt[type(j[0])] for j in world.joints]), jb1=np.array([j[1] for j in world.joints]),
               jb2=np.array([-1 if j[2] is None else j[2] for j in world.joints]),
               jr1=np.array([float(j[0].r1) if isinstance(j[0], C_.Joint) else 0.0 for j in world.joints]),
               jrot1=np.array([float(j[0].rot1) if isinstance(j[0], C_.Joint) else 0.0 for j in world.joints]),
               no_contact=np.array([[i, k] for i, b in enumerate(bodies) for k, o in enumerate(bodies)
                                    if o.geom in b.geom.no_contact], dtype=np.int64).reshape(-1, 2))
    subs = spy_on_substeps(world, nb)
    snap = lambda: (torch.stack([b.p for b in bodies]).numpy().copy(), world.get_v().reshape(nb, 3).numpy().copy())
    p, v = snap()
    P, V, T, NC, NS, SS = [p], [v], [float(world.t)], [len(world.contacts)], [], []
    for k in range(nsteps):
        before = len(subs)
        world.step(fixed_dt=True)
        p, v = snap()
        P.append(p); V.append(v); T.append(float(world.t)); NC.append(len(world.contacts))
        NS.append(len(subs) - before)
        SS += [k] * NS[-1]
    rec.update(p=np.stack(P), v=np.stack(V), t=np.array(T), ncontacts=np.array(NC), nsub=np.array(NS), sub_step=np.array(SS),
               sub_dt=np.array([s[0] for s in subs]), sub_t=np.array([s[1] for s in subs]), sub_f=np.stack([s[2] for s in subs]))
    return rec


def check_force_rule(rec):
    """f(t) of every sub-step is `f` while the clock it started at is below t_switch, `f_off` from then on."""
    t_start = np.concatenate([[rec["t"][0]], rec["sub_t"][:-1]])
    for k in range(len(rec["sub_dt"])):
        want = rec["f"] if t_start[k] < float(rec["t_switch"]) else rec["f_off"]
        assert np.array_equal(rec["sub_f"][k], want), ("force rule", k, t_start[k])


def record_rollout(force0):
    from lcp_physics.physics.forces import ExternalForce
    f0 = torch.tensor(force0, dtype=torch.float64, requires_grad=True)
    world, c, target = R.make_world(lambda t: f0 if t < R.T_PUSH else ExternalForce.ZEROS)
    nb = len(world.bodies)
    rec = dict(Mdiag=torch.diagonal(world.M()).reshape(nb, 3).detach().numpy().copy(),
               rest=np.array([float(b.restitution) for b in world.bodies]), fric=np.array([float(b.fric_coeff) for b in world.bodies]),
               rad=np.array([float(b.rad) for b in world.bodies]),
               p0=torch.stack([b.p for b in world.bodies]).detach().numpy().copy(),
               v0=world.get_v().reshape(nb, 3).detach().numpy().copy())
    inner = world.step_dt
    calls = []

    def step_dt(dt):
        inner(dt)
        calls.append(float(dt))
    world.step_dt = step_dt
    ncs, ts, ns = [], [], []
    for _ in range(R.NSTEPS):
        before = len(calls)
        world.step(fixed_dt=True)
        ncs.append(len(world.contacts)); ts.append(float(world.t)); ns.append(len(calls) - before)
    dist = (target.pos - c.pos).norm()
    dist.backward()
    rec.update(p_final=torch.stack([b.p for b in world.bodies]).detach().numpy().copy(),
               v_final=world.get_v().reshape(nb, 3).detach().numpy().copy(), loss=np.float64(float(dist)), grad=f0.grad.numpy().copy(),
               ncontacts=np.array(ncs), t=np.array(ts), nsub=np.array(ns))
    return rec


def main():
    ref_shim.load_reference()
    torch.set_default_dtype(torch.float64)
    flat, names, recs_w = {}, [], []
    for name, make in GW._scenes().items():
        rec = record_world(name, make)
        again = record_world(name, make)
        assert np.array_equal(rec["nsub"], again["nsub"]) and np.array_equal(rec["t"], again["t"]), (name, "not reproducible")
        assert np.array_equal(rec["sub_dt"], again["sub_dt"]) and np.array_equal(rec["ncontacts"], again["ncontacts"]), name
        check_force_rule(rec)
        assert int(rec["nsub"].max()) > 1, (name, "no step with more than one sub-step")
        assert np.abs(rec["t"][1:] - rec["dt"] * np.arange(1, len(rec["t"]))).max() < 1e-12, (name, "clock off the grid")
        names.append(name)
        recs_w.append(rec)
        print(name, "steps", len(rec["nsub"]), "sub-steps per step", rec["nsub"].tolist(), "min sub dt %.3e" % rec["sub_dt"].min())
    # one entry per FIELD (an .npz entry costs ~200 bytes of zip bookkeeping; 28 fields x 10 scenes of mostly tiny arrays would be
    # half the file): the scenes' arrays flattened and concatenated, their shapes in one table (tests/fixed_dt_io.py unpacks)
    keys = sorted(recs_w[0])
    shapes = np.zeros((len(names), len(keys), 4), dtype=np.int64)       # (ndim, dims ...)
    for i, rec in enumerate(recs_w):
        for j, k in enumerate(keys):
            a = np.asarray(rec[k])
            shapes[i, j, 0] = a.ndim
            shapes[i, j, 1:1 + a.ndim] = a.shape
    for k in keys:
        flat["w_" + k] = np.concatenate([np.asarray(rec[k]).reshape(-1) for rec in recs_w])
    flat.update(w_names=np.array(names), w_keys=np.array(keys), w_shapes=shapes)
    recs = [record_rollout(f) for f in R.FORCES]
    again = [record_rollout(f) for f in R.FORCES]
    for a, b in zip(recs, again):
        assert np.array_equal(a["nsub"], b["nsub"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["ncontacts"], b["ncontacts"])
        assert int(a["nsub"].max()) > 1
    nsub = np.stack([r["nsub"] for r in recs])
    assert any(len(set(nsub[:, k].tolist())) > 1 for k in range(nsub.shape[1])), "the eight scenes take the same counts everywhere"
    flat.update({"g_" + k: np.stack([r[k] for r in recs]) for k in recs[0]})
    flat.update(g_force0=np.array(R.FORCES), g_nsteps=np.int64(R.NSTEPS), g_t_push=np.float64(R.T_PUSH), g_mult=np.float64(R.MULT),
                g_dt=np.float64(1.0 / 30), g_no_contact=np.array([[0, 1], [0, 2]]), g_pushed_body=np.int64(1),
                g_loss_bodies=np.array([0, 2]))
    for i, r in enumerate(recs):
        print("force", R.FORCES[i], "loss %.4f" % r["loss"], "grad", np.array2string(r["grad"], precision=5), "sub-steps",
              r["nsub"].tolist())
    np.savez_compressed(OUT, **flat)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
