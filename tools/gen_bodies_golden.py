"""Generate tests/golden/bodies.npz: what the UNMODIFIED reference's body constructors - `Circle`, `Rect`, `Hull`
(physics/bodies.py:15-290) with `Gravity` attached (forces.py:51-67) - compute from shape and mass, and what its autograd gives
the raw shape and the mass.  TEST INFRASTRUCTURE ONLY; needs the reference tree (oracle/ref_shim.py) and runs on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_bodies_golden.py

Unlike tools/gen_shape_grad_golden.py the leaves are set BEFORE construction, so every path of the constructors is recorded:
centroid, recentred vertices, position, inertia, mass matrix, gravity.

(a) module level, `m_*`: circles, rects and hulls of nv in NV_CHOICES (polygons as `_convex` of the shape-gradient generator,
    radii 15 .. 35, every other one offset from its reference point by up to 300 in each coordinate), masses 0.5 .. 5.  Values:
    pos - ref_point, `verts`, `ang_inertia`, diag `M`, the gravity force; random cotangents on all of them (fp32-representable on
    `M` and the force: those outputs are fp32 in the product); the reference's autograd for d/d(raw vertices, rad, dims, mass).
    Self-check: every hull is evaluated again with its vertex list cyclically shifted by nv / 2 - the same polygon in another
    summation order; values and gradients must agree within SHIFT_TOL = 1e-13 x max(1, largest |value| of the case's quantity) or the
    case is rejected (`m_rejected` counts them).
(b) roll-out level, `r_*`: the ball / box-as-`Hull` / floor scene of the `x_*` records of tests/golden/shape_grad.npz, the box's raw
    vertices given relative to a reference point that is NOT its centroid, six scenes, 40 steps, loss = |ball - box|.  Leaves before
    construction: the box's raw vertices, the ball's radius, both masses; `Gravity` through `add_force`.  d(loss)/d(each leaf),
    per-step contact counts, clocks, final poses.  Every roll-out is run twice and must reproduce itself.
"""
import math
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import make_golden_rollout as R  # noqa: E402
from oracle import ref_shim  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "bodies.npz")
NV_CHOICES = [3, 4, 5, 6, 8, 12, 16, 31, 32, 33, 64]
PER_NV, N_RECT, N_CIRCLE = 7, 20, 23
CAP = 64
G = 100.0
SHIFT_TOL = 1e-13
SEED = 20240911
KIND_CIRCLE, KIND_RECT, KIND_HULL = 0, 1, 2


def _convex(rng, nv):
    """A convex polygon in the reference's vertex order: points of an ellipse at increasing, jittered angles."""
    a, b = rng.uniform(15, 35, 2)
    th = (np.arange(nv) + rng.uniform(-0.3, 0.3, nv)) * (2 * math.pi / nv) + rng.uniform(0, 2 * math.pi)
    return np.stack([a * np.cos(th), b * np.sin(th)], 1)


def _f32(rng, n):
    return rng.standard_normal(n).astype(np.float32).astype(np.float64)


def evaluate(kind, shape, mass, ref, cot):
    """Construct the body from leaves, attach Gravity, return (values, gradients) as numpy."""
    from lcp_physics.physics.bodies import Circle, Hull, Rect
    from lcp_physics.physics.forces import Gravity
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    m = t(mass).requires_grad_(True)
    if kind == KIND_CIRCLE:
        leaf = t(shape).requires_grad_(True)
        body = Circle(list(ref), leaf, mass=m)
        verts = torch.zeros(0, 2)
    elif kind == KIND_RECT:
        leaf = t(shape).requires_grad_(True)
        body = Rect(list(ref), leaf, mass=m)
        verts = torch.stack(body.verts)
    else:
        leaf = [t(v).requires_grad_(True) for v in shape]
        body = Hull(list(ref), leaf, mass=m)
        verts = torch.stack(body.verts)
    grav = Gravity(g=G)
    body.add_force(grav)
    force = body.apply_forces(0.0)
    val = dict(centroid=body.pos - t(ref), verts=verts, inertia=body.ang_inertia.reshape(()), Mdiag=torch.diagonal(body.M), f=force)
    assert float((body.M - torch.diag(torch.diagonal(body.M))).abs().max()) == 0.0 and float(body.p[0]) == 0.0
    loss = sum((t(cot[k][:v.shape[0]] if k == "verts" else cot[k]) * v).sum() for k, v in val.items())
    loss.backward()
    if kind == KIND_HULL:
        d_shape = np.stack([np.zeros(2) if v.grad is None else v.grad.numpy() for v in leaf])
    else:
        d_shape = leaf.grad.numpy().copy()
    return {k: v.detach().numpy().copy() for k, v in val.items()}, dict(shape=d_shape, mass=float(m.grad))


def module_level(rng):
    plan = [KIND_CIRCLE] * N_CIRCLE + [KIND_RECT] * N_RECT + [(KIND_HULL, nv) for nv in NV_CHOICES for _ in range(PER_NV)]
    keys = ("kind", "nverts", "radius", "dims", "verts_raw", "mass", "ref", "centroid", "verts", "inertia", "Mdiag", "f", "g_centroid",
            "g_verts", "g_inertia", "g_Mdiag", "g_f", "d_verts_raw", "d_radius", "d_dims", "d_mass")
    rec = {k: [] for k in keys}
    rejected, worst = 0, 0.0
    i = 0
    while i < len(plan):
        item = plan[i]
        kind, nv = (item, 4 if item == KIND_RECT else 0) if not isinstance(item, tuple) else item
        mass = float(rng.uniform(0.5, 5.0))
        ref = rng.uniform(100, 900, 2)
        cot = dict(centroid=rng.standard_normal(2), verts=rng.standard_normal((CAP, 2)), inertia=float(rng.standard_normal()),
                   Mdiag=_f32(rng, 3), f=_f32(rng, 3))
        radius, dims, raw = 0.0, np.zeros(2), np.zeros((CAP, 2))
        if kind == KIND_CIRCLE:
            radius = float(rng.uniform(10, 35))
            shape = radius
        elif kind == KIND_RECT:
            dims = rng.uniform(10, 70, 2)
            shape = dims
        else:
            shape = _convex(rng, nv) + (rng.uniform(-300, 300, 2) if rng.integers(0, 2) else 0.0)
        val, grad = evaluate(kind, shape, mass, ref, cot)
        if kind == KIND_HULL:                                    # the same polygon summed in another order
            s = nv // 2
            cot2 = dict(cot, verts=np.concatenate([np.roll(cot["verts"][:nv], -s, axis=0), cot["verts"][nv:]]))
            val2, grad2 = evaluate(kind, np.roll(shape, -s, axis=0), mass, ref, cot2)
            val2["verts"], grad2["shape"] = np.roll(val2["verts"], s, axis=0), np.roll(grad2["shape"], s, axis=0)
            pairs = [(val[k], val2[k]) for k in val] + [(grad["shape"], grad2["shape"]), (grad["mass"], grad2["mass"])]
            spread = max(float(np.abs(np.asarray(a) - np.asarray(b)).max()) / max(1.0, float(np.abs(np.asarray(a)).max())) for a, b in pairs)
            if spread > SHIFT_TOL:
                rejected += 1
                continue
            worst = max(worst, spread)
            raw[:nv] = shape
        if kind == KIND_RECT:                                    # bodies.py:260-262
            h = dims / 2
            raw[:4] = np.stack([h, h * np.array([-1.0, 1.0]), -h, -h * np.array([-1.0, 1.0])])
        pad = lambda a: np.concatenate([a, np.zeros((CAP - a.shape[0], 2))])
        vals = dict(kind=np.int32(kind), nverts=np.int32(nv), radius=radius, dims=dims, verts_raw=raw, mass=mass, ref=ref,
                    centroid=val["centroid"], verts=pad(val["verts"]), inertia=float(val["inertia"]), Mdiag=val["Mdiag"], f=val["f"],
                    g_centroid=cot["centroid"], g_verts=cot["verts"] * (np.arange(CAP) < nv)[:, None], g_inertia=cot["inertia"],
                    g_Mdiag=cot["Mdiag"], g_f=cot["f"], d_verts_raw=pad(grad["shape"]) if kind == KIND_HULL else np.zeros((CAP, 2)),
                    d_radius=float(grad["shape"]) if kind == KIND_CIRCLE else 0.0,
                    d_dims=grad["shape"] if kind == KIND_RECT else np.zeros(2), d_mass=grad["mass"])
        for k in keys:
            rec[k].append(vals[k])
        i += 1
    out = {"m_" + k: np.stack([np.asarray(v) for v in vs]) for k, vs in rec.items()}
    out.update(m_g=np.float64(G), m_rejected=np.int64(rejected), m_shift_tol=np.float64(SHIFT_TOL), m_shift_worst=np.float64(worst))
    print("module level: %d bodies (%d circles, %d rects, %d hulls of %s vertices), %d rejected by the shifted-order check, worst "
          "accepted spread %.2g" % (len(plan), N_CIRCLE, N_RECT, len(NV_CHOICES) * PER_NV, NV_CHOICES, rejected, worst))
    return out


BOX = np.array([[20.0, 20.0], [-20.0, 20.0], [-20.0, -20.0], [20.0, -20.0]])    # the 40 x 40 box of the `x_*` records
BOX_OFFSET = np.array([7.0, -3.0])                                              # raw vertices = BOX + offset, reference point = centre - offset
BOX_CENTRE = np.array([470.0, 474.5])


def run_box(fb, fx):
    from lcp_physics.physics.bodies import Circle, Hull, Rect
    from lcp_physics.physics.constraints import TotalConstraint
    from lcp_physics.physics.forces import ExternalForce, Gravity
    from lcp_physics.physics.world import World
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    f1, f2 = t(fb), t(fx)
    rad = t(20.0).requires_grad_(True)
    verts = [t(v).requires_grad_(True) for v in BOX + BOX_OFFSET]
    m_ball, m_box = t(1.0).requires_grad_(True), t(1.0).requires_grad_(True)
    floor = Rect([500, 500], [900, 10])
    ball = Circle([380, 468], rad, mass=m_ball, restitution=0.3, fric_coeff=0.6)
    box = Hull(list(BOX_CENTRE - BOX_OFFSET), verts, mass=m_box, restitution=0.2, fric_coeff=0.4)
    for b, f in ((ball, f1), (box, f2)):
        b.add_force(Gravity(g=G))
        b.add_force(ExternalForce(lambda tt, f=f: f if tt < R.T_PUSH else ExternalForce.ZEROS, multiplier=R.MULT))
    world = World([floor, ball, box], [TotalConstraint(floor)], dt=1.0 / 30)
    rec = dict(Je=world.Je().detach().numpy().copy(), p0=torch.stack([b.p for b in world.bodies]).detach().numpy().copy(),
               Mdiag=torch.diagonal(world.M()).reshape(3, 3).detach().numpy().copy())
    ncs, ts = [], []
    for _ in range(R.H_NSTEPS):
        world.step()
        ncs.append(len(world.contacts)); ts.append(float(world.t))
    dist = (ball.pos - box.pos).norm()
    dist.backward()
    g = lambda x: 0.0 if x.grad is None else float(x.grad)
    rec.update(p_final=torch.stack([b.p for b in world.bodies]).detach().numpy().copy(), loss=np.float64(float(dist)),
               grad_rad=np.float64(g(rad)), grad_verts=np.stack([np.zeros(2) if v.grad is None else v.grad.numpy() for v in verts]),
               grad_mass=np.array([g(m_ball), g(m_box)]), ncontacts=np.array(ncs), t=np.array(ts))
    return rec


def twice(fn, *args):
    a, b = fn(*args), fn(*args)
    for k in a:
        assert np.array_equal(a[k], b[k]), "the reference's roll-out is not reproducible: " + k
    return a


def main():
    ref_shim.load_reference()
    torch.set_default_dtype(torch.float64)
    random.choice = lambda seq: seq[0]                         # contacts.py:87: the GJK start vertex of a fresh body = vertex 0
    out = module_level(np.random.default_rng(SEED))
    boxes = [twice(run_box, a, b) for a, b in R.H_FORCES]
    out.update({"r_" + k: np.stack([r[k] for r in boxes]) for k in boxes[0]})
    out.update(r_force_ball=np.array([a for a, _ in R.H_FORCES]), r_force_box=np.array([b for _, b in R.H_FORCES]),
               r_nsteps=np.int64(R.H_NSTEPS), r_floor_pos=np.array([500.0, 500.0]), r_floor_dims=np.array([900.0, 10.0]),
               r_ball_pos=np.array([380.0, 468.0]), r_ball_rad=np.float64(20.0), r_box_ref=BOX_CENTRE - BOX_OFFSET,
               r_box_verts_raw=BOX + BOX_OFFSET, r_mass=np.array([1.0, 1.0]), r_rest=np.array([0.5, 0.3, 0.2]),
               r_fric=np.array([0.9, 0.6, 0.4]), r_g=np.float64(G), r_t_push=np.float64(R.T_PUSH), r_mult=np.float64(R.MULT),
               r_dt=np.float64(1.0 / 30))
    for f, r in zip(R.H_FORCES, boxes):
        print("box", f, "loss %.4f" % r["loss"], "d/d(rad) %.5f" % r["grad_rad"], "d/d(mass)", np.array2string(r["grad_mass"], precision=4),
              "d/d(raw verts)", np.array2string(r["grad_verts"].reshape(-1), precision=4), "contacts", r["ncontacts"].tolist())
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
