"""Generate tests/golden/shape_grad.npz: what the UNMODIFIED reference's autograd gives the SHAPE of the bodies - `Circle.rad`
(bodies.py:121) and `Hull.verts` (bodies.py:168-171) - through `DiffContactHandler` (physics/contacts.py:57-352).  TEST
INFRASTRUCTURE ONLY; needs the reference tree (oracle/ref_shim.py) and runs on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_shape_grad_golden.py

The leaves are made without touching reference code: after a body is constructed, `body.rad` / `body.verts` are replaced by
detached tensors that require grad (after `Hull.__init__` subtracted the centroid), so the mass matrix stays constant and only
the contact-frame path is recorded.  Bodies whose vertex gradient is compared are `Hull`s (`Rect.rotate_verts`, bodies.py:278-283,
ties vertices 2 and 3 to 0 and 1).  The two history-dependent tie-breakers are fixed to their fresh-body values, as in
oracle/contacts_oracle.py: `last_sat_idx = 0` (fresh bodies) and the GJK start vertex (`random.choice`) = vertex 0.

(a) frame level, `f_*`: pair configurations over every record type - circle / circle, circle / hull in either order (GJK vertex
    region, GJK edge region, deep SAT), hull / hull (either body as the reference, one and two clipped points), hulls of 3 .. 16
    vertices - with random fp32 cotangents g and d(sum g . (n, p1, p2))/d(radius, vertices) of both bodies.  A configuration within
    TIE = 1e-6 of a branch decision (|c1.dist - c2.dist|, a SAT runner-up, a clip distance, a barycentric coordinate of the GJK
    regions, an incident-edge choice, dist - eps) is rejected, so that no case needs excluding later; `f_rejected` counts them.
(b) roll-out level: `b_*` the three balls of oracle/make_golden_rollout.py (`grad_demo`), d(loss)/d(radius of each ball); `x_*`
    its ball / box / floor scene with the box built as a `Hull`, d(loss)/d(ball radius, box vertices); the same initial forces,
    what a ContactWorld needs to rebuild each scene, per-step contact counts and clocks.  Every roll-out is run twice and must
    reproduce its counts and clocks.
"""
import math
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import contacts_oracle as O  # noqa: E402
from oracle import make_golden_rollout as R  # noqa: E402
from oracle import ref_shim  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "shape_grad.npz")
EPS = 0.1
TIE = 1e-6
NVMAX = 16
NV_CHOICES = [3, 4, 5, 6, 8, 12, 16]
# record types and how many configurations of each
TYPES = {"cc": 16, "ch_vertex": 20, "ch_edge": 20, "ch_deep": 20, "hc_vertex": 20, "hc_edge": 20, "hc_deep": 20,
         "hh_ref1_1": 24, "hh_ref1_2": 24, "hh_ref2_1": 24, "hh_ref2_2": 24}
TYPE_CODE = {k: i for i, k in enumerate(TYPES)}


class _FakeWorld:
    def __init__(self, bodies, eps):
        self.bodies, self.eps, self.contacts = bodies, eps, []
        for i, b in enumerate(bodies):
            b.geom.body = i


def _leafify(body):
    """Replace the body's shape tensors by leaves; returns them."""
    from lcp_physics.physics.bodies import Circle
    if isinstance(body, Circle):
        body.rad = body.rad.detach().clone().requires_grad_(True)
        return body.rad
    body.verts = [v.detach().clone().requires_grad_(True) for v in body.verts]
    return list(body.verts)                                  # (rotate_verts replaces the entries of body.verts in place)


def _convex(rng, nv):
    """A convex polygon in the reference's vertex order: points of an ellipse at increasing, jittered angles."""
    a, b = rng.uniform(15, 35, 2)
    th = (np.arange(nv) + rng.uniform(-0.3, 0.3, nv)) * (2 * math.pi / nv) + rng.uniform(0, 2 * math.pi)
    return np.stack([a * np.cos(th), b * np.sin(th)], 1)


# ---- tie margins, from the numpy oracle's own intermediate values ------------------------------------------------------------
class _Margins:
    """Wraps the oracle's helpers for the duration of one collide_pair and keeps |x| of every quantity a branch is taken on."""

    def __enter__(self):
        self.m, self.ids = [], None
        self.saved = {k: getattr(O, k) for k in ("_bary2", "_bary3", "_clip", "_closest", "_incident_edge")}
        sv = self.saved

        def bary2(*a):
            r = sv["_bary2"](*a); self.m.extend(abs(x) for x in r); return r

        def bary3(*a):
            r = sv["_bary3"](*a); self.m.extend(abs(x) for x in r); return r

        def clip(verts, normal, offset):
            self.m.extend([abs(float(normal @ verts[0]) + offset), abs(float(normal @ verts[1]) + offset)])
            return sv["_clip"](verts, normal, offset)

        def closest(point, simplex):
            r = sv["_closest"](point, simplex); self.ids = r[1]; return r

        def incident(ref_normal, inc_verts, inc_vertex):
            nv = len(inc_verts)
            dots = []
            for i in ((inc_vertex - 1) % nv, inc_vertex):
                e = inc_verts[(i + 1) % nv] - inc_verts[i]
                dots.append(float(ref_normal @ (O.left_orthogonal(e) / np.linalg.norm(e))))
            self.m.append(abs(dots[0] - dots[1]))
            return sv["_incident_edge"](ref_normal, inc_verts, inc_vertex)

        O._bary2, O._bary3, O._clip, O._closest, O._incident_edge = bary2, bary3, clip, closest, incident
        return self

    def __exit__(self, *a):
        for k, v in self.saved.items():
            setattr(O, k, v)


def _sat_dists(h1, h2):
    """Distance of h2's support point to every edge of h1 (the candidates of test_separations) and the support runner-up gap."""
    v1, v2 = h1["verts"], h2["verts"]
    out, gap = [], np.inf
    for idx in range(len(v1)):
        e = v1[(idx + 1) % len(v1)] - v1[idx]
        n = O.left_orthogonal(e) / np.linalg.norm(e)
        proj = np.sort(v2 @ -n)
        gap = min(gap, proj[-1] - proj[-2])
        sp, _ = O._support(v2, -n)
        out.append(float(n @ (sp + h2["pos"] - h1["pos"] - v1[idx])))
    return np.array(out), gap


def classify(ob, recs):
    """(type name, smallest margin to a branch decision) of the oracle bodies `ob` with the records `recs`."""
    k = [b["kind"] for b in ob]
    with _Margins() as mg:
        mine = O.collide_pair(ob[0], ob[1], EPS)
    m = list(mg.m) + [abs(r[3] + EPS) for r in mine]
    assert len(mine) == len(recs)
    if k == ["circle", "circle"]:
        return "cc", min(m)
    if "circle" in k:
        name = "ch_" if k[0] == "circle" else "hc_"
        circ, hull = (ob[0], ob[1]) if k[0] == "circle" else (ob[1], ob[0])
        n = len(mg.ids)
        if n == 3:                                            # deep: the SAT winner against its runner-up
            v = hull["verts"]
            d = []
            for idx in range(len(v)):
                e = v[(idx + 1) % len(v)] - v[idx]
                d.append(float((O.left_orthogonal(e) / np.linalg.norm(e)) @ (circ["pos"] - hull["pos"] - v[idx])) - circ["rad"])
            d = np.sort(d)
            m.append(d[-1] - d[-2])
        return name + {1: "vertex", 2: "edge", 3: "deep"}[n], min(m)
    d1, g1 = _sat_dists(ob[0], ob[1])
    d2, g2 = _sat_dists(ob[1], ob[0])
    s1, s2 = np.sort(d1), np.sort(d2)
    m += [abs(s1[-1] - s2[-1]), s1[-1] - s1[-2], s2[-1] - s2[-2], abs(s1[-1] - EPS), abs(s2[-1] - EPS), g1, g2]
    return "hh_ref%d_%d" % (2 if s2[-1] > s1[-1] else 1, len(mine)), min(m)


def frame_level(rng):
    from lcp_physics.physics.bodies import Circle, Hull
    from lcp_physics.physics.contacts import DiffContactHandler
    need = dict(TYPES)
    keys = ("kind", "rad", "nverts", "verts_local", "pose", "count", "normal", "p1", "p2", "pen", "g_n", "g_p1", "g_p2", "d_rad",
            "d_verts", "rtype")
    rec = {k: [] for k in keys}
    rejected = tried = 0
    while any(v > 0 for v in need.values()):
        tried += 1
        want = [k for k, v in need.items() if v > 0][int(rng.integers(0, sum(v > 0 for v in need.values())))]
        kinds = {"cc": (0, 0), "ch": (0, 1), "hc": (1, 0), "hh": (1, 1)}[want[:2]]
        shapes = [float(rng.uniform(10, 35)) if k == 0 else _convex(rng, int(rng.choice(NV_CHOICES))) for k in kinds]
        ext = [s if k == 0 else float(np.abs(s).max()) for k, s in zip(kinds, shapes)]
        ang = float(rng.uniform(0, 2 * math.pi))
        lo = 0.0 if want.endswith("deep") else 0.35
        d = float(rng.uniform(lo, 1.02)) * (ext[0] + ext[1]) * (0.5 if want.endswith("deep") else 1.0)
        poses = [[float(rng.uniform(-math.pi, math.pi)), 300.0, 300.0],
                 [float(rng.uniform(-math.pi, math.pi)), 300.0 + d * math.cos(ang), 300.0 + d * math.sin(ang)]]
        bodies, leaves = [], []
        for k, s, p in zip(kinds, shapes, poses):
            b = Circle([0.0, 0.0], s) if k == 0 else Hull([0.0, 0.0], [list(v) for v in s])
            leaves.append(_leafify(b))
            b.set_p(torch.tensor(p))                          # (a hull's vertices are turned by the increment: bodies.py:202-214)
            bodies.append(b)
        world = _FakeWorld(bodies, EPS)
        try:
            DiffContactHandler()([world], bodies[0].geom, bodies[1].geom)
        except Exception:                                     # (the reference raises on some degenerate GJK configurations)
            continue
        cs = world.contacts
        if not cs:
            continue
        local = [None if k == 0 else torch.stack(l).detach().numpy() for k, l in zip(kinds, leaves)]
        ob = [dict(kind="circle", pos=np.array(p[1:]), rad=float(l)) if k == 0 else
              dict(kind="hull", pos=np.array(p[1:]), verts=local[i] @ O.rotation_matrix(p[0]).T)
              for i, (k, l, p) in enumerate(zip(kinds, leaves, poses))]
        mine = O.collide_pair(ob[0], ob[1], EPS)
        if len(mine) != len(cs):
            rejected += 1
            continue
        err = max(float(np.abs(np.concatenate(m[:3]) - torch.cat(c[0][:3]).detach().numpy()).max()) for m, c in zip(mine, cs))
        assert err < 1e-9, (err, want, kinds, poses, [np.concatenate(m[:3]) for m in mine], [torch.cat(c[0][:3]).detach().numpy() for c in cs])
        name, margin = classify(ob, cs)
        if margin < TIE:
            rejected += 1
            continue
        if need.get(name, 0) <= 0:
            continue
        need[name] -= 1
        g = rng.standard_normal((3, 2, 2)).astype(np.float32)
        loss = sum((torch.tensor(g[q, c].astype(np.float64)) * rc[0][q]).sum() for c, rc in enumerate(cs) for q in range(3))
        loss.backward()
        d_rad, d_verts, vl, nvs, rads = np.zeros(2), np.zeros((2, NVMAX, 2)), np.zeros((2, NVMAX, 2)), np.zeros(2, np.int32), np.zeros(2)
        for i, (k, l) in enumerate(zip(kinds, leaves)):
            if k == 0:
                rads[i] = float(l)
                d_rad[i] = 0.0 if l.grad is None else float(l.grad)
            else:
                nvs[i] = len(l)
                vl[i, :len(l)] = local[i]
                d_verts[i, :len(l)] = np.stack([np.zeros(2) if v.grad is None else v.grad.numpy() for v in l])
        pad = lambda q: np.stack([c[0][q].detach().numpy().reshape(-1) for c in cs] + [np.zeros(2)] * (2 - len(cs)))
        for key, val in (("kind", np.array(kinds, np.int32)), ("rad", rads), ("nverts", nvs), ("verts_local", vl), ("pose", np.array(poses)),
                         ("count", np.int32(len(cs))), ("normal", pad(0)), ("p1", pad(1)), ("p2", pad(2)),
                         ("pen", np.array([float(c[0][3]) for c in cs] + [0.0] * (2 - len(cs)))), ("g_n", g[0]), ("g_p1", g[1]),
                         ("g_p2", g[2]), ("d_rad", d_rad), ("d_verts", d_verts), ("rtype", np.int32(TYPE_CODE[name]))):
            rec[key].append(val)
    out = {"f_" + k: np.stack(v) for k, v in rec.items()}
    out.update(f_rejected=np.int64(rejected), f_tried=np.int64(tried), f_eps=np.float64(EPS), f_tie=np.float64(TIE),
               f_type_names=np.array(list(TYPES)))
    nv = out["f_nverts"].max(axis=1)
    print("frame level: %d configurations (%d tried, %d rejected near a tie), per type %s, with a hull of >= 12 vertices: %d"
          % (len(rec["count"]), tried, rejected, np.bincount(out["f_rtype"]).tolist(), int((nv >= 12).sum())))
    return out


# ---- roll-outs ---------------------------------------------------------------------------------------------------------------
def run_balls(force0):
    from lcp_physics.physics.forces import ExternalForce
    f0 = torch.tensor(force0, dtype=torch.float64)
    world, c, target = R.make_world(lambda t: f0 if t < R.T_PUSH else ExternalForce.ZEROS)
    nb = len(world.bodies)
    rads = [_leafify(b) for b in world.bodies]
    rec = dict(Mdiag=torch.diagonal(world.M()).reshape(nb, 3).detach().numpy().copy(),
               rest=np.array([float(b.restitution) for b in world.bodies]), fric=np.array([float(b.fric_coeff) for b in world.bodies]),
               rad=np.array([float(r) for r in rads]), p0=torch.stack([b.p for b in world.bodies]).detach().numpy().copy(),
               v0=world.get_v().reshape(nb, 3).detach().numpy().copy())
    ncs, ts = [], []
    for _ in range(R.NSTEPS):
        world.step()
        ncs.append(len(world.contacts)); ts.append(float(world.t))
    dist = (target.pos - c.pos).norm()
    dist.backward()
    rec.update(p_final=torch.stack([b.p for b in world.bodies]).detach().numpy().copy(), loss=np.float64(float(dist)),
               grad_rad=np.array([0.0 if r.grad is None else float(r.grad) for r in rads]), ncontacts=np.array(ncs), t=np.array(ts))
    return rec


BOX = [[20.0, 20.0], [-20.0, 20.0], [-20.0, -20.0], [20.0, -20.0]]          # the 40 x 40 Rect of make_world_hulls, as a Hull


def run_box(fb, fx):
    from lcp_physics.physics.bodies import Circle, Hull, Rect
    from lcp_physics.physics.constraints import TotalConstraint
    from lcp_physics.physics.forces import ExternalForce, Gravity
    from lcp_physics.physics.world import World
    f1, f2 = torch.tensor(fb, dtype=torch.float64), torch.tensor(fx, dtype=torch.float64)
    floor = Rect([500, 500], [900, 10])
    ball = Circle([380, 468], 20, restitution=0.3, fric_coeff=0.6)
    box = Hull([470, 474.5], BOX, restitution=0.2, fric_coeff=0.4)
    for b, f in ((ball, f1), (box, f2)):
        b.add_force(Gravity(g=100))
        b.add_force(ExternalForce(lambda t, f=f: f if t < R.T_PUSH else ExternalForce.ZEROS, multiplier=R.MULT))
    rad, verts = _leafify(ball), _leafify(box)
    world = World([floor, ball, box], [TotalConstraint(floor)], dt=1.0 / 30)
    nb = 3
    rec = dict(Mdiag=torch.diagonal(world.M()).reshape(nb, 3).detach().numpy().copy(),
               rest=np.array([float(b.restitution) for b in world.bodies]), fric=np.array([float(b.fric_coeff) for b in world.bodies]),
               floor_dims=floor.dims.numpy().copy(), ball_rad=np.float64(float(rad)), box_verts=torch.stack(verts).detach().numpy().copy(),
               gravity=np.stack([np.zeros(3)] + [np.array([0.0, 0.0, 100.0 * float(b.mass)]) for b in world.bodies[1:]]),
               Je=world.Je().detach().numpy().copy(), p0=torch.stack([b.p for b in world.bodies]).detach().numpy().copy(),
               v0=world.get_v().reshape(nb, 3).detach().numpy().copy())
    ncs, ts = [], []
    for _ in range(R.H_NSTEPS):
        world.step()
        ncs.append(len(world.contacts)); ts.append(float(world.t))
    dist = (ball.pos - box.pos).norm()
    dist.backward()
    rec.update(p_final=torch.stack([b.p for b in world.bodies]).detach().numpy().copy(), loss=np.float64(float(dist)),
               grad_rad=np.float64(0.0 if rad.grad is None else float(rad.grad)),
               grad_verts=np.stack([np.zeros(2) if v.grad is None else v.grad.numpy() for v in verts]), ncontacts=np.array(ncs),
               t=np.array(ts))
    return rec


def twice(fn, *args):
    a, b = fn(*args), fn(*args)
    assert (a["ncontacts"] == b["ncontacts"]).all() and (a["t"] == b["t"]).all(), "the reference's trajectory is not reproducible"
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    return a


def main():
    ref_shim.load_reference()
    torch.set_default_dtype(torch.float64)
    random.choice = lambda seq: seq[0]                         # contacts.py:87: the GJK start vertex of a fresh body = vertex 0
    out = frame_level(np.random.default_rng(20240607))
    balls = [twice(run_balls, f) for f in R.FORCES]
    out.update({"b_" + k: np.stack([r[k] for r in balls]) for k in balls[0]})
    out.update(b_force0=np.array(R.FORCES), b_nsteps=np.int64(R.NSTEPS), b_no_contact=np.array([[0, 1], [0, 2]]),
               b_pushed_body=np.int64(1), b_loss_bodies=np.array([0, 2]))
    for f, r in zip(R.FORCES, balls):
        print("balls", f, "loss %.4f" % r["loss"], "d/d(rad)", np.array2string(r["grad_rad"], precision=5), "steps with contact",
              int((r["ncontacts"] > 0).sum()))
    boxes = [twice(run_box, a, b) for a, b in R.H_FORCES]
    out.update({"x_" + k: np.stack([r[k] for r in boxes]) for k in boxes[0]})
    out.update(x_force_ball=np.array([a for a, _ in R.H_FORCES]), x_force_box=np.array([b for _, b in R.H_FORCES]),
               x_nsteps=np.int64(R.H_NSTEPS))
    for f, r in zip(R.H_FORCES, boxes):
        print("box", f, "loss %.4f" % r["loss"], "d/d(rad) %.5f" % r["grad_rad"], "d/d(verts)",
              np.array2string(r["grad_verts"].reshape(-1), precision=4), "contacts", r["ncontacts"].tolist())
    out.update(t_push=np.float64(R.T_PUSH), mult=np.float64(R.MULT), dt=np.float64(1.0 / 30))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
