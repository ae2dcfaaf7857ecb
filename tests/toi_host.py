"""The time-of-impact query of lcp_toi.hip (include/lcp_hip.h, "time of impact") restated as plain float64 Python on the CPU: the
yardstick of tests/test_hip_toi.py.  Not a test.

The advancement is the header's, one pair at a time: d(t) and n(t) are `tests.proximity_host.pairs_host` on the pair's two bodies at
`p + t (double)v`, without a cutoff.

    out = reference(name)        # dict per case, computed once and shared: toi, status [B,P], normal [B,P,2], iters [B,P], ddot [B,P]
                                 # (n . (V2 - V1) at toi: autograd of the mirror's dist with respect to t), excluded [B,P] bool,
                                 # root [B,P] (brute's first touch, +inf: none), times (the iterates t_k of every pair)
    gradients(case, toi, status, g_toi)      # the implicit gradient at a GIVEN toi (the kernel's own): d(toi) = -(d dist) / ddot through
                                             # autograd of dist at pose(toi), + g / ddot for the margin; dict(p, v, radius, verts_local,
                                             # margin) and live [B,P]
    brute(case, b, r)            # d on a grid of 4000 times over the horizon plus bisection, from a vectorised numpy restatement of the
                                 # rule's VALUE (ties select features, not values): (root or +inf, the smallest d - margin on the grid)

`excluded` marks the pairs the mirror cannot decide itself: the smallest d - margin over the horizon (by `brute`) lies within 1e-6 of
0 (grazing: a HIT or a MISS by rounding), or `pairs_host` marks the iterate at toi as tied (two features: two normals).  The cases
are built so that at most 2 % of a case's pairs are excluded; tests/test_toi_host.py asserts it.

Pairs of two hulls carry a positive margin in every case.  At margin 0 a HIT has 0 < d <= tol, and the unit normal of two hulls that
are apart, (vertex - foot) / d, then carries the rounding of the coordinates divided by d - eps S / d, 1e-8 and more at S = 100 - which
neither side can resolve to the 1e-9 the normals are compared at.  With a margin of 0.02 it is 1e-12.  Margin 0 is covered by the pairs
with a circle (`bullet`, `rod`, `glance`), whose normals are formed over the distance to the circle's CENTRE.

A case is a dict of CPU tensors: kind, radius, verts_local, nverts, p (f64), v (f32), pair_first, pair_second (i32), margin [B,P],
horizon [B] (f64), and the numbers tol, max_iter; `svm` where the scene_verts_max of the call is not the largest scene's."""
import numpy as np
import torch

from tests import proximity_host as PH
from tests.render_host import _hull, _rect
from tests.sensors_host import _assemble

F64 = torch.float64
INF = float("inf")
MISS, HIT, TOUCHING, UNCONVERGED = 0, 1, 2, 3
GRID = 4000
GRAZE = 1e-6
LEAVES = ("p", "v", "radius", "verts_local", "margin")


# ------------------------------------------------------------------------------------------------------------- one pair at one time
def _nvs(case):
    cap = case["verts_local"].shape[2]
    return torch.where(case["kind"] != 0, case["nverts"].clamp(0, cap), torch.zeros_like(case["nverts"]))


def _two(case, b, k1, k2, pose, radius=None, verts_local=None):
    """The two bodies as a scene of their own with the one pair (0, 1); pose [2,3]."""
    idx = [k1, k2]
    return dict(kind=case["kind"][b, idx].unsqueeze(0), nverts=case["nverts"][b, idx].unsqueeze(0),
                radius=(case["radius"][b, idx] if radius is None else radius).unsqueeze(0),
                verts_local=(case["verts_local"][b, idx] if verts_local is None else verts_local).unsqueeze(0), p=pose.unsqueeze(0),
                pair_first=torch.zeros(1, 1, dtype=torch.int32), pair_second=torch.ones(1, 1, dtype=torch.int32),
                pair_max_dist=torch.full((1, 1), INF, dtype=F64))


def evaluate(case, b, k1, k2, t):
    """(d, n [2], tied) of the pair at p + t v."""
    idx = [k1, k2]
    out = PH.pairs_host(_two(case, b, k1, k2, case["p"][b, idx] + t * case["v"][b, idx].double()))
    return float(out["dist"][0, 0]), out["normal"][0, 0], bool(out["excluded"][0, 0])


def valid(case, b, k1, k2):
    nb = case["kind"].shape[1]
    if k1 == k2 or not (0 <= k1 < nb) or not (0 <= k2 < nb):
        return False
    nv = _nvs(case)
    return all(int(case["kind"][b, k]) == 0 or int(nv[b, k]) >= 3 for k in (k1, k2))


def queried(case, b):
    """A scene is queried when its hull vertices fit scene_verts_max and its horizon is positive (a NaN is not)."""
    svm = case.get("svm")
    h = float(case["horizon"][b])
    return (svm is None or int(_nvs(case)[b].sum()) <= svm) and h > 0.0


def rho(case, b, k):
    if int(case["kind"][b, k]) == 0:
        return 0.0
    nv = int(_nvs(case)[b, k])
    return float(case["verts_local"][b, k, :nv].norm(dim=-1).max())


def advance(case, b, r, tol=None, max_iter=None):
    """The header's advancement for pair r of scene b: dict(toi, status, normal [2], iters, times, tied)."""
    tol = case["tol"] if tol is None else tol
    max_iter = case["max_iter"] if max_iter is None else max_iter
    k1, k2 = int(case["pair_first"][b, r]), int(case["pair_second"][b, r])
    hz, mg = float(case["horizon"][b]), float(case["margin"][b, r])
    zero = torch.zeros(2, dtype=F64)
    miss = dict(toi=max(hz, 0.0) if hz == hz else 0.0, status=MISS, normal=zero, iters=0, times=[], tied=False)
    if not queried(case, b) or not valid(case, b, k1, k2):
        return miss
    v1, v2 = case["v"][b, k1].double(), case["v"][b, k2].double()
    dv = v2[1:] - v1[1:]
    turn = abs(float(v1[0])) * rho(case, b, k1) + abs(float(v2[0])) * rho(case, b, k2)
    t, times = 0.0, []
    for k in range(max_iter):
        d, n, tied = evaluate(case, b, k1, k2, t)
        times.append(t)
        if d - mg <= tol:
            return dict(toi=t, status=TOUCHING if k == 0 else HIT, normal=n, iters=k + 1, times=times, tied=tied)
        a = -float((n * dv).sum()) + turn
        if not a > 0.0:
            return dict(miss, iters=k + 1, times=times)
        t1 = t + (d - mg) / a
        if not t1 < hz:
            return dict(miss, iters=k + 1, times=times)
        t = t1
    return dict(toi=times[-1], status=UNCONVERGED, normal=zero, iters=max_iter, times=times, tied=False)


# ------------------------------------------------------------------------------------------------------------- the implicit gradient
def pair_gradient(case, b, r, toi):
    """At pose(toi): ddot = d dist / dt and the gradient of toi, -(d dist / d theta) / ddot, for theta = the two bodies' p [2,3],
    v [2,3], radius [2], verts_local [2,cap,2]; for the margin it is 1 / ddot."""
    k1, k2 = int(case["pair_first"][b, r]), int(case["pair_second"][b, r])
    idx = [k1, k2]
    leaf = lambda x: x.detach().clone().double().requires_grad_(True)
    p, v, rad, vl = leaf(case["p"][b, idx]), leaf(case["v"][b, idx]), leaf(case["radius"][b, idx]), leaf(case["verts_local"][b, idx])
    t = torch.tensor(float(toi), dtype=F64, requires_grad=True)
    out = PH.pairs_host(_two(case, b, k1, k2, p + t * v, rad, vl))
    g = torch.autograd.grad(out["dist"][0, 0], [p, v, rad, vl, t], allow_unused=True)
    g = [torch.zeros_like(x) if gi is None else gi for gi, x in zip(g, (p, v, rad, vl, t))]
    ddot = float(g[4])
    return ddot, [gi / -ddot if ddot != 0.0 else gi * 0.0 for gi in g[:4]], bool(out["excluded"][0, 0])


def gradients(case, toi, status, g_toi):
    """The gradient of sum(g_toi * toi) at the given toi and status: dict(p, v, radius, verts_local, margin), live [B,P], ddot [B,P]."""
    B, P = case["pair_first"].shape
    out = {k: torch.zeros(case[k].shape, dtype=F64) for k in LEAVES}
    live, dd = torch.zeros(B, P, dtype=torch.bool), torch.zeros(B, P, dtype=F64)
    for b in range(B):
        if not queried(case, b):
            continue
        for r in range(P):
            k1, k2 = int(case["pair_first"][b, r]), int(case["pair_second"][b, r])
            if int(status[b, r]) != HIT or not valid(case, b, k1, k2):
                continue
            ddot, (gp, gv, gr, gvl), _ = pair_gradient(case, b, r, float(toi[b, r]))
            dd[b, r] = ddot
            if not ddot < 0.0:
                continue
            live[b, r] = True
            g = float(g_toi[b, r])
            for s, k in enumerate((k1, k2)):
                out["p"][b, k] += g * gp[s]; out["v"][b, k] += g * gv[s]
                out["radius"][b, k] += g * gr[s]; out["verts_local"][b, k] += g * gvl[s]
            out["margin"][b, r] = g / ddot
    return dict(out, live=live, ddot=dd)


# ------------------------------------------------------------------------------------------------------------- brute force
def _world(vl, pose):
    """vl [nv,2], pose [T,3] -> world vertices [T,nv,2] (utils.py:105-112)."""
    sn, cs = np.sin(pose[:, 0:1]), np.cos(pose[:, 0:1])
    return np.stack([pose[:, 1:2] + cs * vl[:, 0] - sn * vl[:, 1], pose[:, 2:3] + sn * vl[:, 0] + cs * vl[:, 1]], -1)


def _pt_hull(w, x):
    """w [T,nv,2], x [T,m,2] -> h [T,nv,m] = n_i . (x - w_i) and the squared point-to-segment distances [T,nv,m]."""
    e = np.roll(w, -1, 1) - w
    l2 = (e * e).sum(-1)
    n = np.stack([e[..., 1], -e[..., 0]], -1) / np.sqrt(l2)[..., None]
    q = x[:, None, :, :] - w[:, :, None, :]
    h = (n[:, :, None, :] * q).sum(-1)
    s = np.clip((q * e[:, :, None, :]).sum(-1) / l2[:, :, None], 0.0, 1.0)
    rr = q - s[..., None] * e[:, :, None, :]
    return h, (rr * rr).sum(-1)


def dist_grid(case, b, k1, k2, ts):
    """The rule's dist of the pair at every time of ts [T] (numpy)."""
    ts = np.asarray(ts, dtype=np.float64).reshape(-1)
    pose = lambda k: case["p"][b, k].numpy()[None, :] + ts[:, None] * case["v"][b, k].double().numpy()[None, :]
    p1, p2 = pose(k1), pose(k2)
    nv = _nvs(case)
    circ = [int(case["kind"][b, k]) == 0 for k in (k1, k2)]
    W = [None if c else _world(case["verts_local"][b, k, :int(nv[b, k])].numpy(), pk) for c, k, pk in zip(circ, (k1, k2), (p1, p2))]
    r1, r2 = float(case["radius"][b, k1]), float(case["radius"][b, k2])
    if circ[0] and circ[1]:
        return np.sqrt(((p2[:, 1:] - p1[:, 1:]) ** 2).sum(-1)) - r1 - r2
    if circ[0] or circ[1]:
        w, c, rad = (W[1], p1[:, 1:], r1) if circ[0] else (W[0], p2[:, 1:], r2)
        h, d2 = _pt_hull(w, c[:, None, :])
        m = h[:, :, 0].max(1)
        return np.where(m <= 0.0, m, np.sqrt(d2[:, :, 0].min(1))) - rad
    ha, d2a = _pt_hull(W[0], W[1])
    hb, d2b = _pt_hull(W[1], W[0])
    m = np.maximum(ha.min(2).max(1), hb.min(2).max(1))
    return np.where(m <= 0.0, m, np.sqrt(np.minimum(d2a.min((1, 2)), d2b.min((1, 2)))))


def brute(case, b, r):
    """(root, gmin): the first time d - margin reaches 0 on [0, horizon] (grid of 4000 times, then bisection; +inf: never), and the
    smallest d - margin on the grid."""
    k1, k2 = int(case["pair_first"][b, r]), int(case["pair_second"][b, r])
    hz, mg = float(case["horizon"][b]), float(case["margin"][b, r])
    ts = np.linspace(0.0, hz, GRID + 1)
    g = dist_grid(case, b, k1, k2, ts) - mg
    below = np.nonzero(g <= 0.0)[0]
    if len(below) == 0:
        return INF, float(g.min())
    i = int(below[0])
    if i == 0:
        return 0.0, float(g.min())
    lo, hi = ts[i - 1], ts[i]
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        if dist_grid(case, b, k1, k2, [mid])[0] - mg <= 0.0:
            hi = mid
        else:
            lo = mid
    return float(hi), float(g.min())


# ------------------------------------------------------------------------------------------------------------- the cases
def _finish(c, vel, pairs, horizon, margin=0.0, tol=1e-6, max_iter=64, svm=None):
    """vel[b][k] = (w, vx, vy); pairs[b] = [(first, second)] or [(first, second, margin)]."""
    B = c["p"].shape[0]
    c["v"] = torch.tensor(vel, dtype=torch.float32)
    c["pair_first"] = torch.tensor([[q[0] for q in row] for row in pairs], dtype=torch.int32)
    c["pair_second"] = torch.tensor([[q[1] for q in row] for row in pairs], dtype=torch.int32)
    c["margin"] = torch.tensor([[q[2] if len(q) > 2 else margin for q in row] for row in pairs], dtype=F64)
    c["horizon"] = torch.tensor([horizon] * B if not isinstance(horizon, (list, tuple)) else list(horizon), dtype=F64)
    c["tol"], c["max_iter"] = tol, max_iter
    if svm is not None:
        c["svm"] = svm
    return c


def _bullet(rng):
    """A ball of radius 1 at 1800 units/s against a wall 10 thick, 44 away: in one dt = 1/30 it would land beyond the wall."""
    c = _assemble([[("circle", (0.0, 0.0, 0.0), 1.0), ("hull", (0.0, 50.0, 0.0), _rect(10.0, 200.0))]], 8)
    return _finish(c, [[(0.0, 1800.0, 0.0), (0.0, 0.0, 0.0)]], [[(0, 1), (1, 0), (0, 1, 0.05)]], 1.0 / 30)


def _rod(rng):
    """A turning rod against an approaching ball."""
    c = _assemble([[("hull", (-0.3, 0.0, 0.0), _rect(40.0, 2.0)), ("circle", (0.0, 30.0, 6.0), 3.0)]], 8)
    return _finish(c, [[(0.4, 0.0, 0.0), (0.0, -8.0, 0.0)]], [[(0, 1), (1, 0)]], 5.0)


def _boxes(rng):
    """Two spinning boxes closing at 10 units/s."""
    c = _assemble([[("hull", (0.3, 0.0, 0.0), _rect(20.0, 10.0)), ("hull", (0.9, 40.0, 3.0), _rect(15.0, 15.0))]], 8)
    return _finish(c, [[(0.3, 5.0, 0.0), (-0.4, -5.0, 0.0)]], [[(0, 1), (1, 0)]], 5.0, margin=0.05)


def _glance(rng):
    """Two circles of radius 5 whose centres pass at a distance of 9: a glancing touch."""
    c = _assemble([[("circle", (0.0, 0.0, 0.0), 5.0), ("circle", (0.0, 30.0, 9.0), 5.0)]], 8)
    return _finish(c, [[(0.0, 10.0, 0.0), (0.0, 0.0, 0.0)]], [[(0, 1), (1, 0)]], 5.0)


def _separating(rng):
    c = _assemble([[("circle", (0.0, 0.0, 0.0), 5.0), ("hull", (0.3, 30.0, 4.0), _rect(10.0, 10.0))]], 8)
    return _finish(c, [[(0.0, -3.0, 0.0), (0.0, 4.0, 1.0)]], [[(0, 1), (1, 0)]], 5.0)


def _spin(rng):
    """A rod spinning at 20 rad/s while a ball approaches at 2 units/s over a horizon of 20: |w| rho dwarfs the approach, the
    advancement creeps and does not converge in 64 evaluations - its toi is a lower bound of the first touch."""
    c = _assemble([[("hull", (0.0, 0.0, 0.0), _rect(40.0, 2.0)), ("circle", (0.0, 40.0, 3.0), 3.0)]], 8)
    return _finish(c, [[(20.0, 0.0, 0.0), (0.0, -2.0, 0.0)]], [[(0, 1)]], 20.0)


def _mixed_bodies(rng, b):
    """A circle, a rect and hulls of 3, 8 and 16 vertices on a ring of radius 60, each heading for the middle at its own speed and
    spin, different in every scene."""
    shapes = [("circle", 7.0 + b), ("hull", _rect(16.0, 9.0)), ("hull", _hull(rng, 3, 10.0, 8.0)), ("hull", _hull(rng, 8, 9.0, 11.0)),
              ("hull", _hull(rng, 16, 12.0, 8.0))]
    bodies, vel = [], []
    for k, (what, shape) in enumerate(shapes):
        th = 2 * np.pi * k / 5 + float(rng.uniform(-0.2, 0.2))
        x, y = 60.0 * np.cos(th), 60.0 * np.sin(th)
        sp = float(rng.uniform(15.0, 40.0))
        aim = th + np.pi + float(rng.uniform(-0.25, 0.25))
        bodies.append((what, (float(rng.uniform(-3, 3)), x, y), shape))
        vel.append((float(rng.uniform(-1.0, 1.0)), sp * np.cos(aim), sp * np.sin(aim)))
    return bodies, vel


def _mixed(rng):
    """B = 3, nb = 5, all 10 pairs, margins of 0.02 and 0.05 in turn."""
    scenes = [_mixed_bodies(rng, b) for b in range(3)]
    c = _assemble([s[0] for s in scenes], 16)
    prs = [(i, j, 0.02 + 0.03 * (n % 2)) for n, (i, j) in enumerate(PH.all_pairs(5))]
    return _finish(c, [s[1] for s in scenes], [prs] * 3, 2.0)


INVALID = ((2, 2), (-1, 3), (5, 0), (1, 7))


def _edges(P):
    """`mixed` with its 10 pairs repeated (in alternating order of the two bodies) up to P pairs per scene, every seventh an invalid
    pair: the pair counts where the mapping lane = pair, 64 a wavefront, 256 a pass, can go wrong."""
    def build(rng):
        c = dict(case("mixed"))
        base = PH.all_pairs(5)
        row = []
        for n in range(P):
            if n % 7 == 3:
                row.append(INVALID[(n // 7) % len(INVALID)] + (0.0,))
            else:
                i, j = base[n % 10]
                row.append(((i, j) if (n // 10) % 2 == 0 else (j, i)) + (0.02 + 0.03 * (n % 2),))
        return _finish(c, c["v"].tolist(), [row] * 3, 2.0)
    return build


def _notqueried(rng):
    """B = 3: scene 0 has more hull vertices (31) than the call's scene_verts_max (20), scene 1 a horizon of 0, scene 2 is queried."""
    full, vel0 = _mixed_bodies(rng, 0)
    small = [(w, pose, shape if w == "circle" or len(shape) <= 4 else _rect(12.0, 9.0)) for w, pose, shape in full]
    c = _assemble([full, small, small], 16)
    return _finish(c, [vel0] * 3, [[(i, j) for i, j in PH.all_pairs(5)]] * 3, [2.0, 0.0, 2.0], margin=0.03, svm=20)


EDGE_COUNTS = (1, 64, 65, 256, 257, 1024)
_BUILD = {"bullet": (_bullet, 0), "rod": (_rod, 0), "boxes": (_boxes, 0), "glance": (_glance, 0), "separating": (_separating, 0),
          "spin": (_spin, 0), "mixed": (_mixed, 11), "notqueried": (_notqueried, 12)}
_BUILD.update({"edges%d" % P: (_edges(P), 0) for P in EDGE_COUNTS})
SIX = ("bullet", "rod", "boxes", "glance", "separating", "spin")
EDGES = tuple("edges%d" % P for P in EDGE_COUNTS)
CASE_NAMES = SIX + ("mixed",) + EDGES + ("notqueried",)
_CACHE, _REF = {}, {}


def case(name):
    """The inputs of case `name` (CPU tensors; treat them as read-only: they are shared)."""
    if name not in _CACHE:
        fn, seed = _BUILD[name]
        _CACHE[name] = fn(np.random.default_rng(seed))
    return _CACHE[name]


def scale(c):
    """The scale S of the coordinates of a case."""
    return float(c["p"][..., 1:].abs().max() + c["verts_local"].abs().max() + c["radius"].abs().max())


def reference(name):
    """Computed once per case and shared.  Pairs that repeat (the same scene, bodies in the same order, margin) are computed once."""
    if name in _REF:
        return _REF[name]
    c = case(name)
    B, P = c["pair_first"].shape
    toi, status, iters = torch.zeros(B, P, dtype=F64), torch.zeros(B, P, dtype=torch.int32), torch.zeros(B, P, dtype=torch.int32)
    normal, ddot = torch.zeros(B, P, 2, dtype=F64), torch.zeros(B, P, dtype=F64)
    excluded, root, gmin = torch.zeros(B, P, dtype=torch.bool), torch.full((B, P), INF, dtype=F64), torch.full((B, P), INF, dtype=F64)
    times, seen = {}, {}
    for b in range(B):
        for r in range(P):
            key = (b, int(c["pair_first"][b, r]), int(c["pair_second"][b, r]), float(c["margin"][b, r]))
            if key not in seen:
                a = advance(c, b, r)
                dd, tied = 0.0, a["tied"]
                rt, gm = INF, INF
                if a["iters"] > 0:                                                       # (evaluated at all: a valid pair of a queried scene)
                    rt, gm = brute(c, b, r)
                    if a["status"] == HIT:
                        dd, _, tied2 = pair_gradient(c, b, r, a["toi"])
                        tied = tied or tied2
                seen[key] = (a, dd, tied or abs(gm) <= GRAZE, rt, gm)
            a, dd, ex, rt, gm = seen[key]
            toi[b, r], status[b, r], iters[b, r], normal[b, r], ddot[b, r] = a["toi"], a["status"], a["iters"], a["normal"], dd
            excluded[b, r], root[b, r], gmin[b, r] = ex, rt, gm
            times[(b, r)] = a["times"]
    _REF[name] = dict(toi=toi, status=status, normal=normal, iters=iters, ddot=ddot, excluded=excluded, root=root, gmin=gmin, times=times)
    return _REF[name]
