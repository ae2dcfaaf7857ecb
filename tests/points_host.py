"""The point probe of lcp_points.hip (include/lcp_hip.h, "point probes") restated as plain float64 torch operations on the CPU: the
yardstick of tests/test_hip_points.py.  Not a test.

    out = points_host(case)      # dict: dist [B,N] f64 (with its graph), body [B,N] i32, normal [B,N,2] f64, excluded [B,N] bool,
                                 #       gap [B,N] f64, live [B,N] bool (a point with a gradient: not void)

The rule is written point by point exactly as the header states it, with exactly its comparisons and its order on ties (vectorised over
the points of a scene; the bodies in a loop).  What is selected - the body, the edge, face or segment - is held as indices, and `dist`
is then the selected expression alone (`|x - c| - r`; `n_i . (x - w_i)` of a face; `|x - foot|` of a segment with its clamped
parameter), so autograd gives every gradient, and gives the header's differential.

`excluded` marks the points the mirror itself cannot decide; their normal, body and gradients are left out of a comparison (their
`dist` is always compared):
  - a second candidate body lies within 1e-9 of the selected distance;
  - within the selected body a second feature lies within 1e-9 of the selected one and is not the same material point (a vertex as
    the end of either edge that meets in it is one feature);
  - max_i h_i of the selected hull, or d - max_dist, lies within 1e-9 of 0;
  - 0 < |x - foot| < 1e-3 outside the selected hull, or 0 < |x - c| < 1e-3 for the selected circle: u is a quotient by that length,
    and 1e-13 of coordinate rounding grows past the tolerance.
`gap` is the distance of every point from its nearest change of branch: finite differences of the mirror are taken where it is not
small.

`case(name)` builds the inputs the GPU tests use, dicts of CPU tensors (kind, radius, verts_local, nverts, p, pt_body, pt_xy,
pt_target, pt_max_dist) plus `names` (the named points' indices); `reference(name)` computes the mirror and its gradients once per
case and shares them."""
import math

import numpy as np
import torch

from tests.proximity_host import _h_and_d2, _Hull
from tests.render_host import _hull, _rect
from tests.sensors_host import _assemble

F64 = torch.float64
INF = float("inf")
TIE = 1e-9
SAME = 1e-6                  # two foot points closer than this are the same material point (the coordinates are of order 100)
NEAR = 1e-3                  # below this length the unit vector u is not compared
LEAVES = ("p", "radius", "verts_local", "pt_xy")


def world_points(p, body, xy):
    """x [B,N,2] and `ok` [B,N] (False: a mounting body outside [0, nb) other than -1 - a void point)."""
    B, N = body.shape
    nb = p.shape[1]
    mounted = (body >= 0) & (body < nb)
    pm = torch.gather(p, 1, body.clamp(0, nb - 1).long().unsqueeze(-1).expand(B, N, 3))
    zero = torch.zeros((), dtype=F64)
    rot, cx, cy = (torch.where(mounted, pm[..., i], zero) for i in range(3))              # the world frame: rot 0 at (0, 0)
    sn, cs = torch.sin(rot), torch.cos(rot)
    lx, ly = xy[..., 0], xy[..., 1]
    return torch.stack([cx + (cs * lx - sn * ly), cy + (sn * lx + cs * ly)], -1), mounted | (body == -1)


def _circle(x, c, r):
    """One circle against the points x [N,2]: d [N] (with its graph), u [N,2], `tied` [N] and the gap [N] (numpy)."""
    q = x - c
    len2 = (q * q).sum(-1)
    pos = len2.detach() > 0.0
    one = torch.ones((), dtype=F64)
    ln = torch.where(pos, torch.sqrt(torch.where(pos, len2, one)), torch.zeros((), dtype=F64))       # (torch.norm's subgradient at 0: 0)
    u = torch.where(pos.unsqueeze(-1), q / torch.where(pos, ln, one).unsqueeze(-1), torch.zeros((), dtype=F64)).detach()
    lnn = ln.detach().numpy()
    return ln - r, u, (lnn > 0.0) & (lnn < NEAR), lnn


def _hull_sd(H, x):
    """hull_sd of lcp_render_common.h for hull H at the points x [N,2]: d [N] (with its graph), u [N,2], `tied` [N], the gap [N]."""
    N = x.shape[0]
    ar = np.arange(N)
    h, d2, foot = _h_and_d2(H, x.detach().numpy())                                       # [nv,N], [nv,N], [nv,N,2]
    m = h.max(0)
    inside = m <= 0.0
    i_out = d2.argmin(0)                                                                 # (the first on ties, either way)
    i = np.where(inside, h.argmax(0), i_out)
    top = np.sort(h, 0)
    dall = np.sqrt(d2)
    dsel = dall[i_out, ar]
    other = np.abs(foot - foot[i_out, ar][None]).max(-1) > SAME                          # a different material point
    sec = np.where(inside, top[-1] - top[-2], np.where(other, np.abs(dall - dsel[None]), INF).min(0))
    tied = (np.abs(m) < TIE) | (sec < TIE) | (~inside & (dsel > 0.0) & (dsel < NEAR))
    # the selected expression, with its graph
    it, ins = torch.as_tensor(i), torch.as_tensor(inside)
    w, e, l2, n = H.w[it], H.e[it], H.l2[it], H.n[it]
    q = x - w
    s = (q * e).sum(-1) / l2
    r = q - s.clamp(0.0, 1.0).unsqueeze(-1) * e
    d_out = torch.sqrt(torch.where(ins, torch.ones((), dtype=F64), (r * r).sum(-1)))      # (apart: > 0)
    d = torch.where(ins, (n * q).sum(-1), d_out)
    u = torch.where(ins.unsqueeze(-1), n, r / d_out.unsqueeze(-1)).detach()
    return d, u, tied, np.minimum(np.abs(m), sec)


def points_host(case, scene_verts_max=None):
    kind, nverts, p, radius, verts_local = case["kind"], case["nverts"], case["p"], case["radius"], case["verts_local"]
    body, target, maxd = case["pt_body"], case["pt_target"], case["pt_max_dist"]
    B, nb = kind.shape
    cap = verts_local.shape[2]
    N = body.shape[1]
    nvs = torch.where(kind != 0, nverts.clamp(0, cap), torch.zeros_like(nverts))
    X, OK = world_points(p, body, case["pt_xy"])
    ar = np.arange(N)
    dist, sel, normal, excluded, gap, live = [], [], [], [], [], []
    for b in range(B):
        queried = scene_verts_max is None or int(nvs[b].sum()) <= scene_verts_max       # a scene with more vertices is not probed
        x, md = X[b], maxd[b].numpy()
        D, U = [], []
        Dn, tied, fgap = np.full((nb, N), INF), np.zeros((nb, N), dtype=bool), np.full((nb, N), INF)
        for k in range(nb):
            circ = int(kind[b, k]) == 0
            cand = OK[b] & (body[b] != k) & ((target[b] == -1) | (target[b] == k))     # a point never tests its own mounting body
            if not queried or not (circ or int(nvs[b, k]) >= 3) or not bool(cand.any()):
                D.append(torch.zeros(N, dtype=F64)); U.append(torch.zeros(N, 2, dtype=F64))
                continue
            if circ:
                d, u, tied[k], fgap[k] = _circle(x, p[b, k, 1:3], radius[b, k])
            else:
                d, u, tied[k], fgap[k] = _hull_sd(_Hull(verts_local[b, k], int(nvs[b, k]), p[b, k]), x)
            D.append(d); U.append(u)
            Dn[k] = np.where(cand.numpy(), d.detach().numpy(), INF)
        kmin = Dn.argmin(0)                                                              # (the smallest k on ties)
        dmin = Dn[kmin, ar]
        lv = np.isfinite(dmin) & (dmin < md)                                             # d >= max_dist: void
        two = np.sort(Dn, 0)[:2] if nb > 1 else np.stack([dmin, np.full(N, INF)])
        with np.errstate(invalid="ignore"):                                              # (inf - inf where there is no candidate)
            body_gap = np.where(np.isfinite(two[0]) & np.isfinite(two[1]), two[1] - two[0], INF)
            cut_gap = np.where(np.isfinite(dmin), np.abs(dmin - md), INF)
        kt, lt = torch.as_tensor(kmin), torch.as_tensor(lv)
        dsel = torch.gather(torch.stack(D, -1), 1, kt.unsqueeze(-1)).squeeze(-1)
        usel = torch.gather(torch.stack(U, 1), 1, kt.reshape(N, 1, 1).expand(N, 1, 2)).squeeze(1)
        dist.append(torch.where(lt, dsel, maxd[b]))
        sel.append(torch.where(lt, kt, torch.full_like(kt, -1)).to(torch.int32))
        normal.append(torch.where(lt.unsqueeze(-1), usel, torch.zeros((), dtype=F64)))
        excluded.append(torch.as_tensor((lv & (tied[kmin, ar] | (body_gap < TIE))) | (cut_gap < TIE)))
        gap.append(torch.as_tensor(np.where(lv, np.minimum(np.minimum(body_gap, fgap[kmin, ar]), cut_gap), cut_gap)))
        live.append(lt)
    st = torch.stack
    return dict(dist=st(dist), body=st(sel), normal=st(normal), excluded=st(excluded), gap=st(gap), live=st(live))


# ------------------------------------------------------------------------------------------------------------- the cases
def _points(rows):
    """rows[b] = [(body, (x, y), target, max_dist)]."""
    t = lambda f, dt_: torch.tensor([[f(r) for r in row] for row in rows], dtype=dt_)
    return dict(pt_body=t(lambda r: r[0], torch.int32), pt_xy=t(lambda r: [float(r[1][0]), float(r[1][1])], F64),
                pt_target=t(lambda r: r[2], torch.int32), pt_max_dist=t(lambda r: r[3], F64))


def _world(pose, verts):
    """World vertices [nv,2] (numpy) of body-frame `verts` at `pose` = (rot, x, y)."""
    v = np.asarray(verts, dtype=np.float64)
    sn, cs = math.sin(pose[0]), math.cos(pose[0])
    return np.stack([pose[1] + (cs * v[:, 0] - sn * v[:, 1]), pose[2] + (sn * v[:, 0] + cs * v[:, 1])], -1)


def _random_points(rng, n, nb, lo, hi, local, mounted_share, cut):
    """n points: `mounted_share` of them mounted on a random body with coordinates within `local` of its origin, the rest in the
    world frame within [lo, hi]^2; three in four test every body, the rest a random target; `cut(i)` is point i's max_dist."""
    row = []
    for i in range(n):
        target = -1 if rng.uniform() < 0.75 else int(rng.integers(0, nb))
        if rng.uniform() < mounted_share:
            row.append((int(rng.integers(0, nb)), rng.uniform(-local, local, 2), target, cut(i)))
        else:
            row.append((-1, rng.uniform(lo, hi, 2), target, cut(i)))
    return row


SMALL_NAMES = dict(centre=0, on_face=1, inside_rect=2, inside_vertex=3, vertex_outer=4, beyond=5, at_cutoff=6, mounted=7,
                   far_target=8, own_mount=9, bad_mount=10, stick=11, stick_alone=12)
RECT = (60.0, 30.0)
RECT_AT = (0.0, 220.0, 100.0)                # rot = 0 at representable coordinates: its faces and normals are exact


def _small(rng):
    """B = 3, nb = 6 (two circles, the unrotated rect, a rotated rect, a pentagon and a two-vertex hull that is never a candidate),
    capacity 8, N = 70: thirteen named points, then random ones, a third of them mounted.  Coordinates of order 100.

    `on_face` (exactly on the rect's right face: max h == 0) and `at_cutoff` (8 from that face with max_dist = 8: d == max_dist) are
    points the mirror excludes by its own rule, so they are exact in scene 0 only; scenes 1 and 2 hold a neighbour that is decided (half
    a unit off the face; max_dist = 8.5)."""
    bodies, rows = [], []
    for b in range(3):
        j = lambda s: float(rng.uniform(-s, s))
        c0 = (j(3), 100.0 + j(3), 100.0 + j(3))
        turned = (0.5 + j(0.2), 100.0 + j(3), 195.0 + j(3))
        pent = (j(3), 185.0 + j(3), 190.0 + j(3))
        pverts = _hull(rng, 5, 26.0, 22.0)
        stick = (j(3), 60.0 + j(3), 150.0 + j(3))
        bodies.append([("circle", c0, 18.0 + j(2)), ("circle", (j(3), 170.0 + j(3), 50.0 + j(3)), 10.0 + j(1)),
                       ("hull", RECT_AT, _rect(*RECT)), ("hull", turned, _rect(50.0, 24.0)), ("hull", pent, pverts),
                       ("hull", stick, [[-10.0, 0.0], [10.0, 0.0]])])
        pw = _world(pent, pverts)
        inward = pw.mean(0) - pw[2]
        inward /= np.linalg.norm(inward)
        side = np.array([-inward[1], inward[0]])
        rx, ry = RECT_AT[1], RECT_AT[2]
        row = [(-1, (c0[1], c0[2]), -1, INF),                                             # at circle 0's centre
               (-1, (rx + 30.0 + (0.0 if b == 0 else 0.5), ry + 4.0), -1, INF),          # on the rect's right face
               (-1, (rx - 12.0, ry + 6.0), -1, INF),                                      # inside the rect: the top face at -9
               (-1, pw[2] + 2.0 * inward + 0.3 * side, -1, INF),                          # inside the pentagon next to vertex 2
               (-1, pw[2] - 4.0 * inward + 0.2 * side, 4, INF),                           # in vertex 2's outer region
               (-1, (rx + 25.0, ry - 60.0), -1, 5.0),                                     # nothing within 5
               (-1, (rx + 38.0, ry + 2.0), 2, 8.0 if b == 0 else 8.5),                    # 8 from the right face
               (3, (30.0, 3.0), -1, INF),                                                 # mounted on the rotated rect
               (-1, (c0[1] + 25.0, c0[2] + 5.0), 4, INF),                                 # next to circle 0, asked about the pentagon
               (2, (40.0, 0.0), 2, INF),                                                  # target == mount
               (9, (100.0, 100.0), -1, INF),                                              # pt_body = nb + 3
               (-1, (stick[1], stick[2]), -1, INF),                                       # on the two-vertex hull: some other body
               (-1, (stick[1], stick[2] + 1.0), 5, INF)]                                  # asked about it alone: void
        row += _random_points(rng, 70 - len(row), 6, 30.0, 270.0, 40.0, 1.0 / 3.0, lambda i: INF if i % 2 else float(rng.uniform(20.0, 80.0)))
        rows.append(row)
    c = _assemble(bodies, 8)
    c.update(_points(rows))
    c["names"] = SMALL_NAMES
    return c


def _wide(rng):
    """B = 2, nb = 64 16-gons on a jittered grid (1024 hull vertices, the limit), capacity 16, N = 1024: a quarter mounted, a quarter
    with one target, max_dist = inf for the first half and a finite cutoff (30 to 120: about a grid step) for the second."""
    bodies, rows = [], []
    for b in range(2):
        j = lambda s: float(rng.uniform(-s, s))
        bodies.append([("hull", (j(3), 100.0 * (k % 8) + j(15), 100.0 * (k // 8) + j(15)), _hull(rng, 16, 30.0 + j(5), 30.0 + j(5)))
                       for k in range(64)])
        rows.append(_random_points(rng, 1024, 64, -60.0, 760.0, 60.0, 0.25, lambda i: INF if i < 512 else float(rng.uniform(30.0, 120.0))))
    c = _assemble(bodies, 16)
    c.update(_points(rows))
    c["names"] = {}
    return c


def _tiny(mounted):
    """B = 7, one circle, N = 1: mounted on that only body (void: a point never tests its mounting body), or in the world frame."""
    def build(rng):
        bodies, rows = [], []
        for b in range(7):
            j = lambda s: float(rng.uniform(-s, s))
            bodies.append([("circle", (j(3), 100.0 + j(20), 100.0 + j(20)), 15.0 + j(5))])
            rows.append([(0, (5.0 + j(3), j(3)), -1, INF)] if mounted else [(-1, (100.0 + j(60), 100.0 + j(60)), -1 if b % 2 else 0, INF if b < 5 else 25.0)])
        c = _assemble(bodies, 8)
        c.update(_points(rows))
        c["names"] = {}
        return c
    return build


def _check(rng):
    """B = 2, nb = 3 (circle, rect, pentagon), N = 6, every point live and far from a change of branch: the inputs of gradcheck."""
    bodies, rows = [], []
    for b in range(2):
        j = lambda s: float(rng.uniform(-s, s))
        circ, rect = (j(1), 100.0 + j(3), 100.0 + j(3)), (0.3 + j(0.2), 190.0 + j(3), 110.0 + j(3))
        pent = (j(1), 140.0 + j(3), 185.0 + j(3))
        bodies.append([("circle", circ, 15.0), ("hull", rect, _rect(40.0, 30.0)), ("hull", pent, _hull(rng, 5, 22.0, 20.0))])
        inner = _world(rect, [[12.0, 3.0]])[0]                                           # inside the rect: the right face at -8, the top at -12
        rows.append([(-1, (70.0 + j(3), 80.0 + j(3)), -1, INF),                            # world -> the circle, outside
                     (-1, inner, -1, INF),                                                 # world -> inside the rect
                     (-1, (140.0 + j(3), 240.0 + j(3)), -1, 200.0),                        # world -> the pentagon
                     (0, (25.0, 4.0), 1, INF),                                             # on the circle -> the rect
                     (1, (-35.0, 2.0), 0, INF),                                            # on the rect -> the circle
                     (2, (3.0, -2.0), 0, INF)])                                            # on the pentagon -> the circle
    c = _assemble(bodies, 8)
    c.update(_points(rows))
    c["names"] = {}
    return c


def probe_circles(c, xy, rho, max_dist=INF):
    """The cross-check with the proximity query: case `c` with M circle bodies of radius `rho` appended at the world points xy
    [B,M,2] (as tensors of a proximity case: body nb0 + j against each of the first nb0 bodies), and the same questions as points of
    `c` itself (world point j with target k).  pair dist = point dist - rho.  Returns (pair case, point case), M * nb0 queries each,
    query j * nb0 + k."""
    B, nb0 = c["kind"].shape
    M, cap = xy.shape[1], c["verts_local"].shape[2]
    pose = torch.cat([torch.zeros(B, M, 1, dtype=F64), xy], -1)
    pc = dict(kind=torch.cat([c["kind"], torch.zeros(B, M, dtype=torch.int32)], 1),
              radius=torch.cat([c["radius"], torch.full((B, M), float(rho), dtype=F64)], 1),
              verts_local=torch.cat([c["verts_local"], torch.zeros(B, M, cap, 2, dtype=F64)], 1),
              nverts=torch.cat([c["nverts"], torch.zeros(B, M, dtype=torch.int32)], 1), p=torch.cat([c["p"], pose], 1))
    jj, kk = torch.meshgrid(torch.arange(M), torch.arange(nb0), indexing="ij")
    rep = lambda t: t.reshape(1, -1).expand(B, M * nb0).contiguous()
    pc.update(pair_first=rep(nb0 + jj).to(torch.int32), pair_second=rep(kk).to(torch.int32),
              pair_max_dist=torch.full((B, M * nb0), float(max_dist), dtype=F64))
    qc = {k: c[k] for k in ("kind", "radius", "verts_local", "nverts", "p")}
    qc.update(pt_body=torch.full((B, M * nb0), -1, dtype=torch.int32), pt_xy=xy[:, jj.reshape(-1)].contiguous(),
              pt_target=rep(kk).to(torch.int32), pt_max_dist=torch.full((B, M * nb0), float(max_dist), dtype=F64))
    return pc, qc


# (seeds: the mirror alone decides at least 98 % of every case's points, tests/test_points_host.py)
_BUILD = {"small": (_small, 1), "wide": (_wide, 2), "tiny_mounted": (_tiny(True), 3), "tiny_world": (_tiny(False), 4), "check": (_check, 7)}
CASE_NAMES = ("small", "wide", "tiny_mounted", "tiny_world")
_CACHE, _REF = {}, {}


def case(name):
    """The inputs of case `name` (CPU tensors; treat them as read-only: they are shared)."""
    if name not in _CACHE:
        fn, seed = _BUILD[name]
        _CACHE[name] = fn(np.random.default_rng(seed))
    return _CACHE[name]


def leaves(c):
    """A copy of case `c` whose p, radius, verts_local and pt_xy are fresh leaves that require grad."""
    out = dict(c)
    for k in LEAVES:
        out[k] = c[k].clone().requires_grad_(True)
    return out


def reference(name, seed=0):
    """Computed once per case and shared: the mirror's outputs, a random cotangent `g_dist` that is zero on the excluded points (so
    that they reach no gradient of either side), and autograd's gradients for it."""
    if name not in _REF:
        c = leaves(case(name))
        out = points_host(c)
        g = torch.randn(out["dist"].shape, generator=torch.Generator().manual_seed(400 + seed), dtype=F64)
        g = torch.where(out["excluded"], torch.zeros_like(g), g)
        if out["dist"].requires_grad:
            grads = torch.autograd.grad(out["dist"], [c[k] for k in LEAVES], g, allow_unused=True)
        else:                                                                             # (every point void: nothing to differentiate)
            grads = [None] * len(LEAVES)
        grads = [torch.zeros_like(c[k]) if gr is None else gr for k, gr in zip(LEAVES, grads)]
        _REF[name] = dict(dist=out["dist"].detach(), body=out["body"], normal=out["normal"], excluded=out["excluded"], gap=out["gap"],
                          live=out["live"], g_dist=g, grads=dict(zip(LEAVES, grads)))
    return _REF[name]
