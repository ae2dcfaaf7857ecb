"""The overlap query of lcp_overlap.hip (include/lcp_hip.h, "overlap queries") restated as plain float64 torch operations on the CPU,
and an independent yardstick for it.  Not a test.

    out = overlaps_host(case)    # dict: area [B,P] f64 (with its graph), kink [B,P] bool
    clip_area(A, B)              # numpy: Sutherland-Hodgman clip of polygon A by the convex polygon B, then the shoelace formula

`overlaps_host` is the header's rule pair by pair with exactly its comparisons: which half-plane bounds a clipped edge at either end is
decided on the detached values and held as an index, and the area is then the selected expression alone, so autograd differentiates
the rule itself - the parameters of the crossings included, which the header's boundary integral leaves out because they cancel.  The
two agree wherever the area is differentiable.  It is not where a piece of one boundary lies in the other's (a box resting on a box,
two identical bodies at one pose, circles that touch): `kink` marks the pairs in which two edges were found on one line (parallel and
|h| <= eps) or a comparison of the rule met an exact tie, and a comparison of gradients gives them a zero cotangent.  Their VALUES are compared like every other pair's.

`clip_area` shares nothing with the rule: it builds the intersection polygon.  `world_polygon(case, b, k)` gives it a body's world
vertices, a circle as its inscribed 4096-gon (`deficit(r)` is what that polygon lacks of the circle's area).

`case(name)` builds the inputs the GPU tests use, dicts of CPU tensors (kind, radius, verts_local, nverts, p, pair_first, pair_second,
pair_max_dist - infinite, and not consulted); `reference(name)` computes the mirror and its gradients once per case and shares them."""
import math

import numpy as np
import torch

from tests.proximity_host import LEAVES, _Hull, _pairs, all_pairs, leaves  # noqa: F401  (re-exported for the tests)
from tests.render_host import _hull, _rect
from tests.sensors_host import _assemble

F64 = torch.float64
INF = float("inf")
NGON = 4096


# ------------------------------------------------------------------------------------------------------------- the yardstick
def clip_area(A, B):
    """Area of polygon A [n,2] clipped by the convex counter-clockwise polygon B [m,2] (numpy); the one with fewer vertices clips."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if len(A) < len(B):
        A, B = B, A
    P = A
    for j in range(len(B)):
        if len(P) == 0:
            return 0.0
        b0, e = B[j], B[(j + 1) % len(B)] - B[j]
        s = e[0] * (P[:, 1] - b0[1]) - e[1] * (P[:, 0] - b0[0])                          # >= 0: inside
        if (s >= 0).all():
            continue
        Q, sq = np.roll(P, -1, 0), np.roll(s, -1)
        cut = (s >= 0) != (sq >= 0)
        den = np.where(cut, s - sq, 1.0)
        X = P + (Q - P) * (s / den)[:, None]
        both = np.stack([P, X], 1).reshape(-1, 2)                                         # each vertex, then the crossing behind it
        P = both[np.stack([s >= 0, cut], 1).reshape(-1)]
    if len(P) < 3:
        return 0.0
    Q = np.roll(P, -1, 0)
    return abs(0.5 * float(np.sum((P[:, 0] - P[0, 0]) * (Q[:, 1] - P[0, 1]) - (Q[:, 0] - P[0, 0]) * (P[:, 1] - P[0, 1]))))


def deficit(r, n=NGON):
    """What the inscribed n-gon lacks of the circle's area."""
    return math.pi * r * r - 0.5 * n * r * r * math.sin(2 * math.pi / n)


def world_polygon(case, b, k, n=NGON):
    """World vertices [nv,2] (numpy) of body k of scene b; a circle as its inscribed n-gon."""
    rot, cx, cy = (float(v) for v in case["p"][b, k].detach())
    if int(case["kind"][b, k]) == 0:
        th = np.arange(n) * (2 * math.pi / n)
        r = float(case["radius"][b, k].detach())
        return np.stack([cx + r * np.cos(th), cy + r * np.sin(th)], -1)
    v = case["verts_local"][b, k, :int(case["nverts"][b, k])].detach().numpy()
    sn, cs = math.sin(rot), math.cos(rot)
    return np.stack([cx + (cs * v[:, 0] - sn * v[:, 1]), cy + (sn * v[:, 0] + cs * v[:, 1])], -1)


def bounding_radius(case, b, k):
    if int(case["kind"][b, k]) == 0:
        return float(case["radius"][b, k].detach())
    v = case["verts_local"][b, k, :int(case["nverts"][b, k])].detach()
    return float(v.norm(dim=-1).max())


def clip_pair(case, b, k1, k2):
    """(the yardstick's area, the bound of its own error: the inscribed polygons' deficits) of the pair (k1, k2) of scene b."""
    slack = sum(deficit(float(case["radius"][b, k].detach())) for k in (k1, k2) if int(case["kind"][b, k]) == 0)
    return clip_area(world_polygon(case, b, k1), world_polygon(case, b, k2)), slack


# ------------------------------------------------------------------------------------------------------------- the mirror
def _cross(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


TAU, EPS_H = 1e-12, 64 * 2.0 ** -52


def _clip(H, i, G, first):
    """Edge i of hull H against the half-planes of hull G: (t0, t1, kink), t0 and t1 with their graph - None when the edge is out.
    first: H is body 1 (the closed form), else body 2.  What an edge of body 1 and an edge of body 2 share - c, h, parallel or not, the
    crossing - is formed from body 1's edge and body 2's line in either role, as the header has it."""
    if first:
        a1, e1, b2, e2, n2, l22 = H.w[i], H.e[i], G.w, G.e, G.n, G.l2
    else:
        a1, e1, b2, e2, n2, l22 = G.w, G.e, H.w[i], H.e[i], H.n[i], H.l2[i]
    c = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
    q = a1 - b2
    h0 = n2[..., 0] * q[..., 0] + n2[..., 1] * q[..., 1]
    l1 = e1[..., 0] * e1[..., 0] + e1[..., 1] * e1[..., 1]
    cn, h = np.broadcast_to(c.detach().numpy(), (G.nv,)), np.broadcast_to(h0.detach().numpy(), (G.nv,))
    par = np.broadcast_to((cn * cn <= (TAU * TAU) * (l1 * l22).detach().numpy()), (G.nv,))
    same = np.broadcast_to(((e1[..., 0] * e2[..., 0] + e1[..., 1] * e2[..., 1]) > 0).numpy(), (G.nv,))
    eps = np.broadcast_to(EPS_H * (a1.detach().abs().sum(-1) + b2.detach().abs().sum(-1)).numpy(), (G.nv,))
    if first:
        out = par & ((h > eps) | ((h >= -eps) & ~same))
    else:
        out = par & np.where(same, ~(h > eps), ~(h < -eps))
    kink = bool((par & (np.abs(h) <= eps)).any())
    if out.any():
        return None, None, kink
    live = torch.as_tensor(~par)
    tx = -h0 / torch.where(live, c / torch.sqrt(l22), torch.ones_like(c))
    if first:
        t, up, lo = tx + torch.zeros(G.nv, dtype=F64), ~par & (cn > 0), ~par & (cn < 0)
    else:
        X = a1 + tx.unsqueeze(-1) * e1
        t, up, lo = ((X - b2) * e2).sum(-1) / l22, ~par & (cn < 0), ~par & (cn > 0)
    tn = t.detach().numpy()
    t0, t1 = torch.zeros((), dtype=F64), torch.ones((), dtype=F64)
    if up.any():
        j = int(np.where(up, tn, INF).argmin())
        if tn[j] < 1.0:
            t1 = t[j]
    if lo.any():
        j = int(np.where(lo, tn, -INF).argmax())
        if tn[j] > 0.0:
            t0 = t[j]
    v0, v1 = float(t0.detach()), float(t1.detach())
    if (v0 > v1) if first else (v0 >= v1):
        return None, None, kink or v0 == v1
    return t0, t1, kink or v0 == v1


def _hull_hull(HA, HB, o):
    total, kink = torch.zeros((), dtype=F64), False
    for H, G, closed in ((HA, HB, True), (HB, HA, False)):
        for i in range(H.nv):
            t0, t1, k = _clip(H, i, G, closed)
            kink = kink or k
            if t0 is not None:
                total = total + (t1 - t0) * _cross(H.w[i] - o, H.e[i])
    return 0.5 * total, kink


def _circle_hull(H, c, r):
    total, kink, within = torch.zeros((), dtype=F64), False, False
    for i in range(H.nv):
        u, e = H.w[i] - c, H.e[i]
        a, bq, cq = (e * e).sum(), (u * e).sum(), (u * u).sum() - r * r
        disc = bq * bq - a * cq
        cuts = [torch.zeros((), dtype=F64)]
        dv = float(disc.detach())
        kink = kink or dv == 0.0
        if dv > 0.0:
            sq = torch.sqrt(disc)
            for root in ((-bq - sq) / a, (-bq + sq) / a):
                if 0.0 < float(root.detach()) < 1.0:
                    cuts.append(root)
        cuts.append(torch.ones((), dtype=F64))
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            if not float(t1.detach()) > float(t0.detach()):
                continue
            pp, q, m = u + t0 * e, u + t1 * e, u + 0.5 * (t0 + t1) * e
            if float((m * m).sum().detach()) <= float((r * r).detach()):
                total = total + 0.5 * (t1 - t0) * _cross(u, e)
                within = True
            else:
                total = total + 0.5 * r * r * torch.atan2(_cross(pp, q), (pp * q).sum())
    if not within:                                                                       # no piece of the hull's boundary in the circle: all or nothing
        h = (H.d[3] * (c.detach().numpy() - H.d[0])).sum(-1)
        return (math.pi * r * r if (h <= 0).all() else None), kink
    return total, kink


def _circle_circle(c1, r1, c2, r2):
    q = c2 - c1
    d2 = (q * q).sum()
    dv, a, b = math.sqrt(float(d2.detach())), float(r1.detach()), float(r2.detach())
    if dv >= a + b:
        return None, dv == a + b
    if dv <= abs(a - b):
        rm = r1 if a <= b else r2                                                        # (a tie: body 1)
        return math.pi * rm * rm, dv == abs(a - b)
    d = torch.sqrt(d2)
    x1 = ((d2 + r1 * r1 - r2 * r2) / (2 * d * r1)).clamp(-1.0, 1.0)
    x2 = ((d2 + r2 * r2 - r1 * r1) / (2 * d * r2)).clamp(-1.0, 1.0)
    k = (-d + r1 + r2) * (d + r1 - r2) * (d - r1 + r2) * (d + r1 + r2)
    return r1 * r1 * torch.acos(x1) + r2 * r2 * torch.acos(x2) - 0.5 * torch.sqrt(k), False


def overlaps_host(case, scene_verts_max=None):
    kind, nverts, p, radius, verts_local = case["kind"], case["nverts"], case["p"], case["radius"], case["verts_local"]
    first, second = case["pair_first"], case["pair_second"]
    B, nb = kind.shape
    cap = verts_local.shape[2]
    P = first.shape[1]
    nvs = torch.where(kind != 0, nverts.clamp(0, cap), torch.zeros_like(nverts))
    zero = torch.zeros((), dtype=F64)
    area, kink = [], torch.zeros(B, P, dtype=torch.bool)
    for b in range(B):
        queried = scene_verts_max is None or int(nvs[b].sum()) <= scene_verts_max       # a scene with more vertices is not queried
        hulls = {}

        def hull(k):
            if k not in hulls:
                hulls[k] = _Hull(verts_local[b, k], int(nvs[b, k]), p[b, k])
            return hulls[k]

        for r in range(P):
            k1, k2 = int(first[b, r]), int(second[b, r])
            ok = queried and k1 != k2 and 0 <= k1 < nb and 0 <= k2 < nb
            ok = ok and all(int(kind[b, k]) == 0 or int(nvs[b, k]) >= 3 for k in (k1, k2))
            a = None
            if ok:
                c1, c2, r1, r2 = p[b, k1, 1:3], p[b, k2, 1:3], radius[b, k1], radius[b, k2]
                circ1, circ2 = int(kind[b, k1]) == 0, int(kind[b, k2]) == 0
                if circ1 and circ2:
                    a, kk = _circle_circle(c1, r1, c2, r2)
                elif circ1 or circ2:
                    a, kk = _circle_hull(hull(k2), c1, r1) if circ1 else _circle_hull(hull(k1), c2, r2)
                else:
                    a, kk = _hull_hull(hull(k1), hull(k2), c1)
                kink[b, r] = kk
                if a is not None and not float(a.detach()) > 0.0:                         # area >= 0: a sum that rounds below it is 0
                    a = None
            area.append(zero if a is None else a)
    return dict(area=torch.stack(area).reshape(B, P), kink=kink)


# ------------------------------------------------------------------------------------------------------------- the cases
def _with_pairs(bodies, cap, rows):
    c = _assemble(bodies, cap)
    c.update(_pairs([[(a, b, INF) for a, b in row] for row in rows]))
    return c


def _tiny(rng):
    """B = 1, two bodies, one pair: a circle over the corner of a rect."""
    return _with_pairs([[("circle", (0.3, 100.0, 100.0), 12.0), ("hull", (0.5, 122.0, 108.0), _rect(40.0, 30.0))]], 8, [[(0, 1)]])


def _small(rng):
    """B = 4, nb = 3 (a circle, a rect, a triangle), all three pairs.  Scene 0: every pair overlaps partially; scene 1: every pair is
    apart (1: the bounding circles of circle and rect still meet); scene 2: the circle inside the rect, the triangle inside the circle;
    scene 3: the rect and the triangle contain the circle's centre but not the circle, the triangle inside the rect."""
    j = lambda s: float(rng.uniform(-s, s))
    tri = lambda s: _hull(rng, 3, s, 0.8 * s)
    bodies = [
        [("circle", (j(3), 100.0 + j(1), 100.0 + j(1)), 14.0), ("hull", (0.4 + j(0.2), 125.0 + j(1), 104.0 + j(1)), _rect(50.0, 24.0)),
         ("hull", (j(3), 110.0 + j(1), 109.0 + j(1)), tri(24.0))],
        [("circle", (j(3), 100.0, 100.0), 10.0), ("hull", (0.7, 132.0, 100.0), _rect(50.0, 16.0)), ("hull", (j(3), 100.0, 160.0), tri(18.0))],
        [("circle", (j(3), 300.0 + j(1), 300.0 + j(1)), 9.0), ("hull", (j(3), 301.0, 299.0), _rect(60.0, 40.0)),
         ("hull", (j(3), 300.5, 300.5), tri(5.0))],
        [("circle", (j(3), 500.0 + j(1), 420.0 + j(1)), 30.0), ("hull", (j(0.3), 505.0, 424.0), _rect(70.0, 44.0)),
         ("hull", (j(3), 498.0, 417.0), tri(16.0))]]
    return _with_pairs(bodies, 8, [all_pairs(3)] * 4)


def _wide(rng):
    """B = 2, nb = 24 on a jittered 6 x 4 grid whose neighbours overlap (hulls of 3 to 8 vertices, every eighth body a circle), all 276
    pairs: more than one chunk of 256."""
    bodies = []
    for b in range(2):
        j = lambda s: float(rng.uniform(-s, s))
        row = []
        for k in range(24):
            pose = (j(3), 200.0 + 40.0 * (k % 6) + j(6), 200.0 + 40.0 * (k // 6) + j(6))
            row.append(("circle", pose, 24.0 + j(3)) if k % 8 == 1 else ("hull", pose, _hull(rng, 3 + (k * 5 + b) % 6, 28.0 + j(4), 24.0 + j(4))))
        bodies.append(row)
    return _with_pairs(bodies, 8, [all_pairs(24)] * 2)


def _big_hulls(rng):
    """B = 2, nb = 4 hulls of 33 to 64 vertices at capacity 64: 0, 1 and 2 overlap each other, 3 is apart from all; every pair, the
    first three in both orders."""
    bodies = []
    for b in range(2):
        j = lambda s: float(rng.uniform(-s, s))
        bodies.append([("hull", (j(3), 400.0, 400.0), _hull(rng, 64, 40.0, 32.0)), ("hull", (j(3), 450.0 + j(2), 410.0 + j(2)), _hull(rng, 33, 36.0, 30.0)),
                       ("hull", (j(3), 425.0 + j(2), 445.0 + j(2)), _hull(rng, 47 + b, 38.0, 35.0)),
                       ("hull", (j(3), 420.0 + j(2), 560.0 + j(2)), _hull(rng, 50, 30.0, 30.0))])
    return _with_pairs(bodies, 64, [all_pairs(4) + [(1, 0), (2, 0), (2, 1)]] * 2)


def _nested(rng):
    """B = 1: a circle in a circle (0 in 1), a hull in a hull (2 in 3), a circle in a hull (4 in 5), a hull in a circle (6 in 7), each
    pair in both orders; and a rect (8) half over hull 3, the one pair whose area depends on the poses.  NESTED_INNER names the inner
    body of the eight nested pairs."""
    bodies = [[("circle", (0.0, 103.0, 98.0), 7.0), ("circle", (0.0, 100.0, 100.0), 20.0),
               ("hull", (0.3, 202.0, 101.0), _hull(rng, 5, 9.0, 7.0)), ("hull", (1.1, 200.0, 100.0), _hull(rng, 7, 30.0, 26.0)),
               ("circle", (0.0, 301.0, 99.0), 8.0), ("hull", (0.6, 300.0, 100.0), _rect(40.0, 30.0)),
               ("hull", (2.0, 399.0, 102.0), _rect(12.0, 9.0)), ("circle", (0.0, 400.0, 100.0), 15.0),
               ("hull", (0.2, 226.0, 100.0), _rect(30.0, 20.0))]]
    return _with_pairs(bodies, 8, [[(0, 1), (1, 0), (2, 3), (3, 2), (4, 5), (5, 4), (6, 7), (7, 6), (3, 8)]])


NESTED_INNER = (0, 0, 2, 2, 4, 4, 6, 6)


def _shared(rng):
    """B = 1, axis-aligned at coordinates that fp64 holds exactly: a 30 x 20 rect (1) resting exactly on a 500 x 10 floor (0): area 0; a
    2 x 1 rect (2) inside a 5 x 3 rect (3) sharing an edge: area 2; a pentagon (4) and its copy (5) at one generic pose: its own area.
    Each pair in both orders.  SHARED_WANT has the values (None: the body's own area)."""
    pent = _hull(rng, 5, 22.0, 18.0)
    bodies = [[("hull", (0.0, 300.0, 400.0), _rect(500.0, 10.0)), ("hull", (0.0, 305.0, 385.0), _rect(30.0, 20.0)),
               ("hull", (0.0, 601.5, 201.0), _rect(2.0, 1.0)), ("hull", (0.0, 600.0, 201.0), _rect(5.0, 3.0)),
               ("hull", (0.7, 811.3, 97.9), pent), ("hull", (0.7, 811.3, 97.9), pent)]]
    return _with_pairs(bodies, 8, [[(0, 1), (1, 0), (2, 3), (3, 2), (4, 5), (5, 4)]])


SHARED_WANT = (0.0, 0.0, 2.0, 2.0, None, None)


def _invalid(rng):
    """B = 1, nb = 4 (a circle, a rect over it, a two-vertex hull over both, a triangle): equal indices, an index = nb, an index = -1,
    the two-vertex hull on either side - and one valid overlapping pair, so that the launch has something to compute."""
    bodies = [[("circle", (0.0, 100.0, 100.0), 12.0), ("hull", (0.2, 105.0, 103.0), _rect(30.0, 20.0)),
               ("hull", (0.0, 102.0, 101.0), [[-10.0, 0.0], [10.0, 0.0]]), ("hull", (0.5, 108.0, 99.0), _hull(rng, 3, 14.0, 12.0))]]
    return _with_pairs(bodies, 8, [[(0, 0), (1, 1), (4, 0), (0, 4), (-1, 1), (1, -1), (2, 0), (1, 2), (2, 3), (7, 9), (0, 1)]])


ROTATED_KINDS = ("touching", "flipped", "half", "resting")


def rotated_pair(rng, what):
    """Two rects at one generic rotation whose edges share lines only up to the rounding of the staged vertices: `touching` - the second
    offset by exactly its width along its own axis (area 0); `flipped` - the same with the second turned by pi; `half` - offset by half
    the width, two shared edge lines (area w h / 2); `resting` - a smaller rect on top of the first, shifted along it (area 0)."""
    w, h = rng.uniform(10.0, 60.0), rng.uniform(10.0, 60.0)
    rot, c = rng.uniform(-3.0, 3.0), rng.uniform(100.0, 900.0, 2)
    ax, ay = np.array([math.cos(rot), math.sin(rot)]), np.array([-math.sin(rot), math.cos(rot)])
    if what == "resting":
        w2, h2 = rng.uniform(5.0, w), rng.uniform(5.0, 40.0)
        c2 = c + ay * (0.5 * (h + h2)) + ax * rng.uniform(-0.4, 0.4) * w
        return [("hull", (rot, c[0], c[1]), _rect(w, h)), ("hull", (rot, c2[0], c2[1]), _rect(w2, h2))]
    c2 = c + ax * (0.5 * w if what == "half" else w)
    return [("hull", (rot, c[0], c[1]), _rect(w, h)), ("hull", (rot + (math.pi if what == "flipped" else 0.0), c2[0], c2[1]), _rect(w, h))]


def rotated_pairs(what, n=300, seed=21):
    """n cases of B = 1 of `rotated_pair(what)`, the pair in both orders."""
    rng = np.random.default_rng(seed + ROTATED_KINDS.index(what))
    return [_with_pairs([rotated_pair(rng, what)], 8, [[(0, 1), (1, 0)]]) for _ in range(n)]


def _rotated(rng):
    """B = 48: twelve scenes of each kind of `rotated_pair`, the pair in both orders - shared edge lines at generic rotations."""
    return _with_pairs([rotated_pair(rng, ROTATED_KINDS[b % 4]) for b in range(48)], 8, [[(0, 1), (1, 0)]] * 48)


def _near(rng):
    """B = 16: the kinds of `rotated_pair` with the second body moved off the shared lines by 1e-6 along both of its axes, in or out:
    the edges are still parallel to rounding, but no two lie on one line, so every pair has a gradient."""
    bodies = []
    for b in range(16):
        one, two = rotated_pair(rng, ROTATED_KINDS[b % 4])
        rot = one[1][0]
        sx, sy = (1e-6 if b & 4 else -1e-6), (1e-6 if b & 8 else -1e-6)
        pose = (two[1][0], two[1][1] + sx * math.cos(rot) - sy * math.sin(rot), two[1][2] + sx * math.sin(rot) + sy * math.cos(rot))
        bodies.append([one, (two[0], pose, two[2])])
    return _with_pairs(bodies, 8, [[(0, 1), (1, 0)]] * 16)


_BUILD = {"tiny": (_tiny, 0), "small": (_small, 1), "wide": (_wide, 2), "big_hulls": (_big_hulls, 3), "nested": (_nested, 4),
          "shared": (_shared, 5), "invalid": (_invalid, 6), "rotated": (_rotated, 7), "near": (_near, 8)}
CASE_NAMES = ("tiny", "small", "wide", "big_hulls", "nested", "shared", "invalid", "rotated", "near")
_CACHE, _REF = {}, {}


def case(name):
    """The inputs of case `name` (CPU tensors; treat them as read-only: they are shared)."""
    if name not in _CACHE:
        fn, seed = _BUILD[name]
        _CACHE[name] = fn(np.random.default_rng(seed))
    return _CACHE[name]


def reference(name, seed=0):
    """Computed once per case and shared: the mirror's area and kinks, a random cotangent `g_area` that is zero on the kinks, and
    autograd's gradients for it."""
    if name not in _REF:
        c = leaves(case(name))
        out = overlaps_host(c)
        g = torch.randn(out["area"].shape, generator=torch.Generator().manual_seed(500 + seed), dtype=F64)
        g = torch.where(out["kink"], torch.zeros_like(g), g)
        if out["area"].requires_grad:
            grads = torch.autograd.grad(out["area"], [c[k] for k in LEAVES], g, allow_unused=True)
        else:
            grads = [None] * len(LEAVES)
        grads = [torch.zeros_like(c[k]) if gr is None else gr for k, gr in zip(LEAVES, grads)]
        _REF[name] = dict(area=out["area"].detach(), kink=out["kink"], g_area=g, grads=dict(zip(LEAVES, grads)))
    return _REF[name]


def random_hull_pairs(n=300, seed=11):
    """n cases of B = 1, two hulls of 3 to 16 vertices and radius 5 to 30 at coordinates around 500, one pair; most overlap."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ra, rb = rng.uniform(5.0, 30.0, 2)
        A = _hull(rng, int(rng.integers(3, 17)), ra, ra * rng.uniform(0.5, 1.0))
        Bv = _hull(rng, int(rng.integers(3, 17)), rb, rb * rng.uniform(0.5, 1.0))
        c = rng.uniform(450.0, 550.0, 2)
        off = rng.uniform(-1.0, 1.0, 2) * 0.7 * (ra + rb)
        out.append(_with_pairs([[("hull", (rng.uniform(-3, 3), c[0], c[1]), A), ("hull", (rng.uniform(-3, 3), c[0] + off[0], c[1] + off[1]), Bv)]],
                               16, [[(0, 1)]]))
    return out
