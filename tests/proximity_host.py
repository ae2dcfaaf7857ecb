"""The proximity query of lcp_proximity.hip (include/lcp_hip.h, "proximity queries") restated as plain float64 torch operations on the
CPU: the yardstick of tests/test_hip_proximity.py.  Not a test.

    out = pairs_host(case)       # dict: dist [B,P] f64 (with its graph), normal, w1, w2 [B,P,2] f64, excluded [B,P] bool,
                                 #       gap [B,P] f64, live [B,P] bool (a pair with a gradient: valid and below its max_dist)

The rule is written pair by pair exactly as the header states it, with exactly its comparisons and its order on ties.  What is selected
- which body carries the edge, the edge, the vertex, face or segment - is held as indices, and `dist` is then the selected
expression alone (`|c2 - c1| - r1 - r2`; `n_i . (x - w_i)` of a face; `|x - foot|` of a segment with its clamped parameter), so
autograd gives every gradient, and gives the header's differential: the parameter t does not move the value to first order where it
is free, and does not move at all where it is clamped.

`excluded` marks the pairs the mirror itself cannot decide, which a comparison of witnesses and gradients leaves out (their `dist` is
always compared): max(sep_A, sep_B), or the circle's max h, within 1e-9 of 0; or a second candidate feature whose value lies within
1e-9 of the selected one's.  Two candidates that name the same material points (a vertex as the end of either edge that meets in it; a
vertex-vertex pair found from either hull) are one feature: they have the same witnesses and the same gradient, and do not count.
`gap` is the distance of every pair from its nearest change of branch: finite differences of the mirror are taken where it is not
small.

`case(name)` builds the inputs the GPU tests use, dicts of CPU tensors (kind, radius, verts_local, nverts, p, pair_first,
pair_second, pair_max_dist); `reference(name)` computes the mirror and its gradients once per case and shares them."""
import numpy as np
import torch

from tests.render_host import _hull, _rect
from tests.sensors_host import _assemble

F64 = torch.float64
INF = float("inf")
TIE = 1e-9
SAME = 1e-6                  # two witnesses closer than this are the same material point (the coordinates are of order 100)
LEAVES = ("p", "radius", "verts_local")


class _Hull:
    """World vertices w [nv,2] (with their graph), edges e_i = w_i+1 - w_i, |e_i|^2 and outward unit normals (contacts.py:229-231);
    `d` holds the same as detached numpy arrays for the selection."""

    def __init__(self, verts_local, nv, pose):
        rot, c = pose[0], pose[1:3]
        sn, cs = torch.sin(rot), torch.cos(rot)
        v = verts_local[:nv]
        self.w = torch.stack([c[0] + (cs * v[:, 0] - sn * v[:, 1]), c[1] + (sn * v[:, 0] + cs * v[:, 1])], -1)   # utils.py:105-112
        self.e = torch.roll(self.w, -1, 0) - self.w
        self.l2 = (self.e * self.e).sum(-1)
        self.n = torch.stack([self.e[:, 1], -self.e[:, 0]], -1) / torch.sqrt(self.l2).unsqueeze(-1)
        self.nv = nv
        self.d = tuple(t.detach().numpy() for t in (self.w, self.e, self.l2, self.n))


def _h_and_d2(H, X):
    """For points X [m,2] (numpy) against every edge i of hull H: h [nv,m] = n_i . (x - w_i), the squared point-to-segment distance
    d2 [nv,m] and the foot points [nv,m,2]."""
    w, e, l2, n = H.d
    q = X[None, :, :] - w[:, None, :]
    h = (n[:, None, :] * q).sum(-1)
    s = (q * e[:, None, :]).sum(-1) / l2[:, None]
    tc = np.clip(s, 0.0, 1.0)
    foot = w[:, None, :] + tc[..., None] * e[:, None, :]
    r = X[None, :, :] - foot
    return h, (r * r).sum(-1), foot


def _second(values, foot, sel):
    """The gap between the selected candidate and the nearest other one that is a different material point: values [k], foot [k,2]."""
    other = np.abs(foot - foot[sel]).max(-1) > SAME
    if not other.any():
        return INF
    return float(np.abs(values[other] - values[sel]).min())


def _point_edge(H, i, x, face):
    """The selected expression, with its graph: d, u [2], t, foot [2] of point x against edge i of H (face: the signed distance from
    the edge's line and the unclamped t; else the distance from the segment and the clamped t)."""
    q = x - H.w[i]
    s = (q * H.e[i]).sum() / H.l2[i]
    if face:
        d = (H.n[i] * q).sum()
        return d, H.n[i], s, x - d * H.n[i]
    tc = s.clamp(0.0, 1.0)
    foot = H.w[i] + tc * H.e[i]
    r = x - foot
    d = torch.sqrt((r * r).sum())
    return d, r / d, tc, foot


def _circle_hull(H, c):
    """hull_sd of lcp_render_common.h at the point c: (edge, face, tied, gap)."""
    x = c.detach().numpy()[None, :]
    h, d2, foot = _h_and_d2(H, x)
    h, d2, foot = h[:, 0], d2[:, 0], foot[:, 0]
    m = h.max()
    if m <= 0.0:
        i = int(h.argmax())                                                              # (the first i on ties)
        top = np.sort(h)[::-1]
        sec = float(top[0] - top[1])
        return i, True, (abs(m) < TIE) or (sec < TIE), min(abs(m), sec)
    i = int(d2.argmin())
    sec = _second(np.sqrt(d2), foot, i)
    return i, False, (abs(m) < TIE) or (sec < TIE), min(abs(m), sec)


def _sep(HA, HB):
    """sep_A = max_i min_j n^A_i . (b_j - a_i) with its (i, j) (first on ties), the gap to the second candidates, and the segment
    distances of every b_j against every edge of A: (sep, i, j, gap, d2 [nvA,nvB], foot)."""
    h, d2, foot = _h_and_d2(HA, HB.d[0])
    mins = h.min(1)
    i = int(mins.argmax())
    j = int(h[i].argmin())
    top = np.sort(mins)[::-1]
    row = np.sort(h[i])
    return float(mins[i]), i, j, min(float(top[0] - top[1]), float(row[1] - row[0])), d2, foot


def _hull_hull(HA, HB):
    """(edge body: 1 or 2, edge, vertex of the other hull, face, tied, gap)."""
    sa, ia, ja, ga, d2a, fa = _sep(HA, HB)
    sb, jb, ib, gb, d2b, fb = _sep(HB, HA)
    m = max(sa, sb)
    if m <= 0.0:
        if sa >= sb:
            gap = min(abs(m), sa - sb, ga)
            return 1, ia, ja, True, gap < TIE, gap
        gap = min(abs(m), sb - sa, gb)
        return 2, jb, ib, True, gap < TIE, gap
    # separated: b_j against A's edges (i outer, j inner), then a_i against B's edges (j outer, i inner); a strict < keeps the first
    ka, kb = int(d2a.argmin()), int(d2b.argmin())
    first = d2a.flat[ka] <= d2b.flat[kb]
    nA, nB = HA.nv, HB.nv
    vals = np.sqrt(np.concatenate([d2a.ravel(), d2b.ravel()]))
    # the witness pair (on A, on B) of every candidate
    wa = np.concatenate([fa.reshape(-1, 2), np.repeat(HA.d[0][None], nB, 0).reshape(-1, 2)])
    wb = np.concatenate([np.repeat(HB.d[0][None], nA, 0).reshape(-1, 2), fb.reshape(-1, 2)])
    sel = ka if first else nA * nB + kb
    sec = _second(vals, np.concatenate([wa, wb], -1), sel)
    gap = min(abs(m), sec)
    if first:
        return 1, ka // nB, ka % nB, False, gap < TIE, gap
    return 2, kb // nA, kb % nA, False, gap < TIE, gap


def pairs_host(case, scene_verts_max=None):
    kind, nverts, p, radius, verts_local = case["kind"], case["nverts"], case["p"], case["radius"], case["verts_local"]
    first, second, maxd = case["pair_first"], case["pair_second"], case["pair_max_dist"]
    B, nb = kind.shape
    cap = verts_local.shape[2]
    P = first.shape[1]
    nvs = torch.where(kind != 0, nverts.clamp(0, cap), torch.zeros_like(nverts))
    zero2 = torch.zeros(2, dtype=F64)
    dist, normal, W1, W2 = [], [], [], []
    excluded, gap, live = torch.zeros(B, P, dtype=torch.bool), torch.full((B, P), INF, dtype=F64), torch.zeros(B, P, dtype=torch.bool)
    for b in range(B):
        queried = scene_verts_max is None or int(nvs[b].sum()) <= scene_verts_max       # a scene with more vertices is not queried
        hulls = {}

        def hull(k):
            if k not in hulls:
                hulls[k] = _Hull(verts_local[b, k], int(nvs[b, k]), p[b, k])
            return hulls[k]

        for r in range(P):
            k1, k2, md = int(first[b, r]), int(second[b, r]), maxd[b, r]
            ok = queried and k1 != k2 and 0 <= k1 < nb and 0 <= k2 < nb
            ok = ok and all(int(kind[b, k]) == 0 or int(nvs[b, k]) >= 3 for k in (k1, k2))
            d = None
            if ok:
                c1, c2, r1, r2 = p[b, k1, 1:3], p[b, k2, 1:3], radius[b, k1], radius[b, k2]
                circ1, circ2 = int(kind[b, k1]) == 0, int(kind[b, k2]) == 0
                if circ1 and circ2:
                    q = c2 - c1
                    len2 = float((q * q).sum().detach())
                    ln = torch.sqrt((q * q).sum()) if len2 > 0.0 else (q * 0.0).sum()    # (torch.norm's subgradient at 0: 0)
                    n = q / ln if len2 > 0.0 else zero2
                    d, w1, w2, tied, g = ln - r1 - r2, c1 + r1 * n, c2 - r2 * n, False, INF
                else:
                    if circ1 or circ2:
                        H, x, rad, edge_body = (hull(k2), c1, r1, 2) if circ1 else (hull(k1), c2, r2, 1)
                        i, face, tied, g = _circle_hull(H, x)
                    else:
                        edge_body, i, j, face, tied, g = _hull_hull(hull(k1), hull(k2))
                        H, x, rad = (hull(k1), hull(k2).w[j], 0.0) if edge_body == 1 else (hull(k2), hull(k1).w[j], 0.0)
                    dd, u, t, foot = _point_edge(H, i, x, face)
                    d = dd - rad
                    # u points from the edge's body to the point's body; the normal from body 1 to body 2
                    n, w1, w2 = (u, foot, x - rad * u) if edge_body == 1 else (-u, x - rad * u, foot)
                if not float(d.detach()) < float(md):                                             # the clamp (a NaN clamps too)
                    d = None
                else:
                    g = min(g, float(md) - float(d.detach()))
            if d is None:
                dist.append(md); normal.append(zero2); W1.append(zero2); W2.append(zero2)
            else:
                dist.append(d); normal.append(n.detach()); W1.append(w1.detach()); W2.append(w2.detach())
                excluded[b, r], gap[b, r], live[b, r] = bool(tied), g, True
    sh = lambda xs: torch.stack(list(xs)).reshape(B, P, 2)
    return dict(dist=torch.stack(dist).reshape(B, P), normal=sh(normal), w1=sh(W1), w2=sh(W2), excluded=excluded, gap=gap, live=live)


# ------------------------------------------------------------------------------------------------------------- the cases
def _pairs(rows):
    """rows[b] = [(first, second, max_dist)]."""
    t = lambda k, dt_: torch.tensor([[r[k] for r in row] for row in rows], dtype=dt_)
    return dict(pair_first=t(0, torch.int32), pair_second=t(1, torch.int32), pair_max_dist=t(2, F64))


def all_pairs(nb):
    return [(i, j) for i in range(nb) for j in range(i + 1, nb)]


def _small(rng):
    """B = 3, nb = 6 (two circles, a rect, a triangle, a pentagon and a hull of two vertices that no query accepts), capacity 8, at
    generic rotations, and 70 pairs: the ten pairs of the five real bodies in both orders, once with max_dist = inf and once with a
    finite one that clamps some of them; repeats; a self pair; the indices -1 and nb; pairs with the two-vertex hull.  Every kind of pair
    occurs overlapping, apart and beyond its max_dist; circle 1's centre lies inside the pentagon."""
    bodies, rows = [], []
    for b in range(3):
        j = lambda s: float(rng.uniform(-s, s))
        bodies.append([("circle", (j(3), 100.0 + j(2), 100.0 + j(2)), 18.0 + j(2)),           # overlaps the rect, apart from the rest
                       ("circle", (j(3), 152.0 + j(1), 188.0 + j(1)), 9.0 + j(1)),            # its centre inside the pentagon
                       ("hull", (0.4 + j(0.3), 140.0 + j(2), 96.0 + j(2)), _rect(60.0, 30.0)),
                       ("hull", (j(3), 176.0 + j(2), 110.0 + j(2)), _hull(rng, 3, 24.0, 20.0)),   # overlaps the rect's far end
                       ("hull", (j(3), 150.0 + j(2), 190.0 + j(2)), _hull(rng, 5, 26.0, 22.0)),
                       ("hull", (j(3), 60.0 + j(3), 200.0 + j(3)), [[-10.0, 0.0], [10.0, 0.0]])])
        row = []
        for a in range(5):
            for c in range(a + 1, 5):
                row += [(a, c, INF), (c, a, INF), (a, c, 55.0 + j(5)), (c, a, 55.0 + j(5))]
        row += [(0, 1, INF), (2, 3, INF), (4, 1, 20.0), (3, 4, 1e-3)]                          # repeats; the last clamps on any gap
        row += [(2, 2, INF), (2, 2, 7.5), (-1, 3, INF), (3, -1, 12.0), (6, 0, INF), (0, 6, 3.0), (7, 9, 2.0)]
        row += [(5, a, INF) for a in range(5)] + [(a, 5, 11.0 + a) for a in range(5)]          # the two-vertex hull
        row += [(0, 2, 1e-3), (1, 4, 1e-3), (0, 1, 50.0), (4, 2, 40.0), (0, 3, INF), (3, 0, 70.0 + j(5)), (1, 2, INF), (2, 1, INF),
                (4, 3, INF)]
        assert len(row) == 70
        rows.append(row)
    c = _assemble(bodies, 8)
    c.update(_pairs(rows))
    return c


def _tiny(rng):
    """B = 1, two bodies, one pair."""
    c = _assemble([[("circle", (0.3, 100.0, 100.0), 12.0), ("hull", (0.5, 150.0, 110.0), _rect(40.0, 30.0))]], 8)
    c.update(_pairs([[(0, 1, INF)]]))
    return c


def _wide(rng):
    """B = 2, nb = 64 16-gons on a jittered grid (1024 hull vertices, the limit), capacity 16, 1024 pairs: the 112 + 98 pairs of grid
    neighbours (some overlap, most are apart), then random pairs in either order; max_dist = inf for the first half, 150 (about two
    grid steps) for the second."""
    bodies, rows = [], []
    for b in range(2):
        j = lambda s: float(rng.uniform(-s, s))
        bodies.append([("hull", (j(3), 75.0 * (k % 8) + j(12), 75.0 * (k // 8) + j(12)), _hull(rng, 16, 34.0 + j(5), 34.0 + j(5)))
                       for k in range(64)])
        prs = [(k, k + 1) for k in range(64) if k % 8 != 7] + [(k + 8, k) for k in range(56)]
        prs += [(k, k + 9) for k in range(55) if k % 8 != 7]
        while len(prs) < 1024:
            a, c = int(rng.integers(0, 64)), int(rng.integers(0, 64))
            if a != c:
                prs.append((a, c))
        rows.append([(a, c, INF if r < 512 else 150.0) for r, (a, c) in enumerate(prs)])
    c = _assemble(bodies, 16)
    c.update(_pairs(rows))
    return c


def _big_hulls(rng):
    """B = 1, three 64-gons (capacity 64): 0 and 1 overlap, 2 is apart from both; the three pairs in both orders."""
    j = lambda s: float(rng.uniform(-s, s))
    bodies = [[("hull", (j(3), 100.0, 100.0), _hull(rng, 64, 40.0, 32.0)), ("hull", (j(3), 160.0 + j(2), 110.0 + j(2)), _hull(rng, 64, 36.0, 30.0)),
               ("hull", (j(3), 130.0 + j(2), 210.0 + j(2)), _hull(rng, 64, 38.0, 35.0))]]
    c = _assemble(bodies, 64)
    c.update(_pairs([[(0, 1, INF), (1, 0, INF), (0, 2, INF), (2, 0, INF), (1, 2, INF), (2, 1, 500.0)]]))
    return c


STACK_PAIRS = ((0, 1), (1, 0), (1, 2), (2, 1), (1, 3), (3, 1), (0, 2), (2, 3), (0, 3), (3, 0))


def _stack(rng):
    """Axis-aligned boxes: 1 rests on the floor 0 (touching within rounding), 2 rests 0.02 deep on 1, 3 stands beside 1 at a gap of 2
    with parallel faces.  One pair per scene, the same bodies in every scene (B = 10, P = 1): a scene's gradient is its pair's."""
    boxes = [("hull", (0.0, 300.0, 400.0), _rect(500.0, 10.0)), ("hull", (0.0, 300.0, 380.0), _rect(40.0, 30.0)),
             ("hull", (0.0, 305.0, 355.02), _rect(30.0, 20.0)), ("hull", (0.0, 347.0, 382.5), _rect(50.0, 25.0))]
    c = _assemble([boxes] * len(STACK_PAIRS), 8)
    c.update(_pairs([[(a, b, INF)] for a, b in STACK_PAIRS]))
    return c


_BUILD = {"small": (_small, 1), "tiny": (_tiny, 0), "wide": (_wide, 2), "big_hulls": (_big_hulls, 3), "stack": (_stack, 0)}
CASE_NAMES = ("small", "tiny", "wide", "big_hulls", "stack")
GENERIC = ("small", "wide", "big_hulls")                  # built so that the mirror alone decides at least 98 % of their pairs
_CACHE, _REF = {}, {}


def case(name):
    """The inputs of case `name` (CPU tensors; treat them as read-only: they are shared)."""
    if name not in _CACHE:
        fn, seed = _BUILD[name]
        _CACHE[name] = fn(np.random.default_rng(seed))
    return _CACHE[name]


def leaves(c):
    """A copy of case `c` whose p, radius and verts_local are fresh leaves that require grad."""
    out = dict(c)
    for k in LEAVES:
        out[k] = c[k].clone().requires_grad_(True)
    return out


def reference(name, seed=0):
    """Computed once per case and shared: the mirror's outputs, a random cotangent `g_dist` that is zero on the excluded pairs (so that
    they reach no gradient of either side; `stack` keeps it everywhere: only what every tied feature shares is compared there), and
    autograd's gradients for it."""
    if name not in _REF:
        c = leaves(case(name))
        out = pairs_host(c)
        g = torch.randn(out["dist"].shape, generator=torch.Generator().manual_seed(300 + seed), dtype=F64)
        if name != "stack":
            g = torch.where(out["excluded"], torch.zeros_like(g), g)
        grads = torch.autograd.grad(out["dist"], [c[k] for k in LEAVES], g, allow_unused=True)
        grads = [torch.zeros_like(c[k]) if gr is None else gr for k, gr in zip(LEAVES, grads)]
        _REF[name] = dict(dist=out["dist"].detach(), normal=out["normal"], w1=out["w1"], w2=out["w2"], excluded=out["excluded"],
                          gap=out["gap"], live=out["live"], g_dist=g, grads=dict(zip(LEAVES, grads)))
    return _REF[name]


def fixture_case():
    """tests/golden/contacts_pairs.npz as one batch of 600 scenes x 2 bodies x 1 pair: (case, has_record [600] bool, pen [600] f64 =
    the largest penetration over the pair's records)."""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contacts_pairs.npz"))
    n = len(d["count"])
    bodies = []
    for i in range(n):
        row = []
        for k in range(2):
            pose = tuple(float(v) for v in d["pos"][i, k])
            if int(d["kind"][i, k]) == 0:
                row.append(("circle", pose, float(d["size"][i, k, 0])))
            else:
                row.append(("hull", pose, _rect(float(d["size"][i, k, 0]), float(d["size"][i, k, 1]))))
        bodies.append(row)
    c = _assemble(bodies, 8)
    c.update(_pairs([[(0, 1, INF)]] * n))
    count = torch.tensor(d["count"])
    pen = torch.tensor(d["pen"], dtype=F64)
    pen = torch.where(torch.arange(2).unsqueeze(0) < count.unsqueeze(1), pen, torch.full_like(pen, -INF)).max(1).values
    return c, count > 0, pen
