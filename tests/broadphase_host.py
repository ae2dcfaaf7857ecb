"""The cull rule of lcp_contacts_bp.hip (`lcp_move_find_contacts_bp_f64`) restated in numpy fp64 over the contact oracle's body
dicts (`oracle.world_oracle.bodies_at`), and the scenes the broadphase tests share.  TEST INFRASTRUCTURE ONLY.

The rule (the kernel's header has the proof that it drops no record): per body R = the bounding radius about the position, box =
(min, max) of the vertices relative to the position, mitre = (min, max) over the vertices of m_k = (n_{k-1} + n_k) / (1 + n_{k-1} . n_k)
(n: outward unit edge normals), kappa = max |m_k|; a circle: R = rad, box = -+ rad, mitre = -+ 1, kappa = 1.  For the ordered pair
(a, b), r = R_b + eps, S = R_a + kappa_a r, d = pos_b - pos_a:
    T(a, b):  |d|^2 <= S^2 (1 + 4e-9)  and  box_a.min + r mitre_a.min - 1e-9 S <= d <= box_a.max + r mitre_a.max + 1e-9 S.
A pair i < j is a candidate iff it is not masked and T(i, j) and T(j, i) hold."""
import numpy as np

EPS = 0.1
NEAR = 1e-9           # no scene of the device tests has a pair this close (relative) to a threshold: the device's last bits cannot decide


def bounds(body):
    """(R, kappa, box_lo[2], box_hi[2], mitre_lo[2], mitre_hi[2]) of an oracle body dict."""
    if body["kind"] == "circle":
        r = float(body["rad"])
        return r, 1.0, np.array([-r, -r]), np.array([r, r]), np.array([-1.0, -1.0]), np.array([1.0, 1.0])
    v = np.asarray(body["verts"], dtype=np.float64)
    e = np.roll(v, -1, axis=0) - v
    n = np.stack([e[:, 1], -e[:, 0]], axis=1) / np.sqrt((e * e).sum(axis=1))[:, None]      # utils.py:99-102, outward for this order
    npv = np.roll(n, 1, axis=0)
    m = (npv + n) / (1.0 + (npv * n).sum(axis=1))[:, None]
    return (float(np.sqrt((v * v).sum(axis=1).max())), float(np.sqrt((m * m).sum(axis=1).max())), v.min(axis=0), v.max(axis=0),
            m.min(axis=0), m.max(axis=0))


def candidate_pairs(bodies, eps=EPS, no_contact=()):
    """The pairs (i, j), i < j, in lexicographic order, that pass the cull, and the smallest relative distance of any unmasked pair to
    a threshold (|d^2 / (S^2 (1 + 4e-9)) - 1| of the circle tests, |d - bound| / S of the eight box bounds)."""
    masked = {(min(a, b), max(a, b)) for a, b in no_contact}
    bnd = [bounds(b) for b in bodies]
    pos = [np.asarray(b["pos"], dtype=np.float64) for b in bodies]
    out, near = [], np.inf
    for i in range(len(bodies)):
        for j in range(i + 1, len(bodies)):
            if (i, j) in masked:
                continue
            ok = True
            for a, b in ((i, j), (j, i)):
                Ra, ka, lo, hi, mlo, mhi = bnd[a]
                r = bnd[b][0] + eps
                S = Ra + ka * r
                d = pos[b] - pos[a]
                d2, thr = float(d @ d), S * S * (1.0 + 4e-9)
                up, dn = hi + r * mhi + 1e-9 * S, lo + r * mlo - 1e-9 * S
                near = min(near, abs(d2 / thr - 1.0), float(np.abs(np.concatenate([d - up, d - dn])).min()) / S)
                ok = ok and d2 <= thr and bool((d <= up).all()) and bool((d >= dn).all())
            if ok:
                out.append((i, j))
    return out, near


def contact_pairs(records):
    """The distinct body pairs of a reference-format contact list."""
    return sorted({(c[1], c[2]) for c in records})


# ---- scenes ----------------------------------------------------------------------------------------------------------------
# (nb, scenes, vertex range of the n-gons, vertex capacity): nb = 3 is the smallest; 7 and 12 at capacity 8 are otherwise served by
# lcp_contacts.hip, and 12 bodies are 66 pairs - the cull walk crosses one 64-pair boundary; 64 bodies are 2016 pairs
PILES = ((3, 24, (3, 9), 8), (7, 24, (3, 9), 8), (12, 16, (3, 9), 8), (20, 8, (9, 65), 64), (40, 6, (9, 49), 64), (64, 6, (9, 41), 64))


def piles(nb, B, nv_range, seed=None, **kw):
    """B seeded `_wide_scene` piles of nb bodies (circles, rects and n-gons mixed), none with a pair within NEAR of a threshold."""
    from oracle import world_oracle as W
    from tests.test_hip_wide_contacts import _wide_scene
    rng = np.random.default_rng(9000 + nb if seed is None else seed)
    scenes = [_wide_scene(rng, nb, nv_range=nv_range, **kw) for _ in range(B)]
    for shapes, pose in scenes:
        assert candidate_pairs(W.bodies_at(shapes, pose))[1] > NEAR
    return scenes


def plank_scene():
    """13 rects of 200 x 2, all at rot = pi / 4, centres stepped by 2.05 along the plank normal: every one of the 78 pairs passes the
    cull (the bounding circles and boxes all overlap), only the 12 neighbour pairs are within eps = 0.1 (gap 0.05) - two records each,
    at pair indices 0, 12, 23, 33, 42, 50, 57, 63 | 68, 72, 75, 77: both narrow passes of the candidate list produce records."""
    rot = np.pi / 4
    normal = np.array([-np.sin(rot), np.cos(rot)])
    shapes = [("rect", (200.0, 2.0))] * 13
    pose = np.array([[rot, 300.0 + 2.05 * k * normal[0], 300.0 + 2.05 * k * normal[1]] for k in range(13)])
    return shapes, pose


def far_scene():
    """5 bodies 1000 apart: nothing passes the cull."""
    shapes = [("circle", 20.0), ("rect", (30.0, 20.0)), ("circle", 15.0), ("rect", (25.0, 25.0)), ("circle", 10.0)]
    pose = np.array([[0.1 * k, 1000.0 * k, 300.0] for k in range(5)])
    return shapes, pose


def corner_scene(d=0.09):
    """Two rect(40, 40) at rot 0 whose nearest features are two corners, d apart on both axes: the edge-normal separations are d <= eps,
    the corners are sqrt(2) d > eps apart, and the narrow phase reports one record (the clip's extrapolated point) with pen = -d."""
    return [("rect", (40.0, 40.0))] * 2, np.array([[0.0, 300.0, 300.0], [0.0, 340.0 + d, 340.0 + d]])


def near_corner_pairs(n, seed=5):
    """n seeded two-body scenes with a corner of one hull placed within a few eps of a corner of the other, at random rotations: rects,
    triangles (needles included: interior angles down to a few degrees) and n-gons.  What a bound on the distance between the
    bodies would lose: the narrow phase tests the separation along edge normals only."""
    rng = np.random.default_rng(seed)

    def hull():
        r = rng.random()
        if r < 0.4:
            w, h = rng.uniform(5, 60, size=2)
            v = np.array([[w / 2, h / 2], [-w / 2, h / 2], [-w / 2, -h / 2], [w / 2, -h / 2]])
        elif r < 0.8:                                       # a triangle, counter-clockwise, centred on its centroid
            L, wd = rng.uniform(20, 80), rng.uniform(2, 40)
            v = np.array([[L, 0.0], [-L / 2, wd], [-L / 2, -wd]])
            v = v - v.mean(axis=0)
        else:
            nv = int(rng.integers(5, 9))
            ang = (np.arange(nv) + rng.uniform(-0.3, 0.3, nv)) * (2 * np.pi / nv)
            v = rng.uniform(10, 30) * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        return v

    rot = lambda v, t: v @ np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]).T

    def bisector(v, k):                                     # outward unit bisector of corner k
        e0, e1 = v[k] - v[k - 1], v[(k + 1) % len(v)] - v[k]
        m = np.array([e0[1], -e0[0]]) / np.linalg.norm(e0) + np.array([e1[1], -e1[0]]) / np.linalg.norm(e1)
        return m / np.linalg.norm(m)

    out = []
    for q in range(n):
        va, vb = hull(), hull()
        ka, kb = int(rng.integers(len(va))), int(rng.integers(len(vb)))
        ra = rng.uniform(-np.pi, np.pi)
        ua = bisector(rot(va, ra), ka)
        if q % 2:                                            # apex to apex: b's corner faces a's, a little beyond it along a's bisector
            ub = bisector(vb, kb)
            rb = np.arctan2(-ua[1], -ua[0]) - np.arctan2(ub[1], ub[0]) + rng.uniform(-0.2, 0.2)
            off = ua * rng.uniform(0.0, 4.0) * EPS + rng.uniform(-0.5, 0.5, size=2) * EPS
        else:
            rb = rng.uniform(-np.pi, np.pi)
            off = rng.uniform(-3, 3, size=2) * EPS
        ca, cb = rot(va, ra)[ka], rot(vb, rb)[kb]
        pa = np.array([300.0, 300.0])
        pb = pa + ca - cb + off                              # corner of b = corner of a + off
        out.append(([("hull", va), ("hull", vb)], np.array([[ra, pa[0], pa[1]], [rb, pb[0], pb[1]]])))
    return out
