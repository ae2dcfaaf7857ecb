"""The ray caster of lcp_sensors.hip (include/lcp_hip.h, "range sensors") restated as plain float64 torch operations on the CPU: the
yardstick of tests/test_hip_sensors.py.  Not a test.

    out = cast_host(case)        # dict: dist [B,R] f64 (with its graph), hit [B,R] i32, normal [B,R,2] f64, excluded [B,R] bool,
                                 #       gap [B,R] f64

The rule is written per body exactly as the header states it, with exactly its comparisons, vectorised over the rays (and over a
hull's edges).  The hit that is selected - the body, the entering edge - is an index, so autograd differentiates the selected
expression alone (`-b - sqrt(b^2 - cc)` of the circle, `-h_i / den_i` of the hull's edge i) and gives every gradient.

`excluded` marks the rays the mirror itself cannot decide, which a comparison leaves out: |n . u| < 0.05 at the hit (a grazing ray:
the distance is ill-conditioned), or two nearest candidate distances closer than 1e-9 - the two nearest bodies (which one is hit is
rounding) or the two latest entering edges of the hull that is hit (a ray through a vertex: which normal is rounding).  `gap` is the
distance of every ray from its nearest change of branch (another body or entering edge, its range, 0): finite differences of the
mirror are taken where it is not small.

`case(name)` builds the inputs the GPU tests use, dicts of CPU tensors (kind, radius, verts_local, nverts, p, ray_body, ray_origin,
ray_angle, ray_range) plus `names` (the named rays' indices); `reference(name)` computes the mirror and its gradients once per case
and shares them."""
import math

import numpy as np
import torch

from tests.render_host import _hull, _rect

F64 = torch.float64
INF = float("inf")
GRAZING, TIE = 0.05, 1e-9
LEAVES = ("p", "radius", "verts_local", "ray_origin", "ray_angle")


def world_rays(p, body, origin, angle):
    """o [B,R,2], u [B,R,2] and `ok` [B,R] (False: a mounting body outside [0, nb) other than -1 - the ray misses)."""
    B, R = body.shape
    nb = p.shape[1]
    mounted = (body >= 0) & (body < nb)
    pm = torch.gather(p, 1, body.clamp(0, nb - 1).long().unsqueeze(-1).expand(B, R, 3))
    zero = torch.zeros((), dtype=F64)
    rot, cx, cy = (torch.where(mounted, pm[..., i], zero) for i in range(3))              # the world frame: rot 0 at (0, 0)
    sn, cs = torch.sin(rot), torch.cos(rot)
    lx, ly = origin[..., 0], origin[..., 1]
    o = torch.stack([cx + (cs * lx - sn * ly), cy + (sn * lx + cs * ly)], -1)
    a = rot + angle
    return o, torch.stack([torch.cos(a), torch.sin(a)], -1), mounted | (body == -1)


def _circle(o, u, c, r):
    """s [B,R] (+inf: a miss) and n [B,R,2] of one circle per scene: c [B,1,2], r [B,1]."""
    q = o - c
    b = (q * u).sum(-1)
    cc = (q * q).sum(-1) - r * r
    disc = b * b - cc
    inside = cc <= 0
    miss = ~inside & ((b >= 0) | (disc < 0))
    root = torch.sqrt(torch.where(inside | miss, torch.ones_like(disc), disc))
    s = torch.where(inside, torch.zeros_like(b), torch.where(miss, torch.full_like(b, INF), -b - root))
    sf = torch.where(torch.isfinite(s), s, torch.zeros_like(s)).detach()
    n = (o + sf.unsqueeze(-1) * u - c) / r.unsqueeze(-1)
    return s, n


def _hull_world(verts_local, nv, pose):
    """World vertices, edges, outward normals [B,cap,2] and `live` [B,cap] of one hull per scene (render_host.signed_distance)."""
    cap = verts_local.shape[1]
    ar = torch.arange(cap)
    live = ar.unsqueeze(0) < nv.unsqueeze(1)
    zero = torch.zeros((), dtype=F64)
    lx, ly = torch.where(live, verts_local[..., 0], zero), torch.where(live, verts_local[..., 1], zero)     # slots >= nverts: never used
    rot, cx, cy = pose[:, 0:1], pose[:, 1:2], pose[:, 2:3]
    sn, cs = torch.sin(rot), torch.cos(rot)
    wx, wy = cx + (cs * lx - sn * ly), cy + (sn * lx + cs * ly)                          # utils.py:105-112
    nxt = torch.where(ar.unsqueeze(0) + 1 >= nv.unsqueeze(1), torch.zeros_like(nv).unsqueeze(1), (ar + 1).expand_as(live)).clamp(max=cap - 1)
    ex, ey = torch.gather(wx, 1, nxt) - wx, torch.gather(wy, 1, nxt) - wy
    ex, ey = torch.where(live, ex, torch.ones((), dtype=F64)), torch.where(live, ey, zero)
    L = torch.sqrt(ex * ex + ey * ey)
    return torch.stack([wx, wy], -1), torch.stack([ex, ey], -1), torch.stack([ey / L, -ex / L], -1), live   # contacts.py:229-231


def _hull_cast(o, u, w, e, n, live, nv):
    """s [B,R] (+inf: a miss), the normal [B,R,2] and the gap between the two latest entering edges [B,R] of one hull per scene."""
    B, R = o.shape[:2]
    e4 = lambda t: t.unsqueeze(1)                                                        # [B,1,cap,..]
    q = o.unsqueeze(2) - e4(w)                                                           # [B,R,cap,2]
    h = (e4(n) * q).sum(-1)
    den = (e4(n) * u.unsqueeze(2)).sum(-1)
    lv = e4(live).expand_as(h)
    inside = ((h <= 0) | ~lv).all(-1)
    miss = (lv & (den == 0) & (h > 0)).any(-1)
    cand = -h / torch.where(den == 0, torch.ones_like(den), den)
    enter = torch.where(lv & (den < 0), cand, torch.full_like(cand, -INF))
    leave = torch.where(lv & (den > 0), cand, torch.full_like(cand, INF))
    s_in, e_in = enter.detach().max(-1)                                                  # (the first index on ties)
    s_out = leave.detach().min(-1).values
    hit = ~inside & ~miss & (0 <= s_in) & (s_in <= s_out) & (nv >= 3).unsqueeze(1)
    s_sel = torch.gather(cand, 2, e_in.unsqueeze(-1)).squeeze(-1)                        # -h_i / den_i of the selected edge, with its graph
    s = torch.where(inside & (nv >= 3).unsqueeze(1), torch.zeros_like(s_sel), torch.where(hit, s_sel, torch.full_like(s_sel, INF)))
    nrm = torch.gather(e4(n).expand(B, R, *n.shape[1:]), 2, e_in.reshape(B, R, 1, 1).expand(B, R, 1, 2)).squeeze(2)
    top2 = enter.detach().topk(2, dim=-1).values
    gap = torch.where(hit, top2[..., 0] - top2[..., 1], torch.full_like(s_in, INF))
    return s, nrm, gap


def cast_host(case, scene_verts_max=None):
    kind, nverts, p = case["kind"], case["nverts"], case["p"]
    radius, verts_local = case["radius"], case["verts_local"]
    body, rng = case["ray_body"], case["ray_range"]
    B, nb = kind.shape
    cap = verts_local.shape[2]
    R = body.shape[1]
    o, u, ok = world_rays(p, body, case["ray_origin"], case["ray_angle"])
    nvs = torch.where(kind != 0, nverts.clamp(0, cap), torch.zeros_like(nverts))
    if scene_verts_max is not None:                                                      # a scene with more vertices is not sensed
        ok = ok & (nvs.sum(1) <= scene_verts_max).unsqueeze(1)
    S, N, G = [], [], []
    for k in range(nb):
        # (a body is a circle in some scenes and a hull in others: both are evaluated, the kind selects)
        sc, nc = _circle(o, u, p[:, k, 1:3].unsqueeze(1), radius[:, k].unsqueeze(1))
        w, e, n, live = _hull_world(verts_local[:, k], nvs[:, k], p[:, k])
        sh, nh, gh = _hull_cast(o, u, w, e, n, live, nvs[:, k])
        circ = (kind[:, k] == 0).unsqueeze(1)
        s = torch.where(circ, sc, sh)
        s = torch.where(ok & (body != k), s, torch.full_like(s, INF))                    # a ray never tests its own mounting body
        S.append(s)
        N.append(torch.where(circ.unsqueeze(-1), nc, nh))
        G.append(torch.where(circ, torch.full_like(gh, INF), gh))
    S, N, G = torch.stack(S, -1), torch.stack(N, 2), torch.stack(G, -1)                  # [B,R,nb], [B,R,nb,2], [B,R,nb]
    smin, kmin = S.detach().min(-1)                                                      # (the smallest k on ties)
    s = torch.gather(S, 2, kmin.unsqueeze(-1)).squeeze(-1)
    struck = torch.isfinite(smin) & (smin < rng)
    dist = torch.where(struck, s, rng)
    hit = torch.where(struck, kmin, torch.full_like(kmin, -1)).to(torch.int32)
    n = torch.gather(N.detach(), 2, kmin.reshape(B, R, 1, 1).expand(B, R, 1, 2)).squeeze(2)
    moving = struck & (smin > 0)
    normal = torch.where(moving.unsqueeze(-1), n, torch.zeros_like(n))
    with torch.no_grad():
        nu = (normal * u).sum(-1).abs()
        two = S.detach().topk(2, dim=-1, largest=False).values if nb > 1 else torch.stack([smin, torch.full_like(smin, INF)], -1)
        body_gap = torch.where(torch.isfinite(two[..., 0]), two[..., 1] - two[..., 0], torch.full_like(smin, INF))
        edge_gap = torch.where(moving, torch.gather(G, 2, kmin.unsqueeze(-1)).squeeze(-1), torch.full_like(smin, INF))
        excluded = (moving & (nu < GRAZING)) | (struck & (body_gap < TIE)) | (edge_gap < TIE)
        gap = torch.minimum(torch.minimum(body_gap, edge_gap), torch.where(torch.isfinite(smin), (smin - rng).abs(), torch.full_like(smin, INF)))
        gap = torch.where(struck & ~moving, torch.zeros_like(gap), gap)                  # (s = 0: on a branch by definition)
    return dict(dist=dist, hit=hit, normal=normal, excluded=excluded, gap=gap, nu=nu)


# ------------------------------------------------------------------------------------------------------------- the cases
def _assemble(bodies, cap):
    """bodies[b][k] = ("circle", (rot, x, y), r) | ("hull", (rot, x, y), verts [nv,2])."""
    B, nb = len(bodies), len(bodies[0])
    kind, nverts = torch.zeros(B, nb, dtype=torch.int32), torch.zeros(B, nb, dtype=torch.int32)
    radius = torch.zeros(B, nb, dtype=F64)
    verts, p = torch.zeros(B, nb, cap, 2, dtype=F64), torch.zeros(B, nb, 3, dtype=F64)
    for b in range(B):
        for k, (what, pose, shape) in enumerate(bodies[b]):
            p[b, k] = torch.tensor(pose, dtype=F64)
            if what == "circle":
                radius[b, k] = shape
            else:
                kind[b, k], nverts[b, k] = 1, len(shape)
                verts[b, k, :len(shape)] = torch.tensor(np.asarray(shape), dtype=F64)
    return dict(kind=kind, radius=radius, verts_local=verts, nverts=nverts, p=p)


def _rays(rows):
    """rows[b] = [(body, (ox, oy), angle, range)]."""
    t = lambda f, dt_: torch.tensor([[f(r) for r in row] for row in rows], dtype=dt_)
    return dict(ray_body=t(lambda r: r[0], torch.int32), ray_origin=t(lambda r: list(r[1]), F64), ray_angle=t(lambda r: r[2], F64),
                ray_range=t(lambda r: r[3], F64))


def _fan(body, n, origin, centre, fov, rng_):
    return [(body, origin, centre + fov * (i / n - 0.5), rng_) for i in range(n)]


SMALL_NAMES = dict(miss=0, clamp=1, inside_circle=2, inside_rect=3, parallel_outside=4, parallel_between=5, vertex=6, body_high=7,
                   body_low=8)
RECT = (60.0, 30.0)


def _small(rng):
    """B = 3, nb = 5 (a circle, an axis-aligned rect, a pentagon, a triangle, a two-vertex hull that is never hit), capacity 8, R = 70:
    nine named rays, a fan on each body and one on the world frame.  Coordinates of order 100."""
    bodies, rows = [], []
    for b in range(3):
        j = lambda s: float(rng.uniform(-s, s))
        circ = (j(3), 100.0 + j(5), 100.0 + j(5))
        rect = (0.0, 220.0 + j(5), 100.0 + j(5))                                         # rot = 0: its normals are exact
        bodies.append([("circle", circ, 18.0 + j(2)), ("hull", rect, _rect(*RECT)),
                       ("hull", (j(3), 150.0 + j(5), 190.0 + j(5)), _hull(rng, 5, 26.0, 22.0)),
                       ("hull", (j(3), 80.0 + j(5), 200.0 + j(5)), _hull(rng, 3, 24.0, 20.0)),
                       ("hull", (j(3), 160.0 + j(3), 60.0 + j(3)), [[-10.0, 0.0], [10.0, 0.0]])])
        rx, ry = rect[1], rect[2]
        eye = (rx - 80.0, ry + 60.0)
        vx, vy = rx - RECT[0] / 2, ry + RECT[1] / 2
        row = [(-1, (0.0, 0.0), math.pi + 0.3, 500.0),                                   # miss: away from everything
               (-1, (20.0, circ[2]), 0.0, 30.0),                                          # clamp: the circle is about 60 away
               (-1, (circ[1] + 3.0, circ[2] + 2.0), 1.0 + j(1), 300.0),                   # inside the circle
               (-1, (rx - 7.0, ry + 4.0), 2.0 + j(1), 300.0),                             # inside the rect
               (-1, (rx - 50.0, ry + RECT[1] / 2 + 5.0), 0.0, 300.0),                     # parallel to the rect's long edges, outside
               (-1, (rx - 50.0, ry + 5.0), 0.0, 300.0),                                   # parallel, between them: the left face at 20
               (-1, eye, math.atan2(vy - eye[1], vx - eye[0]), 300.0),                    # aimed at a vertex of the rect
               (7, (0.0, 0.0), 0.0, 300.0), (-2, (0.0, 0.0), 0.0, 300.0)]                 # mounting bodies out of range
        row += _fan(0, 12, (0.0, 0.0), j(3), 5.8, 300.0)                                 # on the circle, from its centre
        row += _fan(1, 12, (5.0, -3.0), j(3), 5.8, 300.0)                                # on the rect
        row += _fan(2, 12, (2.0, 1.0), j(3), 5.8, 60.0)                                  # on the pentagon, short range: some clamp
        row += _fan(3, 12, (-1.0, 2.0), j(3), 5.8, 300.0)                                # on the triangle
        row += _fan(4, 4, (0.0, 3.0), j(3), 5.0, 300.0)                                  # on the two-vertex hull
        row += _fan(-1, 9, (150.0 + j(5), 130.0 + j(5)), j(3), 5.6, 300.0)               # on the world frame
        rows.append(row)
    c = _assemble(bodies, 8)
    c.update(_rays(rows))
    c["names"] = SMALL_NAMES
    return c


def _wide(rng):
    """B = 2, nb = 64 16-gons on a grid (1024 hull vertices), capacity 16, R = 1024: four fans of 256 rays."""
    bodies, rows = [], []
    for b in range(2):
        j = lambda s: float(rng.uniform(-s, s))
        bodies.append([("hull", (j(3), 100.0 * (k % 8) + j(15), 100.0 * (k // 8) + j(15)), _hull(rng, 16, 30.0 + j(5), 30.0 + j(5)))
                       for k in range(64)])
        row = _fan(0, 256, (0.0, 0.0), j(3), 6.2, 400.0) + _fan(27, 256, (3.0, -2.0), j(3), 6.2, 400.0)
        row += _fan(63, 256, (0.0, 0.0), j(3), 6.2, 150.0) + _fan(-1, 256, (350.0 + j(5), 450.0 + j(5)), j(3), 6.2, 400.0)
        rows.append(row)
    c = _assemble(bodies, 16)
    c.update(_rays(rows))
    c["names"] = {}
    return c


def _tiny(rng):
    """B = 2, nb = 3 (circle, rect, pentagon), R = 6, every ray a clean hit: the inputs of gradcheck."""
    bodies, rows = [], []
    for b in range(2):
        j = lambda s: float(rng.uniform(-s, s))
        bodies.append([("circle", (j(1), 100.0 + j(3), 100.0 + j(3)), 15.0), ("hull", (0.3 + j(0.2), 180.0 + j(3), 110.0 + j(3)), _rect(40.0, 30.0)),
                       ("hull", (j(1), 140.0 + j(3), 170.0 + j(3)), _hull(rng, 5, 22.0, 20.0))])
        rows.append([(0, (1.0, 2.0), math.atan2(10.0, 80.0) - bodies[-1][0][1][0] + j(0.05), 300.0),       # circle -> rect
                     (0, (0.0, 0.0), math.atan2(70.0, 40.0) - bodies[-1][0][1][0] + j(0.05), 300.0),       # circle -> pentagon
                     (1, (2.0, 1.0), math.pi - bodies[-1][1][1][0] + math.atan2(10.0, 80.0) + j(0.03), 300.0),   # rect -> circle
                     (2, (0.0, 1.0), math.atan2(-70.0, -40.0) - bodies[-1][2][1][0] + j(0.05), 300.0),     # pentagon -> circle
                     (-1, (140.0, 60.0), math.atan2(40.0, -40.0) + j(0.05), 300.0),                        # world -> circle
                     (-1, (240.0, 200.0), math.atan2(-30.0, -100.0) + j(0.03), 300.0)])                    # world -> pentagon
    c = _assemble(bodies, 8)
    c.update(_rays(rows))
    c["names"] = {}
    return c


_BUILD = {"small": (_small, 1), "wide": (_wide, 2), "tiny": (_tiny, 7)}          # (seeds: the mirror alone decides them, test_sensors_host.py)
CASE_NAMES = ("small", "wide")
_CACHE, _REF = {}, {}


def case(name):
    """The inputs of case `name` (CPU tensors; treat them as read-only: they are shared)."""
    if name not in _CACHE:
        fn, seed = _BUILD[name]
        _CACHE[name] = fn(np.random.default_rng(seed))
    return _CACHE[name]


def leaves(c):
    """A copy of case `c` whose p, radius, verts_local, ray_origin and ray_angle are fresh leaves that require grad."""
    out = dict(c)
    for k in LEAVES:
        out[k] = c[k].clone().requires_grad_(True)
    return out


def reference(name, seed=0):
    """Computed once per case and shared: the mirror's outputs, a random cotangent `g_dist` that is zero on the excluded rays (so
    that they reach no gradient of either side), and autograd's gradients for it."""
    if name not in _REF:
        c = leaves(case(name))
        out = cast_host(c)
        g = torch.randn(out["dist"].shape, generator=torch.Generator().manual_seed(200 + seed), dtype=F64)
        g = torch.where(out["excluded"], torch.zeros_like(g), g)
        grads = torch.autograd.grad(out["dist"], [c[k] for k in LEAVES], g, allow_unused=True)
        grads = [torch.zeros_like(c[k]) if gr is None else gr for k, gr in zip(LEAVES, grads)]
        _REF[name] = dict(dist=out["dist"].detach(), hit=out["hit"], normal=out["normal"].detach(), excluded=out["excluded"],
                          gap=out["gap"], g_dist=g, grads=dict(zip(LEAVES, grads)))
    return _REF[name]
