"""The drawing of lcp_render_marks.hip (include/lcp_hip.h, "drawing": bodies, their marks, the joints' markers) restated as plain
float64 torch operations on the CPU, so that autograd gives all eight gradients: the yardstick of tests/test_hip_render_marks.py.
Not a test.  The pixel centres and the bodies' signed distance are those of tests/render_host.py.

    image, ids, margin = render_marks_host(case)    # image [B,C,H,W] f64 (with its graph), ids [B,H,W] i32, margin: float

A case is a case of render_host.py plus: mark [B,nb] i32 or None, mark_colors [B,nb,C] f32, jtype / jb1 / jb2 [B,nj] i32, jr1 / jrot1
[B,nj] f64, joint_colors [B,nj,C] f32 (nj may be 0), order, line_w, dot_r, joint_w, joint_r.

`margin` extends render_host's: for every primitive (segment, disc, ring) the distance of every pixel from the ends of its coverage
ramps, | |d + s| - w/2 | for s in {0, ring thickness}, and, for a pixel strictly inside a ramp, its distance from the segment's LINE (a
segment of no length: from its point) or the disc's centre - where the direction dd/dx is undefined.  With no marks and no joints the
function performs render_host's operations in render_host's order: the same bits."""
import math

import numpy as np
import torch

from tests import render_host as RH
from tests.render_host import pixel_centres, signed_distance

F64 = torch.float64
INF = float("inf")
SPOKE, CENTRE, DIAGONALS = 1, 2, 3
JOINT, FIXED, XCON, YCON, ROTCON, TOTAL = 1, 2, 3, 4, 5, 6          # lcp_physics_amd/physics/joints.py


def _e(t):
    """[B] -> [B,1,1]"""
    return t.reshape(-1, 1, 1)


def segment(A, B_, X, Y):
    """Distance of every pixel from the segment A -> B (each [B,2]) and from its line (a segment of no length: from A), [B,H,W].  The
    projection parameter of a segment of no length is 0: nothing is divided by |AB|^2."""
    ax, ay, bx, by = _e(A[:, 0]), _e(A[:, 1]), _e(B_[:, 0]), _e(B_[:, 1])
    qx, qy = X - ax, Y - ay
    ex, ey = bx - ax, by - ay
    l2 = ex * ex + ey * ey
    has = l2 > 0
    t = torch.where(has, (qx * ex + qy * ey) / torch.where(has, l2, torch.ones_like(l2)), torch.zeros((), dtype=F64)).clamp(0.0, 1.0)
    dist = torch.linalg.vector_norm(torch.stack([qx - t * ex, qy - t * ey], -1), dim=-1)
    with torch.no_grad():
        L = torch.sqrt(torch.where(has, l2, torch.ones_like(l2)))
        line = torch.where(has, (qx * ey - qy * ex).abs() / L, dist.detach())
    return dist, line


def point(A, X, Y):
    return torch.linalg.vector_norm(torch.stack([X - _e(A[:, 0]), Y - _e(A[:, 1])], -1), dim=-1)


class _Painter:
    """Back-to-front compositing with the margin's terms collected on the way."""

    def __init__(self, image, w):
        self.image, self.w, self.terms = image, w, []

    def cov(self, d):
        return (0.5 - d / self.w).clamp(0.0, 1.0)

    def paint(self, alpha, colour):
        """alpha [B,H,W], colour [B,C]"""
        a = alpha.unsqueeze(1)
        self.image = self.image * (1 - a) + a * colour.reshape(*colour.shape, 1, 1)

    def primitive(self, live, d, sing, colour, ring=None):
        """A primitive drawn in the scenes `live` [B] bool: signed distance d [B,H,W], `sing`: each pixel's distance from where the
        direction of d is undefined."""
        w = self.w
        alpha = self.cov(d) if ring is None else self.cov(d) - self.cov(d + ring)
        self.paint(torch.where(_e(live), alpha, torch.zeros((), dtype=F64)), colour)
        with torch.no_grad():
            dd, big = d.detach(), torch.full((), INF, dtype=F64)
            on = _e(live) & torch.isfinite(dd)
            self.terms.append(torch.where(on, (dd.abs() - w / 2).abs(), big))
            band = dd.abs() < w / 2
            if ring is not None:
                self.terms.append(torch.where(on, ((dd + ring).abs() - w / 2).abs(), big))
                band = band | ((dd + ring).abs() < w / 2)
            self.terms.append(torch.where(on & band, sing, big))


def render_marks_host(case):
    """image [B,C,H,W] f64, ids [B,H,W] i32, margin; the tensors of the case that require grad stay connected."""
    H, W, x0, y0, ppm, w = case["H"], case["W"], case["x0"], case["y0"], case["ppm"], case["w"]
    kind, nverts, thickness = case["kind"], case["nverts"], case["thickness"]
    colors, background = case["colors"].to(F64), case["background"].to(F64)
    p, radius, verts_local = case["p"], case["radius"], case["verts_local"]
    B, nb = kind.shape
    C = colors.shape[-1]
    cap = verts_local.shape[2]
    mark = case.get("mark")
    order = case.get("order", 0)
    line_w, dot_r, joint_w, joint_r = (case.get(k) for k in ("line_w", "dot_r", "joint_w", "joint_r"))
    X, Y = pixel_centres(H, W, x0, y0, ppm)
    d, gap = signed_distance(kind, radius, verts_local, nverts, p, X, Y)
    cov = lambda dd: (0.5 - dd / w).clamp(0.0, 1.0)
    th = thickness.reshape(B, nb, 1, 1)
    outlined = th > 0
    alpha = torch.where(outlined, cov(d) - cov(d + th), cov(d))
    P = _Painter(background.reshape(1, C, 1, 1).expand(B, C, H, W), w)
    ids = torch.full((B, H, W), -1, dtype=torch.int32)
    hull = kind != 0
    nv = torch.where(hull, nverts.clamp(0, cap), torch.zeros_like(nverts))
    if mark is not None:
        mcol = case["mark_colors"].to(F64)
        rot, c = p[..., 0], p[..., 1:]
        sn, cs = torch.sin(rot), torch.cos(rot)

    def draw_mark(k, codes):
        for code in codes:
            live = mark[:, k] == code
            if code == SPOKE:
                live = live & ~hull[:, k]
            elif code == DIAGONALS:
                live = live & hull[:, k] & (nv[:, k] == 4)
            if not bool(live.any()):
                continue
            ck = c[:, k]
            if code == SPOKE:
                tip = ck + radius[:, k:k + 1] * torch.stack([cs[:, k], sn[:, k]], -1)
                dist, line = segment(ck, tip, X, Y)
                P.primitive(live, dist - line_w / 2, line, mcol[:, k])
            elif code == CENTRE:
                dist = point(ck, X, Y)
                P.primitive(live, dist - dot_r, dist.detach(), mcol[:, k])
            else:
                v = verts_local[:, k, :4]
                wv = ck.unsqueeze(1) + torch.stack([cs[:, k:k + 1] * v[..., 0] - sn[:, k:k + 1] * v[..., 1],
                                                    sn[:, k:k + 1] * v[..., 0] + cs[:, k:k + 1] * v[..., 1]], -1)      # utils.py:105-112
                for a, b in ((0, 2), (1, 3)):
                    dist, line = segment(wv[:, a], wv[:, b], X, Y)
                    P.primitive(live, dist - line_w / 2, line, mcol[:, k])

    for k in range(nb):
        if mark is not None:
            draw_mark(k, (SPOKE, DIAGONALS) if order == 0 else ())
        P.paint(alpha[:, k], colors[:, k])
        ids = torch.where(d[:, k].detach() <= 0, torch.full_like(ids, k), ids)
        if mark is not None:
            draw_mark(k, (CENTRE,) if order == 0 else (SPOKE, CENTRE, DIAGONALS))

    jtype = case.get("jtype")
    nj = 0 if jtype is None else jtype.shape[1]
    for j in range(nj):
        jb1, jb2, jcol = case["jb1"][:, j].long(), case["jb2"][:, j].long(), case["joint_colors"].to(F64)[:, j]
        ok1, ok2 = (jb1 >= 0) & (jb1 < nb), (jb2 >= 0) & (jb2 < nb)
        pick = lambda idx: torch.gather(p[..., 1:], 1, idx.clamp(0, nb - 1).reshape(B, 1, 1).expand(B, 1, 2)).squeeze(1)
        c1, c2 = pick(jb1), pick(jb2)
        t = jtype[:, j]
        off = lambda dx, dy: c1 + torch.tensor([dx, dy], dtype=F64)

        def tick(live, A, B_):
            dist, line = segment(A, B_, X, Y)
            P.primitive(live, dist - joint_w / 2, line, jcol)

        def ring(live):
            dist = point(c1, X, Y)
            P.primitive(live, dist - joint_r, dist.detach(), jcol, ring=line_w)

        live = ok1 & (t == JOINT)
        if bool(live.any()):
            at = c1 + case["jr1"][:, j:j + 1] * torch.stack([torch.cos(case["jrot1"][:, j]), torch.sin(case["jrot1"][:, j])], -1)
            dist = point(at, X, Y)
            P.primitive(live, dist - dot_r, dist.detach(), jcol)
        live = ok1 & ok2 & (t == FIXED)
        if bool(live.any()):
            tick(live, c1, c2)
        live = ok1 & (t == YCON)
        if bool(live.any()):
            tick(live, off(-joint_r, 0.0), off(joint_r, 0.0))
        live = ok1 & (t == XCON)
        if bool(live.any()):
            tick(live, off(0.0, -joint_r), off(0.0, joint_r))
        live = ok1 & (t == ROTCON)
        if bool(live.any()):
            ring(live)
        live = ok1 & (t == TOTAL)
        if bool(live.any()):
            ring(live)
            tick(live, off(-joint_r, 0.0), off(joint_r, 0.0))
            tick(live, off(0.0, -joint_r), off(0.0, joint_r))

    with torch.no_grad():
        dd = d.detach()
        fin = torch.isfinite(dd)
        big = torch.full((), INF, dtype=F64)
        ramp0, ramp1 = (dd.abs() - w / 2).abs(), ((dd + th).abs() - w / 2).abs()
        terms = [torch.where(fin, ramp0, big), torch.where(fin & outlined, ramp1, big), torch.where(fin, dd.abs(), big)]
        band = (dd.abs() < w / 2) | (outlined & ((dd + th).abs() < w / 2))
        terms.append(torch.where(fin & (dd <= 0) & band, gap, big))
        margin = float(min(t.min() for t in terms + P.terms))
    return P.image, ids, margin


# ------------------------------------------------------------------------------------------------------------- the cases
def _with_marks(c, mark, seed, nj=0, joints=None, order=0, per_scene=False, sizes=None):
    """Case `c` of render_host._assemble with marks [nb] / [B,nb], joints [(type, b1, b2, r1, rot1)] and random colours."""
    rng = np.random.default_rng(seed + 2000)
    B, nb = c["kind"].shape
    C = c["colors"].shape[2]
    ppm = c["ppm"]
    out = dict(c)
    out["mark"] = torch.tensor(np.broadcast_to(np.asarray(mark), (B, nb)).copy(), dtype=torch.int32)
    col = lambda n: torch.tensor(rng.uniform(0, 1, (B if per_scene else 1, n, C)), dtype=torch.float32).expand(B, n, C).contiguous()
    out["mark_colors"] = col(nb)
    joints = joints or []
    nj = len(joints)
    arr = lambda q, dt_: torch.tensor([[jn[q] for jn in joints]] * B, dtype=dt_).reshape(B, nj)
    out.update(jtype=arr(0, torch.int32), jb1=arr(1, torch.int32), jb2=arr(2, torch.int32), jr1=arr(3, F64), jrot1=arr(4, F64))
    if nj:                                                            # (the scenes' joints differ a little)
        out["jr1"] = out["jr1"] * torch.tensor(rng.uniform(0.9, 1.1, (B, nj)))
        out["jrot1"] = out["jrot1"] + torch.tensor(rng.uniform(-0.3, 0.3, (B, nj)))
    out["joint_colors"] = col(nj)
    line_w, dot_r, joint_w, joint_r = sizes or (1.0 / ppm, 2.0 / ppm, 2.0 / ppm, 5.0 / ppm)      # the reference's pixel sizes
    out.update(order=order, line_w=line_w, dot_r=dot_r, joint_w=joint_w, joint_r=joint_r)
    return out


def _marks3(rng):
    """19 x 23, w != one pixel: an outlined rect, circle and pentagon that overlap, with diagonals, spoke and centre dot."""
    cam = RH._CAM_SMALL
    rows = []
    for _ in range(3):
        a, b, c = RH._three_bodies(rng, cam)
        rows.append([a[:3] + (1.1 + rng.uniform(0, 0.4),), b[:3] + (0.9 + rng.uniform(0, 0.4),), c])
    return rows, cam


def _joints_bodies(rng):
    """40 x 70, five bodies: a tilted rect, a pentagon close to the top edge, a zero-radius circle and a circle on the same point, a
    circle at 1e15."""
    H, W, x0, y0, ppm, w = RH._CAM_TILES
    mx, my = x0 + W / ppm / 2, y0 + H / ppm / 2
    rows = []
    for _ in range(3):
        j = lambda s: rng.uniform(-s, s)
        px, py = mx + 31.3 + j(4), my + 9.1 + j(4)
        rows.append([("hull", (0.5 + j(0.2), mx - 28.0 + j(4), my + 6.0 + j(4)), RH._rect(44.0 + j(3), 25.0 + j(3)), 3.0 + j(0.5)),
                     ("hull", (j(1), mx + 3.0 + j(4), y0 + 6.5 + j(2)), RH._hull(rng, 5, 15.0, 12.0), 2.5 + j(0.5)),
                     ("circle", (j(1), px, py), 0.0, 0.0),
                     ("circle", (j(1), px, py), 13.0 + j(2), 3.0 + j(0.5)),
                     ("circle", (0.3, 1e15, my + j(3)), 25.0, 3.0)])
    return rows


_JOINTS = [(JOINT, 0, -1, 17.0, 0.7), (FIXED, 0, 1, 0.0, 0.0), (YCON, 4, -1, 0.0, 0.0), (XCON, 1, -1, 0.0, 0.0), (ROTCON, 2, -1, 0.0, 0.0),
           (TOTAL, 0, -1, 0.0, 0.0), (JOINT, 1, 0, 11.0, 2.1), (FIXED, 2, 3, 0.0, 0.0), (FIXED, 3, -1, 0.0, 0.0)]
# marks of the `joints` case: a spoke on a hull, diagonals on a pentagon, the zero-radius circle's spoke, code 7, a centre dot at 1e15
_JOINTS_MARKS = [SPOKE, DIAGONALS, SPOKE, 7, CENTRE]


def _limits(rng):
    """16 x 16, 64 bodies with a mark each and 64 joints, every circle meeting the image and every other circle."""
    cam = (16, 16, 100.7, 50.3, 1.25, 1.1)
    H, W, x0, y0, ppm, w = cam
    rows, marks = [], []
    for b in range(3):
        row = []
        for k in range(64):
            pose = (rng.uniform(-3, 3), x0 + rng.uniform(0.3, 0.7) * W / ppm, y0 + rng.uniform(0.3, 0.7) * H / ppm)
            th = 0.0 if rng.uniform() < 0.3 else rng.uniform(0.3, 0.9)
            what = k % 3
            if what == 0:
                row.append(("circle", pose, rng.uniform(3.7, 5.0), th))
            elif what == 1:
                row.append(("hull", pose, RH._rect(rng.uniform(7.5, 10.0), rng.uniform(7.5, 10.0)), th))
            else:
                row.append(("hull", pose, RH._hull(rng, int(rng.integers(3, 9)), rng.uniform(4.2, 5.0), rng.uniform(4.2, 5.0)), th))
        rows.append(row)
    marks = [(SPOKE, DIAGONALS, CENTRE)[k % 3] for k in range(64)]
    joints = []
    for j in range(64):
        b1 = int(rng.integers(0, 64))
        b2 = int((b1 + 1 + rng.integers(0, 63)) % 64)
        joints.append((1 + j % 6, b1, b2 if (1 + j % 6) in (JOINT, FIXED) else -1, rng.uniform(0.5, 3.0), rng.uniform(0, 2 * math.pi)))
    return rows, cam, marks, joints


# the seeds were chosen so that every case's decision margin exceeds 1e-6 (tests/test_render_marks_host.py checks it)
_SEEDS = {"marks3": 1, "marks3_over": 1, "joints": 1, "limits": 1}
CASE_NAMES = ("marks3", "marks3_over", "joints", "limits")
_CACHE, _REF = {}, {}


def _build(name, seed=None):
    seed = _SEEDS[name] if seed is None else seed
    rng = np.random.default_rng(seed)
    if name in ("marks3", "marks3_over"):
        rows, cam = _marks3(rng)
        c = RH._assemble(rows, cam, 3, seed, False, 8)
        return _with_marks(c, [DIAGONALS, SPOKE, CENTRE], seed, order=int(name == "marks3_over"))
    if name == "joints":
        c = RH._assemble(_joints_bodies(rng), RH._CAM_TILES, 4, seed, True, 8)
        return _with_marks(c, _JOINTS_MARKS, seed, joints=_JOINTS, per_scene=True)
    if name == "limits":
        rows, cam, marks, joints = _limits(rng)
        ppm = cam[4]
        c = RH._assemble(rows, cam, 3, seed, False, 8)
        # lines, dots and ticks small enough for 128 layers to leave something of each other
        return _with_marks(c, marks, seed, joints=joints, sizes=(0.6 / ppm, 1.0 / ppm, 0.8 / ppm, 2.5 / ppm))
    raise KeyError(name)


def case(name):
    """The inputs of case `name` (CPU tensors; treat them as read-only: they are shared)."""
    if name not in _CACHE:
        _CACHE[name] = _build(name)
    return _CACHE[name]


def spin_case(rot, mark):
    """One outlined circle at angle `rot`, with its spoke or without (19 x 23, w != one pixel, one channel, white on black)."""
    white = dict(colors=torch.ones(1, 1, 1, dtype=torch.float32), background=torch.zeros(1, dtype=torch.float32))
    c = dict(RH._assemble([[("circle", (rot, 11.3, 14.9), 7.5, 1.2)]], RH._CAM_SMALL, 1, 11, False, 8), **white)
    c = _with_marks(c, [mark], 11, sizes=(2.0, 2.0, 2.0, 5.0))
    c["mark_colors"] = torch.ones_like(c["mark_colors"])
    return c


GRAD_NAMES = ("p", "radius", "verts_local", "colors", "mark_colors", "joint_colors", "jrot1", "jr1")


def leaves(c):
    """A copy of case `c` whose eight differentiable inputs are fresh leaves that require grad."""
    out = dict(c)
    for k in GRAD_NAMES:
        if c.get(k) is not None:
            out[k] = c[k].clone().requires_grad_(True)
    return out


def reference(name, seed=0):
    """Computed once per case and shared: image, ids, margin, a random float32 cotangent and autograd's gradients for it."""
    if name not in _REF:
        c = leaves(case(name))
        image, ids, margin = render_marks_host(c)
        g = torch.randn(image.shape, generator=torch.Generator().manual_seed(200 + seed), dtype=torch.float32)
        grads = torch.autograd.grad(image, [c[k] for k in GRAD_NAMES], g.to(F64), allow_unused=True)
        grads = [torch.zeros_like(c[k]) if gr is None else gr for k, gr in zip(GRAD_NAMES, grads)]
        _REF[name] = dict(image=image.detach(), ids=ids, margin=margin, g_image=g, grads=dict(zip(GRAD_NAMES, grads)))
    return _REF[name]
