"""The drawing of lcp_render.hip (include/lcp_hip.h, "drawing") restated as plain float64 torch operations on the CPU, so that
autograd gives every gradient: the yardstick of tests/test_hip_render.py.  Not a test.

    image, ids, margin = render_host(case)          # image [B,C,H,W] f64 (with its graph), ids [B,H,W] i32, margin: float

`margin` is the decision margin of the inputs: how far every pixel is from a point where the formulas change branch - the ends of
a coverage ramp (| |d_k + s| - w/2 | for s in {0, thickness_k}), the silhouette (|d_k|) and, for pixels inside a hull and within a
ramp, a tie of the two largest half-plane distances.  A parity test asserts `margin > 1e-6` before it compares anything: a condition
on its INPUTS (no pixel is ever left out), under which a difference of 1e-12 in d cannot change a branch.

`case(name)` builds the inputs the GPU tests use: dicts of CPU tensors (kind, radius, verts_local, nverts, p, colors,
background, thickness) plus the camera (H, W, x0, y0, ppm, w); `reference(name)`
computes the restatement and its gradients once per case and shares them."""
import math

import numpy as np
import torch

F64 = torch.float64
INF = float("inf")


def pixel_centres(H, W, x0, y0, ppm):
    X = x0 + (torch.arange(W, dtype=F64) + 0.5) / ppm
    Y = y0 + (torch.arange(H, dtype=F64) + 0.5) / ppm
    return X.reshape(1, W).expand(H, W), Y.reshape(H, 1).expand(H, W)


def signed_distance(kind, radius, verts_local, nverts, p, X, Y):
    """d [B,nb,H,W] (+inf for a hull of fewer than three vertices: not drawn) and the gap between the two largest half-plane
    distances of every hull pixel [B,nb,H,W] (+inf for circles)."""
    B, nb, cap, _ = verts_local.shape
    hull = kind != 0
    ar = torch.arange(cap)
    nv = torch.where(hull, nverts.clamp(0, cap), torch.zeros_like(nverts)).unsqueeze(-1)
    live = ar < nv                                                                   # [B,nb,cap]
    zero = torch.zeros((), dtype=F64)
    lx, ly = torch.where(live, verts_local[..., 0], zero), torch.where(live, verts_local[..., 1], zero)      # slots >= nverts: never used
    rot, cx, cy = p[..., 0:1], p[..., 1:2], p[..., 2:3]
    sn, cs = torch.sin(rot), torch.cos(rot)
    wx, wy = cx + (cs * lx - sn * ly), cy + (sn * lx + cs * ly)                      # utils.py:105-112
    nxt = torch.where(ar + 1 >= nv, torch.zeros_like(nv), (ar + 1).expand_as(live)).clamp(max=cap - 1)
    ex, ey = torch.gather(wx, 2, nxt) - wx, torch.gather(wy, 2, nxt) - wy
    ex, ey = torch.where(live, ex, torch.ones((), dtype=F64)), torch.where(live, ey, zero)
    L = torch.sqrt(ex * ex + ey * ey)
    nx, ny = ey / L, -ex / L                                                         # left_orthogonal(e) / |e|, contacts.py:229-231
    e5 = lambda t: t.reshape(B, nb, 1, 1, cap)
    qx, qy = X.reshape(1, 1, *X.shape, 1) - e5(wx), Y.reshape(1, 1, *Y.shape, 1) - e5(wy)       # [B,nb,H,W,cap]
    live5 = e5(live)
    h = torch.where(live5, e5(nx) * qx + e5(ny) * qy, torch.full((), -INF, dtype=F64))
    m = h.max(-1).values
    t = ((qx * e5(ex) + qy * e5(ey)) / e5(L * L)).clamp(0.0, 1.0)
    r = torch.stack([qx - t * e5(ex), qy - t * e5(ey)], -1)
    dist = torch.where(live5, torch.linalg.vector_norm(r, dim=-1), torch.full((), INF, dtype=F64))
    d_hull = torch.where(m <= 0, m, dist.min(-1).values)
    d_hull = torch.where((nv >= 3).reshape(B, nb, 1, 1), d_hull, torch.full((), INF, dtype=F64))
    c4 = lambda t: t.reshape(B, nb, 1, 1)
    d_circ = torch.linalg.vector_norm(torch.stack([X - c4(p[..., 1]), Y - c4(p[..., 2])], -1), dim=-1) - c4(radius)
    d = torch.where(c4(hull), d_hull, d_circ)
    with torch.no_grad():
        if cap >= 2:
            top2 = h.detach().topk(2, dim=-1).values
            gap = torch.where(c4(hull) & (nv >= 3).reshape(B, nb, 1, 1), top2[..., 0] - top2[..., 1], torch.full((), INF, dtype=F64))
        else:
            gap = torch.full(d.shape, INF, dtype=F64)
    return d, gap


def render_host(case):
    """image [B,C,H,W] f64, ids [B,H,W] i32, margin - from a case of `case()` (or any dict with its keys); the tensors of the
    case that require grad stay connected.  `colors` may be float32 (it is widened here, so its gradient comes back as float32)."""
    H, W, x0, y0, ppm, w = case["H"], case["W"], case["x0"], case["y0"], case["ppm"], case["w"]
    kind, nverts, thickness = case["kind"], case["nverts"], case["thickness"]
    colors, background = case["colors"].to(F64), case["background"].to(F64)
    B, nb = kind.shape
    C = colors.shape[-1]
    X, Y = pixel_centres(H, W, x0, y0, ppm)
    d, gap = signed_distance(kind, case["radius"], case["verts_local"], nverts, case["p"], X, Y)
    cov = lambda dd: (0.5 - dd / w).clamp(0.0, 1.0)
    th = thickness.reshape(B, nb, 1, 1)
    outlined = th > 0
    alpha = torch.where(outlined, cov(d) - cov(d + th), cov(d))
    image = background.reshape(1, C, 1, 1).expand(B, C, H, W)
    ids = torch.full((B, H, W), -1, dtype=torch.int32)
    for k in range(nb):
        a = alpha[:, k].unsqueeze(1)
        image = image * (1 - a) + a * colors[:, k].reshape(B, C, 1, 1)
        ids = torch.where(d[:, k].detach() <= 0, torch.full_like(ids, k), ids)
    with torch.no_grad():
        dd = d.detach()
        fin = torch.isfinite(dd)
        big = torch.full((), INF, dtype=F64)
        ramp0, ramp1 = (dd.abs() - w / 2).abs(), ((dd + th).abs() - w / 2).abs()
        terms = [torch.where(fin, ramp0, big), torch.where(fin & outlined, ramp1, big), torch.where(fin, dd.abs(), big)]
        band = (dd.abs() < w / 2) | (outlined & ((dd + th).abs() < w / 2))
        terms.append(torch.where(fin & (dd <= 0) & band, gap, big))
        margin = float(min(t.min() for t in terms))
    return image, ids, margin


# ------------------------------------------------------------------------------------------------------------- the cases
def _hull(rng, nv, a, b):
    """nv vertices on an ellipse at increasing angles: convex, the reference's order (bodies.py:228-235)."""
    th = (np.arange(nv) + rng.uniform(-0.3, 0.3, nv)) * (2 * math.pi / nv) + rng.uniform(0, 2 * math.pi)
    return np.stack([a * np.cos(th), b * np.sin(th)], -1) + rng.uniform(-0.1, 0.1, 2) * min(a, b)


def _rect(wd, ht):
    hw, hh = wd / 2, ht / 2
    return np.array([[hw, hh], [-hw, hh], [-hw, -hh], [hw, -hh]])                    # bodies.py:260-262


def _assemble(bodies, cam, C, seed, per_scene_colors, cap, background=None):
    """bodies[b][k] = ("circle", (rot, x, y), r, thickness) | ("hull", (rot, x, y), verts [nv,2], thickness)."""
    rng = np.random.default_rng(seed + 1000)
    B, nb = len(bodies), len(bodies[0])
    kind, nverts = torch.zeros(B, nb, dtype=torch.int32), torch.zeros(B, nb, dtype=torch.int32)
    radius, thick = torch.zeros(B, nb, dtype=F64), torch.zeros(B, nb, dtype=F64)
    verts, p = torch.zeros(B, nb, cap, 2, dtype=F64), torch.zeros(B, nb, 3, dtype=F64)
    for b in range(B):
        for k, (what, pose, shape, th) in enumerate(bodies[b]):
            p[b, k] = torch.tensor(pose, dtype=F64)
            thick[b, k] = th
            if what == "circle":
                radius[b, k] = shape
            else:
                kind[b, k], nverts[b, k] = 1, len(shape)
                verts[b, k, :len(shape)] = torch.tensor(np.asarray(shape), dtype=F64)
    colors = torch.tensor(rng.uniform(0, 1, (B if per_scene_colors else 1, nb, C)), dtype=torch.float32)
    bg = torch.tensor(rng.uniform(0, 1, C) if background is None else background, dtype=torch.float32)
    H, W, x0, y0, ppm, w = cam
    return dict(kind=kind, radius=radius, verts_local=verts, nverts=nverts, p=p, colors=colors.expand(B, nb, C).contiguous(), background=bg,
                thickness=thick, H=H, W=W, x0=x0, y0=y0, ppm=ppm, w=w, per_scene_colors=per_scene_colors)


def _random_bodies(rng, B, nb, cap, cam, size, nv_of=None):
    H, W, x0, y0, ppm, w = cam
    ext_x, ext_y = W / ppm, H / ppm
    out = []
    for b in range(B):
        row = []
        for k in range(nb):
            pose = (rng.uniform(-3, 3), x0 + rng.uniform(-0.1, 1.1) * ext_x, y0 + rng.uniform(-0.1, 1.1) * ext_y)
            th = 0.0 if rng.uniform() < 0.6 else rng.uniform(0.15, 0.5) * size
            if rng.uniform() < 0.3:
                row.append(("circle", pose, rng.uniform(0.4, 1.0) * size, th))
            else:
                nv = int(rng.integers(3, cap + 1)) if nv_of is None else nv_of(b, k)
                row.append(("hull", pose, _hull(rng, nv, rng.uniform(0.5, 1.2) * size, rng.uniform(0.5, 1.2) * size), th))
        out.append(row)
    return out


def _three_bodies(rng, cam):
    """A tilted rect, a circle and an outlined pentagon that overlap, somewhere inside the view."""
    H, W, x0, y0, ppm, w = cam
    mx, my = x0 + W / ppm / 2, y0 + H / ppm / 2
    j = lambda s: rng.uniform(-s, s)
    return [("hull", (0.4 + j(0.3), mx - 3 + j(2), my + j(2)), _rect(11.0 + j(1), 6.0 + j(1)), 0.0),
            ("circle", (j(1), mx + 2 + j(2), my - 2 + j(2)), 4.5 + j(1), 0.0),
            ("hull", (j(1), mx + j(2), my + 3 + j(2)), _hull(rng, 5, 6.0 + j(1), 5.0 + j(1)), 1.3 + j(0.3))]


_CAM_SMALL = (19, 23, -3.3, 2.1, 0.75, 1.7)          # smaller than a tile and not a multiple of one; w is not one pixel
_CAM_TILES = (40, 70, 10.3, -7.7, 0.5, 2.0)          # several tiles both ways (tile: 16 x 64), w = one pixel


def _special(rng):
    """40 x 70: a body covering the image, one partly off it, one wholly off it, one at 1e15, a zero-radius circle, overlaps."""
    H, W, x0, y0, ppm, w = _CAM_TILES
    mx, my = x0 + W / ppm / 2, y0 + H / ppm / 2
    j = lambda s: rng.uniform(-s, s)
    return [("hull", (0.05 + j(0.02), mx + j(3), my + j(3)), _rect(420.0, 300.0), 0.0),                 # covers every pixel
            ("circle", (0.0, x0 + 2.0 + j(1), my + j(10)), 17.0 + j(2), 0.0),                             # partly off the left edge
            ("hull", (j(1), x0 + 400.0 + j(5), my + j(5)), _hull(rng, 7, 20.0, 15.0), 0.0),               # wholly off the image
            ("circle", (0.0, 1e15, my + j(3)), 25.0, 3.0),                                                # at 1e15
            ("circle", (0.0, mx + 20.3 + j(3), my - 10.7 + j(3)), 0.0, 0.0),                              # zero radius
            ("hull", (j(1), x0 + 15.0 + j(3), my + j(5)), _hull(rng, 5, 16.0, 13.0), 4.0 + j(1)),         # outlined, over the circle
            ("hull", (0.6 + j(0.2), mx + 25.0 + j(5), my + 8.0 + j(3)), _rect(50.0, 21.0), 5.0 + j(1)),   # outlined tilted rect
            ("hull", (j(1), mx + 30.0 + j(5), my + j(5)), _hull(rng, 12, 22.0, 17.0), 0.0)]               # 12 vertices at capacity 12


def _build(name):
    seed = {"three": 1, "one": 2, "special": 3, "nb33": 4, "nb64": 5, "grey": 6}[name]
    rng = np.random.default_rng(seed)
    B = 3
    if name == "three":          # 19 x 23, circle + rect + hull, filled and outlined, overlapping, C = 3
        return _assemble([_three_bodies(rng, _CAM_SMALL) for _ in range(B)], _CAM_SMALL, 3, seed, False, 8)
    if name == "one":            # one body, one channel
        return _assemble([[_three_bodies(rng, _CAM_SMALL)[b]] for b in range(B)], _CAM_SMALL, 1, seed, False, 8)
    if name == "special":        # per-scene colours, C = 4, capacity 12
        return _assemble([_special(rng) for _ in range(B)], _CAM_TILES, 4, seed, True, 12)
    if name == "nb33":           # more bodies than the small detection kernels take, capacity 12, several tiles
        return _assemble(_random_bodies(rng, B, 33, 12, _CAM_TILES, 14.0), _CAM_TILES, 3, seed, True, 12)
    if name == "nb64":           # the most bodies and the largest capacity, nverts from 3 up to 64 (at most 992 hull vertices)
        cam = (16, 16, 100.7, 50.3, 1.25, 1.1)
        nv_of = lambda b, k: (3, 4, 5, 6, 7, 11, 17, 64)[(k + b) % 8] if k % 8 else 3 + (k // 8)
        return _assemble(_random_bodies(rng, B, 64, 64, cam, 3.0, nv_of), cam, 3, seed, False, 64)
    raise KeyError(name)


CASE_NAMES = ("three", "one", "special", "nb33", "nb64")
_CACHE = {}


def case(name):
    """The inputs of case `name` (CPU tensors; treat them as read-only: they are shared)."""
    if name not in _CACHE:
        _CACHE[name] = _build(name)
    return _CACHE[name]


def leaves(c):
    """A copy of case `c` whose p, radius, verts_local and colors are fresh leaves that require grad."""
    out = dict(c)
    for k in ("p", "radius", "verts_local", "colors"):
        out[k] = c[k].clone().requires_grad_(True)
    return out


_REF = {}


def reference(name, seed=0):
    """Computed once per case and shared: image, ids, margin, a random float32 cotangent and autograd's gradients for it."""
    if name not in _REF:
        c = leaves(case(name))
        image, ids, margin = render_host(c)
        g = torch.randn(image.shape, generator=torch.Generator().manual_seed(100 + seed), dtype=torch.float32)
        grads = torch.autograd.grad(image, [c["p"], c["radius"], c["verts_local"], c["colors"]], g.to(F64))
        _REF[name] = dict(image=image.detach(), ids=ids, margin=margin, g_image=g,
                          grads=dict(zip(("p", "radius", "verts_local", "colors"), grads)))
    return _REF[name]
