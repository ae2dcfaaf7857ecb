"""Time the point probes (lcp_points.hip through `physics.points.point_distances`) against the route a user had before they existed:
the same rule (include/lcp_hip.h, "point probes") as vectorised torch operations on the same device, with torch's autograd as their
backward.  The torch composition exists here only as the comparison partner; it is written the way a user would write it - one pass
per body over [scenes, points, vertices] tensors, the kind and vertex count of each body and the mounting body of each point known on
the host (no masks) - and runs over the scenes in chunks where the intermediates of the whole batch would not fit the device.

    python tools/bench_points.py [--out profiles/points.json]         # needs the GPU
    python tools/bench_points.py --resources-only [--out ...]         # no GPU: (re)fill the kernels' register / scratch / LDS use
                                                                      # from lcp_physics_amd/csrc/asm/lcp_points.fixed.s

Shapes: A - 4096 scenes x 8 bodies (an agent circle, a floor, three boxes, three circles) x 64 points, an 8 x 8 grid: the upper four
rows in the world frame over the scene, the lower four mounted on the agent around it, no cutoff; B - 4096 scenes x 48 bodies of
16-gons on a grid x 1024 points, a 32 x 32 world-frame grid over the scene with a cutoff of 25 (a quarter of the grid step: about
one point in seven is void); every pose jittered per scene, every point tests every body.  Forward (dist and body) and forward + backward (a random cotangent; gradients of pose, radii,
vertices and the points' coordinates).  After a warm-up of every route, 21 timed repetitions per route by HIP events, the routes
alternating; a repetition is as many calls as take at least 50 ms; the median per call and the spread.
"""
import argparse
import json
import math
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ASM = os.path.join(ROOT, "lcp_physics_amd", "csrc", "asm", "lcp_points.fixed.s")
F64 = torch.float64
INF = float("inf")
REPS = 21


def torch_probe(nvs, mount, radius, verts, p, xy, max_dist):
    """The rule as batched torch operations (differentiable by autograd): the comparison partner.  nvs[k]: the vertex count of body
    k (0: a circle); mount [N] long on the device: the mounting body of each point (-1: the world frame), the same in every scene."""
    B, N = max_dist.shape
    world = (mount < 0).unsqueeze(0)
    pm = p[:, mount.clamp(min=0)]                                                        # [B,N,3]
    zero = torch.zeros((), dtype=F64, device=p.device)
    rot, cx, cy = (torch.where(world, zero, pm[..., i]) for i in range(3))
    sn, cs = torch.sin(rot), torch.cos(rot)
    x, y = cx + (cs * xy[..., 0] - sn * xy[..., 1]), cy + (sn * xy[..., 0] + cs * xy[..., 1])
    best = torch.full((B, N), INF, dtype=F64, device=p.device)
    body = torch.full((B, N), -1, dtype=torch.int32, device=p.device)
    for k, nv in enumerate(nvs):
        if nv == 0:
            qx, qy = x - p[:, k, 1:2], y - p[:, k, 2:3]
            d = torch.sqrt(qx * qx + qy * qy) - radius[:, k:k + 1]
        else:
            sk, ck = torch.sin(p[:, k, 0:1]), torch.cos(p[:, k, 0:1])
            vx, vy = verts[:, k, :nv, 0], verts[:, k, :nv, 1]
            wx, wy = p[:, k, 1:2] + (ck * vx - sk * vy), p[:, k, 2:3] + (sk * vx + ck * vy)
            ex, ey = torch.roll(wx, -1, 1) - wx, torch.roll(wy, -1, 1) - wy
            L2 = ex * ex + ey * ey
            L = torch.sqrt(L2)
            e3 = lambda t: t.reshape(B, 1, nv)
            qx, qy = x.unsqueeze(-1) - e3(wx), y.unsqueeze(-1) - e3(wy)
            m = (e3(ey / L) * qx - e3(ex / L) * qy).max(-1).values
            tc = ((qx * e3(ex) + qy * e3(ey)) / e3(L2)).clamp(0.0, 1.0)
            rx, ry = qx - tc * e3(ex), qy - tc * e3(ey)
            inside = m <= 0
            d = torch.where(inside, m, torch.sqrt(torch.where(inside, 1.0, (rx * rx + ry * ry).min(-1).values)))
        d = torch.where((mount == k).unsqueeze(0), INF, d)
        closer = d < best
        best, body = torch.where(closer, d, best), torch.where(closer, k, body)
    live = best < max_dist
    return torch.where(live, best, max_dist), torch.where(live, body, -1)


def _rect(wd, ht):
    return [[wd / 2, ht / 2], [-wd / 2, ht / 2], [-wd / 2, -ht / 2], [wd / 2, -ht / 2]]          # bodies.py:260-262


def _ngon(n, r):
    return [[r * math.cos(2 * math.pi * i / n), r * math.sin(2 * math.pi * i / n)] for i in range(n)]


def _cells(extent, h, w):
    x0, y0, x1, y1 = extent
    return [(x0 + (j + 0.5) * (x1 - x0) / w, y0 + (i + 0.5) * (y1 - y0) / h) for i in range(h) for j in range(w)]


def layout(name):
    """(B, cap, bodies, points, torch-route chunk): bodies = [(kind, (rot, x, y), radius or vertices, pose jitter)], points =
    [(mounting body, (x, y), max_dist)]."""
    if name == "A_4096x8bodies_x64points":
        bodies = [("circle", (0.0, 480.0, 470.0), 10.0, (3.0, 5.0)), ("rect", (0.0, 484.0, 500.0), _rect(900.0, 10.0), (0.0, 1.0)),
                  ("rect", (0.2, 560.0, 478.0), _rect(30.0, 30.0), (0.3, 5.0)), ("rect", (-0.4, 400.0, 470.0), _rect(26.0, 42.0), (0.3, 5.0)),
                  ("rect", (0.1, 470.0, 380.0), _rect(80.0, 16.0), (0.3, 5.0)), ("circle", (0.0, 530.0, 420.0), 14.0, (0.0, 5.0)),
                  ("circle", (0.0, 420.0, 400.0), 18.0, (0.0, 5.0)), ("circle", (0.0, 620.0, 440.0), 25.0, (0.0, 5.0))]
        points = [(-1, xy, INF) for xy in _cells((360.0, 340.0, 680.0, 520.0), 4, 8)]
        points += [(0, xy, INF) for xy in _cells((-80.0, -40.0, 80.0, 40.0), 4, 8)]
        return 4096, 8, bodies, points, 4096
    bodies = [("hull", (0.0, 100.0 * (k % 8), 100.0 * (k // 8)), _ngon(16, 30.0), (3.0, 15.0)) for k in range(48)]
    return 4096, 16, bodies, [(-1, xy, 25.0) for xy in _cells((-50.0, -50.0, 750.0, 550.0), 32, 32)], 256


def make_shape(name, dev):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.points import PointSet
    B, cap, bodies, points, chunk = layout(name)
    nb, N = len(bodies), len(points)
    rng = np.random.default_rng(5)
    kind, nverts, radius = np.zeros((B, nb), np.int32), np.zeros((B, nb), np.int32), np.zeros((B, nb))
    verts, pose = np.zeros((B, nb, cap, 2)), np.zeros((B, nb, 3))
    for k, (what, ps, shape, (jr, jx)) in enumerate(bodies):
        pose[:, k] = np.asarray(ps) + rng.uniform(-1, 1, (B, 3)) * np.array([jr, jx, jx])
        if what == "circle":
            radius[:, k] = shape
        else:
            kind[:, k], nverts[:, k] = 1, len(shape)
            verts[:, k, :len(shape)] = np.asarray(shape)
    mount = [m for m, _, _ in points]
    t = lambda a, dt_: torch.tensor(np.asarray(a), dtype=dt_, device=dev).contiguous()
    rep = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64), (B,) + np.shape(a)).copy()
    geom = GeometryBatch(t(kind, torch.int32), t(radius, F64), t(verts, F64), t(nverts, torch.int32), None, int(nverts[0].sum()))
    xy = rep([list(q) for _, q, _ in points]) + rng.uniform(-1.0, 1.0, (B, N, 2))           # (off the lattice: no ties by symmetry)
    pts = PointSet(t(np.broadcast_to(np.asarray(mount, np.int32), (B, N)).copy(), torch.int32), t(xy, F64),
                   torch.full((B, N), -1, dtype=torch.int32, device=dev), t(rep([md for _, _, md in points]), F64))
    gen = torch.Generator(device="cpu").manual_seed(3)
    ins = dict(geom=geom, p=t(pose, F64), points=pts, nvs=[int(n) for n in nverts[0]], mount=t(mount, torch.int64), chunk=chunk,
               g=torch.randn(B, N, generator=gen, dtype=F64).to(dev))
    return ins, dict(B=B, nb=nb, cap=cap, N=N, scene_verts=int(nverts[0].sum()), torch_route_scenes_per_chunk=chunk)


def repetition(fn, n):
    """Mean time of one call of `fn` over `n` calls, by HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def measure(name, dev):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.points import PointSet, point_distances
    ins, info = make_shape(name, dev)
    geom, pts, B, chunk = ins["geom"], ins["points"], info["B"], ins["chunk"]
    leaves = [x.clone().requires_grad_(True) for x in (ins["p"], geom.radius, geom.verts_local, pts.xy)]
    lgeom = GeometryBatch(geom.kind, leaves[1], leaves[2], geom.nverts, None, geom.scene_verts_max)
    lpts = PointSet(pts.body, leaves[3], pts.target, pts.max_dist)
    dist_t = torch.empty(B, info["N"], dtype=F64, device=dev)
    body_t = torch.empty(B, info["N"], dtype=torch.int32, device=dev)

    def t_part(p, radius, verts, xy, s):
        return torch_probe(ins["nvs"], ins["mount"], radius[s], verts[s], p[s], xy[s], pts.max_dist[s])

    def k_fwd():
        with torch.no_grad():
            return point_distances(geom, ins["p"], pts)

    def t_fwd():
        with torch.no_grad():
            for lo in range(0, B, chunk):
                s = slice(lo, lo + chunk)
                dist_t[s], body_t[s] = t_part(ins["p"], geom.radius, geom.verts_local, pts.xy, s)
        return dist_t, body_t

    def both(route, g):
        for x in leaves:
            x.grad = None
        if route == "kernel":
            point_distances(lgeom, leaves[0], lpts)[0].backward(g)
        else:
            for lo in range(0, B, chunk):
                s = slice(lo, lo + chunk)
                t_part(*leaves, s)[0].backward(g[s])

    # the two routes compute the same thing before anything is timed: the distances and bodies, and the gradients for a cotangent
    # that is zero on the points the two routes decide differently (ties) or whose unit vector comes from a length below 1e-3
    kd, kb = (x.clone() for x in k_fwd())
    td, tb = (x.clone() for x in t_fwd())
    same = (kb == tb) & ((kd - td).abs() <= 1e-8)
    agree = float(same.double().mean())
    assert agree >= 0.999, "the routes disagree on %.4f of the points" % (1 - agree)
    g = torch.where(same & ((kd.abs() >= 1e-3) | (kb < 0)), ins["g"], torch.zeros_like(ins["g"]))
    both("kernel", g)
    grads = lambda: [torch.zeros_like(x) if x.grad is None else x.grad.clone() for x in leaves]      # (no circle: radius unused)
    kg = grads()
    both("torch", g)
    tg = grads()
    torch.cuda.synchronize()
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp(min=1.0))
    grads_rel = max(rel(x, y) for x, y in zip(kg, tg))
    assert grads_rel < 1e-6, "the routes' gradients disagree: %g" % grads_rel
    fns = {"kernel_forward": k_fwd, "torch_forward": t_fwd, "kernel_forward_backward": lambda: both("kernel", ins["g"]),
           "torch_forward_backward": lambda: both("torch", ins["g"])}
    calls = {}
    for k, fn in fns.items():                                                           # warm-up: clocks, code objects, allocator
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[k] = max(1, int(math.ceil(0.05 / max(repetition(fn, 3), 1e-7))))
    runs = {k: [] for k in fns}
    for _ in range(REPS):                                                               # alternating
        for k, fn in fns.items():
            runs[k].append(repetition(fn, calls[k]))
    res = dict(info, points_agreeing=agree, live_share=float((kb >= 0).double().mean()), gradients_agree_rel=grads_rel, repetitions=REPS,
               calls_per_repetition=calls)
    for k, v in runs.items():
        res[k + "_us"] = round(float(np.median(v)) * 1e6, 2)
        res[k + "_spread_us"] = [round(min(v) * 1e6, 2), round(max(v) * 1e6, 2)]
    res["kernel_over_torch_forward"] = round(res["kernel_forward_us"] / res["torch_forward_us"], 5)
    res["kernel_over_torch_forward_backward"] = round(res["kernel_forward_backward_us"] / res["torch_forward_backward_us"], 5)
    return res


def kernel_resources():
    """Registers, scratch and static LDS of the two kernels of lcp_points.hip, from the metadata of the assembly the build left."""
    if not os.path.exists(ASM):
        return None
    keys = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")
    blocks = []
    for line in open(ASM):
        m = re.match(r"  (- | {2})\.(\w+):\s+(\S+)", line)                # a kernel's metadata: "  - .first_key:" then "    .key:" lines
        if not m:
            continue
        if m.group(1) == "- ":
            blocks.append({})
        if blocks:
            blocks[-1][m.group(2)] = m.group(3)
    out = {}
    for b in blocks:
        if "lcp_point_distance" in b.get("name", ""):
            out["backward" if "backward" in b["name"] else "forward"] = {k: int(b[k]) for k in keys if k in b}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points.json"))
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    if a.resources_only:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    else:
        assert torch.cuda.is_available(), "bench_points.py measures on the GPU; there is no CPU timing"
        dev = torch.device("cuda:0")
        doc = {"device": torch.cuda.get_device_name(0),
               "shapes": {n: measure(n, dev) for n in ("A_4096x8bodies_x64points", "B_4096x48bodies16gons_x1024points")}}
    res = kernel_resources()
    if res is not None or "kernels" not in doc:
        doc["kernels"] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
