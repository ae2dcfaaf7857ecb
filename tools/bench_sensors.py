"""Time the range sensors (lcp_sensors.hip through `physics.sensors.cast_rays`) against the route a user had before they existed: the
same formulas (include/lcp_hip.h, "range sensors") as vectorised torch operations on the same device, with torch's autograd as their
backward.  The torch composition exists here only as the comparison partner; it is written the way a user would write it - one pass
per body over [scenes, rays, vertices] tensors, the kind and vertex count of each body and the mounting body of each ray known on the
host (no masks) - and runs over the scenes in chunks where the intermediates of the whole batch would not fit the device.

    python tools/bench_sensors.py [--out profiles/sensors.json]       # needs the GPU
    python tools/bench_sensors.py --resources-only [--out ...]        # no GPU: (re)fill the kernels' register / scratch / LDS use
                                                                      # from lcp_physics_amd/csrc/asm/lcp_sensors.fixed.s

Shapes: A - 4096 scenes x 8 bodies (an agent circle, a floor, three boxes, three circles) x 64 rays, one fan on the agent;
B - 4096 scenes x 48 bodies of 16-gons on a grid x 256 rays, fans of 64 on three of the bodies and on the world frame; every pose
jittered per scene.  Forward (dist and hit) and forward + backward (a random cotangent; gradients of pose, radii, vertices, ray
origins and angles).  After a warm-up of every route, 21 timed repetitions per route by HIP events, the routes alternating; a
repetition is as many calls as take at least 50 ms; the median per call and the spread.
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
ASM = os.path.join(ROOT, "lcp_physics_amd", "csrc", "asm", "lcp_sensors.fixed.s")
F64 = torch.float64
INF = float("inf")
REPS = 21


def torch_cast(nvs, mount, radius, verts, p, origin, angle, rng):
    """The rule as batched torch operations (differentiable by autograd): the comparison partner.  nvs[k]: the vertex count of body
    k (0: a circle); mount [R] long on the device: the mounting body of each ray (-1: the world frame), the same in every scene."""
    B, R = angle.shape
    world = (mount < 0).unsqueeze(0)
    pm = p[:, mount.clamp(min=0)]                                                        # [B,R,3]
    zero = torch.zeros((), dtype=F64, device=p.device)
    rot, cx, cy = (torch.where(world, zero, pm[..., i]) for i in range(3))
    sn, cs = torch.sin(rot), torch.cos(rot)
    ox, oy = cx + (cs * origin[..., 0] - sn * origin[..., 1]), cy + (sn * origin[..., 0] + cs * origin[..., 1])
    ux, uy = torch.cos(rot + angle), torch.sin(rot + angle)
    best = torch.full((B, R), INF, dtype=F64, device=p.device)
    hit = torch.full((B, R), -1, dtype=torch.int32, device=p.device)
    for k, nv in enumerate(nvs):
        if nv == 0:
            r = radius[:, k:k + 1]
            qx, qy = ox - p[:, k, 1:2], oy - p[:, k, 2:3]
            b, cc = qx * ux + qy * uy, qx * qx + qy * qy - r * r
            disc = b * b - cc
            inside = cc <= 0
            miss = ~inside & ((b >= 0) | (disc < 0))
            s = torch.where(inside, zero, torch.where(miss, INF, -b - torch.sqrt(torch.where(inside | miss, 1.0, disc))))
        else:
            sk, ck = torch.sin(p[:, k, 0:1]), torch.cos(p[:, k, 0:1])
            vx, vy = verts[:, k, :nv, 0], verts[:, k, :nv, 1]
            wx, wy = p[:, k, 1:2] + (ck * vx - sk * vy), p[:, k, 2:3] + (sk * vx + ck * vy)
            ex, ey = torch.roll(wx, -1, 1) - wx, torch.roll(wy, -1, 1) - wy
            L = torch.sqrt(ex * ex + ey * ey)
            e3 = lambda t: t.reshape(B, 1, nv)
            nx, ny = e3(ey / L), e3(-ex / L)
            h = nx * (ox.unsqueeze(-1) - e3(wx)) + ny * (oy.unsqueeze(-1) - e3(wy))
            den = nx * ux.unsqueeze(-1) + ny * uy.unsqueeze(-1)
            cand = -h / torch.where(den == 0, 1.0, den)
            inside = (h <= 0).all(-1)
            miss = ((den == 0) & (h > 0)).any(-1)
            s_in = torch.where(den < 0, cand, -INF).max(-1).values
            s_out = torch.where(den > 0, cand, INF).min(-1).values
            ok = ~inside & ~miss & (s_in >= 0) & (s_in <= s_out)
            s = torch.where(inside, zero, torch.where(ok, s_in, INF))
        s = torch.where((mount == k).unsqueeze(0), INF, s)
        closer = s < best
        best, hit = torch.where(closer, s, best), torch.where(closer, k, hit)
    struck = best < rng
    return torch.where(struck, best, rng), torch.where(struck, hit, -1)


def _rect(wd, ht):
    return [[wd / 2, ht / 2], [-wd / 2, ht / 2], [-wd / 2, -ht / 2], [wd / 2, -ht / 2]]          # bodies.py:260-262


def _ngon(n, r):
    return [[r * math.cos(2 * math.pi * i / n), r * math.sin(2 * math.pi * i / n)] for i in range(n)]


def layout(name):
    """(B, cap, bodies, fans, torch-route chunk): bodies = [(kind, (rot, x, y), radius or vertices, pose jitter)], fans =
    [(mounting body, rays, origin, range)]."""
    if name == "A_4096x8bodies_x64rays":
        bodies = [("circle", (0.0, 480.0, 470.0), 10.0, (3.0, 5.0)), ("rect", (0.0, 484.0, 500.0), _rect(900.0, 10.0), (0.0, 1.0)),
                  ("rect", (0.2, 560.0, 478.0), _rect(30.0, 30.0), (0.3, 5.0)), ("rect", (-0.4, 400.0, 470.0), _rect(26.0, 42.0), (0.3, 5.0)),
                  ("rect", (0.1, 470.0, 380.0), _rect(80.0, 16.0), (0.3, 5.0)), ("circle", (0.0, 530.0, 420.0), 14.0, (0.0, 5.0)),
                  ("circle", (0.0, 420.0, 400.0), 18.0, (0.0, 5.0)), ("circle", (0.0, 620.0, 440.0), 25.0, (0.0, 5.0))]
        return 4096, 8, bodies, [(0, 64, (0.0, 0.0), 300.0)], 4096
    bodies = [("hull", (0.0, 100.0 * (k % 8), 100.0 * (k // 8)), _ngon(16, 30.0), (3.0, 15.0)) for k in range(48)]
    fans = [(0, 64, (0.0, 0.0), 400.0), (21, 64, (3.0, -2.0), 400.0), (47, 64, (0.0, 0.0), 400.0), (-1, 64, (350.0, 250.0), 400.0)]
    return 4096, 16, bodies, fans, 512


def make_shape(name, dev):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.sensors import RaySet
    B, cap, bodies, fans, chunk = layout(name)
    nb = len(bodies)
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
    body, origin, angle, reach = [], [], [], []
    for m, n, org, far in fans:
        body += [m] * n
        origin += [list(org)] * n
        angle += [2 * math.pi * i / n for i in range(n)]
        reach += [far] * n
    R = len(body)
    t = lambda a, dt_: torch.tensor(np.asarray(a), dtype=dt_, device=dev).contiguous()
    rep = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64), (B,) + np.shape(a)).copy()
    geom = GeometryBatch(t(kind, torch.int32), t(radius, F64), t(verts, F64), t(nverts, torch.int32), None, int(nverts[0].sum()))
    rays = RaySet(t(np.broadcast_to(np.asarray(body, np.int32), (B, R)).copy(), torch.int32), t(rep(origin), F64),
                  t(rep(angle) + rng.uniform(-0.3, 0.3, (B, 1)), F64), t(rep(reach), F64))
    gen = torch.Generator(device="cpu").manual_seed(3)
    ins = dict(geom=geom, p=t(pose, F64), rays=rays, nvs=[int(n) for n in nverts[0]], mount=t(body, torch.int64), chunk=chunk,
               g=torch.randn(B, R, generator=gen, dtype=F64).to(dev))
    return ins, dict(B=B, nb=nb, cap=cap, R=R, scene_verts=int(nverts[0].sum()), torch_route_scenes_per_chunk=chunk)


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
    from lcp_physics_amd.physics.sensors import RaySet, cast_rays
    ins, info = make_shape(name, dev)
    geom, rays, B, chunk = ins["geom"], ins["rays"], info["B"], ins["chunk"]
    leaves = [x.clone().requires_grad_(True) for x in (ins["p"], geom.radius, geom.verts_local, rays.origin, rays.angle)]
    lgeom = GeometryBatch(geom.kind, leaves[1], leaves[2], geom.nverts, None, geom.scene_verts_max)
    lrays = RaySet(rays.body, leaves[3], leaves[4], rays.range)
    dist_t = torch.empty(B, info["R"], dtype=F64, device=dev)
    hit_t = torch.empty(B, info["R"], dtype=torch.int32, device=dev)

    def t_part(p, radius, verts, origin, angle, s):
        return torch_cast(ins["nvs"], ins["mount"], radius[s], verts[s], p[s], origin[s], angle[s], rays.range[s])

    def k_fwd():
        with torch.no_grad():
            return cast_rays(geom, ins["p"], rays)

    def t_fwd():
        with torch.no_grad():
            for lo in range(0, B, chunk):
                s = slice(lo, lo + chunk)
                dist_t[s], hit_t[s] = t_part(ins["p"], geom.radius, geom.verts_local, rays.origin, rays.angle, s)
        return dist_t, hit_t

    def both(route, g):
        for x in leaves:
            x.grad = None
        if route == "kernel":
            cast_rays(lgeom, leaves[0], lrays)[0].backward(g)
        else:
            for lo in range(0, B, chunk):
                s = slice(lo, lo + chunk)
                t_part(*leaves, s)[0].backward(g[s])

    # the two routes compute the same thing before anything is timed: the readings, and the gradients for a cotangent that is zero
    # on the rays whose hit the two routes decide differently (ties) or that graze their surface
    kd, kh = (x.clone() for x in k_fwd())
    td, th = (x.clone() for x in t_fwd())
    same = (kh == th) & ((kd - td).abs() <= 1e-8)
    agree = float(same.double().mean())
    assert agree >= 0.999, "the routes disagree on %.4f of the rays" % (1 - agree)
    _, _, normal = cast_rays(geom, ins["p"], rays, normals=True)
    a = rays.angle + torch.where(rays.body < 0, torch.zeros_like(rays.angle),
                                 torch.gather(ins["p"][..., 0], 1, rays.body.clamp(min=0).long()))
    nu = (normal[..., 0] * torch.cos(a) + normal[..., 1] * torch.sin(a)).abs()
    g = torch.where(same & ((nu >= 0.05) | (kh < 0)), ins["g"], torch.zeros_like(ins["g"]))
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
    res = dict(info, rays_agreeing=agree, gradients_agree_rel=grads_rel, repetitions=REPS, calls_per_repetition=calls)
    for k, v in runs.items():
        res[k + "_us"] = round(float(np.median(v)) * 1e6, 2)
        res[k + "_spread_us"] = [round(min(v) * 1e6, 2), round(max(v) * 1e6, 2)]
    res["kernel_over_torch_forward"] = round(res["kernel_forward_us"] / res["torch_forward_us"], 5)
    res["kernel_over_torch_forward_backward"] = round(res["kernel_forward_backward_us"] / res["torch_forward_backward_us"], 5)
    return res


def kernel_resources():
    """Registers, scratch and static LDS of the two kernels of lcp_sensors.hip, from the metadata of the assembly the build left."""
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
        if "lcp_cast_rays" in b.get("name", ""):
            out["backward" if "backward" in b["name"] else "forward"] = {k: int(b[k]) for k in keys if k in b}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensors.json"))
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    if a.resources_only:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    else:
        assert torch.cuda.is_available(), "bench_sensors.py measures on the GPU; there is no CPU timing"
        dev = torch.device("cuda:0")
        doc = {"device": torch.cuda.get_device_name(0),
               "shapes": {n: measure(n, dev) for n in ("A_4096x8bodies_x64rays", "B_4096x48bodies16gons_x256rays")}}
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
