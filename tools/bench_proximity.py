"""Time the proximity queries (lcp_proximity.hip through `physics.proximity.pair_distances`) against the route a user had before they
existed: the same rule (include/lcp_hip.h, "proximity queries") as vectorised torch operations on the same device, with torch's
autograd as their backward.  The torch composition exists here only as the comparison partner; it is written the way a user would
write it - one pass per kind of pair (circle-circle, circle-hull, hull-hull) over [scenes, pairs, edges, vertices] tensors, the kinds
and the vertex count known on the host (no masks), max and min for the selections - and runs over the scenes in chunks where the
intermediates of the whole batch would not fit the device.  It evaluates every pair and clamps afterwards; it has no cull.

    python tools/bench_proximity.py [--out profiles/proximity.json]     # needs the GPU
    python tools/bench_proximity.py --resources-only [--out ...]        # no GPU: (re)fill the kernels' register / scratch / LDS use
                                                                        # from lcp_physics_amd/csrc/asm/lcp_proximity.fixed.s

Shapes: A - 4096 scenes x 8 bodies (four circles, a floor, three boxes) x all 28 pairs, max_dist = inf; B - 4096 scenes x 45 16-gons
x all 990 pairs in a packed pile (five rows of nine in hexagonal packing, neighbours 1.0 apart flat to flat, every pose jittered per
scene: where two corners meet the neighbours overlap slightly, most are just apart), once with max_dist = inf and once with a cutoff of one body diameter.
Forward (dist) and forward + backward (a random cotangent; gradients of pose, radii and vertices).  After a warm-up of every route, 21
timed repetitions per route by HIP events, the routes alternating; a repetition is as many calls as take at least 50 ms; the median per
call and the spread.
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
ASM = os.path.join(ROOT, "lcp_physics_amd", "csrc", "asm", "lcp_proximity.fixed.s")
F64 = torch.float64
INF = float("inf")
REPS = 21


def _edges(p, verts, ks, nv):
    """World vertices, edges, |edge|^2 and outward normals of the hull bodies `ks` (a long tensor): each [B,len(ks),nv,(2)]."""
    rot, cx, cy = (p[:, ks, i].unsqueeze(-1) for i in range(3))
    sn, cs = torch.sin(rot), torch.cos(rot)
    vx, vy = verts[:, ks, :nv, 0], verts[:, ks, :nv, 1]
    w = torch.stack([cx + (cs * vx - sn * vy), cy + (sn * vx + cs * vy)], -1)
    e = torch.roll(w, -1, 2) - w
    l2 = (e * e).sum(-1)
    n = torch.stack([e[..., 1], -e[..., 0]], -1) / torch.sqrt(l2).unsqueeze(-1)
    return w, e, l2, n


def _points_edges(x, hull):
    """h and the squared segment distance of the points x [B,n,m,2] against every edge of `hull` ([B,n,nv,..]): each [B,n,nv,m]."""
    w, e, l2, n = hull
    q = x.unsqueeze(2) - w.unsqueeze(3)
    h = (n.unsqueeze(3) * q).sum(-1)
    tc = ((q * e.unsqueeze(3)).sum(-1) / l2.unsqueeze(3)).clamp(0.0, 1.0)
    r = q - tc.unsqueeze(-1) * e.unsqueeze(3)
    return h, (r * r).sum(-1)


def torch_pairs(nvs, groups, radius, verts, p, max_dist):
    """The rule as batched torch operations (differentiable by autograd): the comparison partner.  nvs[k]: the vertex count of body k
    (0: a circle; every hull of a shape has the same count); groups: {"cc" | "ch" | "hh": (columns, first, second)} long tensors on the
    device - for "ch" `first` is the circle whichever side of the pair it stands on."""
    dist = torch.empty_like(max_dist)
    nv = max(nvs)
    one = torch.ones((), dtype=F64, device=p.device)
    if "cc" in groups:
        col, a, b = groups["cc"]
        q = p[:, b, 1:3] - p[:, a, 1:3]
        dist[:, col] = torch.sqrt((q * q).sum(-1)) - radius[:, a] - radius[:, b]
    if "ch" in groups:
        col, a, b = groups["ch"]
        h, d2 = _points_edges(p[:, a, 1:3].unsqueeze(2), tuple(t for t in _edges(p, verts, b, nv)))
        m, d2m = h[..., 0].max(-1).values, d2[..., 0].min(-1).values
        dist[:, col] = torch.where(m <= 0, m, torch.sqrt(torch.where(m <= 0, one, d2m))) - radius[:, a]
    if "hh" in groups:
        col, a, b = groups["hh"]
        A, Bh = _edges(p, verts, a, nv), _edges(p, verts, b, nv)
        ha, d2a = _points_edges(Bh[0], A)
        hb, d2b = _points_edges(A[0], Bh)
        m = torch.maximum(ha.min(-1).values.max(-1).values, hb.min(-1).values.max(-1).values)
        d2m = torch.minimum(d2a.flatten(2).min(-1).values, d2b.flatten(2).min(-1).values)
        dist[:, col] = torch.where(m <= 0, m, torch.sqrt(torch.where(m <= 0, one, d2m)))
    return torch.where(dist < max_dist, dist, max_dist)


def _rect(wd, ht):
    return [[wd / 2, ht / 2], [-wd / 2, ht / 2], [-wd / 2, -ht / 2], [wd / 2, -ht / 2]]          # bodies.py:260-262


def _ngon(n, r):
    return [[r * math.cos(2 * math.pi * i / n), r * math.sin(2 * math.pi * i / n)] for i in range(n)]


RAD = 30.0                       # circumradius of the pile's 16-gons: one body diameter = 60


def layout(name):
    """(B, cap, bodies, max_dist, torch-route chunk): bodies = [(kind, (rot, x, y), radius or vertices, (rot jitter, xy jitter))]."""
    if name.startswith("A_"):
        bodies = [("circle", (0.0, 480.0, 470.0), 10.0, (3.0, 5.0)), ("rect", (0.0, 484.0, 500.0), _rect(900.0, 10.0), (0.0, 1.0)),
                  ("rect", (0.2, 560.0, 478.0), _rect(30.0, 30.0), (0.3, 5.0)), ("rect", (-0.4, 400.0, 470.0), _rect(26.0, 42.0), (0.3, 5.0)),
                  ("rect", (0.1, 470.0, 380.0), _rect(80.0, 16.0), (0.3, 5.0)), ("circle", (0.0, 530.0, 420.0), 14.0, (0.0, 5.0)),
                  ("circle", (0.0, 420.0, 400.0), 18.0, (0.0, 5.0)), ("circle", (0.0, 620.0, 440.0), 25.0, (0.0, 5.0))]
        return 4096, 8, bodies, INF, 4096
    pitch = 2 * RAD * math.cos(math.pi / 16) + 1.0                                       # flat to flat, plus a gap
    bodies = [("hull", (0.0, 100.0 + pitch * (k % 9) + 0.5 * pitch * ((k // 9) % 2), 100.0 + pitch * math.sqrt(0.75) * (k // 9)),
               _ngon(16, RAD), (3.0, 0.15)) for k in range(45)]
    return 4096, 16, bodies, (2 * RAD if name.endswith("cutoff") else INF), 64


def make_shape(name, dev):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.proximity import PairSet
    B, cap, bodies, max_dist, chunk = layout(name)
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
    t = lambda a, dt_: torch.tensor(np.asarray(a), dtype=dt_, device=dev).contiguous()
    geom = GeometryBatch(t(kind, torch.int32), t(radius, F64), t(verts, F64), t(nverts, torch.int32), None, int(nverts[0].sum()))
    pairs = PairSet.all_pairs(nb, B, max_dist=max_dist).to(dev)
    nvs = [int(n) for n in nverts[0]]
    groups = {}
    for col, (i, j) in enumerate(zip(pairs.first[0].tolist(), pairs.second[0].tolist())):
        key = "cc" if nvs[i] == 0 and nvs[j] == 0 else ("hh" if nvs[i] and nvs[j] else "ch")
        a, b = (j, i) if key == "ch" and nvs[i] else (i, j)
        for lst, v in zip(groups.setdefault(key, ([], [], [])), (col, a, b)):
            lst.append(v)
    groups = {k: tuple(torch.tensor(x, dtype=torch.int64, device=dev) for x in v) for k, v in groups.items()}
    gen = torch.Generator(device="cpu").manual_seed(3)
    ins = dict(geom=geom, p=t(pose, F64), pairs=pairs, nvs=nvs, groups=groups, chunk=chunk,
               g=torch.randn(B, pairs.P, generator=gen, dtype=F64).to(dev))
    return ins, dict(B=B, nb=nb, cap=cap, P=pairs.P, scene_verts=int(nverts[0].sum()), max_dist=max_dist if max_dist < INF else "inf",
                     torch_route_scenes_per_chunk=chunk)


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
    from lcp_physics_amd.physics.proximity import pair_distances
    ins, info = make_shape(name, dev)
    geom, pairs, B, chunk = ins["geom"], ins["pairs"], info["B"], ins["chunk"]
    leaves = [x.clone().requires_grad_(True) for x in (ins["p"], geom.radius, geom.verts_local)]
    lgeom = GeometryBatch(geom.kind, leaves[1], leaves[2], geom.nverts, None, geom.scene_verts_max)
    dist_t = torch.empty(B, info["P"], dtype=F64, device=dev)

    def t_part(p, radius, verts, s):
        return torch_pairs(ins["nvs"], ins["groups"], radius[s], verts[s], p[s], pairs.max_dist[s])

    def k_fwd():
        with torch.no_grad():
            return pair_distances(geom, ins["p"], pairs)

    def t_fwd():
        with torch.no_grad():
            for lo in range(0, B, chunk):
                s = slice(lo, lo + chunk)
                dist_t[s] = t_part(ins["p"], geom.radius, geom.verts_local, s)
        return dist_t

    def both(route, g):
        for x in leaves:
            x.grad = None
        if route == "kernel":
            pair_distances(lgeom, leaves[0], pairs).backward(g)
        else:
            for lo in range(0, B, chunk):
                s = slice(lo, lo + chunk)
                t_part(*leaves, s).backward(g[s])

    # the two routes compute the same thing before anything is timed: every distance, and the gradients (a pair whose two nearest
    # features tie within rounding may take either in either route, so a few entries may differ: their share is recorded)
    kd, td = k_fwd().clone(), t_fwd().clone()
    dist_err = float((kd - td).abs().max())
    assert dist_err <= 1e-8, "the routes' distances disagree: %g" % dist_err
    both("kernel", ins["g"])
    grads = lambda: [torch.zeros_like(x) if x.grad is None else x.grad.clone() for x in leaves]      # (no circle: radius unused)
    kg = grads()
    both("torch", ins["g"])
    tg = grads()
    torch.cuda.synchronize()
    same = [((x - y).abs() <= 1e-6 * y.abs().max().clamp(min=1.0)) for x, y in zip(kg, tg)]
    agree = float(sum(int(s.sum()) for s in same)) / sum(s.numel() for s in same)
    assert agree >= 0.999, "the routes' gradients disagree on %.4f of the entries" % (1 - agree)
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
    res = dict(info, distances_agree_abs=dist_err, gradient_entries_agreeing=agree, repetitions=REPS, calls_per_repetition=calls,
               pairs_below_max_dist=float((kd < pairs.max_dist).double().mean()), pairs_overlapping=float((kd < 0).double().mean()))
    for k, v in runs.items():
        res[k + "_us"] = round(float(np.median(v)) * 1e6, 2)
        res[k + "_spread_us"] = [round(min(v) * 1e6, 2), round(max(v) * 1e6, 2)]
    res["kernel_over_torch_forward"] = round(res["kernel_forward_us"] / res["torch_forward_us"], 5)
    res["kernel_over_torch_forward_backward"] = round(res["kernel_forward_backward_us"] / res["torch_forward_backward_us"], 5)
    return res


def kernel_resources():
    """Registers, scratch and static LDS of the two kernels of lcp_proximity.hip, from the metadata of the assembly the build left."""
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
        if "lcp_pair_distance" in b.get("name", ""):
            out["backward" if "backward" in b["name"] else "forward"] = {k: int(b[k]) for k in keys if k in b}
    return out


SHAPES = ("A_4096x8bodies_x28pairs", "B_4096x45bodies16gons_x990pairs", "B_4096x45bodies16gons_x990pairs_cutoff")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proximity.json"))
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    if a.resources_only:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    else:
        assert torch.cuda.is_available(), "bench_proximity.py measures on the GPU; there is no CPU timing"
        dev = torch.device("cuda:0")
        doc = {"device": torch.cuda.get_device_name(0), "shapes": {n: measure(n, dev) for n in SHAPES}}
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
