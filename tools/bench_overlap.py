"""Time the overlap queries (lcp_overlap.hip through `physics.overlap.pair_overlaps`) against the route a user had before they existed:
the same rule (include/lcp_hip.h, "overlap queries") as vectorised torch operations on the same device, with torch's autograd as their
backward.  The torch composition exists here only as the comparison partner; it is written the way a user would write it - one pass
per kind of pair (circle-circle, circle-hull, hull-hull) over [scenes, pairs, edges, half-planes] tensors, the kinds and the vertex
count known on the host (no masks for them), min and max for the clip parameters - and runs over the scenes in chunks where the
intermediates of the whole batch would not fit the device.  It evaluates every pair; it has no cull.

    python tools/bench_overlap.py [--out profiles/overlap.json]     # needs the GPU
    python tools/bench_overlap.py --resources-only [--out ...]      # no GPU: (re)fill the kernels' register / scratch / LDS use
                                                                    # from lcp_physics_amd/csrc/asm/lcp_overlap.fixed.s

Shapes, those of tools/bench_proximity.py: A - 4096 scenes x 8 bodies (four circles, a floor, three boxes) x all 28 pairs; B - 4096
scenes x 45 16-gons x all 990 pairs in a packed pile (five rows of nine in hexagonal packing), here with the neighbours a tenth of a
radius deep in each other flat to flat, so that clipping actually runs, every pose jittered per scene.  Forward (area) and forward +
backward (a random cotangent; gradients of pose, radii and vertices).  After a warm-up of every route, 5 timed repetitions per route
by HIP events, the routes alternating; a repetition is as many calls as take at least 50 ms; the median per call and the spread.  The
kernel route has to be the faster one at both shapes by more than the spread: its slowest repetition against torch's fastest.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_proximity as BP  # noqa: E402  (the shapes, the hull tables of the torch route, the timing of a repetition)

ASM = os.path.join(ROOT, "lcp_physics_amd", "csrc", "asm", "lcp_overlap.fixed.s")
F64 = torch.float64
INF = float("inf")
REPS = 5
DEPTH = 0.1 * BP.RAD              # how deep neighbours of the pile stand in each other


def _cross(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


TAU, EPS_H = 1e-12, 64 * 2.0 ** -52


def _pieces(E, G, first):
    """t1 - t0 of every edge of the hulls E clipped against the half-planes of the hulls G (0: out): [B,n,nvE].  first: E are the pairs'
    first bodies.  What two edges share (c, h, parallel or not, the crossing) is formed from body 1's edge and body 2's line in
    either role, as the header has it."""
    own = [t.unsqueeze(3) for t in E]                                                    # [B,n,nvE,1,..]
    oth = [t.unsqueeze(2) for t in G]                                                    # [B,n,1,nvG,..]
    (a1, e1, l1, _), (b2, e2, l2, n2) = (own, oth) if first else (oth, own)
    c = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
    q = a1 - b2
    h = n2[..., 0] * q[..., 0] + n2[..., 1] * q[..., 1]
    par = c * c <= (TAU * TAU) * (l1 * l2)
    same = (e1 * e2).sum(-1) > 0
    eps = EPS_H * (a1.abs().sum(-1) + b2.abs().sum(-1))
    tx = -h / torch.where(par, torch.ones_like(c), c / torch.sqrt(l2))
    if first:
        out, t, up, lo = par & ((h > eps) | ((h >= -eps) & ~same)), tx, ~par & (c > 0), ~par & (c < 0)
    else:
        out = par & torch.where(same, ~(h > eps), ~(h < -eps))
        t, up, lo = ((a1 + tx.unsqueeze(-1) * e1 - b2) * e2).sum(-1) / l2, ~par & (c < 0), ~par & (c > 0)
    t1 = torch.where(up, t, torch.full_like(t, INF)).min(-1).values.clamp(max=1.0)
    t0 = torch.where(lo, t, torch.full_like(t, -INF)).max(-1).values.clamp(min=0.0)
    gone = out.any(-1) | ((t0 > t1) if first else (t0 >= t1))
    return torch.where(gone, torch.zeros_like(t0), t1 - t0)


def torch_overlaps(nvs, groups, radius, verts, p, shape):
    """The rule as batched torch operations (differentiable by autograd): the comparison partner.  nvs[k]: the vertex count of body k
    (0: a circle; every hull of a shape has the same count); groups: {"cc" | "ch" | "hh": (columns, first, second)} long tensors on the
    device - for "ch" `first` is the circle whichever side of the pair it stands on."""
    area = torch.zeros(shape, dtype=F64, device=p.device)
    nv = max(nvs)
    zero = torch.zeros((), dtype=F64, device=p.device)
    if "cc" in groups:
        col, a, b = groups["cc"]
        q = p[:, b, 1:3] - p[:, a, 1:3]
        d2 = (q * q).sum(-1)
        d, r1, r2 = torch.sqrt(d2), radius[:, a], radius[:, b]
        lens = (d < r1 + r2) & (d > (r1 - r2).abs())
        ds = torch.where(lens, d, torch.sqrt(r1 * r1 + r2 * r2))                             # (keeps the unused branch's derivative finite)
        x1 = ((ds * ds + r1 * r1 - r2 * r2) / (2 * ds * r1)).clamp(-1.0, 1.0)
        x2 = ((ds * ds + r2 * r2 - r1 * r1) / (2 * ds * r2)).clamp(-1.0, 1.0)
        k = ((-ds + r1 + r2) * (ds + r1 - r2) * (ds - r1 + r2) * (ds + r1 + r2)).clamp(min=0.0)
        val = r1 * r1 * torch.acos(x1) + r2 * r2 * torch.acos(x2) - 0.5 * torch.sqrt(torch.where(lens, k, torch.ones_like(k)))
        rm = torch.where(r1 <= r2, r1, r2)
        area[:, col] = torch.where(lens, val, torch.where(d <= (r1 - r2).abs(), math.pi * rm * rm, zero))
    if "ch" in groups:
        col, a, b = groups["ch"]
        w, e, l2, n = BP._edges(p, verts, b, nv)
        c, r = p[:, a, 1:3].unsqueeze(2), radius[:, a].unsqueeze(-1)
        u, r2 = w - c, r * r
        bq, cq = (u * e).sum(-1), (u * u).sum(-1) - r2
        disc = bq * bq - l2 * cq
        cut = disc > 0
        sq = torch.sqrt(torch.where(cut, disc, torch.ones_like(disc)))
        ra, rb = (-bq - sq) / l2, (-bq + sq) / l2
        ta = torch.where(cut & (ra > 0) & (ra < 1), ra, torch.zeros_like(ra))
        tb = torch.where(cut & (rb > 0) & (rb < 1), rb, torch.ones_like(rb))
        total, within = torch.zeros_like(ta), torch.zeros_like(cut)
        for t0, t1 in ((torch.zeros_like(ta), ta), (ta, tb), (tb, torch.ones_like(tb))):
            live = t1 > t0
            m = u + (0.5 * (t0 + t1)).unsqueeze(-1) * e
            inside = live & ((m * m).sum(-1) <= r2)
            pp, q = u + t0.unsqueeze(-1) * e, u + t1.unsqueeze(-1) * e
            ang = torch.atan2(_cross(pp, q), (pp * q).sum(-1))
            total = total + torch.where(inside, 0.5 * (t1 - t0) * _cross(u, e), torch.where(live, 0.5 * r2 * ang, torch.zeros_like(ang)))
            within = within | inside
        centre_in = ((n * (c - w)).sum(-1) <= 0).all(-1)
        full = math.pi * radius[:, a] * radius[:, a]
        area[:, col] = torch.where(within.any(-1), total.sum(-1), torch.where(centre_in, full, zero))
    if "hh" in groups:
        col, a, b = groups["hh"]
        A, Bh = BP._edges(p, verts, a, nv), BP._edges(p, verts, b, nv)
        o = p[:, a, 1:3].unsqueeze(2)
        area[:, col] = 0.5 * ((_pieces(A, Bh, True) * _cross(A[0] - o, A[1])).sum(-1) + (_pieces(Bh, A, False) * _cross(Bh[0] - o, Bh[1])).sum(-1))
    return area.clamp(min=0.0)


def layout(name):
    """(B, cap, bodies, torch-route chunk): bodies = [(kind, (rot, x, y), radius or vertices, (rot jitter, xy jitter))]."""
    if name.startswith("A_"):
        B, cap, bodies, _, chunk = BP.layout(name)
        return B, cap, bodies, chunk
    pitch = 2 * BP.RAD * math.cos(math.pi / 16) - DEPTH                                  # flat to flat, less the penetration
    bodies = [("hull", (0.0, 100.0 + pitch * (k % 9) + 0.5 * pitch * ((k // 9) % 2), 100.0 + pitch * math.sqrt(0.75) * (k // 9)),
               BP._ngon(16, BP.RAD), (3.0, 0.15)) for k in range(45)]
    return 4096, 16, bodies, 64


def make_shape(name, dev):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.proximity import PairSet
    B, cap, bodies, chunk = layout(name)
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
    pairs = PairSet.all_pairs(nb, B).to(dev)
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
    return ins, dict(B=B, nb=nb, cap=cap, P=pairs.P, scene_verts=int(nverts[0].sum()), torch_route_scenes_per_chunk=chunk)


def measure(name, dev):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.overlap import pair_overlaps
    ins, info = make_shape(name, dev)
    geom, pairs, B, chunk = ins["geom"], ins["pairs"], info["B"], ins["chunk"]
    leaves = [x.clone().requires_grad_(True) for x in (ins["p"], geom.radius, geom.verts_local)]
    lgeom = GeometryBatch(geom.kind, leaves[1], leaves[2], geom.nverts, None, geom.scene_verts_max)
    area_t = torch.empty(B, info["P"], dtype=F64, device=dev)

    def t_part(p, radius, verts, s):
        return torch_overlaps(ins["nvs"], ins["groups"], radius[s], verts[s], p[s], (p[s].shape[0], info["P"]))

    def k_fwd():
        with torch.no_grad():
            return pair_overlaps(geom, ins["p"], pairs)

    def t_fwd():
        with torch.no_grad():
            for lo in range(0, B, chunk):
                s = slice(lo, lo + chunk)
                area_t[s] = t_part(ins["p"], geom.radius, geom.verts_local, s)
        return area_t

    def both(route, g):
        for x in leaves:
            x.grad = None
        if route == "kernel":
            pair_overlaps(lgeom, leaves[0], pairs).backward(g)
        else:
            for lo in range(0, B, chunk):
                s = slice(lo, lo + chunk)
                t_part(*leaves, s).backward(g[s])

    # the two routes compute the same thing before anything is timed: every area, and every gradient entry
    ka, ta = k_fwd().clone(), t_fwd().clone()
    area_err = float((ka - ta).abs().max())
    assert area_err <= 1e-8, "the routes' areas disagree: %g" % area_err
    both("kernel", ins["g"])
    grads = lambda: [torch.zeros_like(x) if x.grad is None else x.grad.clone() for x in leaves]      # (no circle: radius unused)
    kg = grads()
    both("torch", ins["g"])
    tg = grads()
    torch.cuda.synchronize()
    grad_err = max(float((x - y).abs().max() / y.abs().max().clamp(min=1.0)) for x, y in zip(kg, tg))
    assert grad_err <= 1e-6, "the routes' gradients disagree: %g relative" % grad_err
    fns = {"kernel_forward": k_fwd, "torch_forward": t_fwd, "kernel_forward_backward": lambda: both("kernel", ins["g"]),
           "torch_forward_backward": lambda: both("torch", ins["g"])}
    calls = {}
    for k, fn in fns.items():                                                           # warm-up: clocks, code objects, allocator
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        calls[k] = max(1, int(math.ceil(0.05 / max(BP.repetition(fn, 2), 1e-7))))
    runs = {k: [] for k in fns}
    for _ in range(REPS):                                                               # alternating
        for k, fn in fns.items():
            runs[k].append(BP.repetition(fn, calls[k]))
    res = dict(info, areas_agree_abs=area_err, gradients_agree_rel=grad_err, repetitions=REPS, calls_per_repetition=calls,
               pairs_overlapping=float((ka > 0).double().mean()), mean_area_of_overlapping_pairs=float(ka[ka > 0].mean()))
    for k, v in runs.items():
        res[k + "_us"] = round(float(np.median(v)) * 1e6, 2)
        res[k + "_spread_us"] = [round(min(v) * 1e6, 2), round(max(v) * 1e6, 2)]
    for what in ("forward", "forward_backward"):
        res["kernel_over_torch_" + what] = round(res["kernel_%s_us" % what] / res["torch_%s_us" % what], 5)
        res["kernel_faster_beyond_the_spread_" + what] = max(runs["kernel_" + what]) < min(runs["torch_" + what])
        assert res["kernel_faster_beyond_the_spread_" + what], (name, what, res)
    return res


def kernel_resources():
    """Registers, scratch and static LDS of the two kernels of lcp_overlap.hip, from the metadata of the assembly the build left."""
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
        if "lcp_pair_overlap" in b.get("name", ""):
            out["backward" if "backward" in b["name"] else "forward"] = {k: int(b[k]) for k in keys if k in b}
    return out


SHAPES = ("A_4096x8bodies_x28pairs", "B_4096x45bodies16gons_x990pairs_overlapping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap.json"))
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    if a.resources_only:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    else:
        assert torch.cuda.is_available(), "bench_overlap.py measures on the GPU; there is no CPU timing"
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
