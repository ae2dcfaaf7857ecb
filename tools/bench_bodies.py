"""Time the body construction (lcp_bodies.hip through `physics.bodies.MassPropertiesFunction`) against the route the README
prescribed before it existed: the same formulas (bodies.py:125-126, 179-189, 216-226; forces.py:64-67) as vectorised torch
operations on the same device, with torch's autograd as their backward.  The torch composition exists here only as the
comparison partner.

    python tools/bench_bodies.py [--out profiles/bodies_properties.json]        # needs the GPU
    python tools/bench_bodies.py --resources-only [--out ...]                   # no GPU: (re)fill the kernels' register / scratch use
                                                                                # from lcp_physics_amd/csrc/asm/lcp_bodies.fixed.s

Shapes: 4096 scenes x 3 bodies (rect, circle, hull of 6) at capacity 8, and 4096 x 48 hulls of 16 vertices at capacity 16.
Forward and forward + backward (cotangents on all five outputs), HIP events around windows of at least 0.2 s after a spin-up, the
two routes alternating, the median of 7 windows and their spread.  Bytes: what the algorithm has to move - 16 B per vertex read
(nv of them) and written (cap of them) plus the per-body scalars - over the kernel route's time, as a fraction of 8 TB/s.
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
PEAK_BYTES_PER_S = 8.0e12
ASM = os.path.join(ROOT, "lcp_physics_amd", "csrc", "asm", "lcp_bodies.fixed.s")


def torch_body_properties(kind, radius, verts_raw, nverts, mass, g):
    """The formulas as batched torch operations (differentiable by autograd): the comparison partner."""
    cap = verts_raw.shape[2]
    ar = torch.arange(cap, device=verts_raw.device)
    live = (ar < nverts.unsqueeze(-1)) & (kind.unsqueeze(-1) != 0)                    # [B,nb,cap]
    nxt = torch.where(ar + 1 >= nverts.unsqueeze(-1), torch.zeros_like(ar), ar + 1).clamp(max=cap - 1)
    roll = lambda v: torch.gather(v, 2, nxt.unsqueeze(-1).expand_as(v))
    cross = lambda a, b: a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    z = torch.zeros((), dtype=verts_raw.dtype, device=verts_raw.device)
    v = torch.where(live.unsqueeze(-1), verts_raw, z)
    w = roll(v)
    x = torch.where(live, cross(w, v), z)
    hull = kind != 0
    den = torch.where(hull, (x / 2).sum(-1), torch.ones_like(radius))
    c = torch.where(hull.unsqueeze(-1), (1 / 6) * (x.unsqueeze(-1) * (v + w)).sum(2) / den.unsqueeze(-1), z)
    u = torch.where(live.unsqueeze(-1), v - c.unsqueeze(2), z)
    t = roll(u)
    nc = torch.where(live, cross(t, u).abs(), z)
    q = (u * u).sum(-1) + (u * t).sum(-1) + (t * t).sum(-1)
    dsum = torch.where(hull, nc.sum(-1), torch.ones_like(radius))
    inertia = torch.where(hull, 1 / 6 * mass * (nc * q).sum(-1) / dsum, mass * radius * radius / 2)
    Mdiag = torch.stack([inertia, mass, mass], dim=-1).to(torch.float32)
    zero = torch.zeros_like(mass)
    f = torch.stack([zero, zero, mass * g], dim=-1).to(torch.float32)
    return c, u, inertia, Mdiag, f


def make_shape(name, dev):
    rng = np.random.default_rng(5)
    if name == "4096x3_cap8":
        B, nb, cap = 4096, 3, 8
        nv = np.tile(np.array([4, 0, 6], np.int32), (B, 1))
    else:
        B, nb, cap = 4096, 48, 16
        nv = np.full((B, nb), 16, np.int32)
    kind = (nv > 0).astype(np.int32)
    a, b = rng.uniform(15, 35, (2, B, nb, 1))
    th = (np.arange(cap)[None, None] + rng.uniform(-0.3, 0.3, (B, nb, cap))) * (2 * math.pi / np.maximum(nv, 1)[..., None])
    verts = np.stack([a * np.cos(th), b * np.sin(th)], -1) + rng.uniform(-300, 300, (B, nb, 1, 2))
    verts *= (np.arange(cap)[None, None] < nv[..., None])[..., None]
    t = lambda x, dt_: torch.tensor(x, dtype=dt_, device=dev).contiguous()
    ins = dict(kind=t(kind, torch.int32), radius=t(rng.uniform(10, 35, (B, nb)), torch.float64), verts_raw=t(verts, torch.float64),
               nverts=t(nv, torch.int32), mass=t(rng.uniform(0.5, 5, (B, nb)), torch.float64))
    gen = torch.Generator(device="cpu").manual_seed(3)
    r = lambda *s, dt_=torch.float64: torch.randn(*s, generator=gen, dtype=dt_).to(dev)
    cots = (r(B, nb, 2), r(B, nb, cap, 2), r(B, nb), r(B, nb, 3, dt_=torch.float32), r(B, nb, 3, dt_=torch.float32))
    n_hull, n_body = int(kind.sum()), B * nb
    scal_in, scal_out = 4 + 4 + 8 + 8, 16 + 8 + 12 + 12 + 4
    fwd = 16 * int(nv.sum()) + 16 * cap * n_body + (scal_in + scal_out) * n_body
    bwd = 2 * 16 * int(nv.sum()) + 16 * cap * n_body + (scal_in + 16 + 8 + 12 + 12 + 8 + 8) * n_body
    return ins, cots, dict(B=B, nb=nb, cap=cap, hulls=n_hull, bytes_forward=fwd, bytes_forward_backward=fwd + bwd)


def window(fn, seconds=0.2):
    """Mean time of one call of `fn` over a window of at least `seconds`, by HIP events."""
    n = 4
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= seconds * 1e3:
            return ms * 1e-3 / n
        n = max(n * 2, int(n * seconds * 1.2e3 / max(ms, 1e-3)))


def measure(name, dev, g=100.0):
    from lcp_physics_amd.physics.bodies import MassPropertiesFunction
    ins, cots, info = make_shape(name, dev)
    leaves = [ins[k].clone().requires_grad_(True) for k in ("radius", "verts_raw", "mass")]

    def k_fwd():
        with torch.no_grad():
            return MassPropertiesFunction.apply(ins["radius"], ins["verts_raw"], ins["mass"], ins["kind"], ins["nverts"], g)

    def t_fwd():
        with torch.no_grad():
            return torch_body_properties(ins["kind"], ins["radius"], ins["verts_raw"], ins["nverts"], ins["mass"], g)

    def both(route):
        for x in leaves:
            x.grad = None
        if route == "kernel":
            outs = MassPropertiesFunction.apply(leaves[0], leaves[1], leaves[2], ins["kind"], ins["nverts"], g)
        else:
            outs = torch_body_properties(ins["kind"], leaves[0], leaves[1], ins["nverts"], leaves[2], g)
        torch.autograd.backward(outs, cots)
        return outs

    # the two routes compute the same thing (values and gradients) before anything is timed
    ko = both("kernel")
    kg = [x.grad.clone() for x in leaves]
    to = both("torch")
    tg = [x.grad.clone() for x in leaves]
    torch.cuda.synchronize()
    rel = lambda a, b: float((a.detach().double() - b.detach().double()).abs().max() / b.detach().double().abs().max().clamp(min=1.0))
    agree = max(rel(a, b) for a, b in list(zip(ko, to)) + list(zip(kg, tg)))
    assert agree < 1e-6, "the routes disagree: %g" % agree
    fns = {"kernel_forward": k_fwd, "torch_forward": t_fwd, "kernel_forward_backward": lambda: both("kernel"),
           "torch_forward_backward": lambda: both("torch")}
    for fn in fns.values():                                                             # spin-up: clocks, code objects, allocator
        window(fn, 0.3)
    runs = {k: [] for k in fns}
    for _ in range(7):                                                                  # alternating
        for k, fn in fns.items():
            runs[k].append(window(fn))
    res = dict(info, routes_agree_rel=agree)
    for k, v in runs.items():
        res[k + "_us"] = round(float(np.median(v)) * 1e6, 2)
        res[k + "_spread_us"] = [round(min(v) * 1e6, 2), round(max(v) * 1e6, 2)]
    res["forward_fraction_of_peak_bandwidth"] = round(info["bytes_forward"] / (res["kernel_forward_us"] * 1e-6) / PEAK_BYTES_PER_S, 4)
    res["forward_backward_fraction_of_peak_bandwidth"] = round(info["bytes_forward_backward"] / (res["kernel_forward_backward_us"] * 1e-6) / PEAK_BYTES_PER_S, 4)
    res["kernel_over_torch_forward"] = round(res["kernel_forward_us"] / res["torch_forward_us"], 4)
    res["kernel_over_torch_forward_backward"] = round(res["kernel_forward_backward_us"] / res["torch_forward_backward_us"], 4)
    return res


def kernel_resources():
    """Registers and scratch of every kernel of lcp_bodies.hip, from the metadata of the assembly the build left behind."""
    if not os.path.exists(ASM):
        return None
    out, name = {}, None
    for line in open(ASM):
        m = re.match(r"\s+\.(name|vgpr_count|sgpr_count|agpr_count|private_segment_fixed_size|vgpr_spill_count|group_segment_fixed_size):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "name":
            name = m.group(2)
            continue
        if name and "lcp_body_properties" in name:
            short = ("backward_" if "backward" in name else "forward_") + "L" + re.search(r"ILi(\d+)E", name).group(1)
            out.setdefault(short, {})[m.group(1)] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bodies_properties.json"))
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    if a.resources_only:
        doc = json.load(open(a.out))
    else:
        assert torch.cuda.is_available(), "bench_bodies.py measures on the GPU; there is no CPU timing"
        dev = torch.device("cuda:0")
        doc = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK_BYTES_PER_S,
               "shapes": {n: measure(n, dev) for n in ("4096x3_cap8", "4096x48x16_cap16")}}
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
