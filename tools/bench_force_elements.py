"""Time the force elements (lcp_forces.hip through `physics.force_elements.element_forces` and `ContactWorld(elements=...)`) against the
route a user had before they existed: the same rule (include/lcp_hip.h, "force elements") as vectorised torch operations on the same
device - gathers of the two ends, the spring / motor / drag formulas over [scenes, elements], `index_add` onto the bodies - with torch's
autograd as their backward, and in a world as a `force_fn` closure that reads `world.p` and `world.v`.

    python tools/bench_force_elements.py [--out profiles/force_elements.json] [--parent-root DIR]     # needs the GPU
    python tools/bench_force_elements.py --resources-only [--out ...]      # no GPU: (re)fill the kernels' register / scratch / LDS use
                                                                           # from lcp_physics_amd/csrc/asm/lcp_forces.fixed.s

Entry: forward and forward + backward (a random cotangent; gradients of p, v, k, c, x0, w0, a1, a2) at 4096 scenes x 4 bodies x 4
elements and 4096 scenes x 48 bodies x 256 elements.  World: one plain `step()` of 4096 scenes of a floor and four boxes with a world
spring on every box, through `elements=` and through the closure.  After a warm-up of every route, 21 timed repetitions per route by HIP
events, the routes alternating; a repetition is as many calls as take at least 50 ms; the median per call and the spread.
`--parent-root DIR` (a checkout of the parent commit with its library built): the same world WITHOUT elements, stepped by this tree and
by the parent's in fresh processes that alternate - the path runs no new code, so the two must agree within the spread.
"""
import argparse
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, "lcp_physics_amd", "csrc", "asm", "lcp_forces.fixed.s")
F64, F32, I32 = torch.float64, torch.float32, torch.int32
REPS = 21
PLAIN_ROUNDS = 3


def torch_forces(el, p, v, f_base):
    """The rule as batched torch operations (differentiable by autograd): the comparison partner.  `el`: a dict of the element arrays
    (valid elements only: kinds 1 to 3, indices in range, no spring of length 0)."""
    B, nb = p.shape[:2]
    kind, b1, b2 = el["kind"], el["b1"].long(), el["b2"].long()
    v = v.to(F64)

    def end(b, a):
        body = (b >= 0).unsqueeze(-1)
        idx = b.clamp(min=0).unsqueeze(-1).expand(-1, -1, 3)
        st, vel = p.gather(1, idx), v.gather(1, idx)
        cs, sn = torch.cos(st[..., 0]), torch.sin(st[..., 0])
        r = torch.stack([cs * a[..., 0] - sn * a[..., 1], sn * a[..., 0] + cs * a[..., 1]], -1) * body
        P = torch.where(body, st[..., 1:] + r, a)
        V = (vel[..., 1:] + vel[..., :1] * torch.stack([-r[..., 1], r[..., 0]], -1)) * body
        return r, P, V, st[..., 0] * body.squeeze(-1), vel[..., 0] * body.squeeze(-1)

    r1, P1, V1, rot1, w1 = end(b1, el["a1"])
    r2, P2, V2, rot2, w2 = end(b2, el["a2"])
    d = P2 - P1
    L = d.norm(dim=-1).clamp(min=1e-300)
    u = d / L.unsqueeze(-1)
    clamp = lambda raw: torch.where(raw.abs() >= el["limit"], (torch.sign(raw) * el["limit"].clamp(max=1e300)).detach(), raw)
    s = clamp(el["k"] * (L - el["x0"]) + el["c"] * (u * (V2 - V1)).sum(-1))
    F = s.unsqueeze(-1) * u
    tau = clamp(el["k"] * (el["x0"] - (rot2 - rot1)) + el["c"] * (el["w0"] - (w2 - w1)))
    cross = lambda a, b: a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    zero = torch.zeros_like(tau)
    vel1 = v.gather(1, b1.clamp(min=0).unsqueeze(-1).expand(-1, -1, 3))
    spring, motor, drag = ((kind == k).unsqueeze(-1) for k in (1, 2, 3))
    W1 = (spring * torch.cat([cross(r1, F).unsqueeze(-1), F], -1) + motor * torch.stack([-tau, zero, zero], -1)
          + drag * torch.stack([-el["c"] * vel1[..., 0], -el["k"] * vel1[..., 1], -el["k"] * vel1[..., 2]], -1))
    W2 = spring * torch.cat([cross(r2, -F).unsqueeze(-1), -F], -1) + motor * torch.stack([tau, zero, zero], -1)
    offs = (torch.arange(B, device=p.device) * nb).unsqueeze(1)
    out = torch.zeros(B * nb, 3, dtype=F64, device=p.device)
    out = out.index_add(0, (offs + b1.clamp(min=0)).reshape(-1), (W1 * (b1 >= 0).unsqueeze(-1)).reshape(-1, 3))
    out = out.index_add(0, (offs + b2.clamp(min=0)).reshape(-1), (W2 * ((b2 >= 0) & (kind != 3)).unsqueeze(-1)).reshape(-1, 3))
    return (f_base.to(F64) + out.reshape(B, nb, 3)).to(F32)


def make_shape(B, nb, E, dev, seed=11):
    """Seeded elements over `nb` bodies: springs (a quarter of their ends on the world), motors and drag in equal parts."""
    g = torch.Generator().manual_seed(seed)
    U = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g, dtype=F64)
    kind = (1 + torch.arange(E) % 3).to(I32).unsqueeze(0).expand(B, E).contiguous()
    i1 = torch.where(torch.rand(B, E, generator=g) < 0.25, torch.zeros(B, E, dtype=torch.long), 1 + torch.randint(0, nb, (B, E), generator=g))
    i2 = (i1 + 1 + torch.randint(0, nb, (B, E), generator=g)) % (nb + 1)
    b1 = torch.where(kind == 3, torch.randint(0, nb, (B, E), generator=g), i1 - 1).to(I32)
    b2 = (i2 - 1).to(I32)
    anchor = lambda b: torch.where((b >= 0).unsqueeze(-1), U(-1.5, 1.5, B, E, 2), U(-10.0, 10.0, B, E, 2))
    el = {"kind": kind, "b1": b1, "b2": b2, "a1": anchor(b1), "a2": anchor(b2), "k": U(5.0, 50.0, B, E), "c": U(0.1, 2.0, B, E),
          "x0": U(0.5, 3.0, B, E), "w0": U(-1.0, 1.0, B, E), "limit": torch.full((B, E), 1e4, dtype=F64)}
    st = {"p": torch.cat([U(-3.0, 3.0, B, nb, 1), U(-10.0, 10.0, B, nb, 2)], -1), "v": (2.0 * torch.randn(B, nb, 3, generator=g)).to(F32),
          "f_base": torch.randn(B, nb, 3, generator=g).to(F32), "g": torch.randn(B, nb, 3, generator=g).to(F32)}
    mv = lambda d: {k: t.to(dev).contiguous() for k, t in d.items()}
    return mv(el), mv(st)


def repetition(fn, n):
    """Mean time of one call of `fn` over `n` calls, by HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def alternate(fns, reps=REPS):
    """Warm every route up, then `reps` repetitions per route, the routes alternating: {route: (median, min, max)} seconds a call."""
    calls = {}
    for k, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[k] = max(1, int(math.ceil(0.05 / max(repetition(fn, 3), 1e-7))))
    runs = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            runs[k].append(repetition(fn, calls[k]))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in runs.items()}, calls


def _report(res, runs, calls, pairs):
    res["repetitions"], res["calls_per_repetition"] = REPS, calls
    for k, (med, lo, hi) in runs.items():
        res[k + "_us"] = round(med * 1e6, 2)
        res[k + "_spread_us"] = [round(lo * 1e6, 2), round(hi * 1e6, 2)]
    for name, (a, b) in pairs.items():
        res[name] = round(res[a + "_us"] / res[b + "_us"], 5)
    return res


def measure_entry(B, nb, E, dev):
    from lcp_physics_amd.physics.force_elements import ForceSet, element_forces
    el, st = make_shape(B, nb, E, dev)
    names = ("k", "c", "x0", "w0", "a1", "a2")
    leaves = {n: t.clone().requires_grad_(True) for n, t in list((n, el[n]) for n in names) + [("p", st["p"]), ("v", st["v"])]}
    fs = ForceSet(**el)
    lfs = ForceSet(**dict(el, **{n: leaves[n] for n in names}))
    lel = dict(el, **{n: leaves[n] for n in names})
    out = torch.empty(B, nb, 3, dtype=F32, device=dev)

    def k_fwd():
        return element_forces(fs, st["p"], st["v"], f_base=st["f_base"], out=out)

    def t_fwd():
        with torch.no_grad():
            return torch_forces(el, st["p"], st["v"], st["f_base"])

    def both(route):
        for x in leaves.values():
            x.grad = None
        f = element_forces(lfs, leaves["p"], leaves["v"], f_base=st["f_base"]) if route == "kernel" else \
            torch_forces(lel, leaves["p"], leaves["v"], st["f_base"])
        f.backward(st["g"])

    # the two routes compute the same thing before anything is timed
    kf, tf = k_fwd().clone(), t_fwd().clone()
    f_err = float((kf - tf).abs().max() / tf.abs().max())
    assert f_err <= 1e-6, "the routes' forces disagree: %g" % f_err
    both("kernel")
    kg = {n: x.grad.clone() for n, x in leaves.items()}
    both("torch")
    g_err = max(float((kg[n].double() - x.grad.double()).abs().max() / x.grad.double().abs().max().clamp(min=1e-30)) for n, x in leaves.items())
    assert g_err <= 1e-5, "the routes' gradients disagree: %g" % g_err
    runs, calls = alternate({"kernel_forward": k_fwd, "torch_forward": t_fwd, "kernel_forward_backward": lambda: both("kernel"),
                             "torch_forward_backward": lambda: both("torch")})
    res = dict(B=B, nb=nb, E=E, forces_agree_rel=f_err, gradients_agree_rel=g_err)
    return _report(res, runs, calls, {"kernel_over_torch_forward": ("kernel_forward", "torch_forward"),
                                      "kernel_over_torch_forward_backward": ("kernel_forward_backward", "torch_forward_backward")})


def box_world(B, dev, route):
    """4096 scenes of a floor and four boxes settling (scenes.make_drop_world) with a soft world spring on every box: `route` "kernel"
    (elements=), "closure" (force_fn over torch_forces) or "plain" (no elements at all)."""
    from lcp_physics_amd import scenes
    from lcp_physics_amd.physics import batched_world as bw
    from lcp_physics_amd.physics import contacts as ct
    w = scenes.make_drop_world(B, nbox=4)
    geom = ct.GeometryBatch.from_shapes(w["shapes"], B).to(dev)
    g = lambda k: w[k].to(dev)
    kw = {}
    if route != "plain":
        from lcp_physics_amd.physics.force_elements import ForceSet
        fs = ForceSet.from_list([("spring", -1, i, (500.0, 300.0 - 45.0 * i), (0.0, 0.0), {"k": 0.5, "c": 0.2, "rest": 20.0}) for i in range(1, 5)],
                                B).to(dev)
        if route == "kernel":
            kw["elements"] = fs
    world = bw.ContactWorld(geom, g("p"), g("v"), g("Mdiag"), g("f"), g("rest"), g("fric"), Je=g("Je"), maxc=16, **kw)
    if route == "closure":
        el = {n: getattr(fs, n) for n in ("kind", "b1", "b2", "a1", "a2", "k", "c", "x0", "w0", "limit")}
        world.force_fn = lambda t: torch_forces(el, world.p, world.v, world.f)
    return world


def measure_world(B, dev):
    worlds = {r: box_world(B, dev, r) for r in ("kernel", "closure", "plain")}
    for _ in range(60):                                                                    # settle: the timed steps see resting stacks
        for w in worlds.values():
            w.step()
    torch.cuda.synchronize()
    err = float((worlds["kernel"].p - worlds["closure"].p).abs().max())
    runs, calls = alternate({"step_" + r: w.step for r, w in worlds.items()})
    res = dict(B=B, nb=5, E=4, settle_steps=60, pose_difference_after_settling=err,
               mean_contacts=float(worlds["kernel"].contacts.count.double().mean()))
    return _report(res, runs, calls, {"kernel_over_closure_step": ("step_kernel", "step_closure"),
                                      "kernel_over_plain_step": ("step_kernel", "step_plain")})


def plain_child(B):
    """One process: the median time of a plain step of the box world WITHOUT elements, package imported from sys.path[0]."""
    dev = torch.device("cuda:0")
    w = box_world(B, dev, "plain")
    for _ in range(60):
        w.step()
    runs, calls = alternate({"step": w.step}, reps=7)
    med, lo, hi = runs["step"]
    print("PLAIN " + json.dumps({"us": round(med * 1e6, 2), "spread_us": [round(lo * 1e6, 2), round(hi * 1e6, 2)]}))


def plain_against_parent(parent_root, B):
    """This tree and the parent's, alternated in fresh processes (before this process opens the GPU)."""
    rows = {"this": [], "parent": []}
    for _ in range(PLAIN_ROUNDS):
        for who, root in (("this", ROOT), ("parent", os.path.abspath(parent_root))):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-child", "--root", root, "--batch", str(B)],
                                 check=True, capture_output=True, text=True, timeout=300).stdout
            rows[who].append(json.loads([l for l in out.splitlines() if l.startswith("PLAIN ")][-1][6:]))
    res = {"rounds": PLAIN_ROUNDS, "processes": rows}
    for who in rows:
        res[who + "_us"] = round(float(np.median([r["us"] for r in rows[who]])), 2)
        res[who + "_spread_us"] = [min(r["spread_us"][0] for r in rows[who]), max(r["spread_us"][1] for r in rows[who])]
    res["this_over_parent"] = round(res["this_us"] / res["parent_us"], 5)
    lo, hi = res["parent_spread_us"]
    res["within_parent_spread"] = bool(lo <= res["this_us"] <= hi)
    return res


def kernel_resources():
    """Registers, scratch and static LDS of the two kernels of lcp_forces.hip, from the metadata of the assembly the build left."""
    if not os.path.exists(ASM):
        return None
    keys = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
            "group_segment_fixed_size")
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
        if "lcp_force_elements" in b.get("name", ""):
            out["backward" if "backward" in b["name"] else "forward"] = {k: int(b[k]) for k in keys if k in b}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "force_elements.json"))
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--plain-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    if a.plain_child:
        return plain_child(a.batch)
    if a.resources_only:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    else:
        plain = plain_against_parent(a.parent_root, a.batch) if a.parent_root else None
        assert torch.cuda.is_available(), "bench_force_elements.py measures on the GPU; there is no CPU timing"
        dev = torch.device("cuda:0")
        doc = {"device": torch.cuda.get_device_name(0),
               "entry": {"A_4096x4bodies_x4elements": measure_entry(a.batch, 4, 4, dev),
                         "B_4096x48bodies_x256elements": measure_entry(a.batch, 48, 256, dev)},
               "world_4boxes_4springs": measure_world(a.batch, dev)}
        if plain is not None:
            doc["world_without_elements_against_parent"] = plain
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
