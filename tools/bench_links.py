"""Time the mechanism links (lcp_links.hip through `physics.links.LinkSet.jacobian`, `link_jacobian` and `ContactWorld(links=...)`)
against the route a user would have without them: the same rule (include/lcp_hip.h, "mechanism links") as vectorised torch operations on
the same device - gathers of the two ends, the closed forms over [scenes, links], one scatter into the matrix - with torch's autograd as
their backward.

    python tools/bench_links.py [--out profiles/links.json] [--parent-root DIR]     # needs the GPU
    python tools/bench_links.py --resources-only [--out ...]      # no GPU: (re)fill the kernels' register / scratch / LDS use from
                                                                  # lcp_physics_amd/csrc/asm/lcp_links.fixed.s

Entry: the forward launch and forward + backward (a random cotangent; gradients of p, a1, a2, phi) at 4096 scenes x 4 bodies x 4 links and
4096 x 48 bodies x 64 links, below three constant base rows.  World: a plain `step()` of 4096 scenes of a floor and four boxes with one
rod per box to a world point, against the same world without links.  Every measurement runs in FRESH processes, 5 of them per
measurement, the measurements alternating; inside a process the routes alternate too (7 repetitions by HIP events after a warm-up, a
repetition as many calls as take at least 50 ms).  Reported: the median of the 5 processes' medians, and the spread over all their
repetitions.  `--parent-root DIR` (a checkout of the parent commit with its library built): the four-box world WITHOUT links, stepped by
this tree and by the parent's in fresh processes that alternate - that path runs no new code, so the two must agree within the spread.
The drift of a rod's length over 30 steps of a swinging circle (the constraint is held at velocity level) is recorded as well.
None of the ratios is gated.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_force_elements as bfe  # noqa: E402  (the timing protocol and the four-box world, shared)

ASM = os.path.join(ROOT, "lcp_physics_amd", "csrc", "asm", "lcp_links.fixed.s")
F64, F32, I32 = torch.float64, torch.float32, torch.int32
ROUNDS = 5
E0 = 3


def row_plan(kind):
    """Scene 0's kinds -> the first row of every link and the row count."""
    rows, e = [], 0
    for k in kind[0].tolist():
        rows.append(e)
        e += {1: 1, 2: 1, 3: 2}.get(int(k), 0)
    return torch.tensor(rows, dtype=torch.long, device=kind.device), e


def torch_links(ln, p, base, plan):
    """The rule as batched torch operations (differentiable by autograd): the comparison partner.  `ln`: a dict of the link arrays
    (valid links only: kinds 1 to 3, indices in range, no rod of length 0); `plan`: `row_plan(ln["kind"])`."""
    B, nb = p.shape[:2]
    nz = 3 * nb
    row0, e = plan
    kind, b1, b2 = ln["kind"], ln["first"].long(), ln["second"].long()
    world = b2 < 0
    body2 = (~world).unsqueeze(-1)
    gat = lambda b: p.gather(1, b.clamp(min=0).unsqueeze(-1).expand(-1, -1, 3))
    rot = lambda th, a: torch.stack([torch.cos(th) * a[..., 0] - torch.sin(th) * a[..., 1],
                                     torch.sin(th) * a[..., 0] + torch.cos(th) * a[..., 1]], -1)
    cross = lambda a, b: a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    p1, p2 = gat(b1), gat(b2)
    r1 = rot(p1[..., 0], ln["a1"])
    w1 = p1[..., 1:] + r1
    rot2 = p2[..., 0] * (~world)
    r2 = rot(rot2, ln["a2"]) * body2
    w2 = torch.where(body2, p2[..., 1:] + r2, ln["a2"])
    d = w2 - w1
    n = d / d.norm(dim=-1, keepdim=True).clamp(min=1e-300)
    th = rot2 + ln["phi"]
    t = torch.stack([-torch.sin(th), torch.cos(th)], -1)
    u = r2 + (w1 - w2)
    rod = (kind == 1).unsqueeze(-1)
    e1 = torch.where(rod, torch.cat([-cross(r1, n).unsqueeze(-1), -n], -1), torch.cat([cross(r1, t).unsqueeze(-1), t], -1))
    e2 = torch.where(rod, torch.cat([cross(r2, n).unsqueeze(-1), n], -1), torch.cat([-cross(u, t).unsqueeze(-1), -t], -1))
    # one scatter: six entries of a link's first row, two of a slider's second; what the world would receive lands in three spare columns
    c1 = 3 * b1
    c2 = torch.where(world, torch.full_like(b2, nz), 3 * b2)
    q = torch.arange(3, device=p.device)
    base_idx = row0.unsqueeze(0).unsqueeze(-1) * (nz + 3)
    idx = torch.cat([base_idx + c1.unsqueeze(-1) + q, base_idx + c2.unsqueeze(-1) + q], -1)                  # [B,L,6]
    val = torch.cat([e1, e2], -1)
    slider = kind == 3
    idx2 = torch.stack([base_idx[..., 0] + (nz + 3) + c1, base_idx[..., 0] + (nz + 3) + c2], -1)             # [B,L,2]
    idx2 = torch.where(slider.unsqueeze(-1), idx2, torch.full_like(idx2, e * (nz + 3)))                      # (not a slider: a spare slot)
    val2 = torch.stack([torch.ones_like(th), -torch.ones_like(th)], -1) * slider.unsqueeze(-1)
    flat = torch.zeros(B, e * (nz + 3) + 1, dtype=F64, device=p.device)
    flat = flat.scatter(1, torch.cat([idx.reshape(B, -1), idx2.reshape(B, -1)], 1), torch.cat([val.reshape(B, -1), val2.reshape(B, -1)], 1))
    rows = flat[:, :-1].reshape(B, e, nz + 3)[:, :, :nz].to(F32)
    return rows if base is None else torch.cat([base, rows], 1)


def make_shape(B, nb, L, dev, seed=23):
    """Seeded links over `nb` bodies: rods, slots and sliders in equal parts, a quarter of their second ends on the world."""
    g = torch.Generator().manual_seed(seed)
    U = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g, dtype=F64)
    kind = (1 + torch.arange(L) % 3).to(I32).unsqueeze(0).expand(B, L).contiguous()
    first = torch.randint(0, nb, (B, L), generator=g)
    second = (first + 1 + torch.randint(0, nb - 1, (B, L), generator=g)) % nb
    second = torch.where(torch.rand(B, L, generator=g) < 0.25, torch.full_like(second, -1), second)
    ln = {"kind": kind, "first": first.to(I32), "second": second.to(I32), "a1": U(-1.5, 1.5, B, L, 2),
          "a2": torch.where((second >= 0).unsqueeze(-1), U(-1.5, 1.5, B, L, 2), U(-10.0, 10.0, B, L, 2)), "phi": U(-3.0, 3.0, B, L)}
    e = row_plan(kind)[1]
    base = torch.zeros(B, E0, 3 * nb, dtype=F32)
    base[:, :, :3] = torch.eye(3)
    st = {"p": torch.cat([U(-3.0, 3.0, B, nb, 1), U(-10.0, 10.0, B, nb, 2)], -1), "base": base,
          "g": torch.randn(B, E0 + e, 3 * nb, generator=g).to(F32)}
    mv = lambda d: {k: t.to(dev).contiguous() for k, t in d.items()}
    return mv(ln), mv(st), e


def measure_entry(B, nb, L, dev):
    from lcp_physics_amd.physics.links import LinkSet, link_jacobian
    ln, st, e = make_shape(B, nb, L, dev)
    plan = row_plan(ln["kind"])
    names = ("a1", "a2", "phi")
    leaves = {n: t.clone().requires_grad_(True) for n, t in [(n, ln[n]) for n in names] + [("p", st["p"])]}
    rest = torch.zeros(B, e, dtype=F64, device=dev)
    ls = LinkSet(**ln, rest=rest, e=e)
    lls = LinkSet(**dict(ln, **{n: leaves[n] for n in names}), rest=rest, e=e)
    lln = dict(ln, **{n: leaves[n] for n in names})
    out = torch.empty(B, E0 + e, 3 * nb, dtype=F32, device=dev)

    def k_fwd():
        return ls.jacobian(st["p"], Je_base=st["base"], out=out)

    def t_fwd():
        with torch.no_grad():
            return torch_links(ln, st["p"], st["base"], plan)

    def both(route):
        for x in leaves.values():
            x.grad = None
        Je = link_jacobian(lls, leaves["p"], Je_base=st["base"]) if route == "kernel" else torch_links(lln, leaves["p"], st["base"], plan)
        Je.backward(st["g"])

    # the two routes compute the same thing before anything is timed
    kf, tf = k_fwd().clone(), t_fwd().clone()
    f_err = float((kf - tf).abs().max() / tf.abs().max())
    assert f_err <= 1e-6, "the routes' matrices disagree: %g" % f_err
    both("kernel")
    kg = {n: x.grad.clone() for n, x in leaves.items()}
    both("torch")
    g_err = max(float((kg[n] - x.grad).abs().max() / x.grad.abs().max().clamp(min=1e-30)) for n, x in leaves.items())
    assert g_err <= 1e-9, "the routes' gradients disagree: %g" % g_err
    runs, calls = bfe.alternate({"kernel_forward": k_fwd, "torch_forward": t_fwd, "kernel_forward_backward": lambda: both("kernel"),
                                 "torch_forward_backward": lambda: both("torch")}, reps=7)
    return dict(B=B, nb=nb, L=L, rows=E0 + e, matrix_bytes=int(out.numel() * 4), matrices_agree_rel=f_err, gradients_agree_rel=g_err), runs, calls


def rod_world(B, dev, links):
    """4096 scenes of a floor and four boxes settling (the world of tools/bench_force_elements.py); `links`: every box on a rod from its
    centre to a world point 200 to its left - the stack settles along the rods' arcs as it does without them."""
    from lcp_physics_amd import scenes
    from lcp_physics_amd.physics import batched_world as bw
    from lcp_physics_amd.physics import contacts as ct
    w = scenes.make_drop_world(B, nbox=4)
    kw = {}
    if links:
        from lcp_physics_amd.physics.links import LinkSet
        anchor = lambda i: torch.stack([w["p"][:, i, 1] - 200.0, w["p"][:, i, 2]], -1)
        kw["links"] = LinkSet.from_list([("distance", i, None, (0.0, 0.0), anchor(i)) for i in range(1, 5)], w["p"]).to(dev)
    geom = ct.GeometryBatch.from_shapes(w["shapes"], B).to(dev)
    g = lambda k: w[k].to(dev)
    return bw.ContactWorld(geom, g("p"), g("v"), g("Mdiag"), g("f"), g("rest"), g("fric"), Je=g("Je"), maxc=16, **kw)


def measure_world(B, dev):
    worlds = {"links": rod_world(B, dev, True), "plain": rod_world(B, dev, False)}
    for _ in range(60):                                                                    # settle: the timed steps see resting stacks
        for w in worlds.values():
            w.step()
    torch.cuda.synchronize()
    ls = worlds["links"].links
    runs, calls = bfe.alternate({"step_" + r: w.step for r, w in worlds.items()}, reps=7)
    return dict(B=B, nb=5, L=4, rows=worlds["links"].e, settle_steps=60, rod_length_error_after_settling=float(ls.residual(worlds["links"].p).abs().max()),
                mean_contacts=float(worlds["links"].contacts.count.double().mean()),
                mean_contacts_plain=float(worlds["plain"].contacts.count.double().mean())), runs, calls


def rod_drift(dev, steps=30):
    """A circle of radius 10 and mass 1 on a rod of length 40 to a world point, released 0.5 rad from the vertical under gravity 100:
    the largest |length - 40| over `steps` plain steps of 1/30 (no `post_stab`), and the largest |Je v_new| after a solve."""
    from lcp_physics_amd.physics import batched_world as bw
    from lcp_physics_amd.physics import contacts as ct
    from lcp_physics_amd.physics.links import LinkSet
    pin = (300.0, 30.0)
    p0 = torch.tensor([[[0.0, pin[0] + 40.0 * math.sin(0.5), pin[1] + 40.0 * math.cos(0.5)]]], dtype=F64)
    ls = LinkSet.from_list([("distance", 0, None, (0.0, 0.0), pin)], p0).to(dev)
    t = lambda rows, dt_: torch.tensor(rows, dtype=dt_, device=dev)
    world = bw.ContactWorld(ct.GeometryBatch.from_shapes([("circle", 10.0)], 1).to(dev), p0.to(dev), t([[[0.0, 0.0, 0.0]]], F32),
                            t([[[50.0, 1.0, 1.0]]], F32), t([[[0.0, 0.0, 100.0]]], F32), t([[0.5]], F32), t([[0.5]], F32), links=ls, maxc=4)
    drift = resid = 0.0
    for _ in range(steps):
        Je = world.Je.clone()
        world.step()
        resid = max(resid, float((Je.double() @ world.v.double().reshape(1, -1, 1)).abs().max()))
        drift = max(drift, float(ls.residual(world.p).abs().max()))
    return {"steps": steps, "dt": world.dt, "length": 40.0, "largest_length_error": drift, "largest_Je_v_new": resid}


MEASUREMENTS = {"A_4096x4bodies_x4links": lambda B, dev: measure_entry(B, 4, 4, dev),
                "B_4096x48bodies_x64links": lambda B, dev: measure_entry(B, 48, 64, dev),
                "world_4boxes_4rods": measure_world}


def child(name, B):
    """One fresh process: one measurement, its routes alternating; the repetitions' median, least and largest per route."""
    facts, runs, calls = MEASUREMENTS[name](B, torch.device("cuda:0"))
    print("CHILD " + json.dumps({"facts": facts, "calls": calls, "runs": {k: list(v) for k, v in runs.items()}}))


def in_fresh_processes(B):
    rows = {name: [] for name in MEASUREMENTS}
    for _ in range(ROUNDS):
        for name in MEASUREMENTS:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--batch", str(B)], check=True,
                                 capture_output=True, text=True, timeout=300).stdout
            rows[name].append(json.loads([l for l in out.splitlines() if l.startswith("CHILD ")][-1][6:]))
            print("round %d: %s done" % (len(rows[name]), name), file=sys.stderr, flush=True)
    doc = {}
    for name, procs in rows.items():
        res = dict(procs[0]["facts"], processes=ROUNDS, repetitions_per_process=7, calls_per_repetition=procs[0]["calls"])
        for route in procs[0]["runs"]:
            res[route + "_us"] = round(float(np.median([p["runs"][route][0] for p in procs])) * 1e6, 2)
            res[route + "_spread_us"] = [round(min(p["runs"][route][1] for p in procs) * 1e6, 2),
                                         round(max(p["runs"][route][2] for p in procs) * 1e6, 2)]
        pairs = {"links_over_plain_step": ("step_links", "step_plain")} if name.startswith("world") else \
            {"kernel_over_torch_forward": ("kernel_forward", "torch_forward"),
             "kernel_over_torch_forward_backward": ("kernel_forward_backward", "torch_forward_backward")}
        for key, (a, b) in pairs.items():
            res[key] = round(res[a + "_us"] / res[b + "_us"], 5)
        if "matrix_bytes" in res:
            res["kernel_forward_store_GBps"] = round(res["matrix_bytes"] / res["kernel_forward_us"] * 1e-3, 1)
        doc[name] = res
    return doc


def kernel_resources():
    """Registers, scratch and static LDS of the two kernels of lcp_links.hip, from the metadata of the assembly the build left."""
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
        if "lcp_link_jacobian" in b.get("name", ""):
            out["backward" if "backward" in b["name"] else "forward"] = {k: int(b[k]) for k in keys if k in b}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "links.json"))
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.child:
        return child(a.child, a.batch)
    if a.resources_only:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    else:
        # the fresh processes first: this one has not opened the GPU yet
        doc = in_fresh_processes(a.batch)
        if a.parent_root:
            bfe.PLAIN_ROUNDS = ROUNDS
            doc["world_without_links_against_parent"] = bfe.plain_against_parent(a.parent_root, a.batch)
        assert torch.cuda.is_available(), "bench_links.py measures on the GPU; there is no CPU timing"
        doc["device"] = torch.cuda.get_device_name(0)
        doc["rod_drift"] = rod_drift(torch.device("cuda:0"))
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
