"""Time the contact report (lcp_report.hip through `physics.contact_report.contact_report` and `ContactWorld(report=...)`) against the
route a user would have without it: the same rule (include/lcp_hip.h, "contact reports") as torch operations on the same device -
the record's impulse over [scenes, records], `index_add_` onto bodies and pairs, a batched product for Je^T y.

    python tools/bench_contact_report.py [--out profiles/contact_report.json] [--parent-root DIR]     # needs the GPU
    python tools/bench_contact_report.py --resources-only [--out ...]      # no GPU: (re)fill the kernel's register / scratch / LDS use
                                                                           # from lcp_physics_amd/csrc/asm/lcp_report.fixed.s

Entry: the launch alone at 4096 scenes x 4 bodies x 16 contacts x 6 pairs and at 4096 x 48 bodies x 256 contacts x 990 pairs, against
the torch route (the two checked against each other first).  World: a plain `step()` of 4096 scenes of a floor and four boxes with and
without `report`.  After a warm-up of every route, 21 timed repetitions per route by HIP events, the routes alternating; a repetition is
as many calls as take at least 50 ms; the median per call and the spread.  `--parent-root DIR` (a checkout of the parent commit with its
library built): the same world without `report`, stepped by this tree and by the parent's in fresh processes that alternate.
None of the ratios is gated.
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_force_elements import _report, alternate  # noqa: E402  (the timing protocol, shared)

ASM = os.path.join(ROOT, "lcp_physics_amd", "csrc", "asm", "lcp_report.fixed.s")
F64, F32, I32 = torch.float64, torch.float32, torch.int32
PLAIN_ROUNDS = 3


def torch_report(c, nb, min_impulse=0.0):
    """The rule as batched torch operations: the comparison partner.  `c`: c_n, c_p1, c_p2, c_i1, c_i2, z, count, y, Je, first, second
    on the device, every index in range and first != second.  A pair is found through a [nb, nb] table of pair slots per scene."""
    B, maxc = c["c_i1"].shape
    P = c["first"].shape[1]
    dev = c["z"].device
    z = c["z"].to(F64)
    live = (torch.arange(maxc, device=dev).unsqueeze(0) < c["count"].unsqueeze(1)).to(F64)
    zn = z[:, :maxc] * live
    fr = z[:, maxc:3 * maxc].reshape(B, maxc, 2)
    zt = (fr[..., 0] - fr[..., 1]) * live
    n, p1, p2 = c["c_n"].to(F64), c["c_p1"].to(F64), c["c_p2"].to(F64)
    j = zn.unsqueeze(-1) * n + zt.unsqueeze(-1) * torch.stack([n[..., 1], -n[..., 0]], -1)
    cross = lambda a, b: a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    W1 = torch.cat([cross(p1, j).unsqueeze(-1), j], -1).reshape(-1, 3)
    W2 = torch.cat([-cross(p2, j).unsqueeze(-1), -j], -1).reshape(-1, 3)
    i1, i2 = c["c_i1"].long(), c["c_i2"].long()
    offs = (torch.arange(B, device=dev) * nb).unsqueeze(1)
    b1, b2 = (offs + i1).reshape(-1), (offs + i2).reshape(-1)
    pushing = ((zn > min_impulse) & (live > 0)).reshape(-1)
    body = torch.zeros(B * nb, 3, dtype=F64, device=dev).index_add_(0, b1, W1).index_add_(0, b2, W2)
    normal = torch.zeros(B * nb, dtype=F64, device=dev).index_add_(0, b1, zn.reshape(-1)).index_add_(0, b2, zn.reshape(-1))
    touching = torch.zeros(B * nb, dtype=I32, device=dev).index_add_(0, b1, pushing.to(I32)).index_add_(0, b2, pushing.to(I32))
    # the pair slot of (first, second) and of (second, first); P stands for "no such pair"
    slot = torch.full((B, nb * nb), P, dtype=torch.long, device=dev)
    q = torch.arange(P, device=dev).unsqueeze(0).expand(B, P)
    f, s = c["first"].long(), c["second"].long()
    fwd = slot.scatter(1, f * nb + s, q).gather(1, i1 * nb + i2)
    rev = slot.scatter(1, s * nb + f, q).gather(1, i1 * nb + i2)
    po = (torch.arange(B, device=dev) * (P + 1)).unsqueeze(1)
    pf, pr = (po + fwd).reshape(-1), (po + rev).reshape(-1)
    pair = torch.zeros(B * (P + 1), 3, dtype=F64, device=dev).index_add_(0, pf, W1).index_add_(0, pr, W2)
    pnormal = torch.zeros(B * (P + 1), dtype=F64, device=dev).index_add_(0, pf, zn.reshape(-1)).index_add_(0, pr, zn.reshape(-1))
    pcount = torch.zeros(B * (P + 1), dtype=I32, device=dev).index_add_(0, pf, pushing.to(I32)).index_add_(0, pr, pushing.to(I32))
    joint = torch.bmm(c["y"].to(F64).unsqueeze(1), c["Je"].to(F64)).reshape(B, nb, 3)
    return {"body_impulse": body.reshape(B, nb, 3).to(F32), "body_normal": normal.reshape(B, nb).to(F32),
            "body_touching": touching.reshape(B, nb), "joint_impulse": joint.to(F32),
            "pair_impulse": pair.reshape(B, P + 1, 3)[:, :P].to(F32), "pair_normal": pnormal.reshape(B, P + 1)[:, :P].to(F32),
            "pair_contacts": pcount.reshape(B, P + 1)[:, :P]}


def make_shape(B, nb, maxc, P, e, dev, seed=11):
    """Seeded records between different bodies, counts between maxc / 2 and maxc, the first P pairs i < j."""
    g = torch.Generator().manual_seed(seed)
    U = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g, dtype=F64)
    ang = U(0.0, 6.283185307179586, B, maxc)
    i1 = torch.randint(0, nb, (B, maxc), generator=g)
    i2 = (i1 + 1 + torch.randint(0, nb - 1, (B, maxc), generator=g)) % nb
    idx = [(i, j) for i in range(nb) for j in range(i + 1, nb)][:P]
    rep = lambda col: torch.tensor([p[col] for p in idx], dtype=I32).unsqueeze(0).expand(B, P).contiguous()
    c = {"c_n": torch.stack([torch.cos(ang), torch.sin(ang)], -1).to(F32), "c_p1": U(-2.0, 2.0, B, maxc, 2).to(F32),
         "c_p2": U(-2.0, 2.0, B, maxc, 2).to(F32), "c_i1": i1.to(I32), "c_i2": i2.to(I32),
         "z": torch.cat([U(0.0, 5.0, B, maxc), U(0.0, 2.0, B, 2 * maxc), U(0.0, 1.0, B, maxc)], 1).to(F32),
         "count": torch.randint(maxc // 2, maxc + 1, (B,), generator=g).to(I32), "y": torch.randn(B, e, generator=g).to(F32),
         "Je": torch.randn(B, e, 3 * nb, generator=g).to(F32), "first": rep(0), "second": rep(1)}
    return {k: t.to(dev).contiguous() for k, t in c.items()}


def measure_entry(B, nb, maxc, P, e, dev):
    from lcp_physics_amd.physics.contact_report import ContactReport, contact_report
    from lcp_physics_amd.physics.contacts import ContactBuffers
    from lcp_physics_amd.physics.proximity import PairSet
    c = make_shape(B, nb, maxc, P, e, dev)
    frame = ContactBuffers(B, nb, maxc, dev)
    for k in ("c_n", "c_p1", "c_p2", "c_i1", "c_i2"):
        getattr(frame, k).copy_(c[k])
    pairs = PairSet(c["first"], c["second"], torch.ones(B, P, dtype=F64, device=dev))
    out = ContactReport.zeros(B, nb, P, dev)

    def kernel():
        return contact_report(frame, c["z"], count=c["count"], y=c["y"], Je=c["Je"], pairs=pairs, out=out)

    def torch_route():
        return torch_report(c, nb)

    kr, tr = kernel(), torch_route()
    agree = {}
    for n, t in tr.items():                                                                # the routes compute the same thing
        a = getattr(kr, n)
        if a.dtype == I32:
            assert torch.equal(a, t), n
        else:
            agree[n] = float((a.double() - t.double()).abs().max() / t.double().abs().max().clamp(min=1e-30))
            assert agree[n] <= 1e-5, (n, agree[n])
    runs, calls = alternate({"kernel": kernel, "torch": torch_route})
    res = dict(B=B, nb=nb, maxc=maxc, P=P, e=e, routes_agree_rel=agree)
    return _report(res, runs, calls, {"kernel_over_torch": ("kernel", "torch")})


def box_world(B, dev, report):
    """4096 scenes of a floor and four boxes settling (scenes.make_drop_world); `report`: None, True or "pairs" (all 10 pairs)."""
    from lcp_physics_amd import scenes
    from lcp_physics_amd.physics import batched_world as bw
    from lcp_physics_amd.physics import contacts as ct
    w = scenes.make_drop_world(B, nbox=4)
    geom = ct.GeometryBatch.from_shapes(w["shapes"], B).to(dev)
    g = lambda k: w[k].to(dev)
    kw = {}
    if report == "pairs":
        from lcp_physics_amd.physics.proximity import PairSet
        kw["report"] = PairSet.all_pairs(5, B).to(dev)
    elif report:
        kw["report"] = True
    return bw.ContactWorld(geom, g("p"), g("v"), g("Mdiag"), g("f"), g("rest"), g("fric"), Je=g("Je"), maxc=16, **kw)


def measure_world(B, dev):
    worlds = {"plain": box_world(B, dev, None), "report": box_world(B, dev, True), "report_pairs": box_world(B, dev, "pairs")}
    for _ in range(60):                                                                    # settle: the timed steps see resting stacks
        for w in worlds.values():
            w.step()
    torch.cuda.synchronize()
    same = bool(torch.equal(worlds["plain"].p, worlds["report"].p))
    runs, calls = alternate({"step_" + r: w.step for r, w in worlds.items()})
    res = dict(B=B, nb=5, maxc=16, settle_steps=60, same_pose_bits_with_and_without_report=same,
               mean_contacts=float(worlds["report"].contacts.count.double().mean()))
    return _report(res, runs, calls, {"report_over_plain_step": ("step_report", "step_plain"),
                                      "report_pairs_over_plain_step": ("step_report_pairs", "step_plain")})


def plain_child(B):
    """One process: the median time of a plain step of the box world WITHOUT a report, package imported from sys.path[0]."""
    w = box_world(B, torch.device("cuda:0"), None)
    for _ in range(60):
        w.step()
    runs, _ = alternate({"step": w.step}, reps=7)
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
    """Registers, scratch and static LDS of the kernel of lcp_report.hip, from the metadata of the assembly the build left."""
    if not os.path.exists(ASM):
        return None
    keys = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
            "group_segment_fixed_size")
    blocks = []
    for line in open(ASM):
        m = re.match(r"  (- | {2})\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "- ":
            blocks.append({})
        if blocks:
            blocks[-1][m.group(2)] = m.group(3)
    for b in blocks:
        if "lcp_contact_report" in b.get("name", ""):
            return {k: int(b[k]) for k in keys if k in b}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contact_report.json"))
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
        assert torch.cuda.is_available(), "bench_contact_report.py measures on the GPU; there is no CPU timing"
        dev = torch.device("cuda:0")
        doc = {"device": torch.cuda.get_device_name(0),
               "entry": {"A_4096x4bodies_x16contacts_x6pairs": measure_entry(a.batch, 4, 16, 6, 3, dev),
                         "B_4096x48bodies_x256contacts_x990pairs": measure_entry(a.batch, 48, 256, 990, 6, dev)},
               "world_4boxes": measure_world(a.batch, dev)}
        if plain is not None:
            doc["world_without_report_against_parent"] = plain
    res = kernel_resources()
    if res is not None or "kernel" not in doc:
        doc["kernel"] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
