"""Detection with and without the broadphase (the detection kernel of lcp_contacts_wide.hip with the cull of lcp_contacts_bp.hip
against the all-pairs kernels) on one GPU: `--batch` scenes of a floor and nb - 1 circles, rects and n-gons in columns of 8 (the piles of tools/bench_wide_contacts.py; 16 seeded scenes tiled over
the batch), for nb = 12 and 20 (8-gons at capacity 8: the all-pairs side is lcp_contacts.hip, the kernel those sizes run on by
default) and nb = 48 (16-gons at capacity 16: lcp_contacts_wide.hip, the shape of profiles/r07_wide_contacts.json).  Two launches
are timed per size:

    find      `find_contacts` at the settled pose (one trial)
    halving   `move_and_find_contacts` replayed from the step of the settling run with the most trials per scene (pose before the step,
              velocities after its solve): the move / detect / halve loop as a forming pile runs it

`broadphase=False` against `True` in this process: both warmed, then alternated `--reps` times; each measurement is HIP events around
enough back-to-back launches to fill `--window` seconds (well over 0.1 s), reported as ms per launch with the median, min, max and spread
per side.  Also: candidates per scene (mean, max), mean trials, and whether every output of the two sides compared bitwise equal.
Writes one JSON file and prints it.

    python tools/bench_broadphase.py [--batch 4096] [--reps 3] [--window 0.25] [--out profiles/broadphase.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_wide_contacts import pile_scene  # noqa: E402

FIELDS = ("c_n", "c_p1", "c_p2", "c_pen", "c_i1", "c_i2", "count", "p_out", "dt_used", "trials", "max_pen")
NSEED = 16


def pile_world(B, nb, nv, maxc, dev):
    """ContactWorld (all-pairs detection) of NSEED seeded piles tiled over B scenes."""
    from lcp_physics_amd.physics import batched_world as bw
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.scenes import GRAVITY
    assert B % NSEED == 0
    per = {k: [] for k in ("kind", "radius", "verts_local", "nverts", "pose", "Mdiag")}
    cap = max(8, nv)
    for s in range(NSEED):
        shapes, pose = pile_scene(np.random.default_rng(1000 * nb + s), nb, nv=nv)
        g = GeometryBatch.from_shapes(shapes, 1, max_verts=cap)
        Mdiag = np.ones((nb, 3))
        for i, (k, a) in enumerate(shapes[1:], 1):
            Mdiag[i, 0] = 0.5 * a ** 2 if k == "circle" else ((a[0] ** 2 + a[1] ** 2) / 12.0 if k == "rect" else 0.5 * float((np.asarray(a) ** 2).sum(1).mean()))
        for k in ("kind", "radius", "verts_local", "nverts"):
            per[k].append(getattr(g, k))
        per["pose"].append(torch.tensor(pose[None], dtype=torch.float64))
        per["Mdiag"].append(torch.tensor(Mdiag[None], dtype=torch.float32))
    tile = lambda k: torch.cat(per[k]).repeat(B // NSEED, *([1] * (per[k][0].dim() - 1))).contiguous().to(dev)
    geom = GeometryBatch(tile("kind"), tile("radius"), tile("verts_local"), tile("nverts"), None, None)
    f = torch.zeros(B, nb, 3, dtype=torch.float32, device=dev)
    f[:, 1:, 2] = GRAVITY
    Je = torch.zeros(B, 3, 3 * nb, dtype=torch.float32, device=dev)
    Je[:, :, :3] = torch.eye(3, device=dev)
    pose = tile("pose")
    return bw.ContactWorld(geom, pose, torch.zeros(B, nb, 3, device=dev), tile("Mdiag"), f, torch.full((B, nb), 0.3, device=dev),
                           torch.full((B, nb), 0.5, device=dev), Je=Je, maxc=maxc)


def ms_per_launch(fn, n):
    """HIP events around n back-to-back launches."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def ab(fn_off, fn_on, reps, window):
    """Both sides warmed, the launch count sized so that the faster side fills the window, then alternated."""
    for fn in (fn_off, fn_on):
        ms_per_launch(fn, 3)
    single = min(ms_per_launch(fn_off, 5), ms_per_launch(fn_on, 5))
    n = max(10, int(np.ceil(window * 1e3 / single)))
    off, on = [], []
    for _ in range(reps):
        off.append(ms_per_launch(fn_off, n))
        on.append(ms_per_launch(fn_on, n))
    stat = lambda v: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "spread": max(v) - min(v)}
    return {"launches_per_measurement": n, "all_pairs_ms": stat(off), "broadphase_ms": stat(on),
            "all_pairs_over_broadphase": sorted(off)[len(off) // 2] / sorted(on)[len(on) // 2]}


def equal(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in FIELDS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--sizes", default="12:8:64,20:8:96,48:16:128", help="nb:vertices of the n-gons:maxc, comma separated")
    ap.add_argument("--settle", type=int, default=40, help="untimed steps: the piles form and settle")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of launches per measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "broadphase.json"))
    args = ap.parse_args()
    from lcp_physics_amd.physics import contacts as ct
    from lcp_physics_amd.srchash import source_sha256
    dev = torch.device("cuda")
    B = args.batch
    res = {"tool": "bench_broadphase", "batch": B, "gpu": torch.cuda.get_device_name(0), "source_sha256": source_sha256(),
           "clock": "HIP events around back-to-back launches filling %.2f s; both sides warmed, then alternated %d times" % (args.window, args.reps),
           "sizes": []}
    for spec in args.sizes.split(","):
        nb, nv, maxc = (int(x) for x in spec.split(":"))
        world = pile_world(B, nb, nv, maxc, dev)
        geom = world.geom
        worst = (-1.0, None, None)
        for _ in range(args.settle):
            p_before = world.p.clone()
            world.step()
            tr = float(world.contacts.trials.float().mean())
            if tr > worst[0]:
                worst = (tr, p_before, world.v.clone())
        world.check_capacity()
        p = world.p.clone()
        cand = torch.zeros(B, dtype=torch.int32, device=dev)
        row = {"nb": nb, "pairs": nb * (nb - 1) // 2, "ngon_vertices": nv, "nvcap": geom.nvcap, "maxc": maxc, "scene_verts_max": geom.verts_max(),
               "all_pairs_kernel": "lcp_contacts_wide.hip" if geom.wide else "lcp_contacts.hip", "settle_steps": args.settle}
        # find_contacts at the settled pose
        a, b = ct.find_contacts(geom, p, maxc=maxc), ct.find_contacts(geom, p, maxc=maxc, broadphase=True, candidates=cand)
        torch.cuda.synchronize()
        find = {"outputs_equal": equal(a, b), "contacts_mean": float(a.count.float().mean()), "contacts_max": int(a.count.max()),
                "candidates_mean": float(cand.float().mean()), "candidates_max": int(cand.max()), "trials_mean": float(a.trials.float().mean())}
        find.update(ab(lambda: ct.find_contacts(geom, p, maxc=maxc, out=a),
                       lambda: ct.find_contacts(geom, p, maxc=maxc, out=b, broadphase=True, candidates=cand), args.reps, args.window))
        row["find"] = find
        # the move / detect / halve loop of the settling run's step with the most trials
        _, p0, v0 = worst
        dt = world.dt
        mv = lambda out, **kw: ct.move_and_find_contacts(geom, p0, v0, dt, maxc=maxc, eps=world.eps, tol=world.tol, strict=world.strict,
                                                         dt_floor=dt / 4, max_trials=world.max_trials, out=out, **kw)
        a, b = mv(None), mv(None, broadphase=True, candidates=cand)
        torch.cuda.synchronize()
        halv = {"outputs_equal": equal(a, b), "contacts_mean": float(a.count.float().mean()), "candidates_mean": float(cand.float().mean()),
                "candidates_max": int(cand.max()), "trials_mean": float(a.trials.float().mean()), "trials_max": int(a.trials.max())}
        halv.update(ab(lambda: mv(a), lambda: mv(b, broadphase=True, candidates=cand), args.reps, args.window))
        row["halving"] = halv
        res["sizes"].append(row)
        del world
    res["outputs_equal"] = all(r[k]["outputs_equal"] for r in res["sizes"] for k in ("find", "halving"))
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
