"""Time the time-of-impact query (lcp_toi.hip through `physics.impact.time_of_impact`) against the route a user had before it existed:
the same conservative advancement (include/lcp_hip.h, "time of impact") driven from torch - every pair as a two-body scene through
`pair_distances`, one launch and a handful of elementwise operations per iteration - and what `ContactWorld(ccd=True)` costs a step.
Writes profiles/toi.json.

    python tools/bench_toi.py [--out profiles/toi.json] [--parent-root DIR]     # needs the GPU

Shapes (those of tools/bench_proximity.py, with velocities): (a) 4096 scenes x 8 bodies x all 28 pairs at horizon = dt = 1/30;
(b) 4096 scenes x a packed pile of 45 16-gons x all 990 pairs at horizon = dt - most pairs are culled or TOUCHING; (c) the same at
horizon = 1 s.  Each forward and forward + backward.  The torch route runs on the first `baseline_scenes` scenes only (the two-body
scenes of every pair of 4096 piles would take 2 GB) and its time is scaled to the batch; it runs as many iterations as its slowest pair
needs (found beforehand, with one synchronisation per iteration; the timed loop has none).  The evaluations per pair are the torch
route's own count.  HIP events, a spin-up before anything is timed, the routes alternated in one process, the median of REPS
repetitions with the spread.  `--parent-root DIR` (a checkout of the parent commit with its library built): a plain step of the
four-box world without `ccd`, stepped by this tree and by the parent's in fresh processes that alternate
(`bench_contact_report.plain_against_parent`)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
F64, F32 = torch.float64, torch.float32
REPS = 11
DT = 1.0 / 30
TOL, MAX_ITER = 1e-6, 64


def make_shape(name, dev):
    """(geom, p, v, pairs, margin, horizon, info) - the layout of bench_proximity's shape with random velocities."""
    import bench_proximity as BP
    ins, info = BP.make_shape(BP.SHAPES[0] if name == "a" else BP.SHAPES[1], dev)
    B, nb = info["B"], info["nb"]
    gen = torch.Generator().manual_seed(11)
    scale = torch.tensor([2.0, 300.0, 300.0]) if name == "a" else torch.tensor([1.0, 30.0, 30.0])
    v = ((torch.rand(B, nb, 3, generator=gen) * 2 - 1) * scale).to(F32).to(dev)
    horizon = 1.0 if name == "c" else DT
    return ins["geom"], ins["p"], v, ins["pairs"], 0.05, horizon, dict(B=B, nb=nb, P=info["P"], horizon=horizon, margin=0.05)


def two_body_scenes(geom, p, v, pairs, Bs):
    """The pairs of the first Bs scenes as N = Bs P scenes of two bodies with the one pair (0, 1)."""
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.proximity import PairSet
    P = pairs.P
    k = torch.stack([pairs.first[:Bs], pairs.second[:Bs]], -1).long().reshape(Bs * P, 2)
    b = torch.arange(Bs, device=p.device).repeat_interleave(P).unsqueeze(1)
    g2 = GeometryBatch(geom.kind[b, k].contiguous(), geom.radius[b, k].contiguous(), geom.verts_local[b, k].contiguous(),
                       geom.nverts[b, k].contiguous(), None, 2 * geom.nvcap)
    rho = torch.where(geom.kind != 0, geom.verts_local.norm(dim=-1).max(-1).values, torch.zeros_like(geom.radius))[b, k]
    v2 = v[b, k].double()
    turn = (v2[..., 0].abs() * rho).sum(-1)
    return g2, p[b, k].contiguous(), v2, turn, PairSet.all_pairs(2, Bs * P).to(p.device)


def torch_advance(two, margin, horizon, iters=None):
    """The advancement from torch: (toi, status, evaluations per pair, iterations run).  `iters`: run exactly that many, no
    synchronisation; None: until no pair is active (one synchronisation per iteration)."""
    from lcp_physics_amd.physics.proximity import pair_distances
    g2, p2, v2, turn, pr = two
    N = p2.shape[0]
    dev = p2.device
    dv = v2[:, 1, 1:] - v2[:, 0, 1:]
    t = torch.zeros(N, dtype=F64, device=dev)
    toi = torch.full((N,), float(horizon), dtype=F64, device=dev)
    status = torch.zeros(N, dtype=torch.int32, device=dev)
    evals = torch.zeros(N, dtype=torch.int32, device=dev)
    active = torch.ones(N, dtype=torch.bool, device=dev)
    k = 0
    while k < (MAX_ITER if iters is None else iters):
        dist, n, _, _ = pair_distances(g2, p2 + t.reshape(N, 1, 1) * v2, pr, witnesses=True)
        gap = dist[:, 0] - margin
        evals += active
        hit = active & (gap <= TOL)
        a = -(n[:, 0] * dv).sum(-1) + turn
        tn = t + gap / a
        miss = active & ~hit & (~(a > 0) | ~(tn < horizon))
        toi = torch.where(hit, t, toi)
        status = torch.where(hit, torch.full_like(status, 2 if k == 0 else 1), status)
        active = active & ~hit & ~miss
        t = torch.where(active, tn, t)
        k += 1
        if iters is None and not bool(active.any()):
            break
    toi = torch.where(active, t, toi)
    status = torch.where(active, torch.full_like(status, 3), status)
    return toi, status, evals, k


def repetition(fn, n):
    """Mean time of one call of `fn` over `n` calls, by HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def alternate(fns):
    """{name: fn} -> {name_us, name_spread_us}: warm-up, then REPS alternated repetitions of about 50 ms each."""
    calls = {}
    for k, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[k] = max(1, int(math.ceil(0.05 / max(repetition(fn, 3), 1e-7))))
    runs = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            runs[k].append(repetition(fn, calls[k]))
    out = {}
    for k, v in runs.items():
        out[k + "_us"] = round(float(np.median(v)) * 1e6, 2)
        out[k + "_spread_us"] = [round(min(v) * 1e6, 2), round(max(v) * 1e6, 2)]
    return out


def measure(name, dev, baseline_scenes):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.impact import time_of_impact
    geom, p, v, pairs, margin, horizon, info = make_shape(name, dev)
    B, P = info["B"], info["P"]
    Bs = min(B, baseline_scenes)
    two = two_body_scenes(geom, p, v, pairs, Bs)
    leaves = [x.clone().requires_grad_(True) for x in (p, v, geom.radius, geom.verts_local)]
    lgeom = GeometryBatch(geom.kind, leaves[2], leaves[3], geom.nverts, None, geom.scene_verts_max)
    g = torch.randn(B, P, generator=torch.Generator().manual_seed(3), dtype=F64).to(dev)

    def k_fwd():
        with torch.no_grad():
            return time_of_impact(geom, p, v, pairs, horizon, margin=margin, tol=TOL, max_iter=MAX_ITER)

    def k_both():
        for x in leaves:
            x.grad = None
        time_of_impact(lgeom, leaves[0], leaves[1], pairs, horizon, margin=margin, tol=TOL, max_iter=MAX_ITER)[0].backward(g)

    toi, status = k_fwd()
    t_toi, t_status, evals, iters = torch_advance(two, margin, horizon)
    torch.cuda.synchronize()
    same = (t_status.reshape(Bs, P) == status[:Bs]).double().mean()
    hit = (t_status.reshape(Bs, P) == 1) & (status[:Bs] == 1)
    err = float((t_toi.reshape(Bs, P) - toi[:Bs]).abs()[hit].max()) if bool(hit.any()) else 0.0
    assert float(same) >= 0.999, "the routes' statuses disagree on %.4f of the pairs" % (1 - float(same))
    res = dict(info, baseline_scenes=Bs, baseline_iterations=iters, statuses_agreeing=float(same), hit_toi_difference_abs=err,
               status_counts=torch.bincount(status.flatten().long(), minlength=4).tolist(),
               evaluations_per_pair_mean=round(float(evals.double().mean()), 3), evaluations_per_pair_max=int(evals.max()))
    t = alternate({"kernel_forward": k_fwd, "kernel_forward_backward": k_both,
                   "torch_forward_subset": lambda: torch_advance(two, margin, horizon, iters=iters)})
    res.update(t)
    res["torch_forward_scaled_us"] = round(t["torch_forward_subset_us"] * B / Bs, 2)
    res["kernel_over_torch_forward"] = round(t["kernel_forward_us"] / res["torch_forward_scaled_us"], 5)
    return res


def measure_step(dev, B=4096):
    """A plain step of 4096 four-box worlds (scenes.make_drop_world, settled) with ccd=True against without, eager and as a captured
    run of 20 steps."""
    import bench_contact_report as BCR
    from lcp_physics_amd import scenes
    from lcp_physics_amd.physics import batched_world as bw
    from lcp_physics_amd.physics import contacts as ct
    w = scenes.make_drop_world(B, nbox=4)
    geom = ct.GeometryBatch.from_shapes(w["shapes"], B).to(dev)
    g = lambda k: w[k].to(dev)
    plain = BCR.box_world(B, dev, None)
    ccd = bw.ContactWorld(geom, g("p"), g("v"), g("Mdiag"), g("f"), g("rest"), g("fric"), Je=g("Je"), maxc=16, ccd=True)
    for _ in range(60):                                                                    # settle: the timed steps see resting stacks
        plain.step()
        ccd.step()
    torch.cuda.synchronize()
    res = dict(B=B, nb=5, pairs=10, settle_steps=60, same_pose_bits_with_and_without_ccd=bool(torch.equal(plain.p, ccd.p)),
               scenes_clipped_in_the_last_step=int((ccd._ccd.first_pair >= 0).sum()))
    res.update(alternate({"step_without_ccd": plain.step, "step_with_ccd": ccd.step,
                          "run20_graph_without_ccd": lambda: plain.run(20, graph=True),
                          "run20_graph_with_ccd": lambda: ccd.run(20, graph=True)}))
    res["ccd_step_overhead_us"] = round(res["step_with_ccd_us"] - res["step_without_ccd_us"], 2)
    res["ccd_graph_step_overhead_us"] = round((res["run20_graph_with_ccd_us"] - res["run20_graph_without_ccd_us"]) / 20, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "toi.json"))
    ap.add_argument("--baseline-scenes", type=int, default=128)
    ap.add_argument("--parent-root", default=None)
    a = ap.parse_args()
    plain = None
    if a.parent_root:                                                                     # fresh processes, before this one opens the GPU
        import bench_contact_report as BCR
        plain = BCR.plain_against_parent(a.parent_root, 4096)
    assert torch.cuda.is_available(), "bench_toi.py measures on the GPU; there is no CPU timing"
    dev = torch.device("cuda:0")
    x = torch.randn(4096, 4096, device=dev)                                               # spin-up: clocks
    for _ in range(50):
        x = (x @ x).clamp(-1, 1)
    torch.cuda.synchronize()
    doc = {"device": torch.cuda.get_device_name(0), "tol": TOL, "max_iter": MAX_ITER,
           "how": "HIP events, routes alternated in one process, the median of %d repetitions of about 50 ms with [min, max]" % REPS,
           "shapes": {n: measure(n, dev, a.baseline_scenes) for n in ("a", "b", "c")}, "four_box_worlds_4096": measure_step(dev)}
    if plain is not None:
        doc["world_without_ccd_against_parent"] = plain
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
