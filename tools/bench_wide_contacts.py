"""The wide narrow phase (lcp_contacts_wide.hip) on one GPU: detection and frame-backward launch times for B scenes of a floor and
nb - 1 circles, rects and 16-gons settled into piles; the whole `ContactWorld.step()` and a recorded step + backward at that size;
and the wide detection against lcp_contacts.hip on the 4-box BASELINE world (the same scenes, capacity 16 vs 8).
The solve alone: lcp_solve_dynamics_f32 on the settled contact lists, forward and forward + lcp_step_backward_f32, on the kernel
family `--path` picks (auto | generic | primal_wg; the piles always settle on the automatic path, so every path solves the same
lists).  `--solve-only` skips the detection, world-step and BASELINE timings.
Device-synchronised timing after a spin-up; prints one JSON line (stamped with the kernel sources' hash) and writes it to --out.

    python tools/bench_wide_contacts.py [--batch 4096] [--nb 48] [--reps 20] [--path auto] [--solve-only] [--out profiles/wide_contacts.json]
"""
import argparse, json, os, sys, time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pile_scene(rng, nb, nv=16, col=8):
    """Floor + columns of `col` circles / rects / nv-gons, 0.2 apart (settled by the untimed steps)."""
    ncol = (nb - 2) // col + 1
    shapes, pose = [("rect", (100.0 * ncol + 100.0, 10.0))], [[0.0, 300.0, 400.0]]
    x0 = 300.0 - 50.0 * (ncol - 1)
    for c in range(ncol):
        y = 395.0
        for _ in range(min(col, nb - len(shapes))):
            r, sz = rng.random(), rng.uniform(15, 30, size=2)
            if r < 0.3:
                shapes.append(("circle", float(sz[0]))); hh = sz[0]
            elif r < 0.6:
                shapes.append(("rect", (float(sz[0]), float(sz[1])))); hh = sz[1] / 2
            else:
                ang = (np.arange(nv) + rng.uniform(-0.3, 0.3, nv)) * (2 * np.pi / nv)
                shapes.append(("hull", np.stack([sz[0] * np.cos(ang), sz[0] * np.sin(ang)], axis=1))); hh = sz[0]
            y -= hh + 0.2
            pose.append([0.0, x0 + 100.0 * c + float(rng.uniform(-8, 8)), y])
            y -= hh
    return shapes, np.array(pose)


def pile_world(B, nb, maxc, dev, seed=48):
    from lcp_physics_amd.physics import batched_world as bw
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.scenes import GRAVITY
    shapes, pose = pile_scene(np.random.default_rng(seed), nb)
    Mdiag = np.ones((nb, 3))
    for i, (k, a) in enumerate(shapes[1:], 1):
        Mdiag[i, 0] = 0.5 * a ** 2 if k == "circle" else ((a[0] ** 2 + a[1] ** 2) / 12.0 if k == "rect" else 0.5 * float((np.asarray(a) ** 2).sum(1).mean()))
    f = np.zeros((nb, 3)); f[1:, 2] = GRAVITY
    Je = np.zeros((3, 3 * nb)); Je[:, :3] = np.eye(3)
    rep = lambda a, dt_: torch.tensor(np.broadcast_to(a, (B,) + a.shape).copy(), dtype=dt_, device=dev)
    geom = GeometryBatch.from_shapes(shapes, B, max_verts=None).to(dev)
    return bw.ContactWorld(geom, rep(pose, torch.float64), rep(np.zeros_like(pose), torch.float32), rep(Mdiag, torch.float32),
                           rep(f, torch.float32), rep(np.full(nb, 0.3), torch.float32), rep(np.full(nb, 0.5), torch.float32),
                           Je=rep(Je, torch.float32), maxc=maxc)


def timed(fn, reps):
    """Median of `reps` device-synchronised calls (ms)."""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--nb", type=int, default=48)
    ap.add_argument("--maxc", type=int, default=128)
    ap.add_argument("--settle", type=int, default=30, help="untimed steps before the timed region (the piles settle)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spinup", type=float, default=1.0, help="seconds of untimed launches first (device clocks settle)")
    ap.add_argument("--path", default="auto", choices=["auto", "generic", "primal_wg"], help="kernel family of the timed solves")
    ap.add_argument("--solve-only", action="store_true", help="time the solve alone (skip detection, world steps, BASELINE world)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from lcp_physics_amd import _lib, scenes
    from lcp_physics_amd.physics import batched_world as bw
    from lcp_physics_amd.physics import contacts as ct
    from lcp_physics_amd.srchash import source_sha256
    dev = torch.device("cuda")
    B = args.batch
    world = pile_world(B, args.nb, args.maxc, dev)
    for _ in range(args.settle):
        world.step()
    world.check_capacity()
    torch.cuda.synchronize()
    geom, p = world.geom, world.p.clone()
    cb = ct.find_contacts(geom, p, maxc=args.maxc)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.spinup:
        ct.find_contacts(geom, p, maxc=args.maxc, out=cb)
        torch.cuda.synchronize()
    counts = cb.count.float()
    gen = torch.Generator().manual_seed(0)
    gs = [torch.randn(B, args.maxc, 2, generator=gen).to(dev) for _ in range(3)]
    res = {"tool": "bench_wide_contacts", "batch": B, "nb": args.nb, "maxc": args.maxc, "settle_steps": args.settle,
           "scene_verts_max": geom.scene_verts_max, "nvcap": geom.nvcap, "contacts_mean": float(counts.mean()),
           "contacts_max": int(counts.max()), "gpu": torch.cuda.get_device_name(0), "source_sha256": source_sha256(), "path": args.path}
    # the solve alone on the settled lists (what ContactWorld.step launches after detection)
    sc = world
    e = 3
    dl_dv = torch.randn(B, args.nb, 3, generator=gen).to(dev)
    solve = lambda: bw.solve_dynamics(B, args.nb, args.maxc, e, cb.count, sc.Mdiag, sc.v, sc.f, sc.rest, sc.fric, cb, sc.Je, sc.dt,
                                      path=args.path, pinned=sc._pinned)
    out = solve()
    torch.cuda.synchronize()
    res["solve_tag"] = int(out["ws"][-256:-252].cpu().numpy().view(np.int32)[0]) if out["ws"].numel() == _lib.workspace_bytes(
        B, 3 * args.nb, 4 * args.maxc, e, _lib.COMPUTE_F64) else None
    res["solve_status_nan"] = int(((out["status"] & _lib.ST_NAN) != 0).sum())
    sreps = max(3, args.reps // 4) if args.path == "generic" else args.reps

    def solve_fwd_bwd():
        o = solve()
        bw.solve_dynamics_backward(B, args.nb, args.maxc, e, sc.Mdiag, sc.v, sc.f, sc.rest, sc.fric, cb, sc.Je, sc.dt, dl_dv, o)

    solve_fwd_bwd()
    res["solve_forward_ms"] = timed(solve, sreps)
    res["solve_forward_backward_ms"] = timed(solve_fwd_bwd, sreps)
    if args.solve_only:
        line = json.dumps(res)
        print(line)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return
    res["detect_ms"] = timed(lambda: ct.find_contacts(geom, p, maxc=args.maxc, out=cb), args.reps)
    res["frame_backward_ms"] = timed(lambda: ct.contact_frame_backward(geom, p, cb, *gs), args.reps)
    res["world_step_ms"] = timed(world.step, args.reps)
    world.check_capacity()
    p_set = world.p.detach().clone()

    def recorded():
        p0 = p_set.clone().requires_grad_(True)
        world.restart(p0)
        world.step(differentiable=True)
        world.p[:, :, 1:].sum().backward()

    recorded()
    res["recorded_step_backward_ms"] = timed(recorded, max(3, args.reps // 4))
    res["world_steps_per_s"] = B / (res["world_step_ms"] * 1e-3)
    # the 4-box BASELINE world: lcp_contacts.hip (capacity 8) against the wide kernel (capacity 16), same scenes and pose
    w = scenes.make_drop_world(B, nbox=4, box=40.0)
    g8 = ct.GeometryBatch.from_shapes(w["shapes"], B).to(dev)
    g16 = ct.GeometryBatch.from_shapes(w["shapes"], B, max_verts=16).to(dev)
    p4 = w["p"].to(dev)
    v4 = torch.zeros(B, 5, 3, dtype=torch.float32, device=dev)
    v4[:, 1:, 2] = 30.0
    a8, a16 = ct.find_contacts(g8, p4, maxc=16), ct.find_contacts(g16, p4, maxc=16)
    res["baseline4_detect_ms_existing"] = timed(lambda: ct.move_and_find_contacts(g8, p4, v4, 1.0 / 30, maxc=16, out=a8), args.reps)
    res["baseline4_detect_ms_wide"] = timed(lambda: ct.move_and_find_contacts(g16, p4, v4, 1.0 / 30, maxc=16, out=a16), args.reps)
    res["baseline4_ratio_wide_over_existing"] = res["baseline4_detect_ms_wide"] / res["baseline4_detect_ms_existing"]
    res["baseline4_bitwise_equal"] = bool(torch.equal(a8.c_n, a16.c_n) and torch.equal(a8.count, a16.count) and torch.equal(a8.p_out, a16.p_out))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
