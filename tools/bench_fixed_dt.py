"""Cost of fixed-interval stepping, `ContactWorld.step(fixed_dt=True)` (world.py:72-80), on the forming 4-box-stack world of
tools/bench_world.py (4096 scenes): ms per plain step and per fixed-interval step over the same steps from the same start
(a host clock around work that ends in a device synchronise), the histogram of sub-steps per scene and step, and the share
of sub-steps in which fewer than 10 % of the scenes were still active (every sub-step launches the whole batch: DESIGN.md §9).
Writes one JSON file and prints it.

    python tools/bench_fixed_dt.py [--batch 4096] [--steps 60] [--reps 3] [--out profiles/r10_fixed_dt.json]

`--ab-lib OTHER.so [--ab-reps 3]`: also the detection kernels' time in tools/bench_world.py (HIP events around the launch) with
this tree's library and with OTHER.so (a build of another commit, through LCP_HIP_LIB), in child processes run alternately;
reported per side with its spread (max - min over the repetitions).  The children run before this process opens the GPU.
OTHER.so has to export every symbol of this tree's include/lcp_hip.h (the loader binds them all): a build of a commit from
before the fixed-interval entries is linked with tools/ab_stub_fixed_dt.cpp (the recipe is in that file).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def detection_ab(other, reps, batch):
    """tools/bench_world.py (eager: events around each launch) alternately with the other library and with this tree's."""
    sides = {"other": [], "this": []}
    for _ in range(reps):
        for side in ("other", "this"):
            env = dict(os.environ)
            env.pop("LCP_HIP_LIB", None)
            if side == "other":
                env["LCP_HIP_LIB"] = os.path.abspath(other)
            res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_world.py"), "--batch", str(batch), "--cpu-scenes", "0"],
                                 env=env, check=True, capture_output=True, text=True, timeout=600)
            line = json.loads(res.stdout.strip().splitlines()[-1])
            sides[side].append({k: line[k] for k in ("move_find_contacts_ms", "solve_dynamics_ms", "ms_per_step", "mean_trials_last_step")})
    out = {"workload": "tools/bench_world.py --batch %d (40 untimed + 100 timed steps, 4-box stacks forming), alternated other / this" % batch,
           "other_lib": os.path.basename(other), "runs": sides}
    for side, runs in sides.items():
        for k in ("move_find_contacts_ms", "solve_dynamics_ms"):
            v = sorted(r[k] for r in runs)
            out["%s_%s" % (side, k)] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "spread": v[-1] - v[0]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--nbox", type=int, default=4)
    ap.add_argument("--steps", type=int, default=60, help="steps from the start pose (the stacks form: the steps in which dt is halved)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--maxc", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_fixed_dt.json"))
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--ab-reps", type=int, default=3)
    ap.add_argument("--resources", default=None, help="JSON of the detection kernels' compile report to store beside the timings")
    args = ap.parse_args()
    ab = detection_ab(args.ab_lib, args.ab_reps, args.batch) if args.ab_lib else None

    import torch
    from lcp_physics_amd import scenes
    from lcp_physics_amd.physics import batched_world as bw
    from lcp_physics_amd.physics import contacts as ct
    dev = torch.device("cuda")
    w = scenes.make_drop_world(args.batch, nbox=args.nbox)
    geom = ct.GeometryBatch.from_shapes(w["shapes"], args.batch).to(dev)
    g = lambda k: w[k].to(dev)

    def fresh():
        return bw.ContactWorld(geom, g("p"), g("v"), g("Mdiag"), g("f"), g("rest"), g("fric"), Je=g("Je"), maxc=args.maxc)

    def timed(step):
        world = fresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(world)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3, world

    # the sub-step statistics (untimed run): active scenes per sub-step, sub-steps per scene and step
    begin = bw.substep_begin
    active = []

    def begin_counted(*a, **kw):
        out = begin(*a, **kw)
        active.append(out["active"].sum())
        return out

    bw.substep_begin = begin_counted
    world = fresh()
    hist = torch.zeros(bw.ContactWorld.MAX_SUBSTEPS + 1, dtype=torch.int64, device=dev)
    per_step = []
    for _ in range(args.steps):
        world.step(fixed_dt=True)
        hist += torch.bincount(world.substeps.long(), minlength=hist.numel())
        per_step.append(int(world.substeps.max()))
    bw.substep_begin = begin
    world.check_capacity()
    act = torch.stack(active).cpu().numpy() / float(args.batch)
    kmax = max(per_step)
    for _ in range(2):                                                   # warm-up of every shape the timed windows use
        timed(lambda x: x.step())
        timed(lambda x: x.step(fixed_dt=True))
    plain, fixed, capped = [], [], []
    for _ in range(args.reps):                                           # alternated
        plain.append(timed(lambda x: x.step())[0])
        fixed.append(timed(lambda x: x.step(fixed_dt=True))[0])
        ms, wk = timed(lambda x: x.step(fixed_dt=True, max_substeps=kmax))
        wk.assert_on_schedule()
        capped.append(ms)
    stat = lambda v: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "spread": max(v) - min(v)}
    hist = hist.cpu().tolist()
    out = {"workload": "scenes.make_drop_world: floor + %d boxes forming a stack, %d scenes, %d steps from the start pose, eager" % (args.nbox, args.batch, args.steps),
           "clock": "host clock around the steps, device synchronise at both ends; %d alternated repetitions after 2 warm-up rounds" % args.reps,
           "ms_per_plain_step": stat(plain), "ms_per_fixed_dt_step": stat(fixed),
           "ms_per_fixed_dt_step_max_substeps_%d_no_sync" % kmax: stat(capped),
           "substeps_total": int(len(act)), "substeps_per_step_mean": len(act) / float(args.steps), "substeps_per_step_max": kmax,
           "substep_histogram_scene_steps": {str(k): n for k, n in enumerate(hist) if n},
           "share_of_substeps_with_under_10pct_active": float((act < 0.1).mean()),
           "mean_active_share_per_substep": float(act.mean()),
           "mean_t_end": float(world.t.mean()), "all_scenes_on_the_grid": bool((world.t - world.dt * args.steps).abs().max() < 1e-9)}
    if ab is not None:
        out["detection_kernels_ab"] = ab
    if args.resources:
        out["detection_kernels_compile_report"] = json.load(open(args.resources))
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
