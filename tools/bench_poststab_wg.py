"""Post-stabilisation beyond one wavefront: `lcp_post_stabilization_f32` and its backward on the workgroup-per-scene body-space
kernels (`lcp_primal_wg_poststab.hip`, workspace tag 14) against the generic contact-space kernels (`set_path("generic")`, tag 11)
in ONE process, alternating the two: 4096 stacks of 30 and 40 boxes at one and two contact points per interface (`--cases`: other
sizes, padded capacities), perturbed velocities (the contacts have something to correct), full lists.  The workgroup kernels run
under `set_path("primal_wg")`: the same kernels where automatic mode picks them, and the A/B partner where it does not.  HIP events around each call, one warm-up call of every shape and
path, the median of `--reps` alternated repetitions.  Writes one JSON document.

    python tools/bench_poststab_wg.py [--batch 4096] [--reps 5] [--out profiles/r09_poststab_wg.json]
"""
import argparse, json, os, statistics, sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _tag(ws, B, nb, maxc, e):
    from lcp_physics_amd import _lib
    total = _lib.workspace_bytes(B, 3 * nb, 4 * maxc, e, _lib.COMPUTE_F64)
    cls = ((B * 4) + 255) & ~255
    off = B * ((total - cls - 256) // B) + cls
    return int(ws[off:off + 4].cpu().numpy().view(np.int32)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="30:1,30:2,40:1,40:2",
                    help="nbox:pts[:maxc] - boxes on the floor, contact points per interface, capacity (padded slots) if larger than the list")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_poststab_wg.json"))
    args = ap.parse_args()
    from lcp_physics_amd import _lib, scenes
    from lcp_physics_amd.physics.batched_world import post_stabilization, post_stabilization_backward
    from lcp_physics_amd.physics.contacts import ContactBuffers
    if not torch.cuda.is_available():
        raise SystemExit("bench_poststab_wg.py times kernels on the GPU: no device found")
    B = args.batch
    rows = []
    for case in args.cases.split(","):
        for nbox, pts, cap in (tuple(int(t) for t in (case.split(":") + ["0"])[:3]),):
            sc = scenes.make_stack_scenes(B=B, nbox=nbox, pts_per_interface=pts, seed=1400 + 5 * nbox + pts, dtype=torch.float32)
            sc.v = sc.v + 0.3 * torch.randn(sc.v.shape, generator=torch.Generator().manual_seed(1))
            live, maxc = sc.nc, max(sc.nc, cap)
            sc = sc.to(device="cuda")
            cb = ContactBuffers(B, sc.nb, maxc, "cuda")                   # (zeroed: the slots behind the list stay padding)
            for name in ("c_n", "c_p1", "c_p2", "c_i1", "c_i2"):
                getattr(cb, name)[:, :live] = getattr(sc, name)
            count = torch.full((B,), live, dtype=torch.int32, device="cuda")
            cot = torch.randn(B, sc.nb, 3, generator=torch.Generator().manual_seed(6), dtype=torch.float32).cuda()
            outs, times = {}, {"primal_wg": {"f": [], "fb": []}, "generic": {"f": [], "fb": []}}

            def call(path, backward):
                _lib.set_path(path)
                try:
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    prev = outs.get(path)
                    ev[0].record()
                    out = post_stabilization(B, sc.nb, maxc, 3, count, sc.Mdiag, sc.v, sc.rest, cb, sc.Je,
                                             ws=None if prev is None else prev["ws"], out=prev)
                    if backward:
                        post_stabilization_backward(B, sc.nb, maxc, 3, sc.Mdiag, sc.v, sc.rest, cb, sc.Je, cot, out, want_Je=True)
                    ev[1].record()
                    torch.cuda.synchronize()
                finally:
                    _lib.set_path("auto")
                outs[path] = out
                return ev[0].elapsed_time(ev[1])

            for path in ("primal_wg", "generic"):                              # warm-up: code objects, workspaces, output tensors
                call(path, False)
                call(path, True)
            for _ in range(args.reps):                                    # alternated: what shares the machine hits both alike
                for path in ("primal_wg", "generic"):
                    times[path]["f"].append(call(path, False))
                    times[path]["fb"].append(call(path, True))
            a, b = outs["primal_wg"], outs["generic"]
            da, db = a["dp"].double().reshape(B, -1), b["dp"].double().reshape(B, -1)
            err = float(((da - db).abs().max(dim=1)[0] / db.abs().max(dim=1)[0].clamp_min(1.0)).max())
            med = lambda p, k: statistics.median(times[p][k])
            row = {"bodies": sc.nb, "contacts": live, "capacity": maxc, "pts_per_interface": pts,
                   "tag": _tag(a["ws"], B, sc.nb, maxc, 3), "tag_generic": _tag(b["ws"], B, sc.nb, maxc, 3),
                   "forward_ms": med("primal_wg", "f"), "forward_backward_ms": med("primal_wg", "fb"),
                   "generic_forward_ms": med("generic", "f"), "generic_forward_backward_ms": med("generic", "fb"),
                   "forward_ms_min_max": [min(times["primal_wg"]["f"]), max(times["primal_wg"]["f"])],
                   "generic_forward_ms_min_max": [min(times["generic"]["f"]), max(times["generic"]["f"])],
                   "mean_iters": float(a["iters"].float().mean()), "mean_iters_generic": float(b["iters"].float().mean()),
                   "worst_scaled_dp_difference": err,
                   "status_nan": int(((a["status"] & _lib.ST_NAN) != 0).sum())}
            row["forward_ratio"] = row["generic_forward_ms"] / row["forward_ms"]
            row["forward_backward_ratio"] = row["generic_forward_backward_ms"] / row["forward_backward_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    doc = {"tool": "bench_poststab_wg", "batch": B, "reps": args.reps, "gpu": torch.cuda.get_device_name(0), "timing": "HIP events, median",
           "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
