"""Time the shape backward of the contact frame (lcp_contact_frame_backward_shape_f64) beside the pose backward
(lcp_contact_frame_backward[_nv]_f64) on the same records: the settled piles of tools/bench_wide_contacts.py (4096 scenes of 48
bodies with 16-gons) and the 4-box stacks of the BASELINE world.  Prints one JSON line; run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_shape_backward.py` for the per-kernel device times.

    python tools/bench_shape_backward.py --out profiles/shape_backward.json
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_wide_contacts import pile_world, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--nb", type=int, default=48)
    ap.add_argument("--maxc", type=int, default=128)
    ap.add_argument("--settle", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from lcp_physics_amd import scenes
    from lcp_physics_amd.physics import contacts as ct
    from lcp_physics_amd.srchash import source_sha256
    dev = torch.device("cuda")
    B = args.batch
    gen = torch.Generator().manual_seed(0)
    res = {"tool": "bench_shape_backward", "batch": B, "gpu": torch.cuda.get_device_name(0), "source_sha256": source_sha256()}
    world = pile_world(B, args.nb, args.maxc, dev)
    for _ in range(args.settle):
        world.step()
    world.check_capacity()
    w4 = scenes.make_drop_world(B, nbox=4, box=40.0)
    # (the boxes of the drop world start 0.3 .. 2 apart: a detection margin of 3 gives every interface its two records)
    cases = (("piles", world.geom, world.p.clone(), args.maxc, ct.EPSILON),
             ("stack4", ct.GeometryBatch.from_shapes(w4["shapes"], B).to(dev), w4["p"].to(dev), 16, 3.0))
    for name, geom, p, maxc, eps in cases:
        cb = ct.find_contacts(geom, p, maxc=maxc, eps=eps)
        gs = [torch.randn(B, maxc, 2, generator=gen).to(dev) for _ in range(3)]
        pose = lambda: ct.contact_frame_backward(geom, p, cb, *gs, eps=eps)
        shape = lambda: ct.contact_frame_backward_shape(geom, p, cb, *gs, eps=eps)
        for _ in range(3):
            pose(); shape()
        res[name] = {"nb": geom.nb, "nvcap": geom.nvcap, "maxc": maxc, "eps": eps, "contacts_mean": float(cb.count.float().mean()),
                     "pose_backward_ms": timed(pose, args.reps), "shape_backward_ms": timed(shape, args.reps)}
        res[name]["ratio_shape_over_pose"] = res[name]["shape_backward_ms"] / res[name]["pose_backward_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
