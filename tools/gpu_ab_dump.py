"""A/B aid: run one case with the library named by LCP_HIP_LIB and dump its outputs; compare two dumps.
    LCP_HIP_LIB=tools/liblcp_hip_prev.so python tools/gpu_ab_dump.py a.pt ; python tools/gpu_ab_dump.py b.pt
    python tools/gpu_ab_dump.py --diff a.pt b.pt
Without `--case`: the fused step on a seeded stack batch.  `--case NAME[,NAME...]` (or `--case wg`: all of WG_CASES): forward outputs
and every gradient of the workgroup-per-scene kernels (lcp_primal_wg.hip, tag 13; lcp_primal_wg_poststab.hip, tag 14) on B = 8
stack scenes under path "primal_wg", at the pivot counts where the shared LU and sweeps change shape (all pivots in the first lane
half, the lane split at 64, the capacity).  `--diff` prints the largest difference per tensor and, per case, whether every tensor
is bitwise equal; it exits 1 when one is not.
`--case contacts` (all of CONTACT_CASES): every output of find_contacts, move_and_find_contacts, contact_frame_backward and
contact_frame_backward_shape on B = 8 seeded piles of tools/bench_wide_contacts.py::pile_scene, per body count, vertex capacity and
broadphase setting - the sizes at which the parts the contact kernels share change behaviour (see contacts_case)."""
import sys

import torch

import os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name: (kernel, boxes, points per interface, pinned form, variant) - nz = 3 (boxes + 1)
WG_CASES = {
    "step_n60_pinned": ("step", 20, 2, True, None),              # nz 63, n 60: all pivots in the first lane half
    "step_n66": ("step", 20, 2, False, None),                    # the same scene unpinned: just past 64
    "step_n126_pinned": ("step", 42, 1, True, None),             # nz 129: RCAP rows
    "step_n126": ("step", 40, 1, False, None),                   # nz 123: the general form near CAP
    "step_n60_pinned_ragged": ("step", 20, 2, True, "ragged"),   # counts with zero contacts and truncation
    "step_n64": ("step", 19, 2, False, "e4"),                    # nz 60, e 4: the lane split exactly
    "step_n65": ("step", 20, 2, False, "e2"),                    # nz 63, e 2
    "poststab_n63": ("poststab", 19, 2, False, None),
    "poststab_n66": ("poststab", 20, 2, False, None),
    "poststab_n126": ("poststab", 40, 2, False, None),
    "poststab_moving_floor": ("poststab", 30, 1, False, "moving_floor"),     # b = Je v != 0
    "poststab_n64": ("poststab", 19, 2, False, "e4"),
    "poststab_n65": ("poststab", 20, 2, False, "e2"),
}


def _tag(ws, B, nb, maxc, e):
    """The workspace trailer word: which kernel family laid the workspace out."""
    import numpy as np
    from lcp_physics_amd import _lib
    total = _lib.workspace_bytes(B, 3 * nb, 4 * maxc, e, _lib.COMPUTE_F64)
    cls = ((B * 4) + 255) & ~255
    off = B * ((total - cls - 256) // B) + cls
    return int(ws[off:off + 4].cpu().numpy().view(np.int32)[0])


def wg_case(name):
    """One case of WG_CASES: dict of CPU tensors (forward outputs, gradients, the workspace tag)."""
    from lcp_physics_amd import _lib
    from lcp_physics_amd.physics import batched_world as bw
    from lcp_physics_amd.physics.contacts import ContactBuffers
    from lcp_physics_amd.scenes import make_stack_scenes
    kernel, nbox, pts, pinned, variant = WG_CASES[name]
    B = 8
    sc = make_stack_scenes(B=B, nbox=nbox, pts_per_interface=pts, seed=1400 + 5 * nbox + pts, dtype=torch.float32)
    count = torch.full((B,), sc.nc, dtype=torch.int32)
    if kernel == "poststab":                                     # perturbed velocities: the contacts have something to correct
        sc.v = sc.v + 0.3 * torch.randn(sc.v.shape, generator=torch.Generator().manual_seed(1))
    if variant == "ragged":
        count = torch.tensor([sc.nc, 0, sc.nc + 5, 1, 17, sc.nc, 30, sc.nc - 1], dtype=torch.int32)
    elif variant == "moving_floor":
        sc.v[:, 0] = 0.05 * torch.randn(B, 3, generator=torch.Generator().manual_seed(5))
    elif variant == "e4":
        from tests.test_hip_primal import _with_joint_rows
        sc = _with_joint_rows(sc, 4)
    elif variant == "e2":                                        # the floor pinned in two coordinates only
        sc.Je = sc.Je[:, :2].contiguous()
    e = sc.Je.shape[1]
    scg = sc.to(device="cuda")
    cb = ContactBuffers(B, sc.nb, sc.nc, "cuda")
    cb.c_n, cb.c_p1, cb.c_p2, cb.c_i1, cb.c_i2 = scg.c_n, scg.c_p1, scg.c_p2, scg.c_i1, scg.c_i2
    cot = torch.randn(B, sc.nb, 3, generator=torch.Generator().manual_seed(6), dtype=torch.float32).cuda()
    if kernel == "step":
        out = bw.solve_dynamics(B, sc.nb, sc.nc, e, count.cuda(), scg.Mdiag, scg.v, scg.f, scg.rest, scg.fric, cb, scg.Je, sc.dt,
                                path="primal_wg", pinned=pinned)
        g = bw.solve_dynamics_backward(B, sc.nb, sc.nc, e, scg.Mdiag, scg.v, scg.f, scg.rest, scg.fric, cb, scg.Je, sc.dt, cot, out,
                                       want_Je=True)
        keys, want = ("v_new", "z", "s", "y", "iters", "status"), 13
    else:
        _lib.set_path("primal_wg")
        try:
            p = torch.randn(B, sc.nb, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64).cuda()
            dts = (0.01 + 0.02 * torch.rand(B, generator=torch.Generator().manual_seed(4), dtype=torch.float64)).cuda()
            p_out = torch.empty_like(p)
            out = bw.post_stabilization(B, sc.nb, sc.nc, e, count.cuda(), scg.Mdiag, scg.v, scg.rest, cb, scg.Je, p=p, dt_scene=dts,
                                        p_out=p_out)
            out["p_out"] = p_out
            g = bw.post_stabilization_backward(B, sc.nb, sc.nc, e, scg.Mdiag, scg.v, scg.rest, cb, scg.Je, cot, out, want_Je=True)
        finally:
            _lib.set_path("auto")
        keys, want = ("dp", "p_out", "iters", "status"), 14
    torch.cuda.synchronize()
    tag = _tag(out["ws"], B, sc.nb, sc.nc, e)
    assert tag == want, "%s: workspace tag %d, not the workgroup kernels' %d" % (name, tag, want)
    res = {k: out[k].cpu() for k in keys if out.get(k) is not None}
    res.update({"grad_" + k: v.cpu() for k, v in g.items() if v is not None})
    res["tag"] = torch.tensor([tag])
    print(name, "nz", 3 * sc.nb, "e", e, "pivots", 3 * sc.nb - e if pinned else 3 * sc.nb + e, "contacts", sc.nc, "iters", out["iters"].tolist(),
          "status", out["status"].tolist(), "tensors", len(res))
    return res


# name: (bodies, vertex capacity, broadphase).  nb 2: one pair; 12: 66 pairs, two passes of 64; 40: 780 pairs; 64: the body cap, 2016
# pairs.  Capacity 8 with at most 32 bodies and no broadphase is served by lcp_contacts.hip, everything else by lcp_contacts_wide.hip.
CONTACT_CASES = {"contacts_nb%d_cap%d%s" % (nb, cap, "_bp" if bp else ""): (nb, cap, bp)
                 for nb in (2, 12, 40, 64) for cap in (8, 16, 64) for bp in (False, True)}


def contacts_case(name):
    """One case of CONTACT_CASES: dict of CPU tensors.  Eight different piles, pressed together until neighbours are 0.05 apart (inside
    the detection margin), and these runs: `find` (detection at that pose); `move` (the move / halve loop from one dt, strict: velocities
    that overshoot, so several halvings); `dts` (per-scene dt, not strict: scene 1 finished at dt = 0, scene 2 at dt < 0, scene 3 from a
    dt eight times larger); `nc` (a no_contact mask); `small` (maxc below the list: count > maxc); `svm` (scene_verts_max one below the
    largest scene: count = -1 there on the kernels that look at it); the frame backward for the pose and for the shape on `find`, `small`
    and `svm`."""
    import numpy as np
    from lcp_physics_amd.physics import contacts as ct
    from tools.bench_wide_contacts import pile_scene
    nb, cap, bp = CONTACT_CASES[name]
    B, dev = 8, torch.device("cuda")
    geoms, poses = [], []
    for b in range(B):
        shapes, pose = pile_scene(np.random.default_rng(9000 + 100 * nb + b), nb, nv=min(cap, 16))
        pose[1:, 2] += 0.15 * (1 + (np.arange(1, nb) - 1) % 8)            # (columns of 8: the k-th body above the floor comes down 0.15 k)
        geoms.append(ct.GeometryBatch.from_shapes(shapes, 1, max_verts=cap))
        poses.append(pose)
    cat = lambda f: torch.cat([getattr(g, f) for g in geoms])
    gen = torch.Generator().manual_seed(nb * 100 + cap)
    mask = (torch.rand(B, nb, nb, generator=gen) < 0.15).to(torch.uint8)

    def geometry(no_contact=None, svm=None):
        return ct.GeometryBatch(cat("kind"), cat("radius"), cat("verts_local"), cat("nverts"), no_contact,
                                max(g.scene_verts_max for g in geoms) if svm is None else svm).to(dev)

    geom = geometry()
    p = torch.tensor(np.stack(poses), dtype=torch.float64, device=dev)
    v = (torch.randn(B, nb, 3, generator=gen) * torch.tensor([0.3, 5.0, 5.0])).float()
    v[:, 1:, 2] += 30.0
    v[:, 0] = 0.0
    v = v.to(dev)
    dt = 1.0 / 30
    dts = torch.full((B,), dt, dtype=torch.float64)
    dts[1], dts[2], dts[3], dts[4] = 0.0, -1.0, 8 * dt, dt / 16
    maxc = 4 * nb
    res = {}

    def keep(run, cb, cand):
        for k in ("p_out", "c_pen", "max_pen", "dt_used", "c_n", "c_p1", "c_p2", "c_i1", "c_i2", "count", "trials"):
            res[run + "." + k] = getattr(cb, k).cpu()
        if cand is not None:
            res[run + ".candidates"] = cand.cpu()

    def detect(run, g, maxc_, **kw):
        cand = torch.full((B,), -7, dtype=torch.int32, device=dev) if bp else None
        cb = ct.move_and_find_contacts(g, p, kw.pop("v", None), kw.pop("dt", 0.0), maxc=maxc_, broadphase=bp, candidates=cand, **kw)
        keep(run, cb, cand)
        return cb

    def backward(run, g, cb):
        gs = [torch.randn(B, cb.c_n.shape[1], 2, generator=gen).to(dev) for _ in range(3)]
        res[run + ".dp"] = ct.contact_frame_backward(g, p, cb, *gs).cpu()
        d_rad, d_verts = ct.contact_frame_backward_shape(g, p, cb, *gs)
        res[run + ".d_radius"], res[run + ".d_verts_local"] = d_rad.cpu(), d_verts.cpu()

    found = detect("find", geom, maxc, max_trials=1)
    backward("find", geom, found)
    moved = detect("move", geom, maxc, v=v, dt=dt, strict=True)
    stepped = detect("dts", geom, maxc, v=v, dt=dt, strict=False, dt_scene=dts.to(dev))
    detect("nc", geometry(no_contact=mask), maxc, v=v, dt=dt, strict=True)
    nmax = int(found.count.max())
    small = detect("small", geom, max(1, nmax // 2), max_trials=1)
    backward("small", geom, small)
    short = geometry(svm=max(0, geom.scene_verts_max - 1))
    cut = detect("svm", short, maxc, max_trials=1)
    backward("svm", short, cut)
    torch.cuda.synchronize()
    print(name, "contacts", found.count.tolist(), "trials move", moved.trials.tolist(), "trials dts", stepped.trials.tolist(), "count small",
          small.count.tolist(), "maxc small", small.maxc, "count svm", cut.count.tolist(), "tensors", len(res))
    return res


def diff(fa, fb):
    a, b = torch.load(fa), torch.load(fb)
    assert set(a) == set(b), (sorted(a), sorted(b))
    cases = {}
    for k in a:
        d = (a[k].double() - b[k].double()).abs()
        same = torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8))     # (bit for bit: NaN payloads and signed zeros too)
        cases.setdefault(k.split("/")[0] if "/" in k else "", []).append(same)
        print("%-40s %s max|a-b| %.3e  (max|a| %.3e)  worst scene %d" % (k, "equal  " if same else "DIFFERS", float(d.nan_to_num().max()), float(a[k].double().abs().nan_to_num().max()),
                                                                         int(d.nan_to_num().reshape(d.shape[0], -1).max(dim=1)[0].argmax())))
    for c, v in cases.items():
        print("bitwise_equal", c or "fused_step", all(v), "(%d tensors)" % len(v))
    return all(all(v) for v in cases.values())


def main():
    if sys.argv[1] == "--diff":
        sys.exit(0 if diff(sys.argv[2], sys.argv[3]) else 1)
    if sys.argv[1] == "--case":
        names = {"wg": list(WG_CASES), "contacts": list(CONTACT_CASES)}.get(sys.argv[2]) or sys.argv[2].split(",")
        res = {}
        for name in names:
            res.update({name + "/" + k: v for k, v in (contacts_case if name in CONTACT_CASES else wg_case)(name).items()})
        torch.save(res, sys.argv[3])
        return
    from lcp_physics_amd.physics.batched_world import fused_step
    from lcp_physics_amd.scenes import make_stack_scenes
    sc = make_stack_scenes(64, nbox=4, pts_per_interface=4, seed=1).to("cuda", torch.float32)
    out = fused_step(sc)
    torch.cuda.synchronize()
    torch.save({k: out[k].cpu() for k in ("v_new", "z", "s", "iters", "status")}, sys.argv[1])
    print("iters", out["iters"][:8].tolist(), "status", out["status"][:8].tolist(), "v_new[0]", out["v_new"][0].reshape(-1)[:6].tolist())


if __name__ == "__main__":
    main()
