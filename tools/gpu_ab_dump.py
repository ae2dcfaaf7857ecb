"""A/B aid: run one case with the library named by LCP_HIP_LIB and dump its outputs; compare two dumps.
    LCP_HIP_LIB=tools/liblcp_hip_prev.so python tools/gpu_ab_dump.py a.pt ; python tools/gpu_ab_dump.py b.pt
    python tools/gpu_ab_dump.py --diff a.pt b.pt
Without `--case`: the fused step on a seeded stack batch.  `--case NAME[,NAME...]` (or `--case wg`: all of WG_CASES): forward outputs
and every gradient of the workgroup-per-scene kernels (lcp_primal_wg.hip, tag 13; lcp_primal_wg_poststab.hip, tag 14) on B = 8
stack scenes under path "primal_wg", at the pivot counts where the shared LU and sweeps change shape (all pivots in the first lane
half, the lane split at 64, the capacity).  `--diff` prints the largest difference per tensor and, per case, whether every tensor
is bitwise equal; it exits 1 when one is not."""
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
        names = list(WG_CASES) if sys.argv[2] == "wg" else sys.argv[2].split(",")
        res = {}
        for name in names:
            res.update({name + "/" + k: v for k, v in wg_case(name).items()})
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
