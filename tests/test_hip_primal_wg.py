"""The workgroup-per-scene body-space step kernels (`lcp_primal_wg.hip`: one workgroup of 256 threads per scene, the fp64
system of up to 128 pivots in LDS) behind `lcp_solve_dynamics_f32` / `lcp_step_fused_f32` / `lcp_step_backward_f32` at the
sizes beyond one wavefront (21-43 bodies, 65-256 contacts).  Checked against the generic contact-space kernels they replace
there (LCP_PATH_GENERIC, the A/B partner) and against the fp64 oracle."""
import glob
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import pdipm_oracle as O
from tests import parity

DEV = "cuda"
TAG_PRIMAL_WG, TAG_GENERIC = 13, 9
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lcp_physics_amd", "csrc")


def _tag(ws, B, nb, maxc, e):
    """The workspace trailer word: behind the B scene blocks and the per-scene class words."""
    from lcp_physics_amd import _lib
    total = _lib.workspace_bytes(B, 3 * nb, 4 * maxc, e, _lib.COMPUTE_F64)
    cls = ((B * 4) + 255) & ~255
    per_scene = (total - cls - 256) // B
    off = B * per_scene + cls
    return int(ws[off:off + 4].cpu().numpy().view(np.int32)[0])


def _solve(sc, count, path="auto", pinned=False):
    from lcp_physics_amd.physics.batched_world import solve_dynamics
    from lcp_physics_amd.physics.contacts import ContactBuffers
    scg = sc.to(device=DEV)
    cb = ContactBuffers(sc.B, sc.nb, sc.nc, DEV)
    cb.c_n, cb.c_p1, cb.c_p2, cb.c_i1, cb.c_i2 = scg.c_n, scg.c_p1, scg.c_p2, scg.c_i1, scg.c_i2
    e = 0 if scg.Je is None else scg.Je.shape[1]
    out = solve_dynamics(sc.B, sc.nb, sc.nc, e, count.to(DEV), scg.Mdiag, scg.v, scg.f, scg.rest, scg.fric, cb, scg.Je, sc.dt,
                         path=path, pinned=pinned)
    torch.cuda.synchronize()
    return scg, cb, out


def _backward(sc, scg, cb, out, cot):
    from lcp_physics_amd.physics.batched_world import solve_dynamics_backward
    e = 0 if scg.Je is None else scg.Je.shape[1]
    g = solve_dynamics_backward(sc.B, sc.nb, sc.nc, e, scg.Mdiag, scg.v, scg.f, scg.rest, scg.fric, cb, scg.Je, sc.dt,
                                cot.to(DEV), out, want_Je=e > 0)
    torch.cuda.synchronize()
    return {k: v.double().cpu() for k, v in g.items()}


def _stack(B, nbox, pts, seed=0):
    from lcp_physics_amd import scenes
    return scenes.make_stack_scenes(B=B, nbox=nbox, pts_per_interface=pts, seed=700 + 5 * nbox + pts + seed, dtype=torch.float32)


def _vrel(a, b):
    B = a.shape[0]
    a, b = a.double().cpu().reshape(B, -1), b.double().cpu().reshape(B, -1)
    return (a - b).abs().max(dim=1)[0] / b.abs().max(dim=1)[0].clamp_min(1.0)


def _oracle_lcp(sc, k, n):
    one = lambda t: t[k:k + 1].double()
    args = (one(sc.Mdiag), one(sc.v), one(sc.f), sc.dt, sc.c_n[k:k + 1, :n].double(), sc.c_p1[k:k + 1, :n].double(),
            sc.c_p2[k:k + 1, :n].double(), sc.c_i1[k:k + 1, :n], sc.c_i2[k:k + 1, :n], one(sc.rest), one(sc.fric),
            None if sc.Je is None else one(sc.Je))
    return [None if t is None else t.double() for t in O.assemble_lcp(*args)]


@pytest.mark.gpu
def test_routing_reaches_the_workgroup_kernels():
    """Automatic mode at 31 bodies / 64 contacts and at 13 bodies / 66 contacts takes the new family (tag 13);
    LCP_PATH_GENERIC keeps forcing the generic kernels (tag 9)."""
    from lcp_physics_amd import _lib
    assert _lib.path_bits("primal_wg") == _lib.PATH_PRIMAL_WG
    lib = _lib.load()
    for nbox, pts, maxc in ((30, 2, 64), (12, 4, 66)):
        sc = _stack(4, nbox, pts)
        if sc.nc < maxc:                                        # pad the list: the capacity decides the family
            pad = maxc - sc.nc
            for name in ("c_n", "c_p1", "c_p2"):
                setattr(sc, name, torch.cat([getattr(sc, name), torch.zeros(sc.B, pad, 2)], dim=1))
            for name in ("c_i1", "c_i2"):
                setattr(sc, name, torch.cat([getattr(sc, name), torch.zeros(sc.B, pad, dtype=torch.int32)], dim=1))
        count = torch.full((sc.B,), min(sc.nc, nbox * pts), dtype=torch.int32)
        assert lib.lcp_step_has_backward(sc.nb, sc.nc, 3, _lib.COMPUTE_F64) == 1
        _, _, a = _solve(sc, count)
        assert _tag(a["ws"], sc.B, sc.nb, sc.nc, 3) == TAG_PRIMAL_WG, (nbox, maxc)
        _, _, b = _solve(sc, count, path="generic")
        assert _tag(b["ws"], sc.B, sc.nb, sc.nc, 3) == TAG_GENERIC, (nbox, maxc)
        assert float(_vrel(a["v_new"], b["v_new"]).max()) <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("nbox,pts,pinned", [(n, p, pin) for n in (20, 30, 42) for p in (1, 2) for pin in (True, False)
                                             if pin or n < 42])    # (43 bodies, three general rows: 132 pivots - generic kernels)
def test_forward_matches_the_generic_kernels_and_the_oracle(nbox, pts, pinned):
    B = 1024 if nbox < 42 else 256
    sc = _stack(B, nbox, pts)
    count = torch.full((B,), sc.nc, dtype=torch.int32)
    _, _, a = _solve(sc, count, pinned=pinned)
    assert _tag(a["ws"], B, sc.nb, sc.nc, 3) == TAG_PRIMAL_WG
    _, _, b = _solve(sc, count, path="generic", pinned=pinned)
    err = _vrel(a["v_new"], b["v_new"])
    print(nbox, pts, pinned, "worst scaled |v_new - v_new(generic)|", float(err.max()), "iteration counts differ in",
          int((a["iters"] != b["iters"]).sum()), "of", B)
    assert float(err.max()) <= 1e-6
    from lcp_physics_amd import _lib
    loud = _lib.ST_NAN | _lib.ST_TRUNCATED                    # (the singularity bits name each family's own factorisations)
    assert torch.equal(a["status"].cpu() & loud, b["status"].cpu() & loud)
    assert int((a["status"] & 8).sum()) == 0
    got = a["v_new"].double().cpu()
    same_iters = 0
    K = 32
    for k in range(K):
        lcp64 = _oracle_lcp(sc, k, sc.nc)
        rs = O.lcp_forward(*lcp64)
        ex = float(parity.err_x(-got[k].reshape(1, -1), rs.x, lcp64[0], lcp64[1]).max())
        assert ex <= 1e-6, (k, ex)
        same_iters += int(int(a["iters"][k]) == int(rs.iters[0]) if torch.is_tensor(rs.iters) else int(a["iters"][k]) == int(rs.iters))
    print("iteration counts equal to the oracle's in", same_iters, "of", K)
    assert same_iters >= K - 2


@pytest.mark.gpu
def test_ragged_counts_truncation_and_no_contacts():
    from lcp_physics_amd import _lib
    B = 8
    sc = _stack(B, 40, 2)                                      # 41 bodies, 80 contact slots
    nc = sc.nc
    count = torch.tensor([nc, 64, 30, 0, nc + 5, nc, 1, 57], dtype=torch.int32)
    scg, _, a = _solve(sc, count, pinned=True)
    assert _tag(a["ws"], B, sc.nb, nc, 3) == TAG_PRIMAL_WG
    st = a["status"].cpu()
    assert int(st[4]) & _lib.ST_TRUNCATED and not any(int(st[k]) & _lib.ST_TRUNCATED for k in (0, 1, 2, 3, 5, 6, 7))
    assert int((st & _lib.ST_NAN).sum()) == 0
    _, _, b = _solve(sc, count, path="generic", pinned=True)
    assert float(_vrel(a["v_new"], b["v_new"]).max()) <= 1e-6
    got = a["v_new"].double().cpu()
    z = a["z"].double().cpu()
    for k in range(B):
        n = min(int(count[k]), nc)
        assert float(z[k, n:nc].abs().max() if n < nc else 0.0) == 0.0           # (padded slots 0)
        if n == 0:                                            # engines.py:36-50: a direct solve of [M A^T; A 0]
            md = sc.Mdiag[k].reshape(-1)
            Q = torch.diag(md.double())
            p = (md * sc.v[k].reshape(-1) + sc.dt * sc.f[k].reshape(-1)).double()     # (engines.py:32 in fp32, as the kernels)
            A = sc.Je[k].double()
            nz, e = Q.shape[0], A.shape[0]
            K = torch.zeros(nz + e, nz + e, dtype=torch.float64)
            K[:nz, :nz], K[:nz, nz:], K[nz:, :nz] = Q, A.T, A
            x = torch.linalg.solve(K, torch.cat([-p, torch.zeros(e, dtype=torch.float64)]))[:nz]
            err = float((-got[k].reshape(-1) - x).abs().max() / x.abs().max().clamp_min(1.0))
            assert err <= 1e-6, err
            continue
        lcp64 = _oracle_lcp(sc, k, n)
        rs = O.lcp_forward(*lcp64)
        ex = float(parity.err_x(-got[k].reshape(1, -1), rs.x, lcp64[0], lcp64[1]).max())
        assert ex <= 1e-6, (k, n, ex)


def _grad_err(a, b, keys):
    """Mdiag / v / f: max error over a scene relative to the scene's largest entry; the per-contact and per-body gradients
    relative to the batch's largest entry (a scene whose friction gradient is ~0 has no scale of its own)."""
    out = {}
    for k in keys:
        B = a[k].shape[0]
        x, y = a[k].reshape(B, -1), b[k].reshape(B, -1)
        if k in ("Mdiag", "v", "f"):
            out[k] = float(((x - y).abs().max(dim=1)[0] / y.abs().max(dim=1)[0].clamp_min(1e-30)).max())
        else:
            out[k] = float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("nbox,pts", [(30, 1), (42, 1), (30, 2)])
def test_backward_matches_the_generic_backward_and_the_oracle(nbox, pts):
    from lcp_physics_amd.physics.batched_world import solve_dynamics_backward
    B = 16
    sc = _stack(B, nbox, pts, seed=1)
    count = torch.full((B,), sc.nc, dtype=torch.int32)
    cot = torch.randn(B, sc.nb, 3, generator=torch.Generator().manual_seed(5), dtype=torch.float32)
    scg, cb, a = _solve(sc, count, pinned=True)
    assert _tag(a["ws"], B, sc.nb, sc.nc, 3) == TAG_PRIMAL_WG
    ga = _backward(sc, scg, cb, a, cot)
    for k, v in ga.items():
        assert bool(torch.isfinite(v).all()), k
    keys = ["Mdiag", "v", "f"] + (["rest", "fric", "c_n", "c_p1", "c_p2", "Je"] if pts == 1 else [])
    # the oracle's dense backward at its own solution, contracted through the assembly (tests/parity.py)
    ph = {k: v.double() if v.is_floating_point() else v for k, v in sc.phys_dict().items()}
    ref = {k: [] for k in parity.PHYS_KEYS + ["Je"]}
    for s in range(B):
        lcp64 = _oracle_lcp(sc, s, sc.nc)
        rs = O.lcp_forward(*lcp64)
        g = O.lcp_backward(rs, *lcp64, -cot[s:s + 1].double().reshape(1, -1))
        dense = {"Q": g["dQ"], "p": g["dp"], "G": g["dG"], "h": g["dh"], "F": g["dF"]}
        one = {k: (v[s:s + 1] if torch.is_tensor(v) else v) for k, v in ph.items()}
        pg = parity.physical_grads(one, sc.dt, dense, O)
        for k in parity.PHYS_KEYS:
            ref[k].append(pg[k])
        ref["Je"].append(g["dA"])
    ref = {k: torch.cat(v) for k, v in ref.items()}
    err = _grad_err(ga, ref, keys)
    print(nbox, pts, "gradients against the oracle (scaled max):", err)
    _, cbg, g_out = _solve(sc, count, path="generic", pinned=True)
    gg = _backward(sc, scg, cbg, g_out, cot)
    print(nbox, pts, "generic kernels' gradients against the oracle:", _grad_err(gg, ref, keys))
    for k in keys:
        assert err[k] <= (1e-5 if k in ("Mdiag", "v", "f") else 1e-4), (k, err[k])
    # a backward planned for another family finds the primal_wg tag: NaN gradients
    from lcp_physics_amd import _lib
    bad = dict(a)
    bad["compute"] = a["compute"] | _lib.PATH_GENERIC
    gb = solve_dynamics_backward(B, sc.nb, sc.nc, 3, scg.Mdiag, scg.v, scg.f, scg.rest, scg.fric, cb, scg.Je, sc.dt, cot.to(DEV), bad)
    torch.cuda.synchronize()
    assert bool(torch.isnan(gb["v"]).all())


@pytest.mark.gpu
def test_bitwise_reproducible_across_launches_and_batch_positions():
    B = 64
    sc = _stack(B, 30, 2, seed=2)
    for name in ("Mdiag", "v", "f", "rest", "fric", "c_n", "c_p1", "c_p2", "c_i1", "c_i2", "Je"):
        t = getattr(sc, name)
        t[37] = t[0]
        t[B - 1] = t[0]
    count = torch.full((B,), sc.nc, dtype=torch.int32)
    cot = torch.randn(1, sc.nb, 3, generator=torch.Generator().manual_seed(8), dtype=torch.float32).expand(B, -1, -1).contiguous()
    scg, cb, a = _solve(sc, count, pinned=True)
    ga = _backward(sc, scg, cb, a, cot)
    _, cb2, b = _solve(sc, count, pinned=True)
    gb = _backward(sc, scg, cb2, b, cot)
    for k in ("v_new", "z", "s", "y", "iters", "status"):
        assert torch.equal(a[k], b[k]), k
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    v = a["v_new"]
    assert torch.equal(v[0], v[37]) and torch.equal(v[0], v[B - 1])
    for k in ga:
        assert torch.equal(ga[k][0], ga[k][37]) and torch.equal(ga[k][0], ga[k][B - 1]), k


@pytest.mark.gpu
def test_contact_world_of_40_bodies_runs_on_the_workgroup_kernels():
    """A 40-body ContactWorld pile (floor + circles / rects / 12-gons, maxc = 128) on tag 13: follows the CPU oracle for 8 steps,
    its 4-step differentiable roll-out matches central differences of the oracle, and world.run() (HIP graph replay) equals
    world.step() in a loop."""
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from tests.test_hip_wide_contacts import _geom, _oracle_rollout, _pile_world
    B, nb, maxc = 2, 40, 128
    shapes, pose, Mdiag, f, rest, fric, Je = _pile_world(B, nb)
    geom = _geom([shapes] * B, max_verts=None)
    rep = lambda a, dt_: torch.tensor(np.broadcast_to(a, (B,) + a.shape).copy(), dtype=dt_, device=DEV)

    def make():
        return ContactWorld(geom, rep(pose, torch.float64), rep(np.zeros_like(pose), torch.float32), rep(Mdiag, torch.float32),
                            rep(f, torch.float32), rep(rest, torch.float32), rep(fric, torch.float32), Je=rep(Je, torch.float32),
                            maxc=maxc)
    world = make()
    nsteps = 8
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    p_ref, v_ref, t_ref, sets = _oracle_rollout(shapes, pose, f32(Mdiag), f32(f), f32(rest), f32(fric), f32(Je), nsteps)
    for _ in range(nsteps):
        world.step()
    torch.cuda.synchronize()
    assert _tag(world._ws, B, nb, maxc, 3) == TAG_PRIMAL_WG
    assert len(sets[-1]) >= 8
    for s in range(B):
        assert abs(float(world.t[s]) - t_ref) < 1e-12 and int(world.contacts.count[s]) == len(sets[-1]), s
        assert np.abs(world.p[s].cpu().numpy() - p_ref).max() < 2e-4 and np.abs(world.v[s].double().cpu().numpy() - v_ref).max() < 2e-3, s

    # graph replay against a loop of steps
    w1, w2 = make(), make()
    w1.run(6, graph=True)
    for _ in range(6):
        w2.step()
    torch.cuda.synchronize()
    assert torch.equal(w1.p, w2.p) and torch.equal(w1.v, w2.v)

    # differentiable roll-out: d(w . p_final)/d(p0) against central differences of the oracle
    nroll = 4
    w = np.random.default_rng(3).standard_normal((nb, 3))
    w[0] = 0.0
    v0 = np.zeros((nb, 3))
    spin = np.random.default_rng(4)
    v0[1:, 0] = spin.uniform(0.02, 0.05, nb - 1) * spin.choice([-1.0, 1.0], nb - 1)
    v0 = v0.astype(np.float32).astype(np.float64)
    p0 = rep(pose, torch.float64).requires_grad_(True)
    world.restart(p0, v=rep(v0, torch.float32))
    for _ in range(nroll):
        world.step(differentiable=True)
    loss = (world.p * torch.tensor(w, device=DEV)).sum(dim=(1, 2))
    loss.sum().backward()
    torch.cuda.synchronize()
    assert _tag(world._ws, B, nb, maxc, 3) == TAG_PRIMAL_WG
    grad = p0.grad[0].cpu().numpy()
    base = _oracle_rollout(shapes, pose, f32(Mdiag), f32(f), f32(rest), f32(fric), f32(Je), nroll, v0=v0)
    rng = np.random.default_rng(9)
    touched = sorted({b for st in base[3] for pr in st for b in pr} - {0})
    cand = [(b, c) for b in touched for c in range(3)]
    checked, worst = 0, 0.0
    for i in rng.permutation(len(cand))[:8]:
        b, c = cand[i]
        h = 1e-5 if c == 0 else 1e-4
        vals = []
        for sgn in (1, -1):
            q = pose.copy()
            q[b, c] += sgn * h
            r = _oracle_rollout(shapes, q, f32(Mdiag), f32(f), f32(rest), f32(fric), f32(Je), nroll, v0=v0)
            if r[3] != base[3] or r[2] != base[2]:
                break
            vals.append(float((r[0] * w).sum()))
        if len(vals) < 2:
            continue
        fd = (vals[0] - vals[1]) / (2 * h)
        worst = max(worst, abs(grad[b, c] - fd) / max(abs(fd), 1.0))
        checked += 1
    print("40-body roll-out gradient on the workgroup kernels: %d coordinates, worst relative error %.2e" % (checked, worst))
    assert checked >= 4 and worst <= 2e-3


def test_unit_assembly_has_no_calls_and_no_scratch():
    """no s_swappc_b64 and a zero private segment in the unit's device assembly."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the device assembly is not built here")
    files = glob.glob(os.path.join(CSRC, "asm", "lcp_primal_wg*.fixed.s"))
    if not files:
        pytest.skip("lcp_primal_wg.o not built")
    for fn in files:
        text = open(fn).read()
        assert "s_swappc_b64" not in text, fn
        sizes = [int(l.split(":")[1]) for l in text.splitlines() if l.strip().startswith(".private_segment_fixed_size:")]
        assert sizes and all(s == 0 for s in sizes), (fn, sizes)
