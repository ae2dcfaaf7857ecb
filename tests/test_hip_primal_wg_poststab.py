"""Post-stabilisation on the workgroup-per-scene body-space kernels (`lcp_primal_wg_poststab.hip`: one workgroup of 256 threads
per scene, the fp64 system of up to 128 pivots in LDS) behind `lcp_post_stabilization_f32` / `lcp_post_stabilization_backward_f32`
at the sizes beyond one wavefront (21-41 bodies, 65-256 contact slots; automatic mode from three contact slots per two bodies on,
`set_path("primal_wg")` wherever the kernels fit).  Checked against the generic contact-space kernels they replace there
(`set_path("generic")`, the A/B partner) and against the fp64 oracle.

Iteration counts are never asserted equal at the default `max_iter`: a converged solve of this LCP leaves the exit tests of
pdipm.py:133 comparing rounding noise, and two eliminations of one Newton trajectory stop a pass apart on a third of the scenes.
The backward is compared like for like at `max_iter = 5`, where no scene has converged and both families keep the same iterate."""
import glob
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import pdipm_oracle as O
from tests.test_hip_primal_wg import _grad_err, _tag

DEV = "cuda"
TAG_WG, TAG_ONE_WAVE, TAG_GENERIC = 14, 10, 11
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lcp_physics_amd", "csrc")


def _scenes(B, nbox, pts):
    """The scenes every test here shares: a stack with perturbed velocities (so that the contacts have something to correct) and
    ragged contact counts, the first half of the batch full."""
    from lcp_physics_amd import scenes
    sc = scenes.make_stack_scenes(B=B, nbox=nbox, pts_per_interface=pts, seed=1400 + 5 * nbox + pts, dtype=torch.float32)
    sc.v = sc.v + 0.3 * torch.randn(sc.v.shape, generator=torch.Generator().manual_seed(1))
    count = torch.randint(1, sc.nc + 1, (B,), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    count[:B // 2] = sc.nc
    return sc, count


def _pad(sc, maxc):
    pad = maxc - sc.nc
    for name in ("c_n", "c_p1", "c_p2"):
        setattr(sc, name, torch.cat([getattr(sc, name), torch.zeros(sc.B, pad, 2)], dim=1))
    for name in ("c_i1", "c_i2"):
        setattr(sc, name, torch.cat([getattr(sc, name), torch.zeros(sc.B, pad, dtype=torch.int32)], dim=1))


def _run(sc, count, path="auto", poses=None, **kw):
    """One forward on `path`; returns (device scenes, contact buffers, out)."""
    from lcp_physics_amd import _lib
    from lcp_physics_amd.physics.batched_world import post_stabilization
    from lcp_physics_amd.physics.contacts import ContactBuffers
    scg = sc.to(device=DEV)
    maxc = sc.c_n.shape[1]
    cb = ContactBuffers(sc.B, sc.nb, maxc, DEV)
    cb.c_n, cb.c_p1, cb.c_p2, cb.c_i1, cb.c_i2 = scg.c_n, scg.c_p1, scg.c_p2, scg.c_i1, scg.c_i2
    pose = {} if poses is None else {"p": poses[0], "dt_scene": poses[1], "p_out": poses[2]}
    _lib.set_path(path)
    try:
        out = post_stabilization(sc.B, sc.nb, maxc, 3, count.to(DEV), scg.Mdiag, scg.v, scg.rest, cb, scg.Je, **pose, **kw)
        torch.cuda.synchronize()
    finally:
        _lib.set_path("auto")
    return scg, cb, out


def _bwd(sc, scg, cb, out, cot):
    from lcp_physics_amd.physics.batched_world import post_stabilization_backward
    g = post_stabilization_backward(sc.B, sc.nb, sc.c_n.shape[1], 3, scg.Mdiag, scg.v, scg.rest, cb, scg.Je, cot.to(DEV), out, want_Je=True)
    torch.cuda.synchronize()
    return {k: v.double().cpu() for k, v in g.items()}


def _scaled(a, b):
    """max |a - b| of every scene over max(1, max |b|)."""
    B = a.shape[0]
    a, b = a.double().cpu().reshape(B, -1), b.double().cpu().reshape(B, -1)
    return (a - b).abs().max(dim=1)[0] / b.abs().max(dim=1)[0].clamp_min(1.0)


@pytest.mark.gpu
def test_routing_reaches_the_workgroup_post_stabilization_kernels():
    """31 bodies / 60 contacts and 13 bodies / 66 padded slots: tag 14 in automatic mode, tag 11 under set_path("generic").
    20 bodies (63 rows: the largest world of the one-wave kernels): tag 10 in automatic mode, tag 14 under set_path("primal_wg");
    21 bodies (66 rows, beyond one wavefront): tag 14 either way; 31 / 41 bodies with one contact slot per body: tag 11 in
    automatic mode (the generic kernels are as fast there), tag 14 under set_path("primal_wg")."""
    from lcp_physics_amd import _lib
    lib = _lib.load()
    for nbox, pts, maxc in ((30, 2, 60), (12, 4, 66)):
        sc, count = _scenes(4, nbox, pts)
        if sc.nc < maxc:
            _pad(sc, maxc)
        assert lib.lcp_post_stabilization_has_backward(sc.nb, maxc, 3, _lib.COMPUTE_F64) == 1
        _, _, a = _run(sc, count)
        assert _tag(a["ws"], sc.B, sc.nb, maxc, 3) == TAG_WG, (nbox, maxc)
        _, _, b = _run(sc, count, path="generic")
        assert _tag(b["ws"], sc.B, sc.nb, maxc, 3) == TAG_GENERIC, (nbox, maxc)
    # (30, 1) / (40, 1): one contact slot per body - automatic mode stays on the generic kernels (no faster there), the switch forces
    for nbox, pts, auto_tag in ((19, 2, TAG_ONE_WAVE), (20, 2, TAG_WG), (30, 1, TAG_GENERIC), (40, 1, TAG_GENERIC)):
        sc, count = _scenes(4, nbox, pts)
        assert sc.nb == nbox + 1
        assert lib.lcp_post_stabilization_has_backward(sc.nb, sc.nc, 3, _lib.COMPUTE_F64) == 1
        assert lib.lcp_post_stabilization_has_backward(sc.nb, sc.nc, 3, _lib.COMPUTE_F64 | _lib.PATH_PRIMAL_WG) == 1
        _, _, a = _run(sc, count)
        assert _tag(a["ws"], sc.B, sc.nb, sc.nc, 3) == auto_tag, nbox
        _, _, b = _run(sc, count, path="primal_wg")
        assert _tag(b["ws"], sc.B, sc.nb, sc.nc, 3) == TAG_WG, nbox
        _, _, c = _run(sc, count, path="generic")
        assert _tag(c["ws"], sc.B, sc.nb, sc.nc, 3) == TAG_GENERIC, nbox


def _forward_checks(sc, count, path, label, oracle_every=8):
    """The new family on `path` against the generic kernels on every scene and against the oracle on every `oracle_every`-th."""
    from lcp_physics_amd import _lib
    B, nc = sc.B, sc.nc
    p = torch.randn(B, sc.nb, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(DEV)
    dts = (0.01 + 0.02 * torch.rand(B, generator=torch.Generator().manual_seed(4), dtype=torch.float64)).to(DEV)
    pa, pb = torch.empty_like(p), torch.empty_like(p)
    _, _, a = _run(sc, count, path=path, poses=(p, dts, pa))
    assert _tag(a["ws"], B, sc.nb, nc, 3) == TAG_WG
    _, _, b = _run(sc, count, path="generic", poses=(p, dts, pb))
    assert _tag(b["ws"], B, sc.nb, nc, 3) == TAG_GENERIC
    err = _scaled(a["dp"], b["dp"])
    di = (a["iters"].cpu() - b["iters"].cpu()).abs()
    print(label, "worst scaled |dp - dp(generic)| %.2e, moved poses %.2e, iteration counts differ on %d of %d (at most by %d)" % (
        float(err.max()), float((pa - pb).abs().max()), int((di != 0).sum()), B, int(di.max())))
    assert float(err.max()) <= 1e-5
    assert float((pa - pb).abs().max()) <= 1e-5
    move = p + (a["dp"].double() * 0.5) * dts.reshape(B, 1, 1)           # world.py:110-117 (the kernel moves with its fp64 dp)
    assert float((pa - move).abs().max()) <= 1e-7
    loud = _lib.ST_NAN | _lib.ST_TRUNCATED
    assert torch.equal(a["status"].cpu() & loud, b["status"].cpu() & loud)
    assert int(di.max()) <= 4
    da, db = a["dp"].double().cpu(), b["dp"].double().cpu()
    worst_a = worst_b = 0.0
    for k in range(B):
        n = min(int(count[k]), nc)
        if n == 0:                                            # engines.py:92-103: x = [M -Je^T; Je 0]^-1 [0; Je v]
            nz = 3 * sc.nb
            Md, Je = sc.Mdiag[k].reshape(-1).double(), sc.Je[k].double()
            K = torch.zeros(nz + 3, nz + 3, dtype=torch.float64)
            K[:nz, :nz], K[:nz, nz:], K[nz:, :nz] = torch.diag(Md), -Je.T, Je
            x = torch.linalg.solve(K, torch.cat([torch.zeros(nz, dtype=torch.float64), Je @ sc.v[k].reshape(-1).double()]))[:nz]
            e0 = float((-da[k].reshape(-1) - x).abs().max() / x.abs().max().clamp_min(1.0))
            print(label, "scene", k, "without contacts: scaled error against the direct solve %.2e" % e0)
            assert e0 <= 1e-6
            assert int(a["iters"][k]) == 0
            continue
        if k % oracle_every:
            continue
        one = lambda t: t[k:k + 1].double()
        lcp = O.assemble_post_stabilization(one(sc.Mdiag), one(sc.v), one(sc.c_n[:, :n]), one(sc.c_p1[:, :n]), one(sc.c_p2[:, :n]),
                                            sc.c_i1[k:k + 1, :n], sc.c_i2[k:k + 1, :n], one(sc.rest), one(sc.Je))
        ref = -O.lcp_forward(*lcp).x.reshape(1, -1)
        ea, eb = float(_scaled(da[k:k + 1], ref)), float(_scaled(db[k:k + 1], ref))
        worst_a, worst_b = max(worst_a, ea), max(worst_b, eb)
        # (both are fp64 solves of one Newton trajectory: within a factor 2 of each other; 1e-6: the fp32 store)
        assert ea <= 1e-6 + 2.0 * eb, (k, n, ea, eb)
    print(label, "worst scaled error against the oracle: workgroup kernels %.2e, generic kernels %.2e" % (worst_a, worst_b))
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("nbox,pts,path", [(19, 2, "primal_wg"), (20, 2, "primal_wg"), (30, 1, "primal_wg"), (30, 2, "auto"), (40, 1, "primal_wg"),
                                            (40, 2, "auto")])
def test_forward_matches_the_generic_kernels_and_the_oracle(nbox, pts, path):
    """B = 256 with poses and per-scene dt, ragged counts, one scene without contacts and one whose count exceeds the capacity.
    (19, 2): a size of the one-wave kernels, forced onto the workgroup kernels (the A/B switch); one point per interface (one
    contact slot per body): automatic mode keeps these sizes on the generic kernels, which are as fast there - forced as well."""
    from lcp_physics_amd import _lib
    B = 256
    sc, count = _scenes(B, nbox, pts)
    count[B // 2 + 3] = 0
    count[B // 2 + 5] = sc.nc + 5
    a, _ = _forward_checks(sc, count, path, "(%d, %d)" % (nbox, pts))
    st = a["status"].cpu()
    assert int(st[B // 2 + 5]) & _lib.ST_TRUNCATED and int(((st & _lib.ST_TRUNCATED) != 0).sum()) == 1
    assert int((st & _lib.ST_NAN).sum()) == 0


def _oracle_grads(sc, k, n, cot, max_iter):
    """The oracle's gradients of scene k with n contacts: lcp.py:37-64 at its own iterate, autograd through the assembly."""
    leaf = lambda t: t[k:k + 1].double().clone().requires_grad_(True)
    Md, v, rest, Je = leaf(sc.Mdiag), leaf(sc.v), leaf(sc.rest), leaf(sc.Je)
    cn, cp1, cp2 = leaf(sc.c_n[:, :n]), leaf(sc.c_p1[:, :n]), leaf(sc.c_p2[:, :n])
    cx = -cot[k:k + 1].double().reshape(1, -1)                                  # dp = -x
    lcp = O.assemble_post_stabilization(Md, v, cn, cp1, cp2, sc.c_i1[k:k + 1, :n], sc.c_i2[k:k + 1, :n], rest, Je)
    det = [None if t is None else t.detach() for t in lcp]
    sol = O.lcp_forward(*det, max_iter=max_iter)
    gr = O.lcp_backward(sol, *det, cx)
    outs, cots = [], []
    for t, key in zip(lcp, ("dQ", "dp", "dG", "dh", "dA", "db", "dF")):
        if t is not None and t.requires_grad and gr[key] is not None:
            outs.append(t); cots.append(gr[key])
    torch.autograd.backward(outs, cots)
    padded = lambda g: torch.cat([g, torch.zeros(1, sc.nc - n, 2, dtype=torch.float64)], dim=1)
    return {"Mdiag": Md.grad, "v": v.grad, "rest": rest.grad, "Je": Je.grad, "c_n": padded(cn.grad), "c_p1": padded(cp1.grad),
            "c_p2": padded(cp2.grad)}, int(sol.iters[0]) if torch.is_tensor(sol.iters) else int(sol.iters)


GRAD_KEYS = ("Mdiag", "v", "rest", "Je", "c_n", "c_p1", "c_p2")
GRAD_BOUND = {"Mdiag": 1e-5, "v": 1e-5, "rest": 1e-4, "Je": 1e-4, "c_n": 1e-4, "c_p1": 1e-4, "c_p2": 1e-4}


@pytest.mark.gpu
@pytest.mark.parametrize("nbox,pts", [(30, 1), (40, 1), (30, 2), (40, 2)])
def test_backward_matches_the_generic_backward_and_the_oracle(nbox, pts):
    """Like for like at max_iter = 5: no scene has converged, both families keep the iterate of the fifth pass."""
    from lcp_physics_amd import _lib
    from lcp_physics_amd.physics.batched_world import post_stabilization_backward
    B = 32
    sc, count = _scenes(B, nbox, pts)
    nc = sc.nc
    cot = torch.randn(B, sc.nb, 3, generator=torch.Generator().manual_seed(6), dtype=torch.float32)
    path = "auto" if pts > 1 else "primal_wg"                  # (one slot per body: automatic mode keeps the generic kernels)
    scg, cb, a = _run(sc, count, path=path, max_iter=5)
    assert _tag(a["ws"], B, sc.nb, nc, 3) == TAG_WG
    ga = _bwd(sc, scg, cb, a, cot)
    scg2, cb2, b = _run(sc, count, path="generic", max_iter=5)
    assert _tag(b["ws"], B, sc.nb, nc, 3) == TAG_GENERIC
    gg = _bwd(sc, scg2, cb2, b, cot)
    print((nbox, pts), "iterations: workgroup", sorted(set(a["iters"].cpu().tolist())), "generic", sorted(set(b["iters"].cpu().tolist())))
    assert bool((a["iters"] == 5).all()) and bool((b["iters"] == 5).all())
    err = _grad_err(ga, gg, GRAD_KEYS)
    print((nbox, pts), "gradients against the generic backward (scaled max):", {k: "%.1e" % v for k, v in err.items()})
    for k in GRAD_KEYS:
        assert bool(torch.isfinite(ga[k]).all()), k
        assert err[k] <= GRAD_BOUND[k], (k, err[k])
    for k in range(B):                                        # padded slots of the frame gradients: exactly 0
        n = int(count[k])
        if n < nc:
            for key in ("c_n", "c_p1", "c_p2"):
                assert float(ga[key][k, n:].abs().max()) == 0.0, (k, key)
    # the oracle on four scenes (two full lists, two ragged ones)
    pick = [0, 1, B // 2, B - 1]
    refs = [_oracle_grads(sc, k, int(count[k]), cot, 5) for k in pick]
    assert all(it == 5 for _, it in refs)
    ref = {key: torch.cat([r[key] for r, _ in refs]) for key in GRAD_KEYS}
    ea = _grad_err({k: v[pick] for k, v in ga.items()}, ref, GRAD_KEYS)
    eg = _grad_err({k: v[pick] for k, v in gg.items()}, ref, GRAD_KEYS)
    print((nbox, pts), "against the oracle: workgroup", {k: "%.1e" % v for k, v in ea.items()}, "generic", {k: "%.1e" % v for k, v in eg.items()})
    for k in GRAD_KEYS:
        # (where the generic backward itself is farther from the oracle than the bound: at most twice as far)
        assert ea[k] <= (GRAD_BOUND[k] if eg[k] <= GRAD_BOUND[k] else 2.0 * eg[k]), (k, ea[k], eg[k])
    # default max_iter: finite gradients
    scg3, cb3, c = _run(sc, count, path=path)
    gc = _bwd(sc, scg3, cb3, c, cot)
    for k, v in gc.items():
        assert bool(torch.isfinite(v).all()), k
    # a backward planned for the generic kernels finds the workgroup family's tag: NaN gradients
    bad = dict(c)
    bad["compute"] = (c["compute"] & ~_lib.PATH_PRIMAL_WG) | _lib.PATH_GENERIC
    gb = post_stabilization_backward(B, sc.nb, nc, 3, scg3.Mdiag, scg3.v, scg3.rest, cb3, scg3.Je, cot.to(DEV), bad)
    torch.cuda.synchronize()
    assert bool(torch.isnan(gb["v"]).all())


@pytest.mark.gpu
def test_bitwise_reproducible_across_launches_and_batch_positions():
    B = 64
    sc, count = _scenes(B, 30, 2)
    for name in ("Mdiag", "v", "rest", "c_n", "c_p1", "c_p2", "c_i1", "c_i2", "Je"):
        t = getattr(sc, name)
        t[37] = t[0]
        t[B - 1] = t[0]
    count[37] = count[B - 1] = count[0]
    cot = torch.randn(1, sc.nb, 3, generator=torch.Generator().manual_seed(8), dtype=torch.float32).expand(B, -1, -1).contiguous()
    scg, cb, a = _run(sc, count)
    assert _tag(a["ws"], B, sc.nb, sc.nc, 3) == TAG_WG
    ga = _bwd(sc, scg, cb, a, cot)
    scg2, cb2, b = _run(sc, count)
    gb = _bwd(sc, scg2, cb2, b, cot)
    for k in ("dp", "iters", "status"):
        assert torch.equal(a[k], b[k]), k
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    d = a["dp"]
    assert torch.equal(d[0], d[37]) and torch.equal(d[0], d[B - 1])
    for k in ga:
        assert torch.equal(ga[k][0], ga[k][37]) and torch.equal(ga[k][0], ga[k][B - 1]), k


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["moving_floor", "scaled"])
def test_moving_floor_and_general_equality_rows(rows):
    """b = Je v != 0 (the pinned body has a velocity) and A = 2 [I 0]: the general form takes both."""
    B = 64
    sc, count = _scenes(B, 30, 1)
    if rows == "moving_floor":
        sc.v[:, 0] = 0.05 * torch.randn(B, 3, generator=torch.Generator().manual_seed(5))
        assert float(sc.v[:, 0].abs().min()) > 0.0
    else:
        sc.Je = sc.Je * 2.0
    _forward_checks(sc, count, "primal_wg", "(30, 1) " + rows)


@pytest.mark.gpu
def test_contact_world_of_40_bodies_with_post_stabilization():
    """`ContactWorld(post_stab=True)` at 40 bodies / maxc = 128: the correction runs on tag 14, follows the same world on the
    generic kernels, replays from a HIP graph bitwise and differentiates."""
    from lcp_physics_amd import _lib
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from tests.test_hip_wide_contacts import _geom, _pile_world
    B, nb, maxc = 2, 40, 128
    shapes, pose, Mdiag, f, rest, fric, Je = _pile_world(B, nb)
    geom = _geom([shapes] * B, max_verts=None)
    rep = lambda a, dt_: torch.tensor(np.broadcast_to(a, (B,) + a.shape).copy(), dtype=dt_, device=DEV)

    def make():
        return ContactWorld(geom, rep(pose, torch.float64), rep(np.zeros_like(pose), torch.float32), rep(Mdiag, torch.float32),
                            rep(f, torch.float32), rep(rest, torch.float32), rep(fric, torch.float32), Je=rep(Je, torch.float32),
                            maxc=maxc, post_stab=True)

    def rollout(w, p0):
        v0 = np.zeros((nb, 3))
        spin = np.random.default_rng(4)
        v0[1:, 0] = spin.uniform(0.02, 0.05, nb - 1) * spin.choice([-1.0, 1.0], nb - 1)
        w.restart(p0, v=rep(v0.astype(np.float32), torch.float32))
        for _ in range(3):
            w.step(differentiable=True)
        wt = np.random.default_rng(3).standard_normal((nb, 3))
        wt[0] = 0.0
        (w.p * torch.tensor(wt, device=DEV)).sum().backward()
        torch.cuda.synchronize()
        return p0.grad.cpu()

    world = make()
    for _ in range(6):
        world.step()
    torch.cuda.synchronize()
    assert _tag(world._ps_ws, B, nb, maxc, 3) == TAG_WG
    p6, v6, n6, t6 = world.p.clone(), world.v.clone(), world.contacts.count.clone(), world.t.clone()
    _lib.set_path("generic")
    try:
        other = make()
        for _ in range(6):
            other.step()
        torch.cuda.synchronize()
        assert _tag(other._ps_ws, B, nb, maxc, 3) == TAG_GENERIC
        assert torch.equal(n6, other.contacts.count) and torch.equal(t6, other.t)
        ep, ev = float((p6 - other.p).abs().max()), float((v6.double() - other.v.double()).abs().max())
        g_gen = rollout(other, rep(pose, torch.float64).requires_grad_(True))
    finally:
        _lib.set_path("auto")
    print("40-body world with post-stabilisation, six steps against the generic kernels: |p - p'| %.2e, |v - v'| %.2e" % (ep, ev))
    assert ep <= 2e-4 and ev <= 2e-3
    w1 = make()
    w1.run(6, graph=True)
    torch.cuda.synchronize()
    assert torch.equal(w1.p, p6) and torch.equal(w1.v, v6)
    g = rollout(world, rep(pose, torch.float64).requires_grad_(True))
    assert bool(torch.isfinite(g).all())
    eg = float(((g - g_gen).abs() / g_gen.abs().clamp_min(1.0)).max())
    print("3-step differentiable roll-out: worst relative difference of d(loss)/d(p0) from the generic path %.2e" % eg)
    assert eg <= 2e-3


def test_unit_assembly_has_no_calls_and_no_scratch():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the device assembly is not built here")
    files = glob.glob(os.path.join(CSRC, "asm", "lcp_primal_wg_poststab*.fixed.s"))
    if not files:
        pytest.skip("lcp_primal_wg_poststab.o not built")
    for fn in files:
        text = open(fn).read()
        assert "s_swappc_b64" not in text, fn
        sizes = [int(l.split(":")[1]) for l in text.splitlines() if l.strip().startswith(".private_segment_fixed_size:")]
        assert sizes and all(s == 0 for s in sizes), (fn, sizes)
