"""GPU: fixed-interval stepping, `ContactWorld.step(fixed_dt=True)` = the reference's `World.step(fixed_dt=True)`
(physics/world.py:72-80) for a batch - the per-scene dt of the detection kernels (`lcp_move_find_contacts_dts_f64`), the
sub-step bookkeeping kernels (lcp_substep.hip), the arithmetic the design rests on, and whole trajectories, roll-outs and
gradients against the unmodified reference (tests/golden/fixed_dt.npz, tools/gen_fixed_dt_golden.py)."""
import numpy as np
import pytest
import torch

from oracle import contacts_oracle as C
from oracle import world_oracle as W
from tests.fixed_dt_io import load_fixed_dt
from tests.test_hip_contacts import _compare_lists, _geom, _random_scene
from tests.world_io import shapes_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = 1.0 / 30
RECORDS = ("c_n", "c_p1", "c_p2", "c_pen", "c_i1", "c_i2", "count", "max_pen", "dt_used", "trials")


def _bits(a, b):
    """Bitwise equality of two tensors (NaN-safe, sign-of-zero-strict)."""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(-1).view(torch.uint8), b.view(-1).view(torch.uint8))


# ---------------------------------------------------------------------------------------------- per-scene dt in the detection
def _thrown_scenes(nb, B, seed=11):
    """The scenes of tests/test_hip_contacts.py::test_move_and_halve_matches_oracle at other sizes: bodies lifted clear of each other
    and thrown down, so that most scenes penetrate at the full dt."""
    rng = np.random.default_rng(seed)
    scenes = [_random_scene(rng, nb, hulls=False, rotate=False) for _ in range(B)]
    p0 = np.stack([s[1] for s in scenes])
    p0[:, 1:, 2] -= rng.uniform(0.5, 3.0, size=(B, nb - 1)).cumsum(axis=1)
    v = np.zeros((B, nb, 3))
    v[:, 1:, 2] = rng.uniform(20, 120, size=(B, nb - 1))
    v[:, 1:, 1] = rng.uniform(-20, 20, size=(B, nb - 1))
    v[:, 1:, 0] = rng.uniform(-0.5, 0.5, size=(B, nb - 1))
    return scenes, p0, torch.tensor(v, dtype=torch.float32)


# nb = 3, B = 5: four scenes per wave plus a tail row; nb = 7: the <64, 16> instantiation; 33 bodies: lcp_contacts_wide.hip
SIZES = [(3, 5, 16), (7, 5, 32), (33, 3, 160)]


@pytest.mark.parametrize("nb,B,maxc", SIZES, ids=["nb3-quad-wave", "nb7-one-wave", "nb33-wide"])
@pytest.mark.parametrize("strict", [True, False])
def test_per_scene_dt_matches_the_oracle_scene_by_scene(nb, B, maxc, strict):
    """A DIFFERENT starting dt per scene - the full dt, 0, 1e-9 and fractions: accepted dt, trials, pose and records are those of
    `world_oracle.move_and_find` run on each scene with its own dt (the non-strict floor stays the world's dt / 4)."""
    from lcp_physics_amd.physics.contacts import move_and_find_contacts
    scenes, p0, v32 = _thrown_scenes(nb, B)
    geom = _geom([s[0] for s in scenes])
    assert geom.wide == (nb > 32)
    # (nb = 3, scene 0, non-strict: DT / 3 penetrates, DT / 6 < the WORLD's dt / 4 is accepted with the penetration - a floor taken
    #  from the sub-step's own dt would go on halving)
    dts = np.array([DT / 3, 0.0, 1e-9, DT, 0.7 * DT] if B == 5 else [DT, 0.0, 1e-9])
    t0 = np.linspace(0.5, 1.5, B)
    t = torch.tensor(t0, dtype=torch.float64, device=DEV)
    p_start = torch.tensor(p0, dtype=torch.float64, device=DEV)
    cb = move_and_find_contacts(geom, p_start, v32.to(DEV), DT, maxc=maxc, strict=strict, t=t,
                                dt_scene=torch.tensor(dts, dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    assert int(cb.count.max()) <= maxc
    for k in range(B):
        if dts[k] == 0.0:
            continue                                                     # (its own test below: the oracle's loop would spin)
        p_ref, ref, dt_ref, trials = W.move_and_find(scenes[k][0], p0[k], v32[k].double().numpy(), float(dts[k]), strict=strict,
                                                     dt_floor=DT / 4)
        assert int(cb.trials[k]) == trials, (k, int(cb.trials[k]), trials)
        assert float(cb.dt_used[k]) == dt_ref and float(t[k]) == t0[k] + dt_ref, (k, float(cb.dt_used[k]), dt_ref)
        assert np.abs(cb.p_out[k].cpu().numpy() - p_ref).max() < 1e-10
        _compare_lists(cb, k, ref, "strict=%s scene %d" % (strict, k))
    assert int(cb.trials.max()) > 1                                      # somebody halved


# the last and the first body count on either side of an instantiation of lcp_move_find_contacts_kernel: <16, 6> up to 6 bodies,
# <64, 16> up to 16, <64, MAXB> for 17 .. 32 (33 bodies: the wide kernel, above)
EDGE_SIZES = [(6, 5, 32), (16, 3, 96), (17, 3, 96), (32, 3, 160)]


@pytest.mark.parametrize("nb,B,maxc", SIZES + EDGE_SIZES,
                         ids=["nb3-quad-wave", "nb7-one-wave", "nb33-wide", "nb6-quad-wave-last", "nb16-one-wave-last", "nb17-maxb-first",
                              "nb32-maxb-last"])
def test_equal_per_scene_dts_are_bitwise_the_scalar_entry(nb, B, maxc):
    from lcp_physics_amd.physics.contacts import move_and_find_contacts
    scenes, p0, v32 = _thrown_scenes(nb, B)
    geom = _geom([s[0] for s in scenes])
    p_start, v = torch.tensor(p0, dtype=torch.float64, device=DEV), v32.to(DEV)
    for strict in (True, False):
        ta, tb = (torch.full((B,), 0.25, dtype=torch.float64, device=DEV) for _ in range(2))
        a = move_and_find_contacts(geom, p_start, v, DT, maxc=maxc, strict=strict, t=ta)
        b = move_and_find_contacts(geom, p_start, v, DT, maxc=maxc, strict=strict, t=tb,
                                   dt_scene=torch.full((B,), DT, dtype=torch.float64, device=DEV))
        torch.cuda.synchronize()
        assert int(a.count.max()) <= maxc
        assert int(a.trials.max()) > 1
        assert _bits(ta, tb) and _bits(a.p_out, b.p_out)
        for n in RECORDS:
            assert _bits(getattr(a, n), getattr(b, n)), (strict, n)


@pytest.mark.parametrize("nb,B,maxc", SIZES, ids=["nb3-quad-wave", "nb7-one-wave", "nb33-wide"])
def test_a_finished_scene_stays_where_it_is(nb, B, maxc):
    """dt = 0 (also -0.0 and a negative dt): p_out = p_start bitwise, t unchanged, dt_used = 0, one trial, the records of
    `find_contacts(p_start)` - also when that pose PENETRATES (strict mode would halve zero for ever), while its wave neighbours
    still halve."""
    from lcp_physics_amd.physics.contacts import find_contacts, move_and_find_contacts
    scenes, p0, v32 = _thrown_scenes(nb, B)
    p0 = p0.copy()
    p0[1, 1, 2] += 6.0                                                   # scene 1: its first body 3 - 6 deep in the floor
    p0[0, 1, 0] = -0.0                                                   # a negative zero must come back as one
    geom = _geom([s[0] for s in scenes])
    p_start, v = torch.tensor(p0, dtype=torch.float64, device=DEV), v32.to(DEV)
    dts = torch.tensor([0.0, 0.0, DT, DT, -0.0][:B], dtype=torch.float64, device=DEV)
    if B == 3:
        dts = torch.tensor([-1e-3, 0.0, DT], dtype=torch.float64, device=DEV)
    done = (dts <= 0).cpu()
    t0 = torch.linspace(0.5, 1.5, B, dtype=torch.float64, device=DEV)
    t0[1] = -0.0
    t = t0.clone()
    here = find_contacts(geom, p_start, maxc=maxc)
    cb = move_and_find_contacts(geom, p_start, v, DT, maxc=maxc, strict=True, t=t, dt_scene=dts)
    torch.cuda.synchronize()
    assert float(here.max_pen[1]) > 1e-6, "scene 1 does not penetrate at its start pose"
    assert int(cb.trials[~done].max()) > 1, "no neighbour halved"
    for k in torch.nonzero(done).flatten().tolist():
        assert _bits(cb.p_out[k], p_start[k]) and _bits(t[k], t0[k]), k
        assert float(cb.dt_used[k]) == 0.0 and int(cb.trials[k]) == 1
        for n in ("c_n", "c_p1", "c_p2", "c_pen", "c_i1", "c_i2", "count", "max_pen"):
            assert _bits(getattr(cb, n)[k], getattr(here, n)[k]), (k, n)
        ref = C.find_contacts(W.bodies_at(scenes[k][0], p0[k]), eps=0.1)
        _compare_lists(cb, k, ref, "finished scene %d" % k)
    for k in torch.nonzero(~done).flatten().tolist():                   # ... and the others are what they are without it
        p_ref, ref, dt_ref, trials = W.move_and_find(scenes[k][0], p0[k], v32[k].double().numpy(), float(dts[k]), strict=True, dt_floor=DT / 4)
        assert int(cb.trials[k]) == trials and float(cb.dt_used[k]) == dt_ref
        _compare_lists(cb, k, ref, "live scene %d" % k)


def test_dts_entry_checks_its_arguments_before_any_launch():
    from lcp_physics_amd import _lib
    from lcp_physics_amd.physics.contacts import ContactBuffers
    scenes, p0, v32 = _thrown_scenes(3, 2)
    geom = _geom([s[0] for s in scenes])
    B, nb, maxc = 2, 3, 8
    out = ContactBuffers(B, nb, maxc, DEV)
    p_start, v = torch.tensor(p0, dtype=torch.float64, device=DEV), v32.to(DEV)
    dts = torch.full((B,), DT, dtype=torch.float64, device=DEV)
    P = _lib.ptr

    def call(nb_=nb, nvcap=8, svm=0, dts_=dts):
        return _lib.load().lcp_move_find_contacts_dts_f64(
            B, nb_, maxc, nvcap, svm, P(geom.kind), P(geom.radius), P(geom.verts_local), P(geom.nverts), None, P(p_start), P(v), DT, DT / 4,
            1, 64, 0.1, 1e-6, P(out.p_out), P(out.c_n), P(out.c_p1), P(out.c_p2), P(out.c_pen), P(out.c_i1), P(out.c_i2), P(out.count),
            P(out.max_pen), P(out.dt_used), None, P(out.trials), P(dts_), _lib.stream_ptr(torch.device(DEV)))
    assert call(dts_=None) == -1                                          # LCP_E_BADARG: dt_scene is required
    assert call(nb_=65) == -2 and call(nvcap=7) == -2 and call(nvcap=65) == -2 and call(svm=1025) == -2    # the wide entry's limits
    assert call() == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- begin / commit
@pytest.mark.parametrize("B", [1, 5, 257])
def test_substep_begin_and_commit_are_bitwise_the_torch_expressions(B):
    from lcp_physics_amd.physics.batched_world import substep_begin, substep_commit
    nb = 3
    g = torch.Generator().manual_seed(B)
    t = torch.rand(B, generator=g, dtype=torch.float64)
    end_t = t + DT * torch.rand(B, generator=g, dtype=torch.float64)
    end_t[::3] = t[::3]                                                   # finished: t == end_t
    if B > 4:
        end_t[4] = t[4] - 1e-3                                           # ... and past it
    f = torch.randn(B, nb, 3, generator=g) * 100
    count = torch.randint(0, 9, (B,), generator=g, dtype=torch.int32)
    t, end_t, f, count = t.to(DEV), end_t.to(DEV), f.to(DEV), count.to(DEV)
    out = substep_begin(t, end_t, f, count)
    active = t < end_t
    dt_k = torch.where(active, end_t - t, torch.zeros_like(t))
    assert _bits(out["dt_k"], dt_k) and _bits(out["active"], active.to(torch.int32))
    assert _bits(out["count_eff"], torch.where(active, count, torch.zeros_like(count)))
    assert _bits(out["f_eff"], dt_k.to(torch.float32).reshape(B, 1, 1) * f)
    again = substep_begin(t, end_t, f, count, out={k: torch.full_like(x, -1) for k, x in out.items()})   # (into given buffers)
    assert all(_bits(again[k], out[k]) for k in out)
    v_old, v_new = torch.randn(B, nb, 3, generator=g).to(DEV), torch.randn(B, nb, 3, generator=g).to(DEV)
    want = torch.where(active.reshape(B, 1, 1), v_new, v_old)
    keep = v_old.clone()
    assert substep_commit(out["active"], v_old, v_new) is v_new
    assert _bits(v_new, want) and _bits(v_old, keep)
    assert bool(active.any()) or B == 1


def test_state_update_backward_gives_a_finished_scene_exactly_zero():
    """`lcp_state_update_backward_f64` at dt_used = 0 (a scene that was finished in a sub-step) with non-zero velocities and
    cotangents: g_v is exactly 0 - not NaN -, and the scenes beside it get scale * dt_used * (g_p + g_g)."""
    from lcp_physics_amd import _lib
    B, nb = 5, 3
    g = torch.Generator().manual_seed(4)
    g_p, g_g = (torch.randn(B, nb, 3, generator=g, dtype=torch.float64).to(DEV) for _ in range(2))
    v = (torch.randn(B, nb, 3, generator=g) + 3.0).to(DEV)
    dt_used = torch.tensor([DT, 0.0, DT / 2, 0.0, DT], dtype=torch.float64, device=DEV)
    g_v = torch.full((B, nb, 3), float("nan"), dtype=torch.float32, device=DEV)
    P = _lib.ptr
    rc = _lib.load().lcp_state_update_backward_f64(B, nb, 0, P(g_p), P(g_g), None, P(v), P(dt_used), 1.0, None, None, P(g_v),
                                                   _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    done = dt_used == 0
    assert bool((g_v[done] == 0).all())                                   # (tot * 0: a zero of either sign, never NaN)
    assert _bits(g_v[~done], ((g_p + g_g) * dt_used.reshape(B, 1, 1))[~done].to(torch.float32))


# ---------------------------------------------------------------------------------------------- the arithmetic the design rests on
@pytest.mark.parametrize("path,tag", [("quad", 4), ("solo", 4), ("primal", 6), ("primal_wg", 13), ("generic", 9)])
def test_solve_with_dt_equals_solve_with_the_force_premultiplied(path, tag):
    """Every contact-list family forms u = md * v + dt * f in fp32 with contraction off (lcp_device.h momentum_entry): the solve with
    (f, dt) and the solve with (fl(float(dt) * f), 1) are the same launch on the same bits.  The sub-steps rely on it (no per-scene
    dt inside the solve kernels)."""
    from lcp_physics_amd import scenes
    from lcp_physics_amd.physics.batched_world import solve_dynamics
    from lcp_physics_amd.physics.contacts import ContactBuffers
    B = 8
    sc = scenes.make_stack_scenes(B=B, nbox=2, pts_per_interface=4, seed=7, dtype=torch.float32).to(device=DEV)
    cb = ContactBuffers(B, sc.nb, sc.nc, DEV)
    cb.c_n, cb.c_p1, cb.c_p2, cb.c_i1, cb.c_i2 = sc.c_n, sc.c_p1, sc.c_p2, sc.c_i1, sc.c_i2
    cnt = torch.tensor([sc.nc, sc.nc, 0, sc.nc - 1, 3, sc.nc, 1, sc.nc], dtype=torch.int32, device=DEV)
    f = (sc.f + 3.0 * torch.randn(B, sc.nb, 3, generator=torch.Generator().manual_seed(2)).to(DEV)).contiguous()
    e = sc.Je.shape[1]
    for dt in (DT, 0.0123456789, 1e-3):
        a = solve_dynamics(B, sc.nb, sc.nc, e, cnt, sc.Mdiag, sc.v, f, sc.rest, sc.fric, cb, sc.Je, dt, path=path, pinned=True)
        f_eff = torch.tensor(dt, dtype=torch.float64).to(torch.float32).to(DEV) * f
        b = solve_dynamics(B, sc.nb, sc.nc, e, cnt, sc.Mdiag, sc.v, f_eff.contiguous(), sc.rest, sc.fric, cb, sc.Je, 1.0, path=path, pinned=True)
        torch.cuda.synchronize()
        tags = [int(o["ws"][-256:-252].cpu().numpy().view(np.int32)[0]) for o in (a, b)]
        assert tags == [tag, tag], (path, tags)
        assert bool(torch.isfinite(a["v_new"]).all())
        assert _bits(a["v_new"], b["v_new"]), (path, dt, float((a["v_new"] - b["v_new"]).abs().max()))


# ---------------------------------------------------------------------------------------------- trajectories of the reference
WORLDS, ROLLOUT = load_fixed_dt()


def _world_of(rec, B, k=0):
    from lcp_physics_amd.physics.batched_world import ContactWorld
    shapes = shapes_of(rec)
    nb = len(shapes)
    geom = _geom([shapes] * B)
    rep = lambda a, dt_: torch.tensor(np.broadcast_to(a, (B,) + a.shape).copy(), dtype=dt_, device=DEV)
    if rec["no_contact"].size:
        nocon = torch.zeros(B, nb, nb, dtype=torch.uint8, device=DEV)
        for i, j in rec["no_contact"].tolist():
            nocon[:, i, j] = 1
        geom.no_contact = nocon
    kw = {}
    if any(int(x) in (1, 2) for x in rec["jtype"]):
        from lcp_physics_amd.physics.joints import JointSet
        kw["joints"] = JointSet.from_arrays(rec["jtype"], rec["jb1"], rec["jb2"], rec["jr1"], rec["jrot1"], B).to(DEV)
    else:
        kw["Je"] = rep(rec["Je"], torch.float32)
    if float(np.abs(rec["f"] - rec["f_off"]).max()) > 0:                 # forces.py:14-18: on the per-scene clock, per sub-step
        f_on, f_off, t_switch = rep(rec["f"], torch.float32), rep(rec["f_off"], torch.float32), float(rec["t_switch"])
        kw["force_fn"] = lambda t: torch.where((t < t_switch).reshape(-1, 1, 1), f_on, f_off)
    return ContactWorld(geom, rep(rec["p"][k], torch.float64), rep(rec["v"][k], torch.float32), rep(rec["Mdiag"], torch.float32),
                        rep(rec["f"], torch.float32), rep(rec["rest"], torch.float32), rep(rec["fric"], torch.float32), dt=float(rec["dt"]),
                        eps=float(rec["eps"]), tol=float(rec["tol"]), strict_no_penetration=bool(rec["strict"]), maxc=8,
                        post_stab=bool(rec["post_stab"]), **kw)


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_fixed_dt_world_follows_the_reference(name):
    """`step(fixed_dt=True)` on B = 5 replicas against the unmodified reference's `world.step(fixed_dt=True)`, ONE free run per record
    (the three with post-stabilisation included), after every step: clocks to 1e-12, the sub-step count and the contact count exactly
    (every halving decision of every sub-step is the reference's), poses and velocities to 2e-4 - the bound of
    test_contact_world_follows_reference_trajectory for these scenes and step counts.  Measured worst over all ten records:
    pose 1.5e-5 (mixed_poststab), velocity 2.5e-5 (mixed_nonstrict)."""
    rec = WORLDS[name]
    B = 5
    world = _world_of(rec, B)
    assert world.contacts.count.cpu().tolist() == [int(rec["ncontacts"][0])] * B
    worst_p = worst_v = 0.0
    for k in range(1, len(rec["t"])):
        world.step(fixed_dt=True)
        t = world.t.cpu().numpy()
        ep = np.abs(world.p.cpu().numpy() - rec["p"][k]).max()
        ev = np.abs(world.v.double().cpu().numpy() - rec["v"][k]).max()
        worst_p, worst_v = max(worst_p, ep), max(worst_v, ev)
        print(name, "step", k, "sub-steps", world.substeps.tolist(), "reference", int(rec["nsub"][k - 1]), "|dp| %.2e |dv| %.2e" % (ep, ev))
        assert np.abs(t - rec["t"][k]).max() < 1e-12, (name, k, "t", t, rec["t"][k])
        assert world.substeps.cpu().tolist() == [int(rec["nsub"][k - 1])] * B, (name, k, "sub-steps")
        assert world.contacts.count.cpu().tolist() == [int(rec["ncontacts"][k])] * B, (name, k, "contact count")
        assert ep <= 2e-4 and ev <= 2e-4, (name, k, ep, ev)
    assert not bool(world.behind.any())
    print(name, "worst |dp|", worst_p, "worst |dv|", worst_v)


# ---------------------------------------------------------------------------------------------- the batched grad_demo
def _grad_demo_world(scenes_idx, rep=1, requires_grad=False):
    """The `grad_demo` scenes `scenes_idx` of part (b) of the fixture, `rep` replicas each (tests/test_hip_contacts.py::_rollout_world)."""
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.contacts import GeometryBatch
    d = ROLLOUT
    idx = np.repeat(np.asarray(scenes_idx), rep)
    B, nb = len(idx), d["rad"].shape[1]
    rp = lambda a, dt_: torch.tensor(a[idx], dtype=dt_, device=DEV)
    geom = GeometryBatch.from_shapes([("circle", float(r)) for r in d["rad"][0]], B)
    nocon = torch.zeros(B, nb, nb, dtype=torch.uint8)
    for i, j in d["no_contact"].tolist():
        nocon[:, i, j] = nocon[:, j, i] = 1
    geom.no_contact = nocon
    geom = geom.to(DEV)
    force0 = rp(d["force0"], torch.float32).requires_grad_(requires_grad)
    mult, t_push, pushed = float(d["mult"]), float(d["t_push"]), int(d["pushed_body"])
    z = torch.zeros(B, 1, 3, dtype=torch.float32, device=DEV)

    def force_fn(t):
        on = (t < t_push).to(torch.float32).unsqueeze(1)
        parts = [z] * nb
        parts[pushed] = (force0 * mult * on).unsqueeze(1)
        return torch.cat(parts, dim=1)

    world = ContactWorld(geom, rp(d["p0"], torch.float64), rp(d["v0"], torch.float32), rp(d["Mdiag"], torch.float32),
                         torch.zeros(B, nb, 3, device=DEV), rp(d["rest"], torch.float32), rp(d["fric"], torch.float32), Je=None,
                         dt=float(d["dt"]), maxc=2, force_fn=force_fn)
    return world, force0


STATE = ("p", "v", "t")
FRAME = ("c_n", "c_p1", "c_p2", "c_i1", "c_i2", "count")


def _snapshot(world):
    out = {n: getattr(world, n).detach().clone() for n in STATE}
    out.update({n: getattr(world.contacts, n).clone() for n in FRAME})
    return out


def test_a_scene_in_a_batch_is_bitwise_the_scene_alone():
    """The eight scenes in ONE batch finish the collision step after 2 .. 7 sub-steps; p, v, t and the contact records of every
    scene after every step are bitwise those of the same scene stepped alone (B = 1): a finished scene does not change while the
    others go on, and nobody's arithmetic depends on its neighbours."""
    nsteps = 8                                                           # (the collision is in steps 5 and 6)
    world, _ = _grad_demo_world(range(8))
    snaps, subs = [], []
    for _ in range(nsteps):
        world.step(fixed_dt=True)
        snaps.append(_snapshot(world))
        subs.append(world.substeps.cpu().numpy().copy())
    subs = np.stack(subs, 1)
    assert (subs == ROLLOUT["nsub"][:, :nsteps]).all(), subs
    assert any(len(set(subs[:, k].tolist())) > 2 for k in range(nsteps)), "the scenes never differ within a step"
    for s in range(8):
        alone, _ = _grad_demo_world([s])
        for k in range(nsteps):
            alone.step(fixed_dt=True)
            one = _snapshot(alone)
            for n in STATE + FRAME:
                assert _bits(one[n][0], snaps[k][n][s]), ("scene", s, "step", k, n)


def test_max_substeps_runs_without_synchronising_and_flags_the_scenes_behind():
    nsteps = 8
    a, _ = _grad_demo_world(range(8))
    for _ in range(nsteps):
        a.step(fixed_dt=True)
    b, _ = _grad_demo_world(range(8))
    b.step(fixed_dt=True, max_substeps=8)                                 # (the first call allocates: allocation may synchronise)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(nsteps - 1):
            b.step(fixed_dt=True, max_substeps=8)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    sa, sb = _snapshot(a), _snapshot(b)
    for n in STATE + FRAME:
        assert _bits(sa[n], sb[n]), n
    assert not bool(b.behind.any())
    b.assert_on_schedule()
    # two sub-steps are not enough for the collision step of six of the scenes (the fixture says which)
    c, _ = _grad_demo_world(range(8))
    first = int(np.argmax((ROLLOUT["nsub"] > 2).any(axis=0)))            # the first step somebody needs more than two in
    for _ in range(first):
        c.step(fixed_dt=True, max_substeps=2)
    assert not bool(c.behind.any())
    c.step(fixed_dt=True, max_substeps=2)
    want = ROLLOUT["nsub"][:, first] > 2
    assert 0 < want.sum() < 8
    assert c.behind.cpu().numpy().tolist() == want.tolist()
    with pytest.raises(RuntimeError, match="max_substeps"):
        c.assert_on_schedule()
    on_time = torch.tensor(~want, device=DEV)
    assert float((c.t[on_time] - a.dt * (first + 1)).abs().max()) < 1e-12 and bool((c.t[~on_time] < a.dt * (first + 1) - 1e-6).all())


def test_fixed_dt_run_from_a_graph_equals_the_eager_run():
    nsteps = 8
    a, _ = _grad_demo_world(range(8))
    for _ in range(nsteps):
        a.step(fixed_dt=True, max_substeps=8)
    b, _ = _grad_demo_world(range(8))
    b.run(nsteps, graph=True, fixed_dt=True, max_substeps=8)
    torch.cuda.synchronize()
    assert b._graphs and all(K == 8 for _, K in b._graphs), "nothing was captured"
    sa, sb = _snapshot(a), _snapshot(b)
    for n in STATE + FRAME:
        assert _bits(sa[n], sb[n]), n
    with pytest.raises(ValueError):
        b.run(2, graph=True, fixed_dt=True)
    # both modes on ONE world: fixed and plain runs alternate, the odd plain count flips the buffer parity between the two K = 8 runs, and
    # K = 9 is a second sub-step count on a world that already holds fixed-interval graphs.  Three plain steps are spent on the warm-up
    # (two) and the tail (one), so a five-step plain run follows to put a plain graph next to the fixed ones; the last run replays the
    # graph of the FIRST, across everything captured in between.
    runs = [(4, 8), (3, None), (4, 8), (4, 9), (5, None), (2, 8)]         # (steps, max_substeps; None: plain steps)
    a, _ = _grad_demo_world(range(8))
    b, _ = _grad_demo_world(range(8))
    for r, (n, K) in enumerate(runs):
        mode = {} if K is None else {"fixed_dt": True, "max_substeps": K}
        for _ in range(n):
            a.step(**mode)
            if K is not None:
                print("run", r, "K", K, "sub-steps of the eager twin", a.substeps.tolist())
        b.run(n, graph=True, **mode)
        torch.cuda.synchronize()
        sa, sb = _snapshot(a), _snapshot(b)
        for name in STATE + FRAME:
            assert _bits(sa[name], sb[name]), (r, name)
    assert not bool(a.behind.any()) and not bool(b.behind.any())
    assert {K for _, K in b._graphs} == {None, 8, 9}, "plain and fixed graphs side by side"
    assert len(b._graphs) == 4 and not a._graphs                          # (parity 0 and 1 at K = 8, one each at K = 9 and for plain steps)


def test_fixed_dt_rollout_gradient_matches_the_reference_autograd():
    """The batched `grad_demo` of tests/test_hip_contacts.py::test_rollout_gradient_matches_the_reference_autograd under
    `step(differentiable=True, fixed_dt=True)` (B = 8 x 128): the forward values are bitwise those of the non-differentiable route;
    clocks, sub-step counts and contact counts are the reference's; final poses to 1e-4, the loss to 1e-5 relative and
    d(loss)/d(force) - back-propagated through every sub-step, finished scenes passing state and gradient through - to 1e-4 relative
    (that test's bounds); replicas are bitwise replicas."""
    d = ROLLOUT
    rep = 128
    nsteps = int(d["nsteps"])
    world, force0 = _grad_demo_world(range(8), rep, requires_grad=True)
    ncs, subs, ts = [], [], []
    for _ in range(nsteps):
        world.step(differentiable=True, fixed_dt=True)
        ncs.append(world.contacts.count.clone()); subs.append(world.substeps.clone()); ts.append(world.t.clone())
    a, b = [int(i) for i in d["loss_bodies"]]
    pos = world.p[:, :, 1:]
    loss = (pos[:, a] - pos[:, b]).norm(dim=1)
    loss.sum().backward()
    plain, _ = _grad_demo_world(range(8), rep)
    for _ in range(nsteps):
        plain.step(fixed_dt=True)
    torch.cuda.synchronize()
    for n in STATE:
        assert _bits(getattr(world, n).detach(), getattr(plain, n)), n
    for n in FRAME:
        assert _bits(getattr(world.contacts, n), getattr(plain.contacts, n)), n
    assert np.abs(torch.stack(ts, 1).cpu().numpy()[::rep] - d["t"]).max() < 1e-12
    assert (torch.stack(subs, 1).cpu().numpy()[::rep] == d["nsub"]).all()
    assert (torch.stack(ncs, 1).cpu().numpy()[::rep] == d["ncontacts"]).all()
    pf = world.p.detach().cpu().numpy()[::rep]
    print("final pose error", np.abs(pf - d["p_final"]).max())
    assert np.abs(pf - d["p_final"]).max() <= 1e-4, np.abs(pf - d["p_final"]).max()
    ls = loss.detach().cpu().numpy()[::rep]
    print("loss error (relative)", np.abs(ls - d["loss"]).max() / np.abs(d["loss"]).max())
    assert np.abs(ls - d["loss"]).max() <= 1e-5 * np.abs(d["loss"]).max()
    gr = force0.grad.cpu().numpy()
    assert np.isfinite(gr).all()
    assert np.abs(gr.reshape(-1, rep, 3) - gr[::rep][:, None]).max() == 0.0          # replicas are bitwise replicas
    ref = d["grad"]
    err = np.abs(gr[::rep] - ref).max(axis=1) / np.abs(ref).max(axis=1)
    print("fixed-dt roll-out gradient: worst relative error", err.max(), "per scene", np.array2string(err, precision=2))
    assert err.max() <= 1e-4, err
