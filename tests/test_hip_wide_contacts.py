"""GPU: the wide narrow phase (lcp_contacts_wide.hip: `lcp_move_find_contacts_nv_f64`, `lcp_contact_frame_backward_nv_f64`) -
hulls of up to 64 vertices, scenes of up to 64 bodies - against the CPU oracles (oracle/contacts_oracle.py, pinned on the
reference for such hulls by tests/test_wide_contacts_host.py; oracle/world_oracle.py), against the existing kernels on the
sizes both take (bitwise), and end to end through `ContactWorld`.  Tolerances of the contact lists: tests/test_hip_contacts.py."""
import numpy as np
import pytest
import torch

from oracle import contacts_oracle as C
from oracle import world_oracle as W
from tests.test_hip_contacts import _compare_lists, _random_scene

from lcp_physics_amd.scenes import GRAVITY

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ngon(rng, nv, rad):
    """A perturbed regular n-gon, counter-clockwise (the construction of _random_scene's hulls)."""
    ang = (np.arange(nv) + rng.uniform(-0.3, 0.3, nv)) * (2 * np.pi / nv) + rng.uniform(0, 2 * np.pi)
    return np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)


def _wide_scene(rng, nb, nv_range=(9, 65), col=8, rotate=True, jitter=(-0.3, 0.1), hull_h=0.95, gap=0.0):
    """_random_scene with n-gons of `nv_range` vertices and the bodies dropped in columns of `col` on a wide floor
    (`jitter`: vertical offset from resting on the body below; `hull_h`: a hull's half height as a fraction of its radius;
    `gap`: added space between neighbours)."""
    ncol = (nb - 2) // col + 1
    width = 100.0 * ncol + 100.0
    shapes, pose = [("rect", (width, 10.0))], [[0.0, 300.0, 400.0]]
    x0 = 300.0 - 50.0 * (ncol - 1)
    for c in range(ncol):
        y = 395.0
        for _ in range(min(col, nb - len(shapes))):
            r = rng.random()
            sz = rng.uniform(15, 30, size=2)
            if r < 0.3:
                shapes.append(("circle", float(sz[0]))); hh = sz[0]
            elif r < 0.55:
                shapes.append(("rect", (float(sz[0]), float(sz[1])))); hh = sz[1] / 2
            else:
                nv = int(rng.integers(*nv_range)) if len(nv_range) == 2 else int(rng.choice(nv_range))
                rad = float(sz[0])
                shapes.append(("hull", _ngon(rng, nv, rad))); hh = rad * hull_h
            y -= hh + gap
            rot = 0.0 if (rng.random() < 0.5 or not rotate) else float(rng.uniform(-0.4, 0.4))
            pose.append([rot, x0 + 100.0 * c + float(rng.uniform(-8, 8)), y + float(rng.uniform(*jitter))])
            y -= hh
    return shapes, np.array(pose)


def _geom(shape_lists, max_verts=None):
    """GeometryBatch of several scenes (equal body counts) at one vertex capacity."""
    from lcp_physics_amd.physics.contacts import GeometryBatch
    cap = max_verts
    if cap is None:
        cap = max(8, max((len(a) for sh in shape_lists for k, a in sh if k == "hull"), default=0))
    gs = [GeometryBatch.from_shapes(sh, 1, max_verts=cap) for sh in shape_lists]
    cat = lambda k: torch.cat([getattr(g, k) for g in gs])
    return GeometryBatch(cat("kind"), cat("radius"), cat("verts_local"), cat("nverts"), None,
                         max(g.scene_verts_max for g in gs)).to(DEV)


def _oracle_list(shapes, pose, no_contact=()):
    try:
        return C.find_contacts(W.bodies_at(shapes, pose), eps=0.1, no_contact=no_contact)
    except ValueError:                  # get_closest raises on a degenerate simplex (contacts.py:330): no reference answer
        return None


def test_random_wide_scenes_match_oracle():
    """n-gons of 9..64 vertices with circles and rects, nb in {5, 12, 40, 64}, against oracle/contacts_oracle.py."""
    from lcp_physics_amd.physics.contacts import find_contacts
    rng = np.random.default_rng(2064)
    total, per_nb = 0, {}
    for nb, nsc, nvr in ((5, 48, (9, 65)), (12, 24, (9, 65)), (40, 10, (9, 49)), (64, 6, (9, 41))):    # (<= 1024 vertices a scene)
        scenes = [_wide_scene(rng, nb, nv_range=nvr) for _ in range(nsc)]
        geom = _geom([s[0] for s in scenes], max_verts=64)
        assert geom.scene_verts_max <= 1024
        p = torch.tensor(np.stack([s[1] for s in scenes]), dtype=torch.float64, device=DEV)
        cb = find_contacts(geom, p, maxc=192)
        torch.cuda.synchronize()
        for k, (shapes, pose) in enumerate(scenes):
            ref = _oracle_list(shapes, pose)
            if ref is None:
                continue
            _compare_lists(cb, k, ref, "nb%d scene %d" % (nb, k))
            total += len(ref)
            per_nb[nb] = per_nb.get(nb, 0) + len(ref)
    print("contacts compared per nb:", per_nb)
    assert total >= 1000 and all(per_nb.get(nb, 0) > 0 for nb in (5, 12, 40, 64)), per_nb


def _bitwise(a, b, what):
    for name in ("c_n", "c_p1", "c_p2", "c_pen", "c_i1", "c_i2", "count", "p_out", "dt_used", "trials", "max_pen"):
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x, y), (what, name, float((x.double() - y.double()).abs().max()))


def test_small_scenes_are_bitwise_the_existing_kernel():
    """The seeded scenes of test_random_scenes_match_oracle and test_move_and_halve_matches_oracle through
    lcp_move_find_contacts_f64 and through the wide entry (capacity 16): every output bitwise equal."""
    from lcp_physics_amd.physics.contacts import GeometryBatch, find_contacts, move_and_find_contacts
    from tests.test_hip_contacts import _geom as small_geom
    rng = np.random.default_rng(7)
    for nb in (3, 4, 6, 7, 12):
        scenes = [_random_scene(rng, nb) for _ in range(97 if nb < 12 else 24)]
        g8, g16 = small_geom([s[0] for s in scenes]), _geom([s[0] for s in scenes], max_verts=16)
        assert not g8.wide and g16.wide
        p = torch.tensor(np.stack([s[1] for s in scenes]), dtype=torch.float64, device=DEV)
        _bitwise(find_contacts(g8, p, maxc=48), find_contacts(g16, p, maxc=48), "nb%d" % nb)
    rng = np.random.default_rng(11)
    nb, B = 4, 128
    scenes = [_random_scene(rng, nb, hulls=False, rotate=False) for _ in range(B)]
    p0 = np.stack([s[1] for s in scenes])
    p0[:, 1:, 2] -= rng.uniform(0.5, 3.0, size=(B, nb - 1)).cumsum(axis=1)
    v = np.zeros((B, nb, 3))
    v[:, 1:, 2] = rng.uniform(20, 120, size=(B, nb - 1))
    v[:, 1:, 1] = rng.uniform(-20, 20, size=(B, nb - 1))
    v[:, 1:, 0] = rng.uniform(-0.5, 0.5, size=(B, nb - 1))
    v32 = torch.tensor(v, dtype=torch.float32, device=DEV)
    g8, g16 = small_geom([s[0] for s in scenes]), _geom([s[0] for s in scenes], max_verts=16)
    pt = torch.tensor(p0, dtype=torch.float64, device=DEV)
    for strict in (True, False):
        t8 = torch.zeros(B, dtype=torch.float64, device=DEV)
        t16 = torch.zeros(B, dtype=torch.float64, device=DEV)
        a = move_and_find_contacts(g8, pt, v32, 1.0 / 30, maxc=16, strict=strict, t=t8)
        b = move_and_find_contacts(g16, pt, v32, 1.0 / 30, maxc=16, strict=strict, t=t16)
        _bitwise(a, b, "move strict=%s" % strict)
        assert torch.equal(t8, t16)
        assert int((a.trials > 1).sum()) > B // 4


def test_move_and_halve_at_40_bodies_matches_oracle():
    """world.py:88-101 at nb = 40 with hulls of 9..24 vertices: accepted dt, trials, pose, contact list; a no_contact mask on
    half the scenes; a list truncated at maxc (count reports the full length, the first maxc records are the reference's)."""
    from lcp_physics_amd.physics.contacts import move_and_find_contacts
    rng = np.random.default_rng(40)
    nb, B = 40, 8
    scenes = [_wide_scene(rng, nb, nv_range=(9, 25), rotate=False) for _ in range(B)]
    p0 = np.stack([s[1] for s in scenes])
    v = np.zeros((B, nb, 3))
    v[:, 1:, 2] = rng.uniform(20, 120, size=(B, nb - 1))
    v[:, 1:, 1] = rng.uniform(-20, 20, size=(B, nb - 1))
    v[:, 1:, 0] = rng.uniform(-0.5, 0.5, size=(B, nb - 1))
    v32 = torch.tensor(v, dtype=torch.float32)
    geom = _geom([s[0] for s in scenes])
    masks = []
    mask = torch.zeros(B, nb, nb, dtype=torch.uint8)
    for k in range(B):
        m = []
        if k % 2:
            ref0 = _oracle_list(scenes[k][0], p0[k])
            for c in (ref0 or [])[::3]:
                a, b = c[1], c[2]
                mask[k, a, b] = mask[k, b, a] = 1
                m.append((a, b))
        masks.append(m)
    geom.no_contact = mask.to(DEV)
    dt = 1.0 / 30
    pt = torch.tensor(p0, dtype=torch.float64, device=DEV)
    t = torch.zeros(B, dtype=torch.float64, device=DEV)
    cb = move_and_find_contacts(geom, pt, v32.to(DEV), dt, maxc=160, t=t)
    small = move_and_find_contacts(geom, pt, v32.to(DEV), dt, maxc=8)
    torch.cuda.synchronize()
    halved, masked, checked = 0, 0, 0
    for k in range(B):
        try:
            p_ref, ref, dt_ref, trials = W.move_and_find(scenes[k][0], p0[k], v32[k].double().numpy(), dt, no_contact=masks[k])
        except ValueError:
            continue
        checked += 1
        assert int(cb.trials[k]) == trials and float(cb.dt_used[k]) == dt_ref, (k, int(cb.trials[k]), trials)
        assert abs(float(t[k]) - dt_ref) < 1e-15
        assert np.abs(cb.p_out[k].cpu().numpy() - p_ref).max() < 1e-10
        _compare_lists(cb, k, ref, "scene %d" % k)
        halved += trials > 1
        masked += len(masks[k]) > 0
        # truncated: same decisions, count = the full length, the first 8 records
        assert int(small.count[k]) == len(ref) > 8 and int(small.trials[k]) == trials
        assert small.c_i1[k].cpu().tolist() == [c[1] for c in ref[:8]] and small.c_i2[k].cpu().tolist() == [c[2] for c in ref[:8]]
        assert np.abs(small.c_n[k].double().cpu().numpy() - np.stack([c[0][0] for c in ref[:8]])).max() <= 1e-6
    assert checked >= B - 1 and halved >= 1 and masked >= 2, (checked, halved, masked)


# ---- frame backward ---------------------------------------------------------------------------------------------------
def _frame_loss(recs, g):
    """sum over records k of g[k] . (n, p1, p2)."""
    return sum(float(np.dot(g[k], np.concatenate([c[0][0], c[0][1], c[0][2]]))) for k, c in enumerate(recs))


def _pairs_of(bodies, b, eps=0.1):
    """The records of the pairs that involve body b, in list order (the others do not move with b's pose)."""
    out = []
    for i in range(len(bodies)):
        for j in range(i + 1, len(bodies)):
            if i != b and j != b:
                continue
            d = np.linalg.norm(bodies[i]["pos"] - bodies[j]["pos"])
            if d > _extent(bodies[i]) + _extent(bodies[j]) + 10.0:
                continue                                        # (far apart: no record, as the all-pairs oracle finds)
            for pt in C.collide_pair(bodies[i], bodies[j], eps):
                out.append((pt, i, j))
    return out


def _extent(b):
    return b["rad"] if b["kind"] == "circle" else float(np.linalg.norm(b["verts"], axis=1).max())


@pytest.mark.parametrize("nv,nb", [(16, 12), (48, 12), (16, 40), (48, 40)])
def test_frame_backward_matches_central_differences(nv, nb):
    """d(sum g . (n, p1, p2))/d(pose) from lcp_contact_frame_backward_nv_f64 against central differences of the fp64 oracle
    (h = 1e-6 on positions, 1e-7 on rotations; relative 1e-5), on the coordinates whose contact list keeps its pairs and count."""
    from lcp_physics_amd.physics.contacts import contact_frame_backward, find_contacts
    rng = np.random.default_rng(100 * nv + nb)
    B, maxc = 3, 128
    scenes = []
    while len(scenes) < B:
        sc = _wide_scene(rng, nb, nv_range=(nv, nv + 1))
        if _oracle_list(*sc) is not None:
            scenes.append(sc)
    geom = _geom([s[0] for s in scenes])
    p = torch.tensor(np.stack([s[1] for s in scenes]), dtype=torch.float64, device=DEV)
    cb = find_contacts(geom, p, maxc=maxc)
    g = torch.randn(B, maxc, 6, generator=torch.Generator().manual_seed(nv + nb), dtype=torch.float32)
    gd = g.to(DEV)
    dp = contact_frame_backward(geom, p, cb, gd[..., 0:2].contiguous(), gd[..., 2:4].contiguous(), gd[..., 4:6].contiguous())
    torch.cuda.synchronize()
    dp = dp.cpu().numpy()
    gg = g.double().numpy()
    checked, worst = 0, 0.0
    for k, (shapes, pose) in enumerate(scenes):
        ref = _oracle_list(shapes, pose)
        _compare_lists(cb, k, ref, "scene %d" % k)
        touched = sorted({c[1] for c in ref} | {c[2] for c in ref})
        bodies_sel = [touched[i] for i in np.random.default_rng(k).permutation(len(touched))[:8]]
        for b in bodies_sel:
            base = _pairs_of(W.bodies_at(shapes, pose), b)
            # the record index of each of b's records in the full list, for its cotangent
            rows = [q for q, c in enumerate(ref) if b in (c[1], c[2])]
            assert [(c[1], c[2]) for c in base] == [(ref[q][1], ref[q][2]) for q in rows]
            gb = gg[k, rows]
            for c in range(3):
                h = 1e-7 if c == 0 else 1e-6
                vals = []
                for sgn in (1, -1):
                    q = pose.copy()
                    q[b, c] += sgn * h
                    recs = _pairs_of(W.bodies_at(shapes, q), b)
                    if [(r[1], r[2]) for r in recs] != [(r[1], r[2]) for r in base]:
                        break
                    vals.append(_frame_loss(recs, gb))
                if len(vals) < 2:
                    continue
                fd = (vals[0] - vals[1]) / (2 * h)
                l0 = _frame_loss(base, gb)
                if abs((vals[0] - l0) - (l0 - vals[1])) / h > 1e-3 * max(abs(fd), 1.0):
                    continue                                    # (a branch of the geometry switches inside [-h, h]: no derivative)
                err = abs(dp[k, b, c] - fd) / max(abs(fd), 1.0)
                worst = max(worst, err)
                assert err <= 1e-5, (nv, nb, k, b, c, dp[k, b, c], fd)
                checked += 1
    print("frame backward nv %d nb %d: %d coordinates, worst relative error %.2e" % (nv, nb, checked, worst))
    assert checked >= 30


def test_frame_backward_equals_the_existing_kernel_on_small_scenes():
    from lcp_physics_amd.physics.contacts import contact_frame_backward, find_contacts
    from tests.test_hip_contacts import _geom as small_geom
    rng = np.random.default_rng(5)
    for nb in (5, 7, 12, 20):
        scenes = [_random_scene(rng, nb) for _ in range(40)]
        g8, g16 = small_geom([s[0] for s in scenes]), _geom([s[0] for s in scenes], max_verts=16)
        p = torch.tensor(np.stack([s[1] for s in scenes]), dtype=torch.float64, device=DEV)
        cb = find_contacts(g8, p, maxc=64)
        gen = torch.Generator().manual_seed(nb)
        gs = [torch.randn(len(scenes), 64, 2, generator=gen).to(DEV) for _ in range(3)]
        a = contact_frame_backward(g8, p, cb, *gs)
        b = contact_frame_backward(g16, p, cb, *gs)
        torch.cuda.synchronize()
        scale = torch.clamp(a.abs(), min=1.0)
        assert float(((a - b).abs() / scale).max()) <= 1e-10, (nb, float(((a - b).abs() / scale).max()))
        assert float(a.abs().max()) > 0


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _pile_world(B, nb=40, seed=12):
    """Floor (TotalConstraint) + circles, rects and 12-gons in columns, released just above each other."""
    rng = np.random.default_rng(seed)
    shapes, pose = _wide_scene(rng, nb, nv_range=(12, 13), rotate=False, jitter=(-0.05, 0.0), hull_h=1.0,
                                gap=0.2)                                # (no initial penetration)
    Mdiag = np.ones((nb, 3))
    for i, (k, a) in enumerate(shapes):
        if i == 0:
            continue
        m = 1.0
        if k == "circle":
            inertia = 0.5 * m * a ** 2
        elif k == "rect":
            inertia = m * (a[0] ** 2 + a[1] ** 2) / 12.0
        else:
            inertia = 0.5 * m * float((np.asarray(a) ** 2).sum(axis=1).mean())
        Mdiag[i] = (inertia, m, m)
    f = np.zeros((nb, 3))
    f[1:, 2] = Mdiag[1:, 1] * GRAVITY
    Je = np.zeros((3, 3 * nb))
    Je[:, :3] = np.eye(3)
    rest, fric = np.full(nb, 0.3), np.full(nb, 0.5)
    return shapes, pose, Mdiag, f, rest, fric, Je


def _oracle_rollout(shapes, p, Mdiag, f, rest, fric, Je, nsteps, dt=1.0 / 30, v0=None):
    v = np.zeros_like(p) if v0 is None else v0
    cs = C.find_contacts(W.bodies_at(shapes, p), eps=0.1)
    t, sets = 0.0, []
    for _ in range(nsteps):
        p, v, cs, dt_used, _ = W.step_dt(shapes, p, v, cs, Mdiag, f, rest, fric, Je, dt)
        t += dt_used
        sets.append([(c[1], c[2]) for c in cs])
    return p, v, t, sets


def test_contact_world_of_40_bodies_follows_oracle_and_differentiates():
    from lcp_physics_amd import _lib
    from lcp_physics_amd.physics.batched_world import ContactWorld
    B, nb, maxc = 2, 40, 128
    lib = _lib.load()
    assert lib.lcp_step_has_backward(nb, maxc, 3, _lib.COMPUTE_F64) == 1           # the generic plan takes these sizes
    shapes, pose, Mdiag, f, rest, fric, Je = _pile_world(B, nb)
    geom = _geom([shapes] * B, max_verts=None)
    assert geom.nvcap == 12 and geom.wide
    rep = lambda a, dt_: torch.tensor(np.broadcast_to(a, (B,) + a.shape).copy(), dtype=dt_, device=DEV)
    world = ContactWorld(geom, rep(pose, torch.float64), rep(np.zeros_like(pose), torch.float32), rep(Mdiag, torch.float32),
                         rep(f, torch.float32), rep(rest, torch.float32), rep(fric, torch.float32), Je=rep(Je, torch.float32),
                         maxc=maxc)
    nsteps = 8
    f32 = lambda a: a.astype(np.float32).astype(np.float64)                        # (the world's fp32 inputs)
    p_ref, v_ref, t_ref, sets = _oracle_rollout(shapes, pose, f32(Mdiag), f32(f), f32(rest), f32(fric), f32(Je), nsteps)
    for _ in range(nsteps):
        world.step()
    world.check_capacity()
    assert len(sets[-1]) >= 8                                                      # (the bodies have landed on each other)
    for s in range(B):
        assert abs(float(world.t[s]) - t_ref) < 1e-12 and int(world.contacts.count[s]) == len(sets[-1]), s
        assert np.abs(world.p[s].cpu().numpy() - p_ref).max() < 2e-4 and np.abs(world.v[s].double().cpu().numpy() - v_ref).max() < 2e-3, s

    # a differentiable roll-out of 4 steps: d(w . p_final)/d(p0) through lcp_contact_frame_backward_nv_f64.  Every body spins a
    # little: the reference turns a hull's vertices only by a non-zero rotation increment (bodies.py:199-202), so a step without
    # one has no vertex path in its autograd (nor in ContactWorld's) while a finite difference has - spinning bodies have it always
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
    grad = p0.grad[0].cpu().numpy()
    assert float((p0.grad[0] - p0.grad[1]).abs().max()) <= 1e-9 * max(1.0, float(np.abs(grad).max()))   # (two copies of one scene)
    base = _oracle_rollout(shapes, pose, f32(Mdiag), f32(f), f32(rest), f32(fric), f32(Je), nroll, v0=v0)
    pf = world.p[0].detach().cpu().numpy()
    assert np.abs(pf - base[0]).max() < 2e-4
    rng = np.random.default_rng(9)
    touched = sorted({b for st in base[3] for pr in st for b in pr} - {0})          # (bodies in contact during the roll-out)
    cand = [(b, c) for b in touched for c in range(3)]
    checked, worst, errs = 0, 0.0, []
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
        errs.append((b, c, float(grad[b, c]), fd))
        worst = max(worst, abs(grad[b, c] - fd) / max(abs(fd), 1.0))
        checked += 1
    print("40-body roll-out gradient: %d coordinates, worst relative error %.2e" % (checked, worst))
    assert checked >= 4 and worst <= 2e-3, (checked, worst, errs)
