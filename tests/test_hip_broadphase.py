"""GPU: detection with the broadphase (lcp_contacts_bp.hip, `lcp_move_find_contacts_bp_f64`, `broadphase=True` of the wrappers and of
`ContactWorld`) - every output bitwise that of the all-pairs entries on the same inputs, the candidate counts against the numpy
restatement of the cull rule (tests/broadphase_host.py), the lists against the contact oracle, and end to end through the world."""
import numpy as np
import pytest
import torch

from oracle import world_oracle as W
from tests import broadphase_host as BH
from tests.test_hip_contacts import _compare_lists
from tests.test_hip_wide_contacts import _bitwise, _geom, _oracle_list, _pile_world, _wide_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"

_CACHE = {}


def _pile_run(nb):
    """The piles of BH.PILES with nb bodies through both detections, once: (scenes, geometry, all-pairs buffers, broadphase buffers,
    candidates [B] on the host)."""
    if nb not in _CACHE:
        from lcp_physics_amd.physics.contacts import find_contacts
        _, B, nvr, cap = next(p for p in BH.PILES if p[0] == nb)
        scenes = BH.piles(nb, B, nvr)
        geom = _geom([s[0] for s in scenes], max_verts=cap)
        assert geom.verts_max() <= 1024 and geom.wide == (cap != 8 or nb > 32)
        p = torch.tensor(np.stack([s[1] for s in scenes]), dtype=torch.float64, device=DEV)
        cand = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        ref = find_contacts(geom, p, maxc=192)
        out = find_contacts(geom, p, maxc=192, broadphase=True, candidates=cand)
        torch.cuda.synchronize()
        _CACHE[nb] = (scenes, geom, ref, out, cand.cpu().tolist())
    return _CACHE[nb]


NBS = [p[0] for p in BH.PILES]


@pytest.mark.parametrize("nb", NBS)
def test_detection_is_bitwise_the_all_pairs_detection(nb):
    """nb = 3, 7, 12 at capacity 8 (all pairs: lcp_contacts.hip), 20, 40, 64 at capacity 64 (lcp_contacts_wide.hip)."""
    scenes, geom, ref, out, cand = _pile_run(nb)
    _bitwise(ref, out, "nb%d" % nb)
    assert int(ref.count.max()) > 0 and int(ref.count.max()) <= 192


def _single(shapes, pose, maxc, no_contact=None, broadphase=True):
    from lcp_physics_amd.physics.contacts import find_contacts
    geom = _geom([shapes])
    if no_contact is not None:
        geom.no_contact = no_contact.to(DEV)
    p = torch.tensor(pose[None], dtype=torch.float64, device=DEV)
    cand = torch.full((1,), -7, dtype=torch.int32, device=DEV) if broadphase else None
    cb = find_contacts(geom, p, maxc=maxc, broadphase=broadphase, candidates=cand)
    torch.cuda.synchronize()
    return cb, (None if cand is None else int(cand[0]))


def test_candidate_list_longer_than_one_narrow_pass():
    """13 planks: 78 candidates, 24 records from both narrow passes; with maxc = 16 the list is cut and count still reports 24."""
    shapes, pose = BH.plank_scene()
    ref = _oracle_list(shapes, pose)
    assert len(ref) == 24
    for maxc in (32, 16):
        cb, cand = _single(shapes, pose, maxc)
        allp, _ = _single(shapes, pose, maxc, broadphase=False)
        _bitwise(allp, cb, "planks maxc %d" % maxc)
        assert cand == 78 and int(cb.count[0]) == 24
        if maxc >= 24:
            _compare_lists(cb, 0, ref, "planks")
        else:
            assert cb.c_i1[0].cpu().tolist() == [c[1] for c in ref[:maxc]] and cb.c_i2[0].cpu().tolist() == [c[2] for c in ref[:maxc]]


def test_corner_to_corner_hulls_keep_their_records():
    """Hulls whose nearest features are two corners: the narrow phase tests the separation along edge normals only, so it reports
    records for bodies more than eps apart (the clip's extrapolated point).  The squares of BH.corner_scene, and 512 seeded near-corner
    pairs (rects, needle triangles, n-gons, any rotation): bitwise the all-pairs detection, candidates equal to the host's."""
    from lcp_physics_amd.physics.contacts import find_contacts
    shapes, pose = BH.corner_scene(0.09)
    cb, cand = _single(shapes, pose, 4)
    allp, _ = _single(shapes, pose, 4, broadphase=False)
    _bitwise(allp, cb, "corner squares")
    assert int(cb.count[0]) == 1 and cand == 1 and abs(float(cb.c_pen[0, 0]) + 0.09) < 1e-9
    scenes, host = [], []
    for shapes, pose in BH.near_corner_pairs(512):
        pairs, near = BH.candidate_pairs(W.bodies_at(shapes, pose))
        if near > BH.NEAR:
            scenes.append((shapes, pose))
            host.append(len(pairs))
    assert len(scenes) >= 500
    geom = _geom([s[0] for s in scenes], max_verts=8)
    p = torch.tensor(np.stack([s[1] for s in scenes]), dtype=torch.float64, device=DEV)
    cand = torch.full((len(scenes),), -7, dtype=torch.int32, device=DEV)
    a = find_contacts(geom, p, maxc=4)
    b = find_contacts(geom, p, maxc=4, broadphase=True, candidates=cand)
    torch.cuda.synchronize()
    _bitwise(a, b, "near-corner pairs")
    assert cand.cpu().tolist() == host
    assert int((a.count > 0).sum()) >= 150                                       # (pairs with a record to lose)


def test_nothing_survives_the_cull():
    """5 bodies 1000 apart: no candidate, no record, padded slots; a no_contact mask on a pile removes pairs that would be candidates."""
    from lcp_physics_amd.physics.contacts import find_contacts
    shapes, pose = BH.far_scene()
    cb, cand = _single(shapes, pose, 8)
    allp, _ = _single(shapes, pose, 8, broadphase=False)
    _bitwise(allp, cb, "far")
    assert int(cb.count[0]) == 0 and cand == 0
    for name in ("c_n", "c_p1", "c_p2", "c_pen", "c_i1", "c_i2"):
        assert float(getattr(cb, name).double().abs().max()) == 0.0, name
    scenes, geom0, _, _, cand0 = _pile_run(12)
    B, nb = len(scenes), 12
    mask = torch.zeros(B, nb, nb, dtype=torch.uint8)
    host = []
    for k, (shapes, pose) in enumerate(scenes):
        full, _ = BH.candidate_pairs(W.bodies_at(shapes, pose))
        off = full[::2]
        for a, b in off:
            mask[k, a, b] = mask[k, b, a] = 1
        host.append(len(BH.candidate_pairs(W.bodies_at(shapes, pose), no_contact=off)[0]))
    geom = _geom([s[0] for s in scenes], max_verts=8)
    geom.no_contact = mask.to(DEV)
    p = torch.tensor(np.stack([s[1] for s in scenes]), dtype=torch.float64, device=DEV)
    cand = torch.zeros(B, dtype=torch.int32, device=DEV)
    a = find_contacts(geom, p, maxc=64)
    b = find_contacts(geom, p, maxc=64, broadphase=True, candidates=cand)
    torch.cuda.synchronize()
    _bitwise(a, b, "masked piles")
    assert cand.cpu().tolist() == host and all(h < c for h, c in zip(host, cand0))
    assert int(a.count.sum()) < int(_pile_run(12)[2].count.sum())              # (the mask removed records too)


@pytest.mark.parametrize("nb", NBS)
def test_candidates_equal_the_host_restatement(nb):
    scenes, geom, ref, out, cand = _pile_run(nb)
    npairs = nb * (nb - 1) // 2
    for k, (shapes, pose) in enumerate(scenes):
        host, near = BH.candidate_pairs(W.bodies_at(shapes, pose))
        assert near > BH.NEAR
        n = int(out.count[k])
        pairs = set(zip(out.c_i1[k, :n].cpu().tolist(), out.c_i2[k, :n].cpu().tolist()))
        print("nb %d scene %d: %d candidates of %d pairs, %d contact pairs" % (nb, k, cand[k], npairs, len(pairs)))
        assert cand[k] == len(host), (nb, k, cand[k], len(host))
        assert cand[k] >= len(pairs), (nb, k)
        assert pairs <= set(host), (nb, k)
        if nb >= 12:
            assert cand[k] <= npairs / 4, (nb, k, cand[k])


def _halving_setup(nb, B=8):
    """The velocity set-up of test_hip_wide_contacts.test_move_and_halve_at_40_bodies_matches_oracle."""
    rng = np.random.default_rng(40 + nb)
    scenes = [_wide_scene(rng, nb, nv_range=(9, 25), rotate=False) for _ in range(B)]
    p0 = np.stack([s[1] for s in scenes])
    v = np.zeros((B, nb, 3))
    v[:, 1:, 2] = rng.uniform(20, 120, size=(B, nb - 1))
    v[:, 1:, 1] = rng.uniform(-20, 20, size=(B, nb - 1))
    v[:, 1:, 0] = rng.uniform(-0.5, 0.5, size=(B, nb - 1))
    geom = _geom([s[0] for s in scenes])
    return geom, torch.tensor(p0, dtype=torch.float64, device=DEV), torch.tensor(v, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("nb", [12, 40])
def test_move_and_halve_loop_is_bitwise_the_all_pairs_loop(nb, strict):
    from lcp_physics_amd.physics.contacts import move_and_find_contacts
    geom, p, v = _halving_setup(nb)
    B, dt = p.shape[0], 1.0 / 30
    ta, tb = (torch.zeros(B, dtype=torch.float64, device=DEV) for _ in range(2))
    a = move_and_find_contacts(geom, p, v, dt, maxc=160, strict=strict, t=ta)
    b = move_and_find_contacts(geom, p, v, dt, maxc=160, strict=strict, t=tb, broadphase=True)
    torch.cuda.synchronize()
    _bitwise(a, b, "move nb%d strict=%s" % (nb, strict))
    assert torch.equal(ta, tb) and torch.equal(tb, b.dt_used) and bool((tb > 0).all())
    assert int((a.trials > 1).sum()) > B // 4, a.trials.tolist()
    # per-scene dt: one finished scene, unequal positive values elsewhere - against lcp_move_find_contacts_dts_f64
    dts = torch.tensor([dt / (1 + 0.37 * k) for k in range(B)], dtype=torch.float64, device=DEV)
    dts[3] = 0.0
    ta, tb = (torch.zeros(B, dtype=torch.float64, device=DEV) for _ in range(2))
    a = move_and_find_contacts(geom, p, v, dt, maxc=160, strict=strict, t=ta, dt_scene=dts)
    b = move_and_find_contacts(geom, p, v, dt, maxc=160, strict=strict, t=tb, dt_scene=dts, broadphase=True)
    torch.cuda.synchronize()
    _bitwise(a, b, "move dts nb%d strict=%s" % (nb, strict))
    assert torch.equal(ta, tb) and torch.equal(tb, b.dt_used) and float(tb[3]) == 0.0
    assert torch.equal(b.p_out[3], p[3]) and float(b.dt_used[3]) == 0.0 and int(b.trials[3]) == 1
    assert int((b.trials > 1).sum()) >= 1


def test_lists_match_the_oracle():
    total = 0
    for nb in (12, 40):
        scenes, geom, ref, out, cand = _pile_run(nb)
        for k, (shapes, pose) in enumerate(scenes):
            lst = _oracle_list(shapes, pose)
            if lst is None:
                continue
            _compare_lists(out, k, lst, "nb%d scene %d" % (nb, k))
            total += len(lst)
    print("records compared with the oracle:", total)
    assert total >= 200


def _worlds(post_stab, B=8, nb=12, **kw):
    """Two ContactWorlds of B different 12-body piles, the second with the broadphase."""
    from lcp_physics_amd.physics.batched_world import ContactWorld
    sc = [_pile_world(1, nb, seed=30 + k) for k in range(B)]
    geom = _geom([s[0] for s in sc])
    st = lambda q, dt_: torch.tensor(np.stack([s[q] for s in sc]), dtype=dt_, device=DEV)
    make = lambda bp: ContactWorld(geom, st(1, torch.float64), torch.zeros(B, nb, 3, device=DEV), st(2, torch.float32), st(3, torch.float32),
                                   st(4, torch.float32), st(5, torch.float32), Je=st(6, torch.float32), maxc=64, post_stab=post_stab,
                                   broadphase=bp, **kw)
    return make(False), make(True)


def _same_state(a, b, what):
    assert torch.equal(a.p, b.p) and torch.equal(a.v, b.v) and torch.equal(a.t, b.t), what
    _bitwise(a.contacts, b.contacts, what)


@pytest.mark.parametrize("post_stab", [False, True])
def test_world_with_broadphase_is_bitwise_the_world_without(post_stab):
    a, b = _worlds(post_stab)
    assert a.candidates is None and b.candidates.dtype == torch.int32 and tuple(b.candidates.shape) == (8,)
    _same_state(a, b, "start")
    for _ in range(20):
        a.step()
        b.step()
    _same_state(a, b, "20 steps")
    assert int(b.contacts.count.min()) > 0 and bool((b.candidates >= 1).all())
    a.run(20)
    b.run(20)
    assert b._graphs and len(b._graphs) == len(a._graphs)                       # (both captured: the launch count per step is the same)
    torch.cuda.synchronize()
    _same_state(a, b, "run(20)")
    assert float(b.t.min()) > 0.0


def test_differentiable_steps_give_the_same_gradients():
    grads = []
    for w in _worlds(False):
        Mdiag = w.Mdiag.clone().requires_grad_(True)
        f = w.f.clone().requires_grad_(True)
        v0 = torch.zeros_like(w.v)
        v0[:, 1:, 0] = 0.03                                                    # (every body spins a little: the vertex path exists)
        v0.requires_grad_(True)
        w.Mdiag, w.f = Mdiag, f
        w.restart(w.p.clone(), v=v0)
        for _ in range(3):
            w.step(differentiable=True)
        w.p.sum().backward()
        torch.cuda.synchronize()
        grads.append((Mdiag.grad, f.grad, v0.grad, w.p.detach()))
    for x, y, name in zip(grads[0], grads[1], ("Mdiag", "f", "v0", "p")):
        assert x is not None and torch.equal(x, y), name
    assert float(grads[0][2].abs().max()) > 0


def test_size_errors_and_a_scene_over_scene_verts_max():
    """nb = 65, nvcap = 7, scene_verts_max = 1025: LCP_E_TOOLARGE without a launch (the output buffers keep their fill); a scene whose
    vertex total exceeds the scene_verts_max passed gets count = -1, padded records and candidates = 0."""
    from lcp_physics_amd import _lib
    lib = _lib.load()
    scenes, geom, ref, _, _ = _pile_run(12)
    B, nb, maxc = len(scenes), 12, 32
    p = torch.tensor(np.stack([s[1] for s in scenes]), dtype=torch.float64, device=DEV)
    P = _lib.ptr

    def call(nb_, nvcap, vmax, cb, cand):
        with torch.cuda.device(p.device):
            rc = lib.lcp_move_find_contacts_bp_f64(B, nb_, maxc, nvcap, vmax, P(geom.kind), P(geom.radius), P(geom.verts_local), P(geom.nverts),
                                                   None, P(p), None, 0.0, 0.0, 1, 1, 0.1, 1e-6, P(cb.p_out), P(cb.c_n), P(cb.c_p1), P(cb.c_p2),
                                                   P(cb.c_pen), P(cb.c_i1), P(cb.c_i2), P(cb.count), P(cb.max_pen), P(cb.dt_used), None,
                                                   P(cb.trials), None, P(cand), _lib.stream_ptr(p.device))
        torch.cuda.synchronize()
        return rc

    from lcp_physics_amd.physics.contacts import ContactBuffers
    for nb_, nvcap, vmax in ((65, 8, 64), (12, 7, 64), (12, 8, 1025)):
        cb = ContactBuffers(B, nb, maxc, DEV)
        cb._backing.fill_(0x5A)
        cand = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        assert call(nb_, nvcap, vmax, cb, cand) == -2                          # LCP_E_TOOLARGE
        assert bool((cb._backing == 0x5A).all()) and cand.cpu().tolist() == [-7] * B
    # a NULL where the header requires a buffer, B = 0, max_trials = 0, scene_verts_max < 0: LCP_E_BADARG, nothing written
    cb = ContactBuffers(B, nb, maxc, DEV)
    cb._backing.fill_(0x5A)
    cand = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    args = lambda **kw: [kw.get("B", B), nb, kw.get("maxc", maxc), 8, kw.get("vmax", 64)] + [
        None if kw.get("null") == n else P(t) for n, t in (("kind", geom.kind), ("radius", geom.radius), ("verts_local", geom.verts_local),
                                                           ("nverts", geom.nverts))] + [
        None, None if kw.get("null") == "p_start" else P(p), None, 0.0, 0.0, 1, kw.get("trials", 1), 0.1, 1e-6] + [
        None if kw.get("null") == n else P(getattr(cb, n)) for n in ("p_out", "c_n", "c_p1", "c_p2", "c_pen", "c_i1", "c_i2", "count", "max_pen",
                                                                      "dt_used")] + [None, P(cb.trials), None, P(cand), _lib.stream_ptr(p.device)]
    cases = [dict(null=n) for n in ("kind", "radius", "verts_local", "nverts", "p_start", "c_n", "c_p1", "c_p2", "c_i1", "c_i2", "count")]
    for kw in cases + [dict(B=0), dict(maxc=0), dict(trials=0), dict(vmax=-1)]:
        with torch.cuda.device(p.device):
            rc = lib.lcp_move_find_contacts_bp_f64(*args(**kw))
        torch.cuda.synchronize()
        assert rc == -1, kw                                                  # LCP_E_BADARG
        assert bool((cb._backing == 0x5A).all()) and cand.cpu().tolist() == [-7] * B
    totals = torch.where(geom.kind != 0, geom.nverts, torch.zeros_like(geom.nverts)).sum(dim=1).cpu().tolist()
    order = sorted(range(B), key=lambda k: totals[k])
    assert totals[order[-1]] > totals[order[-2]]
    cb = ContactBuffers(B, nb, maxc, DEV)
    cb._backing.fill_(0x5A)
    cand = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    assert call(nb, 8, totals[order[-2]], cb, cand) == 0
    bad = order[-1]
    assert int(cb.count[bad]) == -1 and int(cand[bad]) == 0
    for name in ("c_n", "c_p1", "c_p2", "c_pen", "c_i1", "c_i2"):
        assert float(getattr(cb, name)[bad].double().abs().max()) == 0.0, name
    good = [k for k in range(B) if k != bad]
    assert cb.count[good].cpu().tolist() == ref.count[good].cpu().tolist() and torch.equal(cb.c_n[good], ref.c_n[good, :maxc])
