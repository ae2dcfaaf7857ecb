"""GPU: the backward of the contact frame with respect to the POSE of the bodies - `lcp_contact_frame_backward_f64`
(lcp_contacts.hip, capacity 8, one thread per scene) and `lcp_contact_frame_backward_nv_f64` (lcp_contacts_wide.hip, one lane per
pair and pose coordinate).

Pair level: every record type against what the unmodified reference's autograd gives the poses (tests/golden/frame_pose_grad.npz,
tools/gen_frame_pose_golden.py; pinned on the CPU by tests/test_frame_pose_fixture.py), at 1e-12 x max(1, largest |gradient|) -
the gate of test_contact_frame_backward_matches_autograd_of_the_circle_record and of the shape derivative (both sides are fp64
autodiff of the same expressions).

List level: the gradient of a scene's whole contact list against the host's fp64 sum of the kernel's own pair-level answers, one
two-body scene per record - the running contact index across pairs, the row offset of the cotangents, skipped `no_contact` pairs,
a list cut at `maxc` inside a pair, cotangent rows beyond the count, bodies that sit in several pairs."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.test_hip_contacts import ATOL_ARM, ATOL_N
from tests.test_hip_shape_grad import _fixture, _frame_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GATE = 1e-12


# ---- pair level -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _pose_fixture():
    return np.load(os.path.join(GOLDEN, "frame_pose_grad.npz"))["f_d_pose"]


class _Padded(dict):
    """The fixture with the body-frame vertices zero-padded to capacity `cap`."""

    def __init__(self, d, cap):
        super().__init__({k: d[k] for k in d.files if k.startswith("f_")})
        vl = np.zeros(d["f_verts_local"].shape[:2] + (cap, 2))
        vl[:, :, :d["f_verts_local"].shape[2]] = d["f_verts_local"]
        self["f_verts_local"] = vl


def _pose_grads(d, sel, cap, rep=2):
    """(contact buffers, dp [len(sel) * rep, 2, 3]) of the configurations `sel` at vertex capacity `cap`."""
    from lcp_physics_amd.physics import contacts as ct
    geom, p, gs = _frame_batch(_Padded(d, cap) if cap > d["f_verts_local"].shape[2] else d, sel, cap, rep)
    assert geom.nvcap == cap and geom.wide == (cap != 8)
    geom.scene_verts_max = int(d["f_nverts"][sel].sum(axis=1).max())          # (circles have nverts 0)
    cb = ct.find_contacts(geom, p, maxc=2, eps=float(d["f_eps"]))
    dp = ct.contact_frame_backward(geom, p, cb, *gs, eps=float(d["f_eps"]))
    torch.cuda.synchronize()
    return cb, dp.cpu().numpy()


def _per_type(d, sel, got, ref, scale):
    names = d["f_type_names"].tolist()
    err = np.abs(got - ref).reshape(len(sel), -1).max(axis=1) / scale
    rt = d["f_rtype"][sel]
    return {n: float(err[rt == t].max()) for t, n in enumerate(names) if (rt == t).any()}


def _subset8(d):
    sel = np.nonzero(d["f_nverts"].max(axis=1) <= 8)[0]
    assert len(sel) >= 100
    return sel


def test_wide_kernel_pose_gradients_match_the_reference_autograd_for_every_record_type():
    """All 232 configurations at capacity 16 (`lcp_contact_frame_backward_nv_f64`), each scene twice, none excluded: the counts are
    the fixture's, replicas are bitwise replicas, and d(sum g . (n, p1, p2))/d(pose) agrees with the reference's autograd to
    1e-12 x max(1, largest |gradient| of the fixture)."""
    d, ref = _fixture(), _pose_fixture()
    n, rep = d["f_count"].shape[0], 2
    sel = np.arange(n)
    cb, dp = _pose_grads(d, sel, 16, rep)
    assert (cb.count.cpu().numpy()[::rep] == d["f_count"]).all()
    assert np.array_equal(dp[0::rep], dp[1::rep])
    scale = max(1.0, np.abs(ref).max())
    per_type = _per_type(d, sel, dp[::rep], ref, scale)
    print("pose gradient at capacity 16 against the reference's autograd, worst |difference| / scale per record type:",
          {k: "%.2g" % v for k, v in per_type.items()})
    assert len(per_type) == len(d["f_type_names"]) and np.abs(ref).max() > 1.0
    assert np.abs(dp[::rep] - ref).max() <= GATE * scale, per_type


def test_narrow_kernel_pose_gradients_match_the_reference_autograd_for_every_record_type():
    """The configurations whose hulls have at most 8 vertices at capacity 8 (`lcp_contact_frame_backward_f64`): the same gate; every
    one of the eleven record types is in that subset."""
    d, ref = _fixture(), _pose_fixture()
    sel, rep = _subset8(d), 2
    missing = sorted(set(range(len(d["f_type_names"]))) - set(d["f_rtype"][sel].tolist()))
    assert not missing, "record types without a configuration of <= 8 vertices: %s" % d["f_type_names"][missing].tolist()
    cb, dp = _pose_grads(d, sel, 8, rep)
    assert (cb.count.cpu().numpy()[::rep] == d["f_count"][sel]).all()
    assert np.array_equal(dp[0::rep], dp[1::rep])
    scale = max(1.0, np.abs(ref).max())
    per_type = _per_type(d, sel, dp[::rep], ref[sel], scale)
    print("pose gradient at capacity 8 (%d configurations) against the reference's autograd, worst |difference| / scale per record "
          "type:" % len(sel), {k: "%.2g" % v for k, v in per_type.items()})
    assert np.abs(dp[::rep] - ref[sel]).max() <= GATE * scale, per_type


def test_narrow_and_wide_kernels_agree_on_every_record_type():
    """The same subset through both kernels: within 1e-12 of the scale (the two run the same dual-number geometry; the wide kernel
    stages values and applies the rotation's derivative on read, the narrow one rotates dual numbers)."""
    d = _fixture()
    sel = _subset8(d)
    cb8, dp8 = _pose_grads(d, sel, 8)
    cb16, dp16 = _pose_grads(d, sel, 16)
    assert torch.equal(cb8.count, cb16.count) and torch.equal(cb8.c_n, cb16.c_n)
    scale = max(1.0, np.abs(dp16).max())
    assert np.abs(dp16).max() > 1.0
    assert np.abs(dp8 - dp16).max() <= GATE * scale, _per_type(d, sel, dp8[::2], dp16[::2], scale)


def test_capacity_64_gives_the_bits_of_capacity_16():
    """All 232 configurations with the vertices zero-padded to capacity 64: one kernel, the same gradients bit for bit."""
    d = _fixture()
    sel = np.arange(d["f_count"].shape[0])
    cb16, dp16 = _pose_grads(d, sel, 16)
    cb64, dp64 = _pose_grads(d, sel, 64)
    assert torch.equal(cb16.count, cb64.count) and torch.equal(cb16.c_n, cb64.c_n)
    assert np.array_equal(dp16, dp64) and np.abs(dp16).max() > 1.0


@pytest.mark.parametrize("cap", [8, 16])
@pytest.mark.parametrize("size", [1, 37])
def test_batches_of_one_scene_and_of_a_size_that_is_no_multiple_of_the_workgroup(cap, size):
    """A batch of exactly one scene (a hull / hull pair with two clipped points) and one of 37 scenes (the narrow kernel runs 32
    scenes per workgroup: the second workgroup has five live threads), against the fixture."""
    d, ref = _fixture(), _pose_fixture()
    sel = _subset8(d)
    if size == 1:
        two = int(d["f_type_names"].tolist().index("hh_ref2_2"))
        sel = sel[d["f_rtype"][sel] == two][:1]
    else:
        sel = sel[np.linspace(0, len(sel) - 1, size).astype(int)]             # (spread over the record types)
        assert len(set(d["f_rtype"][sel].tolist())) == len(d["f_type_names"])
    assert len(sel) == size
    cb, dp = _pose_grads(d, sel, cap, rep=1)
    assert dp.shape == (size, 2, 3) and (cb.count.cpu().numpy() == d["f_count"][sel]).all()
    scale = max(1.0, np.abs(ref).max())
    assert np.abs(ref[sel]).max() > 1.0
    assert np.abs(dp - ref[sel]).max() <= GATE * scale, np.abs(dp - ref[sel]).max() / scale


# ---- list level -----------------------------------------------------------------------------------------------------------------
# name -> (bodies, scenes, column height, vertex counts of the n-gons, vertex capacity; None: the largest hull's)
LAYOUTS = {"narrow_12": (12, 24, 3, (3, 9), 8), "narrow_24": (24, 12, 4, (3, 9), 8), "wide_40": (40, 4, 8, (12, 49), None)}
EPS = 0.1


def _list_scenes(name):
    """The piles of a layout (tests/test_hip_wide_contacts.py::_wide_scene, seed 31) and, last, one scene of the same bodies set so
    far apart that nothing touches."""
    from tests.test_hip_wide_contacts import _wide_scene
    nb, nsc, col, nvr, cap = LAYOUTS[name]
    rng = np.random.default_rng(31)
    scenes = [_wide_scene(rng, nb, nv_range=nvr, col=col) for _ in range(nsc)]
    shapes, pose = scenes[0]
    apart = pose.copy()
    apart[:, 2] = 400.0 - 1000.0 * np.arange(nb)                               # (the floor is at most 600 wide, the bodies at most 60)
    return scenes + [(shapes, apart)], cap


def _rows(cb):
    """The records of every scene's list as flat host arrays: scene, row, the two bodies, the row's position within its pair and
    the pair's record count."""
    cnt, i1, i2 = cb.count.cpu().numpy(), cb.c_i1.cpu().numpy(), cb.c_i2.cpu().numpy()
    assert cnt.max() <= i1.shape[1], "the list does not fit its buffers"
    k, r, a, b, slot, npair = [], [], [], [], [], []
    for s in range(len(cnt)):
        for q in range(int(cnt[s])):
            same = q > 0 and (i1[s, q], i2[s, q]) == (i1[s, q - 1], i2[s, q - 1])
            k.append(s); r.append(q); a.append(int(i1[s, q])); b.append(int(i2[s, q])); slot.append(1 if same else 0); npair.append(1)
            if same:
                assert slot[-2] == 0, "more than two records of a pair"
                npair[-1] = npair[-2] = 2
    return tuple(np.array(x, dtype=np.int64) for x in (k, r, a, b, slot, npair))


def _record_contributions(geom, p, cb, gs, rows):
    """contrib [R, 2, 3]: for every record of every list, the pose gradient of a two-body scene that holds the record's pair at
    the same absolute poses in the same geometry layout, with the list's cotangent on that record alone.  One launch."""
    from lcp_physics_amd.physics import contacts as ct
    k, r, a, b, slot, npair = rows
    kk = torch.tensor(k, device=DEV).unsqueeze(1)
    ab = torch.tensor(np.stack([a, b], 1), device=DEV)
    g2 = ct.GeometryBatch(geom.kind[kk, ab].contiguous(), geom.radius[kk, ab].contiguous(), geom.verts_local[kk, ab].contiguous(),
                          geom.nverts[kk, ab].contiguous(), None, None)
    assert g2.wide == geom.wide
    p2 = p[kk, ab].contiguous()
    cb2 = ct.find_contacts(g2, p2, maxc=2, eps=EPS)
    assert np.array_equal(cb2.count.cpu().numpy(), npair)
    rr, kr, sl = torch.arange(len(k), device=DEV), torch.tensor(k, device=DEV), torch.tensor(slot, device=DEV)
    row = torch.tensor(r, device=DEV)
    for key, tol in (("c_n", ATOL_N), ("c_p1", ATOL_ARM), ("c_p2", ATOL_ARM)):
        assert float((getattr(cb2, key)[rr, sl] - getattr(cb, key)[kr, row]).abs().max()) <= tol, key
    g2s = []
    for g in gs:
        z = torch.zeros(len(k), 2, 2, dtype=torch.float32, device=DEV)
        z[rr, sl] = g[kr, row]
        g2s.append(z)
    contrib = ct.contact_frame_backward(g2, p2, cb2, *g2s, eps=EPS)
    torch.cuda.synchronize()
    return contrib.cpu().numpy()


def _expected(shape, rows, contrib, keep):
    """The host's fp64 sum of the contributions of the rows `keep`, scattered to the pairs' bodies."""
    k, _, a, b = rows[:4]
    out = np.zeros(shape)
    np.add.at(out, (k[keep], a[keep]), contrib[keep, 0])
    np.add.at(out, (k[keep], b[keep]), contrib[keep, 1])
    return out


@functools.lru_cache(None)
def _layout(name):
    """Scenes, geometry, the full lists, random cotangents and the per-record contributions of a layout, computed once."""
    from lcp_physics_amd.physics import contacts as ct
    from tests.test_hip_wide_contacts import _geom
    scenes, cap = _list_scenes(name)
    geom = _geom([s[0] for s in scenes], max_verts=cap)
    assert geom.wide == name.startswith("wide")
    p = torch.tensor(np.stack([s[1] for s in scenes]), dtype=torch.float64, device=DEV)
    B, nb = p.shape[:2]
    probe = ct.find_contacts(geom, p, maxc=1, eps=EPS)                         # (`count` keeps the full length)
    M = int(probe.count.max())
    cb = ct.find_contacts(geom, p, maxc=M, eps=EPS)
    gen = torch.Generator().manual_seed(31)
    gs = [torch.randn(B, M, 2, generator=gen).to(DEV) for _ in range(3)]
    rows = _rows(cb)
    contrib = _record_contributions(geom, p, cb, gs, rows)
    # what keeps the comparisons from passing vacuously
    k, r, a, b, slot, npair = rows
    cnt = cb.count.cpu().numpy()
    assert len(k) == int(cnt.sum()) == contrib.shape[0] and cnt[-1] == 0 and (cnt[:-1] > 0).all()
    pairs = int((slot == 0).sum())
    assert pairs >= 100 and int((slot == 1).sum()) >= 10, (pairs, int((slot == 1).sum()))
    in_pairs = np.zeros((B, nb), dtype=np.int64)
    np.add.at(in_pairs, (k[slot == 0], a[slot == 0]), 1)
    np.add.at(in_pairs, (k[slot == 0], b[slot == 0]), 1)
    assert in_pairs.max() >= 3
    print("%s: %d scenes, %d pairs, %d with two records, counts %d..%d, a body in up to %d pairs"
          % (name, B - 1, pairs, int((slot == 1).sum()), cnt[:-1].min(), M, in_pairs.max()))
    return dict(geom=geom, p=p, B=B, nb=nb, M=M, cb=cb, gs=gs, rows=rows, contrib=contrib, cnt=cnt)


def _check(L, dp, keep, what):
    exp = _expected((L["B"], L["nb"], 3), L["rows"], L["contrib"], keep)
    scale = max(1.0, np.abs(exp).max())
    err = np.abs(dp.cpu().numpy() - exp).max() / scale
    assert err <= GATE, (what, err)
    return exp


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_full_list_is_the_sum_of_its_records(name):
    """The whole list of every scene: dp is the sum of its records' pair-level gradients; the scene without a contact gets exactly
    zero; cotangent rows at or beyond the count do not enter, whatever they hold."""
    from lcp_physics_amd.physics import contacts as ct
    L = _layout(name)
    dp = ct.contact_frame_backward(L["geom"], L["p"], L["cb"], *L["gs"], eps=EPS)
    exp = _check(L, dp, np.ones(len(L["rows"][0]), dtype=bool), name)
    assert np.abs(exp).max() > 1.0
    assert float(dp[-1].abs().max()) == 0.0 and int(L["cb"].count[-1]) == 0
    dead = (torch.arange(L["M"], device=DEV).unsqueeze(0) >= L["cb"].count.unsqueeze(1)).unsqueeze(2)
    assert int(dead.sum()) > L["M"]
    zeros = ct.contact_frame_backward(L["geom"], L["p"], L["cb"], *[torch.where(dead, 0.0, g) for g in L["gs"]], eps=EPS)
    huge = ct.contact_frame_backward(L["geom"], L["p"], L["cb"], *[torch.where(dead, 1e30, g) for g in L["gs"]], eps=EPS)
    assert torch.equal(zeros, dp) and torch.equal(huge, dp)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_list_cut_at_every_capacity_is_the_sum_of_the_rows_that_fit(name):
    """Detection and backward at every `maxc` from 1 to the longest list: `count` keeps the full length, the rows at or beyond `maxc`
    do not count - also where the cut falls between the two records of a pair; cotangent rows beyond min(count, maxc) hold 1e30."""
    from lcp_physics_amd.physics import contacts as ct
    L = _layout(name)
    r, slot = L["rows"][1], L["rows"][4]
    split = 0
    for m in range(1, L["M"] + 1):
        cb = ct.find_contacts(L["geom"], L["p"], maxc=m, eps=EPS)
        assert torch.equal(cb.count, L["cb"].count)
        assert torch.equal(cb.c_i1, L["cb"].c_i1[:, :m]) and torch.equal(cb.c_n, L["cb"].c_n[:, :m])
        dead = (torch.arange(m, device=DEV).unsqueeze(0) >= cb.count.unsqueeze(1)).unsqueeze(2)
        gs = [torch.where(dead, 1e30, g[:, :m]).contiguous() for g in L["gs"]]
        dp = ct.contact_frame_backward(L["geom"], L["p"], cb, *gs, eps=EPS)
        _check(L, dp, r < m, (name, m))
        split += int(((r == m) & (slot == 1)).sum())                          # (row m - 1 is kept, its pair's second record is not)
        assert float(dp[-1].abs().max()) == 0.0
    assert split >= 1


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_masked_pairs_leave_the_list_and_later_rows_move_up(name):
    """`no_contact` on every third contacting pair of the odd scenes, detection and backward with the same mask: the masked pairs'
    rows are gone, the later rows move up and take their cotangent rows with them."""
    from lcp_physics_amd.physics import contacts as ct
    L = _layout(name)
    k, r, a, b, slot, npair = L["rows"]
    B, nb, M = L["B"], L["nb"], L["M"]
    mask = np.zeros((B, nb, nb), dtype=np.uint8)
    keep = np.ones(len(k), dtype=bool)
    before = 0
    for s in range(1, B, 2):
        first = np.nonzero((k == s) & (slot == 0))[0]                          # (the pairs of scene s in list order)
        for j in first[::3]:
            mask[s, a[j], b[j]] = mask[s, b[j], a[j]] = 1
            keep[j:j + npair[j]] = False
        before += int(len(first) >= 2)                                        # (pair 0 is masked, pair 1 follows it and is not)
    assert before >= 1 and (~keep).sum() >= 10
    g = L["geom"]
    geom = ct.GeometryBatch(g.kind, g.radius, g.verts_local, g.nverts, torch.tensor(mask, device=DEV), g.scene_verts_max)
    cb = ct.find_contacts(geom, L["p"], maxc=M, eps=EPS)
    # the masked list is the full list without the masked pairs' rows
    new_row = np.zeros(len(k), dtype=np.int64)
    for s in range(B):
        idx = np.nonzero((k == s) & keep)[0]
        new_row[idx] = np.arange(len(idx))
        assert int(cb.count[s]) == len(idx)
    kt, rt, nt = (torch.tensor(x[keep], device=DEV) for x in (k, r, new_row))
    assert torch.equal(cb.c_i1[kt, nt], L["cb"].c_i1[kt, rt]) and torch.equal(cb.c_i2[kt, nt], L["cb"].c_i2[kt, rt])
    assert torch.equal(cb.c_n[kt, nt], L["cb"].c_n[kt, rt]) and torch.equal(cb.c_p1[kt, nt], L["cb"].c_p1[kt, rt])
    assert int((nt < rt).sum()) >= 10
    # every surviving record keeps its cotangent, at its new row; the rows behind the list hold 1e30
    gs = []
    for g0 in L["gs"]:
        gm = torch.full_like(g0, 1e30)
        gm[kt, nt] = g0[kt, rt]
        gs.append(gm)
    dp = ct.contact_frame_backward(geom, L["p"], cb, *gs, eps=EPS)
    exp = _check(L, dp, keep, name)
    assert np.abs(exp).max() > 1.0 and float(dp[-1].abs().max()) == 0.0
