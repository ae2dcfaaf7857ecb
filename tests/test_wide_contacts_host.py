"""CPU: the host side of the wide narrow phase (lcp_contacts_wide.hip) - `GeometryBatch.from_shapes(max_verts=...)`, the
refusals of the `_nv_` entries before any launch - and the contact oracle (oracle/contacts_oracle.py, which the GPU tests of
tests/test_hip_wide_contacts.py compare against) pinned on the unmodified reference for hulls of 9 to 48 vertices."""
import ctypes
import math
import random

import numpy as np
import pytest
import torch

from oracle import contacts_oracle as C
from oracle import ref_shim


def _ngon(rng, nv, rad):
    """A perturbed regular n-gon, counter-clockwise like the reference's Rect (bodies.py:261-264)."""
    ang = (np.arange(nv) + rng.uniform(-0.3, 0.3, nv)) * (2 * np.pi / nv) + rng.uniform(0, 2 * np.pi)
    r = rad * rng.uniform(0.9, 1.1, nv)
    return np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)


def test_from_shapes_max_verts():
    from lcp_physics_amd.physics.contacts import GeometryBatch
    rng = np.random.default_rng(0)
    h12, h40 = _ngon(rng, 12, 20.0), _ngon(rng, 40, 30.0)
    shapes = [("rect", (500.0, 10.0)), ("circle", 5.0), ("hull", h12), ("hull", h40)]
    g = GeometryBatch.from_shapes(shapes[:3], B=3, max_verts=16)
    assert tuple(g.verts_local.shape) == (3, 3, 16, 2) and g.nvcap == 16
    assert g.nverts.tolist() == [[4, 0, 12]] * 3 and g.kind.tolist() == [[1, 0, 1]] * 3
    assert g.scene_verts_max == 16 and g.wide
    assert torch.equal(g.verts_local[1, 2, :12], torch.tensor(h12)) and float(g.verts_local[:, 2, 12:].abs().max()) == 0.0
    assert float(g.verts_local[:, 0, 4:].abs().max()) == 0.0 and float(g.verts_local[:, 1].abs().max()) == 0.0
    g = GeometryBatch.from_shapes(shapes, B=2, max_verts=None)
    assert tuple(g.verts_local.shape) == (2, 4, 40, 2) and g.scene_verts_max == 56
    assert torch.equal(g.verts_local[0, 3], torch.tensor(h40))
    assert GeometryBatch.from_shapes(shapes[:2], max_verts=None).nvcap == 8           # (at least the default capacity)
    small = GeometryBatch.from_shapes(shapes[:2])
    assert small.nvcap == 8 and not small.wide
    # the cached total travels with to(), and is computed (once) when a batch is built by hand
    assert g.to("cpu").scene_verts_max == 56
    hand = GeometryBatch(g.kind, g.radius, g.verts_local, g.nverts, None)
    assert hand.scene_verts_max is None and hand.verts_max() == 56 and hand.scene_verts_max == 56
    with pytest.raises(ValueError):
        GeometryBatch.from_shapes([("hull", _ngon(rng, 65, 10.0))], max_verts=None)
    with pytest.raises(ValueError):
        GeometryBatch.from_shapes([("hull", _ngon(rng, 17, 10.0))], max_verts=16)
    with pytest.raises(ValueError):
        GeometryBatch.from_shapes([("hull", _ngon(rng, 9, 10.0))])                     # default: 8 vertices, as before
    with pytest.raises(ValueError):
        GeometryBatch.from_shapes([("circle", 1.0)], max_verts=65)


def _fake(n):
    # non-NULL addresses that are never dereferenced: the size checks come first (lcp_contacts_wide.hip)
    return [ctypes.c_void_p(4096 * (k + 1)) for k in range(n)]


@pytest.mark.parametrize("nb,nvcap,vmax", [(65, 8, 64), (40, 65, 64), (40, 7, 64), (12, 16, 1025), (64, 64, 2048)])
def test_wide_entries_refuse_sizes_before_any_launch(nb, nvcap, vmax):
    from lcp_physics_amd import _lib
    lib = _lib.load()
    P = _fake(7)
    rc = lib.lcp_move_find_contacts_nv_f64(4, nb, 16, nvcap, vmax, *P, 1.0 / 30, 1.0 / 120, 1, 8, 0.1, 1e-6, *_fake(12), None)
    assert rc == -2, rc                                                                   # LCP_E_TOOLARGE
    rc = lib.lcp_contact_frame_backward_nv_f64(4, nb, 16, nvcap, vmax, *_fake(6), 0.1, *_fake(7), None)
    assert rc == -2, rc
    # the existing entries keep their limit of 32 bodies
    if nb > 32:
        rc = lib.lcp_move_find_contacts_f64(4, nb, 16, *P, 1.0 / 30, 1.0 / 120, 1, 8, 0.1, 1e-6, *_fake(12), None)
        assert rc == -2, rc


def test_wide_frame_backward_refuses_lds_beyond_the_limit():
    from lcp_physics_amd import _lib
    lib = _lib.load()
    rc = lib.lcp_contact_frame_backward_nv_f64(4, 64, 4096, 64, 1024, *_fake(6), 0.1, *_fake(7), None)
    assert rc == -2, rc


def test_wide_paths_refuse_cpu_tensors():
    from lcp_physics_amd.physics.contacts import GeometryBatch, ContactBuffers, contact_frame_backward, find_contacts
    rng = np.random.default_rng(1)
    g = GeometryBatch.from_shapes([("hull", _ngon(rng, 20, 10.0)), ("circle", 3.0)], B=2, max_verts=None)
    p = torch.zeros(2, 2, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU"):
        find_contacts(g, p)
    cb = ContactBuffers(2, 2, 4, "cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        contact_frame_backward(g, p, cb, cb.c_n, cb.c_p1, cb.c_p2)


# ---- the oracle against the unmodified reference, hulls of 9 .. 48 vertices ---------------------------------------------
def _configs(rng, n):
    """(kind1, size1, kind2, size2, pose1, pose2): a perturbed n-gon against a circle, a rect or another n-gon, at centre
    distances from deep overlap to clearly apart, random rotations (no exact ties)."""
    out = []
    for k in range(n):
        nv1 = int(rng.integers(9, 49))
        r1 = float(rng.uniform(12, 35))
        other = ("circle", "rect", "hull")[k % 3]
        if other == "circle":
            s2, ext2 = float(rng.uniform(8, 30)), None
        elif other == "rect":
            s2 = (float(rng.uniform(10, 40)), float(rng.uniform(10, 40)))
        else:
            s2 = (int(rng.integers(9, 49)), float(rng.uniform(12, 35)))
        ext2 = s2 if other == "circle" else (0.5 * math.hypot(*s2) if other == "rect" else s2[1])
        ang = float(rng.uniform(0, 2 * np.pi))
        d = float(rng.uniform(0.3, 1.1)) * (r1 + ext2)
        pose1 = (float(rng.uniform(-np.pi, np.pi)), 300.0, 300.0)
        pose2 = (float(rng.uniform(-np.pi, np.pi)), 300.0 + d * math.cos(ang), 300.0 + d * math.sin(ang))
        out.append((("hull", (nv1, r1)), (other, s2), pose1, pose2, int(rng.integers(0, 2**31))))
    return out


def _ref_body(kind, size, pose, vrng):
    from lcp_physics.physics.bodies import Circle, Hull, Rect
    if kind == "circle":
        return Circle([pose[1], pose[2]], size)
    if kind == "rect":
        return Rect([pose[0], pose[1], pose[2]], [size[0], size[1]])
    R = C.rotation_matrix(pose[0])
    verts = _ngon(vrng, size[0], size[1]) @ R.T                                 # world-frame vertices around the reference point
    return Hull([pose[1], pose[2]], verts.tolist())


def _oracle_body(b):
    pos = b.pos.detach().numpy().astype(np.float64)
    if hasattr(b, "verts"):
        return dict(kind="hull", pos=pos, verts=np.stack([v.detach().numpy() for v in b.verts]).astype(np.float64))
    return dict(kind="circle", pos=pos, rad=float(b.rad))


@pytest.mark.skipif(not ref_shim.reference_available(), reason="needs the reference tree")
def test_oracle_matches_reference_on_hulls_of_9_to_48_vertices():
    ref_shim.load_reference()
    from oracle.make_golden_contacts import _FakeWorld, _run_pairs
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        rng = np.random.default_rng(4848)
        seen, total, kinds = 0, 0, set()
        for n, (a, b, pose1, pose2, vseed) in enumerate(_configs(rng, 150)):
            vrng = np.random.default_rng(vseed)
            random.seed(n)                                                         # (the GJK start vertex, as the generator sets it)
            bodies = [_ref_body(a[0], a[1], pose1, vrng), _ref_body(b[0], b[1], pose2, vrng)]
            try:
                ref = _run_pairs(_FakeWorld(bodies))
            except Exception:                                                      # (degenerate GJK configurations raise in the reference)
                continue
            ob = [_oracle_body(x) for x in bodies]
            pts = C.collide_pair(ob[0], ob[1], eps=0.1)
            assert len(pts) == len(ref), (n, len(pts), len(ref))
            for k, (nrm, p1, p2, pen) in enumerate(pts):
                rn, r1, r2, rp = (ref[k][0][q].detach().numpy() for q in range(4))
                assert np.allclose(nrm, rn.reshape(-1), atol=1e-9), (n, k, "normal")
                assert np.allclose(p1, r1.reshape(-1), atol=1e-8) and np.allclose(p2, r2.reshape(-1), atol=1e-8), (n, k, "arms")
                assert abs(pen - float(rp)) < 1e-8, (n, k, "pen")
            seen += 1
            total += len(pts)
            kinds.add((b[0], len(pts)))
    finally:
        torch.set_default_dtype(old)
    assert seen >= 140 and total >= 80
    for other in ("circle", "rect", "hull"):
        assert (other, 0) in kinds and (other, 1) in kinds, kinds
    assert ("hull", 2) in kinds or ("rect", 2) in kinds
