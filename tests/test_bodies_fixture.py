"""CPU: tests/golden/bodies.npz (tools/gen_bodies_golden.py: the unmodified reference's `Circle` / `Rect` / `Hull` constructors with
`Gravity` attached, and its autograd with respect to raw vertices, radius, dims and mass) pinned by identities that do not depend on
the product, and reproduced live where the reference tree is present."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "bodies.npz")
NV_CHOICES = [3, 4, 5, 6, 8, 12, 16, 31, 32, 33, 64]


def _fixture():
    return np.load(PATH)


def test_the_fixture_is_small_numeric_and_covers_the_vertex_counts():
    d = _fixture()
    assert os.path.getsize(PATH) < 200 * 1024
    assert all(d[k].dtype.kind in "fiu" for k in d.files)
    kind, nv = d["m_kind"], d["m_nverts"]
    assert 100 <= len(kind) <= 140 and (kind == 0).sum() >= 10 and (kind == 1).sum() >= 10
    assert sorted(set(nv[kind == 2].tolist())) == NV_CHOICES and (nv[kind == 1] == 4).all() and (nv[kind == 0] == 0).all()
    assert d["m_mass"].min() >= 0.5 and d["m_mass"].max() <= 5.0
    off = np.abs(d["m_centroid"][kind == 2]).max(axis=1)
    assert (off > 40).sum() >= 20 and (off < 40).sum() >= 20 and off.max() <= 340            # about half are offset, by up to 300
    # the generator's own check of the summation-order spread: 1e-13, and what it accepted lies well below the 1e-12 gate
    assert float(d["m_shift_tol"]) == 1e-13 and float(d["m_shift_worst"]) <= 1e-13 and int(d["m_rejected"]) <= 12


def test_rect_inertia_is_m_w2_plus_h2_over_12():
    d = _fixture()
    r = d["m_kind"] == 1
    want = d["m_mass"][r] * (d["m_dims"][r] ** 2).sum(axis=1) / 12
    assert np.abs(d["m_inertia"][r] / want - 1).max() <= 1e-13
    # d(sum cot . values)/d(dims) contains g_I m dims / 6; the rest of it goes through the vertices: zero centroid, verts = +-dims / 2
    gI = d["m_g_inertia"][r] + d["m_g_Mdiag"][r, 0]
    sg = np.array([[1, 1], [-1, 1], [-1, -1], [1, -1]], dtype=np.float64)
    want_d = gI[:, None] * d["m_mass"][r, None] * d["m_dims"][r] / 6 + (d["m_g_verts"][r, :4] * sg).sum(axis=1) / 2
    # (+ the centroid's share: d(centroid)/d(dims) = 0 for a box by symmetry)
    assert np.abs(d["m_d_dims"][r] - want_d).max() <= 1e-12 * max(1.0, np.abs(want_d).max())


def test_circle_records():
    d = _fixture()
    c = d["m_kind"] == 0
    m, r = d["m_mass"][c], d["m_radius"][c]
    assert np.array_equal(d["m_inertia"][c], m * r * r / 2) and np.abs(d["m_centroid"][c]).max() == 0.0
    gI = d["m_g_inertia"][c] + d["m_g_Mdiag"][c, 0]
    assert np.abs(d["m_d_radius"][c] - gI * m * r).max() <= 1e-13 * np.abs(d["m_d_radius"]).max()
    assert np.abs(d["m_d_verts_raw"][c]).max() == 0.0


def test_recentred_vertices_have_their_centroid_at_zero_and_raw_minus_centroid_is_verts():
    d = _fixture()
    for i in np.nonzero(d["m_kind"] != 0)[0]:
        nv = int(d["m_nverts"][i])
        u = d["m_verts"][i, :nv]
        w = np.roll(u, -1, axis=0)
        x = w[:, 0] * u[:, 1] - w[:, 1] * u[:, 0]                                          # cross_2d(v2, v1), utils.py:93-96
        c = (x[:, None] * (u + w)).sum(axis=0) / (3 * x.sum())
        rad = np.sqrt((u ** 2).sum(axis=1)).max()
        assert np.abs(c).max() <= 1e-12 * rad, (i, c)
        assert np.abs(d["m_verts"][i, nv:]).max(initial=0.0) == 0.0
        assert np.array_equal(d["m_verts_raw"][i, :nv] - d["m_centroid"][i], u) or \
            np.abs(d["m_verts_raw"][i, :nv] - d["m_centroid"][i] - u).max() <= 1e-12 * rad
        assert ((w[:, 0] - u[:, 0]) * (w[:, 1] + u[:, 1])).sum() < 0                      # bodies.py:228-235


def test_mass_matrix_and_gravity():
    d = _fixture()
    assert np.array_equal(d["m_Mdiag"], np.stack([d["m_inertia"], d["m_mass"], d["m_mass"]], axis=1))
    z = np.zeros_like(d["m_mass"])
    assert np.array_equal(d["m_f"], np.stack([z, z, d["m_mass"] * float(d["m_g"])], axis=1))
    # the cotangents of the two fp32 outputs are fp32 numbers
    for k in ("m_g_Mdiag", "m_g_f"):
        assert np.array_equal(d[k], d[k].astype(np.float32).astype(np.float64))
    # d/d(mass) = g_I I / m + g_M[1] + g_M[2] + g g_f[2]
    gI = d["m_g_inertia"] + d["m_g_Mdiag"][:, 0]
    want = gI * d["m_inertia"] / d["m_mass"] + d["m_g_Mdiag"][:, 1] + d["m_g_Mdiag"][:, 2] + float(d["m_g"]) * d["m_g_f"][:, 2]
    assert np.abs(d["m_d_mass"] - want).max() <= 1e-12 * np.abs(want).max()


def test_rollout_records():
    d = _fixture()
    n, steps = d["r_force_ball"].shape[0], int(d["r_nsteps"])
    assert n == 6 and steps == 40 and d["r_ncontacts"].shape == (n, steps) and d["r_t"].shape == (n, steps)
    assert d["r_grad_verts"].shape == (n, 4, 2) and d["r_grad_mass"].shape == (n, 2) and d["r_grad_rad"].shape == (n,)
    assert np.abs(d["r_grad_mass"]).min() > 0.1 and np.abs(d["r_grad_verts"]).min() > 0.01 and np.abs(d["r_grad_rad"]).min() > 0.1
    # the box's raw vertices are not centred on its reference point: position = reference point + centroid
    c = d["r_box_verts_raw"].mean(axis=0)
    assert np.abs(c).min() >= 3.0 and np.abs(d["r_p0"][:, 2, 1:] - (d["r_box_ref"] + c)).max() <= 1e-12
    assert (d["r_ncontacts"].max(axis=1) >= 2).all()


@pytest.mark.skipif(not ref_shim.reference_available(), reason="needs the reference tree")
def test_module_level_values_reproduced_live_on_the_reference():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_bodies_golden", os.path.join(ROOT, "tools", "gen_bodies_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ref_shim.load_reference()
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        live = gen.module_level(np.random.default_rng(gen.SEED))
    finally:
        torch.set_default_dtype(old)
    d = _fixture()
    for k, v in live.items():
        assert np.array_equal(np.asarray(v), d[k]), k
