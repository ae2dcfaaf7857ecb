"""CPU: tests/golden/shape_grad.npz (tools/gen_shape_grad_golden.py: the unmodified reference's autograd with respect to
`Circle.rad` and `Hull.verts`) pinned against central finite differences of the fp64 numpy oracle (oracle/contacts_oracle.py)."""
import os

import numpy as np

from oracle import contacts_oracle as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shape_grad.npz")
H = 1e-5            # finite-difference step (lengths are 10 .. 40: truncation ~ H^2 / size^2, rounding ~ 1e-16 * 50 / H)
GATE = 9.1e-8       # ten times the measured worst case, see the docstring of the test


def _bodies(d, i, rad, verts):
    out = []
    for q in range(2):
        pos = d["f_pose"][i, q, 1:]
        if d["f_kind"][i, q] == 0:
            out.append(dict(kind="circle", pos=pos, rad=float(rad[q])))
        else:
            n = int(d["f_nverts"][i, q])
            out.append(dict(kind="hull", pos=pos, verts=verts[q, :n] @ C.rotation_matrix(d["f_pose"][i, q, 0]).T))
    return out


def _loss(d, i, rad, verts):
    recs = C.collide_pair(*_bodies(d, i, rad, verts), eps=float(d["f_eps"]))
    assert len(recs) == int(d["f_count"][i]), i              # (a finite-difference step never changes the record count)
    g = [d["f_g_n"][i].astype(np.float64), d["f_g_p1"][i].astype(np.float64), d["f_g_p2"][i].astype(np.float64)]
    return sum(float(g[q][c] @ r[q]) for c, r in enumerate(recs) for q in range(3))


def test_reference_shape_gradients_agree_with_finite_differences_of_the_oracle():
    """Every configuration of the frame-level fixture, every coordinate (both radii, every vertex of both hulls), no exclusions:
    |reference autograd - central difference of the oracle| / max(1, largest |gradient| of the configuration).
    Measured on the CPU the fixture was generated on: worst 9.06e-9 (step 1e-5); the gate is ten times that, because the
    step-size error is not controlled to better than an order."""
    d = np.load(GOLDEN)
    n = d["f_count"].shape[0]
    assert n >= 200 and sorted(set(d["f_rtype"].tolist())) == list(range(len(d["f_type_names"])))
    assert int(d["f_nverts"].max()) == 16 and (d["f_nverts"].max(axis=1) == 12).any()
    worst = 0.0
    for i in range(n):
        rad, verts = d["f_rad"][i].copy(), d["f_verts_local"][i].copy()
        # the fixture's records are the oracle's
        recs = C.collide_pair(*_bodies(d, i, rad, verts), eps=float(d["f_eps"]))
        for c, r in enumerate(recs):
            assert np.abs(r[0] - d["f_normal"][i, c]).max() < 1e-9 and np.abs(r[1] - d["f_p1"][i, c]).max() < 1e-8
            assert np.abs(r[2] - d["f_p2"][i, c]).max() < 1e-8 and abs(r[3] - d["f_pen"][i, c]) < 1e-8
        fd_r, fd_v = np.zeros(2), np.zeros_like(verts)
        for q in range(2):
            if d["f_kind"][i, q] == 0:
                a, b = rad.copy(), rad.copy()
                a[q] += H; b[q] -= H
                fd_r[q] = (_loss(d, i, a, verts) - _loss(d, i, b, verts)) / (2 * H)
            else:
                for k in range(int(d["f_nverts"][i, q])):
                    for x in range(2):
                        a, b = verts.copy(), verts.copy()
                        a[q, k, x] += H; b[q, k, x] -= H
                        fd_v[q, k, x] = (_loss(d, i, rad, a) - _loss(d, i, rad, b)) / (2 * H)
        scale = max(1.0, np.abs(d["f_d_rad"][i]).max(), np.abs(d["f_d_verts"][i]).max())
        err = max(np.abs(fd_r - d["f_d_rad"][i]).max(), np.abs(fd_v - d["f_d_verts"][i]).max()) / scale
        worst = max(worst, err)
    print("reference autograd against the oracle's central differences: worst relative difference %.3g" % worst)
    assert worst <= GATE, worst


def test_rollout_part_of_the_fixture_is_complete():
    d = np.load(GOLDEN)
    assert d["b_grad_rad"].shape == (8, 3) and d["b_ncontacts"].shape == (8, int(d["b_nsteps"])) and d["b_t"].shape == d["b_ncontacts"].shape
    assert d["x_grad_verts"].shape == (6, 4, 2) and d["x_grad_rad"].shape == (6,) and d["x_ncontacts"].shape == (6, int(d["x_nsteps"]))
    assert np.abs(d["x_grad_verts"]).max() > 1e-2 and np.isfinite(d["x_grad_verts"]).all()
    assert float(d["f_tie"]) == 1e-6 and int(d["f_rejected"]) >= 0
