"""CPU: tests/golden/frame_pose_grad.npz (tools/gen_frame_pose_golden.py: the unmodified reference's autograd with respect to the
pose - rot, x, y - of both bodies of every configuration of tests/golden/shape_grad.npz) pinned against central finite differences
of the fp64 numpy oracle (oracle/contacts_oracle.py)."""
import hashlib
import os

import numpy as np

from oracle import contacts_oracle as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# what tools/gen_frame_pose_golden.py replayed and hashed, in its order
REPLAYED = ("f_kind", "f_rad", "f_verts_local", "f_nverts", "f_pose", "f_g_n", "f_g_p1", "f_g_p2", "f_count", "f_normal", "f_p1",
            "f_p2", "f_eps")
# finite-difference steps.  The loss is a sum of g . (n, p1, p2) with arms of 10 .. 40 around positions of 300: it is rounded at
# ~1e-16 * 300 = 3e-14, which a central difference turns into 3e-14 / H.  Positions: the third derivative is ~ gradient / size^2
# ~ 1e-3, truncation H^2 / 6 * 1e-3 - at H = 1e-5 both terms are below 1e-8.  Rotations: a derivative with respect to an angle
# multiplies by the lever (up to 35) each time, so the third derivative is some hundreds of |g| and the truncation ~ 1e2 H^2
# (measured: 5e-8 at 1e-5, 4.6e-7 at 3e-5); it balances the rounding at H^3 ~ 3e-14 / 1e3, H = 3e-6.
H_POS, H_ROT = 1e-5, 3e-6
GATE = 5.4e-8         # ten times the measured worst case, see the docstring of the test


def _sha256(d):
    h = hashlib.sha256()
    for k in REPLAYED:
        a = np.ascontiguousarray(d[k])
        h.update(("%s %s %s;" % (k, a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _bodies(d, i, pose):
    out = []
    for q in range(2):
        if d["f_kind"][i, q] == 0:
            out.append(dict(kind="circle", pos=pose[q, 1:], rad=float(d["f_rad"][i, q])))
        else:
            n = int(d["f_nverts"][i, q])
            out.append(dict(kind="hull", pos=pose[q, 1:], verts=d["f_verts_local"][i, q, :n] @ C.rotation_matrix(pose[q, 0]).T))
    return out


def _loss(d, i, pose):
    recs = C.collide_pair(*_bodies(d, i, pose), eps=float(d["f_eps"]))
    assert len(recs) == int(d["f_count"][i]), i              # (a finite-difference step never changes the record count)
    g = [d["f_g_n"][i].astype(np.float64), d["f_g_p1"][i].astype(np.float64), d["f_g_p2"][i].astype(np.float64)]
    return sum(float(g[q][c] @ r[q]) for c, r in enumerate(recs) for q in range(3))


def _worst(d, dp, h_pos, h_rot):
    """Largest |reference autograd - central difference of the oracle| / max(1, largest |gradient| of the configuration), per
    record type."""
    per_type = np.zeros(len(d["f_type_names"]))
    for i in range(dp.shape[0]):
        fd = np.zeros((2, 3))
        for q in range(2):
            for c in range(3):
                h = h_rot if c == 0 else h_pos
                a, b = d["f_pose"][i].copy(), d["f_pose"][i].copy()
                a[q, c] += h; b[q, c] -= h
                fd[q, c] = (_loss(d, i, a) - _loss(d, i, b)) / (2 * h)
        t = int(d["f_rtype"][i])
        per_type[t] = max(per_type[t], np.abs(fd - dp[i]).max() / max(1.0, np.abs(dp[i]).max()))
    return per_type


def test_fixture_belongs_to_the_shape_fixture_it_was_replayed_from():
    d, f = np.load(os.path.join(GOLDEN, "shape_grad.npz")), np.load(os.path.join(GOLDEN, "frame_pose_grad.npz"))
    assert str(f["source_sha256"]) == _sha256(d)
    assert f["f_d_pose"].shape == (d["f_count"].shape[0], 2, 3) and f["f_d_pose"].dtype == np.float64
    assert np.isfinite(f["f_d_pose"]).all()


def test_reference_pose_gradients_agree_with_finite_differences_of_the_oracle():
    """Every configuration of the frame-level fixture, all six pose coordinates (rot, x, y of both bodies), no exclusions:
    |reference autograd - central difference of the oracle| / max(1, largest |gradient| of the configuration).
    Measured on the CPU the fixture was generated on: worst 5.35e-9 (steps 1e-5 on positions, 3e-6 on rotations; 2.6e-7 at
    1e-6 / 1e-7); the gate, 5.4e-8, is ten times that, because the step-size error is not controlled to better than an order."""
    d, f = np.load(os.path.join(GOLDEN, "shape_grad.npz")), np.load(os.path.join(GOLDEN, "frame_pose_grad.npz"))
    dp = f["f_d_pose"]
    names = d["f_type_names"].tolist()
    assert dp.shape[0] == d["f_count"].shape[0] >= 200 and sorted(set(d["f_rtype"].tolist())) == list(range(len(names)))
    # every record type moves with the pose
    top = [float(np.abs(dp[d["f_rtype"] == t]).max()) for t in range(len(names))]
    assert min(top) > 0.1, dict(zip(names, top))
    # a circle's rotation reaches nothing
    assert np.abs(dp[..., 0][d["f_kind"] == 0]).max() == 0.0
    per_type = _worst(d, dp, H_POS, H_ROT)
    print("reference pose autograd against the oracle's central differences, worst relative difference per record type:",
          dict(zip(names, ["%.3g" % e for e in per_type])))
    assert per_type.max() <= GATE, per_type.max()
