"""Generate tests/golden/frame_pose_grad.npz: what the UNMODIFIED reference's autograd gives the POSE of the bodies (rot, x, y)
through `DiffContactHandler` (physics/contacts.py:57-352), for the pair configurations stored in tests/golden/shape_grad.npz
(tools/gen_shape_grad_golden.py, `f_*`: every record type, 232 configurations, none within 1e-6 of a branch).  TEST
INFRASTRUCTURE ONLY; needs the reference tree (oracle/ref_shim.py) and runs on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_frame_pose_golden.py

Every configuration is replayed, not drawn again: `Circle` / `Hull` are built at the origin from the stored radius / body-frame
vertices, then `set_p` gets a pose tensor that is a leaf (a hull's vertices are turned by the increment, bodies.py:202-214, so the
rotation reaches normals, incident edges and clipped points).  The same two tie-breakers as the shape fixture: fresh bodies
(`last_sat_idx = 0`) and `random.choice` = first element.  The replayed count and records must equal the stored ones to 1e-9;
then sum g . (n, p1, p2) with the stored cotangents is back-propagated and `f_d_pose` [n, 2, 3] written, next to the sha256 of the
arrays that were replayed, so that a regenerated shape_grad.npz cannot drift from this file unnoticed
(tests/test_frame_pose_fixture.py compares the hash).  shape_grad.npz is only read.
"""
import hashlib
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from oracle import ref_shim  # noqa: E402
from gen_shape_grad_golden import _FakeWorld  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(HERE), "tests", "golden")
SRC = os.path.join(GOLDEN, "shape_grad.npz")
OUT = os.path.join(GOLDEN, "frame_pose_grad.npz")
# what a configuration is replayed from and checked against, in hashing order
REPLAYED = ("f_kind", "f_rad", "f_verts_local", "f_nverts", "f_pose", "f_g_n", "f_g_p1", "f_g_p2", "f_count", "f_normal", "f_p1",
            "f_p2", "f_eps")


def replayed_sha256(d):
    """sha256 over name, dtype, shape and bytes of the `REPLAYED` arrays of shape_grad.npz."""
    h = hashlib.sha256()
    for k in REPLAYED:
        a = np.ascontiguousarray(d[k])
        h.update(("%s %s %s;" % (k, a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def replay(d, i):
    """(records, pose leaves) of configuration i through the reference's handler."""
    from lcp_physics.physics.bodies import Circle, Hull
    from lcp_physics.physics.contacts import DiffContactHandler
    bodies, leaves = [], []
    for q in range(2):
        if d["f_kind"][i, q] == 0:
            b = Circle([0.0, 0.0], float(d["f_rad"][i, q]))
        else:
            b = Hull([0.0, 0.0], [list(v) for v in d["f_verts_local"][i, q, :int(d["f_nverts"][i, q])]])
        p = torch.tensor(d["f_pose"][i, q], dtype=torch.float64).requires_grad_(True)
        b.set_p(p)
        bodies.append(b); leaves.append(p)
    world = _FakeWorld(bodies, float(d["f_eps"]))
    DiffContactHandler()([world], bodies[0].geom, bodies[1].geom)
    return world.contacts, leaves


def main():
    ref_shim.load_reference()
    torch.set_default_dtype(torch.float64)
    random.choice = lambda seq: seq[0]                         # contacts.py:87: the GJK start vertex of a fresh body = vertex 0
    d = np.load(SRC)
    n = d["f_count"].shape[0]
    d_pose = np.zeros((n, 2, 3))
    worst = 0.0
    for i in range(n):
        cs, leaves = replay(d, i)
        assert len(cs) == int(d["f_count"][i]), (i, len(cs), int(d["f_count"][i]))
        for c, rc in enumerate(cs):
            assert (rc[1], rc[2]) == (0, 1), (i, rc[1], rc[2])
            for q, key in enumerate(("f_normal", "f_p1", "f_p2")):
                worst = max(worst, float(np.abs(rc[0][q].detach().numpy().reshape(-1) - d[key][i, c]).max()))
        assert worst <= 1e-9, (i, worst)
        g = [d[k][i].astype(np.float64) for k in ("f_g_n", "f_g_p1", "f_g_p2")]
        loss = sum((torch.tensor(g[q][c]) * rc[0][q]).sum() for c, rc in enumerate(cs) for q in range(3))
        loss.backward()
        d_pose[i] = np.stack([np.zeros(3) if p.grad is None else p.grad.numpy() for p in leaves])
    names = d["f_type_names"].tolist()
    top = [float(np.abs(d_pose[d["f_rtype"] == t]).max()) for t in range(len(names))]
    print("%d configurations replayed, records within %.2g of the stored ones; largest |d pose| per record type: %s"
          % (n, worst, dict(zip(names, ["%.3g" % t for t in top]))))
    np.savez_compressed(OUT, f_d_pose=d_pose, source_sha256=np.array(replayed_sha256(d)))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
