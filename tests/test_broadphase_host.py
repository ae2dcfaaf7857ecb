"""CPU: the broadphase of lcp_contacts_bp.hip (`lcp_move_find_contacts_bp_f64`) - the ctypes signature against the header's
declaration, and the cull rule (tests/broadphase_host.py) against the reference's contact lists: it must keep every pair that has a
record (the reference fixtures tests/golden/contacts_*.npz, the contact oracle on piles of 12 .. 64 bodies) and, on piles, keep at most
a quarter of the pairs."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import contacts_oracle as C
from oracle import world_oracle as W
from tests import broadphase_host as BH

NAME = "lcp_move_find_contacts_bp_f64"


def _ctype(decl):
    decl = decl.strip()
    if "*" in decl:
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "double": ctypes.c_double, "float": ctypes.c_float}[decl.split()[-2]]


def _declared(header, name):
    """ctypes argument list of the declaration of `name` in the header text."""
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, header, re.S)
    assert m, name
    return [_ctype(a) for a in m.group(1).split(",")]


def test_signature_matches_the_header():
    from lcp_physics_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "lcp_hip.h")).read()
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and getattr(lib, NAME).argtypes == args
    assert args == _declared(header, NAME)
    # the arguments of the _dts_ entry in the same order, then dt_scene's successor `candidates`, then the stream
    dts = _declared(header, "lcp_move_find_contacts_dts_f64")
    assert args == dts[:-1] + [ctypes.c_void_p, ctypes.c_void_p] and len(args) == 33
    doc = header[:header.index("int %s(" % NAME)][-3000:]
    assert "world.py:139-142" in doc and "bodies.py:_create_geom" in doc and "bitwise" in doc


# the four detection entries: has the entry the (nvcap, scene_verts_max) arguments, a dt_scene, a candidates argument ?
ENTRIES = {"lcp_move_find_contacts_f64": (False, False, False), "lcp_move_find_contacts_nv_f64": (True, False, False),
           "lcp_move_find_contacts_dts_f64": (True, True, False), NAME: (True, True, True)}
BADARG, TOOLARGE, ACCEPTED = -1, -2, -3      # ACCEPTED: the checks passed; without a GPU the launch itself fails (LCP_E_LAUNCH)


def test_sizes_and_required_pointers_are_checked_before_any_launch():
    """The argument and size errors of the four detection entries, with stand-in pointers: every refusal returns before a launch,
    LCP_E_BADARG before LCP_E_TOOLARGE, and the sizes at the edge of each entry's limits are accepted.  Only where no GPU is present, so
    that a regression of these checks cannot launch a kernel on such addresses (an accepted call then fails at the launch and reads no
    pointer); tests/test_hip_broadphase.py repeats the cases of the _bp_ entry with device buffers."""
    import torch
    from lcp_physics_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_hip_broadphase.py checks these cases with device buffers")
    lib = _lib.load()
    for name in ENTRIES:
        _check_refusals(lib, name)


def _check_refusals(lib, name):
    sized, has_dts, has_cand = ENTRIES[name]
    small = not sized                                                        # lcp_contacts.hip alone: 8 vertices, 32 bodies
    fake = lambda n: [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(n)]

    def call(nb=12, nvcap=16, vmax=64, B=4, maxc=16, trials=8, geo=None, outs=None, dt_scene=ctypes.c_void_p(0xa000)):
        geo = fake(4) if geo is None else geo
        outs = fake(12) if outs is None else outs
        sizes = (B, nb, maxc) + ((nvcap, vmax) if sized else ())
        tail = ((dt_scene,) if has_dts else ()) + ((None,) if has_cand else ()) + (None,)      # .., candidates, stream
        return getattr(lib, name)(*sizes, *geo, None, ctypes.c_void_p(0x9000), None, 1.0 / 30, 1.0 / 120, 1, trials, 0.1, 1e-6, *outs,
                                  *tail)

    assert call(nb=33) == (TOOLARGE if small else ACCEPTED), name
    assert call(nb=65) == TOOLARGE
    if sized:
        for kw in (dict(nvcap=7), dict(nvcap=65), dict(vmax=1025)):
            assert call(**kw) == TOOLARGE, kw
        assert call(vmax=-1) == BADARG
    for kw in (dict(B=0), dict(nb=0), dict(maxc=0), dict(trials=0)):
        assert call(**kw) == BADARG, kw
    assert call(nb=65, vmax=-1) == (TOOLARGE if small else BADARG)           # (no scene_verts_max argument: the size alone)
    if has_dts:
        assert call(dt_scene=None) == (ACCEPTED if has_cand else BADARG)     # (_bp_: NULL = the scalar dt)
    for k in range(4):                                                       # kind radius verts_local nverts
        geo = fake(4)
        geo[k] = None
        assert call(geo=geo) == BADARG, k
        if k == 0:
            assert call(nb=65, geo=geo) == BADARG
    for k in (1, 2, 3, 5, 6, 7):                                             # c_n c_p1 c_p2 c_i1 c_i2 count
        outs = fake(12)
        outs[k] = None
        assert call(outs=outs) == BADARG, k
    accepted = [dict(), dict(nb=32)] if small else [dict(), dict(nb=64, nvcap=8), dict(nb=32, nvcap=8), dict(nvcap=64), dict(vmax=0),
                                                    dict(vmax=1024)]
    for kw in accepted:
        assert call(**kw) == ACCEPTED, kw


def _shape(kind, size):
    return ("circle", float(size[0])) if int(kind) == 0 else ("rect", (float(size[0]), float(size[1])))


def test_rule_keeps_every_contact_pair_of_the_pair_fixture():
    """tests/golden/contacts_pairs.npz: 600 reference outputs, one pair per scene, 543 with a contact."""
    from tests.test_contacts_oracle import GOLD
    d = np.load(os.path.join(GOLD, "contacts_pairs.npz"))
    n, hit = len(d["count"]), 0
    assert n == 600
    for i in range(n):
        shapes = [_shape(d["kind"][i, 0], d["size"][i, 0]), _shape(d["kind"][i, 1], d["size"][i, 1])]
        cand, _ = BH.candidate_pairs(W.bodies_at(shapes, d["pos"][i]))
        if int(d["count"][i]) > 0:
            assert cand == [(0, 1)], i
            hit += 1
    assert hit == 543


def test_rule_keeps_every_contact_pair_of_the_scene_fixture():
    """tests/golden/contacts_scenes.npz: 60 multi-body scenes of the reference, 152 contact pairs."""
    from tests.test_contacts_oracle import GOLD
    d = np.load(os.path.join(GOLD, "contacts_scenes.npz"))
    assert int(d["n"]) == 60
    npairs = 0
    for s in range(int(d["n"])):
        g = lambda k: d["s%d_%s" % (s, k)]
        shapes = [_shape(k, z) for k, z in zip(g("kind"), g("size"))]
        cand, _ = BH.candidate_pairs(W.bodies_at(shapes, g("pos")))
        pairs = sorted({(int(a), int(b)) for a, b in zip(g("i1"), g("i2"))})
        assert set(pairs) <= set(cand), (s, sorted(set(pairs) - set(cand)))
        npairs += len(pairs)
    assert npairs == 152


@pytest.mark.parametrize("nb,B,nvr,cap", [p for p in BH.PILES if p[0] >= 12], ids=lambda v: str(v))
def test_rule_on_piles_keeps_the_contact_pairs_and_a_quarter_of_the_pairs_at_most(nb, B, nvr, cap):
    kept, checked = [], 0
    for shapes, pose in BH.piles(nb, B, nvr):
        bodies = W.bodies_at(shapes, pose)
        cand, _ = BH.candidate_pairs(bodies)
        assert cand == sorted(cand)
        share = len(cand) / (nb * (nb - 1) // 2)
        assert share <= 0.25, (nb, share)
        kept.append(share)
        try:
            ref = C.find_contacts(bodies, eps=BH.EPS)
        except ValueError:                  # get_closest raises on a degenerate simplex (contacts.py:330): no reference answer
            continue
        pairs = BH.contact_pairs(ref)
        assert set(pairs) <= set(cand), (nb, sorted(set(pairs) - set(cand)))
        checked += len(pairs)
    print("nb %d: share of pairs kept, worst %.3f mean %.3f; %d contact pairs checked" % (nb, max(kept), float(np.mean(kept)), checked))
    assert checked >= nb // 2


def test_special_scenes():
    """The plank scene: all 78 pairs are candidates, 24 records from the 12 neighbour pairs at the stated pair indices; the far scene:
    no candidate; a mask removes candidates."""
    shapes, pose = BH.plank_scene()
    bodies = W.bodies_at(shapes, pose)
    cand, _ = BH.candidate_pairs(bodies)
    assert len(cand) == 78
    ref = C.find_contacts(bodies, eps=BH.EPS)
    assert len(ref) == 24 and BH.contact_pairs(ref) == [(k, k + 1) for k in range(12)]
    index = {pr: q for q, pr in enumerate((i, j) for i in range(13) for j in range(i + 1, 13))}
    assert [index[pr] for pr in BH.contact_pairs(ref)] == [0, 12, 23, 33, 42, 50, 57, 63, 68, 72, 75, 77]
    shapes, pose = BH.far_scene()
    assert BH.candidate_pairs(W.bodies_at(shapes, pose))[0] == []
    shapes, pose = BH.piles(12, 1, (3, 9))[0]
    cand, _ = BH.candidate_pairs(W.bodies_at(shapes, pose))
    masked, _ = BH.candidate_pairs(W.bodies_at(shapes, pose), no_contact=cand[::2])
    assert masked == cand[1::2] and len(masked) < len(cand)


def _distance_rule_keeps(bodies, eps=BH.EPS):
    """Would a bound on the DISTANCE between the bodies (bounding circles and boxes at most eps apart) keep the pair?  Not the rule:
    the yardstick that shows the scenes below are the ones such a bound loses."""
    (Ra, _, loa, hia, _, _), (Rb, _, lob, hib, _, _) = BH.bounds(bodies[0]), BH.bounds(bodies[1])
    d = bodies[1]["pos"] - bodies[0]["pos"]
    gaps = np.concatenate([d + lob - hia, loa - d - hib])
    return float(d @ d) <= (Ra + Rb + eps) ** 2 and bool((gaps <= eps).all())


@pytest.mark.parametrize("d", [0.05, 0.08, 0.09, 0.099])
def test_corner_to_corner_rects_keep_their_record(d):
    """Two squares whose corners are sqrt(2) d apart: the separations along the edge normals are d <= eps, the narrow phase reports the
    clip's extrapolated point, and the rule keeps the pair although the bodies are more than eps apart."""
    shapes, pose = BH.corner_scene(d)
    bodies = W.bodies_at(shapes, pose)
    ref = C.find_contacts(bodies, eps=BH.EPS)
    assert len(ref) == 1 and abs(ref[0][0][3] + d) < 1e-9
    assert BH.candidate_pairs(bodies)[0] == [(0, 1)]
    assert _distance_rule_keeps(bodies) == (np.sqrt(2) * d <= BH.EPS)


def test_rule_keeps_every_record_of_a_near_corner_search():
    """3000 seeded hull pairs with two corners within a few eps of each other (rects, needle triangles, n-gons, any rotation): every pair
    the oracle reports a record for is a candidate; dozens of them are pairs a bound on the distance would have dropped."""
    records, beyond = 0, 0
    for shapes, pose in BH.near_corner_pairs(3000):
        bodies = W.bodies_at(shapes, pose)
        try:
            ref = C.find_contacts(bodies, eps=BH.EPS)
        except ValueError:
            continue
        if ref:
            records += 1
            assert BH.candidate_pairs(bodies)[0] == [(0, 1)], (shapes, pose.tolist())
            beyond += not _distance_rule_keeps(bodies)
    print("near-corner search: %d pairs with a record, %d of them beyond a distance bound" % (records, beyond))
    assert records >= 1000 and beyond >= 20
