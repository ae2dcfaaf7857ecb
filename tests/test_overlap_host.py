"""CPU: the host mirror of the overlap query (tests/overlap_host.py: the rule of include/lcp_hip.h, "overlap queries") against an
independent yardstick, Sutherland-Hodgman clipping with the shoelace formula (`clip_area`), and `body_areas` / the IoU formula of
physics/overlap.py.

Bounds.  Hull against hull: |mirror - clip| <= 1e-10 R^2, R the pair's larger bounding radius (measured: 5e-11 at R <= 30 and
coordinates around 500 - the rounding of the clipped polygon's vertices at those coordinates times R).  With a circle the yardstick
clips the inscribed 4096-gon, which lacks pi r^2 - N/2 r^2 sin(2 pi / N) of the circle: that deficit, computed here, is added."""
import math

import numpy as np
import pytest
import torch

from tests import overlap_host as OH

F64 = torch.float64
TOL = 1e-10


def _R(c, b, k1, k2):
    return max(OH.bounding_radius(c, b, k1), OH.bounding_radius(c, b, k2))


def _valid(c, b, r):
    nb = c["kind"].shape[1]
    k1, k2 = int(c["pair_first"][b, r]), int(c["pair_second"][b, r])
    ok = k1 != k2 and 0 <= k1 < nb and 0 <= k2 < nb
    return ok and all(int(c["kind"][b, k]) == 0 or int(c["nverts"][b, k]) >= 3 for k in (k1, k2)), k1, k2


@pytest.mark.parametrize("name", OH.CASE_NAMES)
def test_the_mirror_against_the_clip(name):
    c, ref = OH.case(name), OH.reference(name)
    B, P = c["pair_first"].shape
    worst, positive = 0.0, 0
    for b in range(B):
        for r in range(P):
            ok, k1, k2 = _valid(c, b, r)
            got = float(ref["area"][b, r])
            if not ok:
                assert got == 0.0
                continue
            want, slack = OH.clip_pair(c, b, k1, k2)
            R2 = _R(c, b, k1, k2) ** 2
            assert got >= 0.0 and abs(got - want) <= slack + TOL * R2, (name, b, r, got, want)
            if slack == 0.0:
                worst = max(worst, abs(got - want) / R2)
            positive += got > 0.0
    print("%s: |mirror - clip| / R^2 over the hull pairs %.3g   pairs with area > 0: %d of %d" % (name, worst, positive, B * P))
    assert positive > 0 or name == "shared"


@pytest.mark.parametrize("what", OH.ROTATED_KINDS)
def test_300_pairs_that_share_edge_lines_at_generic_rotations(what):
    """Rects at one generic rotation that touch from outside, share two edge lines or rest on each other: the staged edges are
    parallel and on one line only up to rounding.  Both orders against the clip, and against each other."""
    worst, kinks = 0.0, 0
    for c in OH.rotated_pairs(what, 300):
        out = OH.overlaps_host(c)
        want = OH.clip_area(OH.world_polygon(c, 0, 0), OH.world_polygon(c, 0, 1))
        R2 = _R(c, 0, 0, 1) ** 2
        got = out["area"][0]
        assert abs(float(got[0]) - want) <= TOL * R2 and abs(float(got[1]) - want) <= TOL * R2, (what, got.tolist(), want)
        if what != "half":                                                                # touching from outside: nothing but the slivers
            assert float(got.max()) <= 1e-12 * R2                                         # of pieces a few roundings of t long, times R^2
        worst = max(worst, float((got - want).abs().max()) / R2)
        kinks += int(out["kink"].all())
    print("%s: |mirror - clip| / R^2 %.3g   pairs found on one line %d of 300" % (what, worst, kinks))
    assert kinks == 300


def test_300_random_hull_pairs_against_the_clip():
    worst, positive = 0.0, 0
    for c in OH.random_hull_pairs(300):
        got = float(OH.overlaps_host(c)["area"][0, 0])
        want = OH.clip_area(OH.world_polygon(c, 0, 0), OH.world_polygon(c, 0, 1))
        worst = max(worst, abs(got - want) / _R(c, 0, 0, 1) ** 2)
        positive += got > 0.0
    print("|mirror - clip| / R^2 %.3g   overlapping %d of 300" % (worst, positive))
    assert worst <= TOL and 100 <= positive < 300


@pytest.mark.parametrize("name", ["small", "wide", "big_hulls", "rotated"])
def test_symmetry(name):
    c, ref = OH.case(name), OH.reference(name)
    swapped = dict(c, pair_first=c["pair_second"], pair_second=c["pair_first"])
    back = OH.overlaps_host(swapped)["area"]
    B, P = c["pair_first"].shape
    for b in range(B):
        for r in range(P):
            k1, k2 = int(c["pair_first"][b, r]), int(c["pair_second"][b, r])
            assert abs(float(back[b, r] - ref["area"][b, r])) <= TOL * _R(c, b, k1, k2) ** 2, (b, r)


def _geom(c):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    return GeometryBatch(c["kind"], c["radius"], c["verts_local"], c["nverts"], None, None)


def test_nested_gives_the_inner_bodys_own_area():
    from lcp_physics_amd.physics.overlap import body_areas
    c, ref = OH.case("nested"), OH.reference("nested")
    own = body_areas(_geom(c))
    for r, k in enumerate(OH.NESTED_INNER):
        assert abs(float(ref["area"][0, r] - own[0, k])) <= TOL * OH.bounding_radius(c, 0, k) ** 2 + 1e-12 * float(own[0, k]), r
    assert not bool(ref["kink"].any())


def test_shared_boundaries_count_once():
    from lcp_physics_amd.physics.overlap import body_areas
    c, ref = OH.case("shared"), OH.reference("shared")
    own = body_areas(_geom(c))
    for r, want in enumerate(OH.SHARED_WANT):
        want = float(own[0, 4]) if want is None else want
        assert abs(float(ref["area"][0, r]) - want) <= TOL * 22.0 ** 2, (r, float(ref["area"][0, r]), want)
    assert float(ref["area"][0, 0]) == 0.0 and float(ref["area"][0, 1]) == 0.0 and float(ref["area"][0, 2]) == 2.0 and float(ref["area"][0, 3]) == 2.0
    assert bool(ref["kink"].all())


def test_invalid_pairs_and_scenes_over_the_vertex_limit():
    c, ref = OH.case("invalid"), OH.reference("invalid")
    assert float(ref["area"][0, :-1].abs().max()) == 0.0 and float(ref["area"][0, -1]) > 0.0
    w = OH.case("wide")
    total = int(torch.where(w["kind"] != 0, w["nverts"], torch.zeros_like(w["nverts"])).sum(1).max())
    assert float(OH.overlaps_host(w, scene_verts_max=total - 1)["area"][int(torch.where(w["kind"] != 0, w["nverts"], 0).sum(1).argmax())].abs().max()) == 0.0


def test_the_mirrors_autograd_against_central_differences_of_the_clip():
    """The pair rect (1) - triangle (2) of scene 0 of `small`, which overlaps partially: d(area) by the pose of body 1 (three entries)
    and by one vertex of the triangle (two entries) against central differences of `clip_area` at the step h = 1e-5.  The area is C1
    and piecewise C2, so a central difference errs by at most h max|f''| / 2; |f(x + h) - 2 f(x) + f(x - h)| / h, twice that for a
    constant f'', is the bound, plus the rounding of two clipped areas over 2 h: the clip's vertices carry 2^-52 X (X = 130, the
    coordinates), an area R times that (R = 30) from each of a handful of vertices - 16 2^-52 X R / h = 1.4e-6."""
    h = 1e-5
    c = OH.leaves(OH.case("small"))
    area = OH.overlaps_host(c)["area"][0, 2]
    assert float(area) > 10.0
    gp, gv = torch.autograd.grad(area, [c["p"], c["verts_local"]])

    def clip_at(leaf, idx, dx):
        d = {k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
        d[leaf][idx] += dx
        return OH.clip_area(OH.world_polygon(d, 0, 1), OH.world_polygon(d, 0, 2))

    floor = 16 * 2.0 ** -52 * 130.0 * 30.0 / h
    checks = [("p", (0, 1, i), float(gp[0, 1, i])) for i in range(3)] + [("verts_local", (0, 2, 1, i), float(gv[0, 2, 1, i])) for i in range(2)]
    seen = 0.0
    for leaf, idx, got in checks:
        f0, fp, fm = clip_at(leaf, idx, 0.0), clip_at(leaf, idx, h), clip_at(leaf, idx, -h)
        fd, bound = (fp - fm) / (2 * h), abs(fp - 2 * f0 + fm) / h + floor
        print("%s%s: autograd %.9g   central difference %.9g   bound %.3g" % (leaf, idx, got, fd, bound))
        assert abs(got - fd) <= bound, (leaf, idx)
        seen = max(seen, abs(got))
    assert seen > 1.0


def test_body_areas_and_the_iou_formula():
    from lcp_physics_amd.physics.overlap import body_areas, iou_of
    c = OH.leaves(OH.case("small"))
    own = body_areas(_geom(c))
    assert own.shape == c["kind"].shape and own.dtype == F64
    for b in range(c["kind"].shape[0]):
        for k in range(c["kind"].shape[1]):
            if int(c["kind"][b, k]) == 0:
                want = math.pi * float(c["radius"][b, k]) ** 2
            else:
                v = c["verts_local"][b, k, :int(c["nverts"][b, k])].detach().numpy()
                want = 0.5 * float(np.sum(v[:, 0] * np.roll(v[:, 1], -1) - np.roll(v[:, 0], -1) * v[:, 1]))
            assert abs(float(own[b, k]) - want) <= 1e-12 * want and want > 0, (b, k)
    gr, gv = torch.autograd.grad(own.sum(), [c["radius"], c["verts_local"]])
    circ = c["kind"] == 0
    assert torch.allclose(gr[circ], 2 * math.pi * c["radius"].detach()[circ], rtol=1e-14) and float(gr[~circ].abs().max()) == 0.0
    assert float(gv[0, 1, :4].abs().min()) > 0 and float(gv[0, 1, 4:].abs().max()) == 0.0 and float(gv[circ].abs().max()) == 0.0
    # slots >= nverts are not read, a hull of two vertices has no area
    d = OH.case("invalid")
    poisoned = dict(d, verts_local=d["verts_local"].clone())
    poisoned["verts_local"][0, 2, 2:] = float("nan")
    poisoned["verts_local"][0, 0] = float("nan")
    assert torch.equal(body_areas(_geom(poisoned)), body_areas(_geom(d))) and float(body_areas(_geom(d))[0, 2]) == 0.0
    # IoU: identical bodies 1, bodies apart 0, a body inside another the ratio of the areas, nothing at all 0
    a = torch.tensor([6.0, 0.0, 2.0, 0.0], dtype=F64)
    a1, a2 = torch.tensor([6.0, 3.0, 2.0, 0.0], dtype=F64), torch.tensor([6.0, 5.0, 15.0, 0.0], dtype=F64)
    assert iou_of(a, a1, a2).tolist() == [1.0, 0.0, 2.0 / 15.0, 0.0]
    ref = OH.reference("nested")["area"]
    on = body_areas(_geom(OH.case("nested")))
    assert abs(float(iou_of(ref[0, 0], on[0, 0], on[0, 1])) - (7.0 / 20.0) ** 2) <= 1e-12
