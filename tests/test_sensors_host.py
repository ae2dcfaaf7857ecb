"""CPU: the host mirror of the ray caster (tests/sensors_host.py) against answers known by hand, the edge rules of the header
(include/lcp_hip.h, "range sensors"), central differences of itself, and the condition the GPU comparison puts on its cases: at most
2 % of a case's rays are ones the mirror cannot decide."""
import math

import pytest
import torch

from tests import sensors_host as SH
from tests.render_host import _rect

F64 = torch.float64


def _scene(bodies, rays, cap=8):
    c = SH._assemble([bodies], cap)
    c.update(SH._rays([rays]))
    return c


def _cast(bodies, rays):
    out = SH.cast_host(_scene(bodies, rays))
    return out["dist"][0], out["hit"][0], out["normal"][0]


# ------------------------------------------------------------------------------------------------------------- known answers
def test_a_ray_along_x_meets_a_circle_of_radius_2_at_10_at_distance_8():
    d, k, n = _cast([("circle", (0.0, 10.0, 0.0), 2.0)], [(-1, (0.0, 0.0), 0.0, 100.0)])
    assert float(d[0]) == 8.0 and int(k[0]) == 0 and n[0].tolist() == [-1.0, 0.0]


def test_a_ray_meets_an_axis_aligned_rect_at_a_known_face():
    rect = ("hull", (0.0, 10.0, 0.0), _rect(4.0, 6.0))                                  # x in [8, 12], y in [-3, 3]
    d, k, n = _cast([rect], [(-1, (0.0, 1.0), 0.0, 100.0), (-1, (10.5, 20.0), -math.pi / 2, 100.0), (-1, (20.0, -1.0), math.pi, 100.0)])
    assert torch.allclose(d, torch.tensor([8.0, 17.0, 8.0], dtype=F64), rtol=0, atol=1e-13) and k.tolist() == [0, 0, 0]
    assert torch.allclose(n, torch.tensor([[-1.0, 0.0], [0.0, 1.0], [1.0, 0.0]], dtype=F64), rtol=0, atol=1e-15)


def test_a_ray_at_45_degrees_meets_a_rotated_square():
    """A square of side 2 turned by 45 degrees at (10, 10): corners at (10 -+ sqrt 2, 10) and (10, 10 -+ sqrt 2).  The ray from (1, 0)
    at 45 degrees runs along x - y = 1 and meets the face x + y = 20 - sqrt 2 (between the corners at x - y = -+ sqrt 2) at
    s = (19 - sqrt 2) / sqrt 2, where the outward normal is (-1, -1) / sqrt 2."""
    sq = ("hull", (math.pi / 4, 10.0, 10.0), _rect(2.0, 2.0))
    d, k, n = _cast([sq], [(-1, (1.0, 0.0), math.pi / 4, 100.0)])
    r2 = math.sqrt(2.0)
    assert abs(float(d[0]) - (19.0 - r2) / r2) < 1e-13 and int(k[0]) == 0
    assert torch.allclose(n[0], torch.tensor([-1.0 / r2, -1.0 / r2], dtype=F64), rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------------------------------------- edge rules
def test_an_origin_inside_a_body_gives_zero_and_no_normal():
    bodies = [("circle", (0.0, 10.0, 0.0), 2.0), ("hull", (0.3, 30.0, 0.0), _rect(4.0, 6.0))]
    d, k, n = _cast(bodies, [(-1, (10.5, 0.5), 1.0, 100.0), (-1, (30.5, 0.5), 2.0, 100.0), (-1, (12.0, 0.0), 0.0, 100.0)])
    assert d.tolist() == [0.0, 0.0, 0.0] and k.tolist() == [0, 1, 0] and float(n.abs().max()) == 0.0      # (the last: on the circle)


def test_a_ray_parallel_to_an_edge_and_outside_it_misses():
    rect = ("hull", (0.0, 10.0, 0.0), _rect(4.0, 6.0))
    d, k, n = _cast([rect], [(-1, (0.0, 3.5), 0.0, 100.0), (-1, (0.0, 2.5), 0.0, 100.0)])
    assert d.tolist() == [100.0, 8.0] and k.tolist() == [-1, 0]


def test_a_ray_that_stops_short_returns_its_range():
    d, k, n = _cast([("circle", (0.0, 10.0, 0.0), 2.0)], [(-1, (0.0, 0.0), 0.0, 7.5), (-1, (0.0, 0.0), 0.0, 8.0), (-1, (0.0, 0.0), math.pi, 50.0)])
    assert d.tolist() == [7.5, 8.0, 50.0] and k.tolist() == [-1, -1, -1] and float(n.abs().max()) == 0.0   # (s >= range: clamped)


def test_the_mounting_body_is_skipped_and_a_bad_mount_misses():
    bodies = [("circle", (math.pi / 2, 0.0, 0.0), 5.0), ("circle", (0.0, 0.0, 20.0), 2.0)]
    # mounted on body 0 (turned by 90 degrees): origin (1, 0) -> world (0, 1), angle 0 -> world +y: body 1 at 20 - 2 - 1
    d, k, n = _cast(bodies, [(0, (1.0, 0.0), 0.0, 100.0), (-1, (0.0, 1.0), math.pi / 2, 100.0), (2, (0.0, 1.0), 0.0, 100.0),
                             (-2, (0.0, 1.0), 0.0, 100.0)])
    assert abs(float(d[0]) - 17.0) < 1e-13 and k.tolist() == [1, 0, -1, -1] and d[1:].tolist() == [0.0, 100.0, 100.0]


def test_the_smaller_index_wins_a_tie_and_a_two_vertex_hull_is_never_hit():
    twin = ("circle", (0.0, 10.0, 0.0), 2.0)
    stick = ("hull", (0.0, 5.0, 0.0), [[0.0, -3.0], [0.0, 3.0]])
    d, k, n = _cast([stick, twin, twin], [(-1, (0.0, 0.0), 0.0, 100.0)])
    assert float(d[0]) == 8.0 and int(k[0]) == 1


def test_a_scene_over_the_vertex_limit_is_not_sensed():
    c = _scene([("hull", (0.0, 10.0, 0.0), _rect(4.0, 6.0))], [(-1, (0.0, 0.0), 0.0, 100.0)])
    assert SH.cast_host(c, scene_verts_max=4)["hit"].tolist() == [[0]] and SH.cast_host(c, scene_verts_max=3)["hit"].tolist() == [[-1]]


# ------------------------------------------------------------------------------------------------------------- the cases
def test_the_named_rays_of_small_are_what_they_are_called():
    ref, nm = SH.reference("small"), SH.case("small")["names"]
    d, k, ex = ref["dist"], ref["hit"], ref["excluded"]
    rng = SH.case("small")["ray_range"]
    for r in (nm["miss"], nm["clamp"], nm["parallel_outside"], nm["body_high"], nm["body_low"]):
        assert k[:, r].tolist() == [-1] * 3 and torch.equal(d[:, r], rng[:, r]), r
    assert k[:, nm["inside_circle"]].tolist() == [0] * 3 and k[:, nm["inside_rect"]].tolist() == [1] * 3
    assert float(d[:, [nm["inside_circle"], nm["inside_rect"]]].abs().max()) == 0.0
    assert k[:, nm["parallel_between"]].tolist() == [1] * 3 and float((d[:, nm["parallel_between"]] - 20.0).abs().max()) < 1e-12
    assert torch.equal(ref["normal"][:, nm["parallel_between"]], torch.tensor([[-1.0, 0.0]] * 3, dtype=F64))
    assert k[:, nm["vertex"]].tolist() == [1] * 3
    want = torch.tensor([math.hypot(50.0, 45.0)] * 3, dtype=F64)
    assert float((d[:, nm["vertex"]] - want).abs().max()) < 1e-9
    body = SH.case("small")["ray_body"]
    assert sorted(set(body.flatten().tolist())) == [-2, -1, 0, 1, 2, 3, 4, 7]             # every kind of body mounts a ray
    assert int((k == 4).sum()) == 0                                                       # the two-vertex hull is never hit
    assert all(int((k == b).sum()) > 0 for b in range(4)) and int((k == -1).sum()) > 0
    assert body.shape[1] == 70


@pytest.mark.parametrize("name", SH.CASE_NAMES + ("tiny",))
def test_at_most_two_percent_of_a_case_are_rays_the_mirror_cannot_decide(name):
    ref = SH.reference(name)
    ex = ref["excluded"]
    assert int(ex.sum()) <= 0.02 * ex.numel(), (int(ex.sum()), ex.numel())
    assert bool(torch.isfinite(ref["dist"]).all())
    for k, g in ref["grads"].items():
        assert bool(torch.isfinite(g).all()), k
    if name == "tiny":                                                                    # gradcheck's inputs: every ray a clean hit
        assert int(ex.sum()) == 0 and int((ref["hit"] < 0).sum()) == 0 and float(ref["dist"].min()) > 0 and float(ref["gap"].min()) > 1.0
    if name == "wide":
        c = SH.case(name)
        assert int(c["nverts"].sum(1).max()) == 1024 and c["ray_body"].shape == (2, 1024)
        assert int((ref["hit"] >= 0).sum()) > 1000 and int((ref["hit"] < 0).sum()) > 20


# ------------------------------------------------------------------------------------------------------------- gradient
@pytest.mark.parametrize("name", ["small", "tiny"])
@pytest.mark.parametrize("leaf", SH.LEAVES)
def test_autograd_of_the_mirror_equals_its_central_differences(name, leaf):
    """Directional: sum_r g_r (dist_r(x + h d) - dist_r(x - h d)) / 2h against <autograd's gradient, d> for random directions d of
    one input array at a time and the reference's cotangent g, zeroed on the rays within 1e-3 of a change of branch (finite
    differences do not cross one).  h = 1e-6, 1e-6 relative to sum_r |g_r| |d dist_r|: a second-order scheme on a smooth function of
    order-100 coordinates."""
    ref, c = SH.reference(name), SH.case(name)
    g = torch.where(ref["gap"] < 1e-3, torch.zeros_like(ref["g_dist"]), ref["g_dist"])
    cl = SH.leaves(c)
    grad = torch.autograd.grad(SH.cast_host(cl)["dist"], cl[leaf], g, allow_unused=True)[0]
    assert grad is not None and float(grad.abs().max()) > 0
    h = 1e-6
    for seed in range(3):
        d = torch.randn(c[leaf].shape, generator=torch.Generator().manual_seed(seed), dtype=F64)
        with torch.no_grad():
            hi = SH.cast_host(dict(c, **{leaf: c[leaf] + h * d}))
            lo = SH.cast_host(dict(c, **{leaf: c[leaf] - h * d}))
        assert torch.equal(hi["hit"], lo["hit"]) or bool((g[hi["hit"] != lo["hit"]] == 0).all())
        fd = (hi["dist"] - lo["dist"]) / (2 * h)
        scale = float((g.abs() * fd.abs()).sum())
        assert abs(float((g * fd).sum()) - float((grad * d).sum())) <= 1e-6 * scale, (leaf, seed)
