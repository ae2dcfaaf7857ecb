"""CPU: the two force-element entries are exported and bound as the header declares them and refuse bad arguments before any launch;
the host mirror (tests/force_elements_host.py) obeys action = reaction and derives its springs from a potential; the condition the
GPU comparison puts on the cases (no clamp or zero-length decision within rounding) holds on the mirror alone; `ForceSet` validates
and its builders build."""
import ctypes
import os
import re

import pytest
import torch

from tests import force_elements_host as FH

F64, F32, I32 = torch.float64, torch.float32, torch.int32
FWD, BWD = "lcp_force_elements_f64", "lcp_force_elements_backward_f64"


# ------------------------------------------------------------------------------------------------------------- the C ABI
def _ctype(decl):
    decl = decl.strip()
    return ctypes.c_void_p if "*" in decl else {"int": ctypes.c_int, "double": ctypes.c_double}[decl.split()[0]]


def test_the_library_exports_both_entries_and_their_ctypes_signatures_match_the_header():
    from lcp_physics_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "lcp_hip.h")).read()
    for name, nargs in ((FWD, 18), (BWD, 25)):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        declared = [_ctype(a) for a in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == declared and len(args) == nargs
        assert getattr(lib, name).argtypes == args


def _fake(n):
    return [ctypes.c_void_p(4096 * (k + 1)) for k in range(n)]


def test_bad_arguments_are_refused_before_any_launch_and_an_empty_batch_is_accepted():
    """Fake pointers: a call that launched would fault, one that is refused (or has B == 0) never touches them."""
    from lcp_physics_amd import _lib
    lib = _lib.load()
    fwd = lambda sizes=(2, 3, 4), ins=None, base=ctypes.c_void_p(64), out=ctypes.c_void_p(128): getattr(lib, FWD)(
        *sizes, *(_fake(12) if ins is None else ins), base, out, None)
    bwd = lambda sizes=(2, 3, 4), ins=None, g=ctypes.c_void_p(64), outs=None: getattr(lib, BWD)(
        *sizes, *(_fake(12) if ins is None else ins), g, *(_fake(8) if outs is None else outs), None)
    for sizes in ((-1, 3, 4), (2, 0, 4), (2, 65, 4), (2, 3, 0), (2, 3, 1025)):
        assert fwd(sizes) == -1 and bwd(sizes) == -1, sizes                 # LCP_E_BADARG
    for k in range(12):                                                     # the ten element arrays, p, v
        ins = _fake(12)
        ins[k] = None
        assert fwd(ins=ins) == -1 and bwd(ins=ins) == -1, k
    assert fwd(out=None) == -1 and bwd(g=None) == -1 and bwd(outs=[None] * 8) == -1
    assert fwd((0, 3, 4)) == 0 and bwd((0, 3, 4)) == 0                      # B == 0: success without a launch
    assert fwd((0, 3, 4), base=None) == 0


# ------------------------------------------------------------------------------------------------------------- the mirror
def test_a_world_spring_and_a_drag_by_hand():
    """A body at (3, 0) turned by pi / 2 with its anchor (1, 0) - so at (3, 1) in the world - tied to the world point (3, 5) by a
    spring of rest length 1 and stiffness 2: length 4, tension 6 towards +y; the lever (0, 1) is parallel, no torque."""
    z = lambda *s: torch.zeros(*s, dtype=F64)
    c = {"kind": torch.tensor([[1, 3]], dtype=I32), "b1": torch.tensor([[0, 0]], dtype=I32), "b2": torch.tensor([[-1, 5]], dtype=I32),
         "a1": torch.tensor([[[1.0, 0.0], [0.0, 0.0]]], dtype=F64), "a2": torch.tensor([[[3.0, 5.0], [0.0, 0.0]]], dtype=F64),
         "k": torch.tensor([[2.0, 0.5]], dtype=F64), "c": torch.tensor([[0.0, 0.25]], dtype=F64), "x0": torch.tensor([[1.0, 0.0]], dtype=F64),
         "w0": z(1, 2), "limit": torch.full((1, 2), FH.INF, dtype=F64),
         "p": torch.tensor([[[torch.pi / 2, 3.0, 0.0]]], dtype=F64), "v": torch.tensor([[[4.0, 2.0, -2.0]]], dtype=F32), "f_base": None}
    out = FH.forces_host(c)
    want = torch.tensor([[[0.0 - 1.0, 0.0 - 1.0, 6.0 + 1.0]]], dtype=F64)   # spring (0, 0, 6) + drag (-0.25 * 4, -0.5 * 2, 0.5 * 2)
    assert float((out["f64"] - want).abs().max()) < 1e-14
    assert float((out["S"] - torch.tensor([[[1.0, 1.0, 7.0]]], dtype=F64)).abs().max()) < 1e-14
    c["limit"][0, 0] = 4.5                                                  # clamped: 4.5 towards +y, gap (6 - 4.5) / 4.5
    out = FH.forces_host(c)
    assert abs(float(out["f64"][0, 0, 2]) - 5.5) < 1e-14 and bool(out["sat"][0, 0])
    assert abs(float(out["gap"]["sat"][0, 0]) - 1.5 / 4.5) < 1e-14 and abs(float(out["gap"]["L"][0, 0]) - 4.0) < 1e-14


def _body_to_body(seed, kinds):
    c = FH._random(seed, 4, 6, 30, kinds=kinds, world=0.0)
    c["f_base"] = None
    c["b2"] = torch.where(c["b2"] < 0, (c["b1"] + 1) % 6, c["b2"])          # (world = 0 keeps only the first end off the world)
    assert bool(((c["b1"] >= 0) & (c["b2"] >= 0) & (c["b1"] != c["b2"])).all())
    return c


def test_action_equals_reaction_between_bodies():
    """Body-to-body springs and motors: the net force and the net torque about the origin vanish to 1e-12 of the terms' size."""
    c = _body_to_body(21, (1, 2))
    out = FH.forces_host(c)
    f, S, x, y = out["f64"], out["S"], c["p"][..., 1], c["p"][..., 2]
    assert bool(out["valid"].all())
    net_f = f[..., 1:].sum(1).abs()
    net_t = (f[..., 0] + x * f[..., 2] - y * f[..., 1]).sum(1).abs()
    size_t = (S[..., 0] + x.abs() * S[..., 2] + y.abs() * S[..., 1]).sum(1)
    assert bool((net_f <= 1e-12 * S[..., 1:].sum(1)).all()), (net_f, S[..., 1:].sum(1))
    assert bool((net_t <= 1e-12 * size_t).all()), (net_t, size_t)
    assert float(f.abs().max()) > 1.0


def test_an_undamped_spring_is_minus_the_gradient_of_its_energy():
    """c = 0, no clamp: the wrench on every body is -d/dp of sum 1/2 k (L - x0)^2, by autograd of the energy alone."""
    c = FH._random(22, 3, 5, 12, kinds=(1,))
    c["c"] = torch.zeros_like(c["c"])
    c["f_base"] = None
    p = c["p"].clone().requires_grad_(True)
    out = FH.forces_host(c)
    assert bool(out["valid"].all()) and not bool(out["sat"].any())

    def point(b, a):
        st = FH._gather(p, b)
        cs, sn = torch.cos(st[..., 0]), torch.sin(st[..., 0])
        w = st[..., 1:] + torch.stack([cs * a[..., 0] - sn * a[..., 1], sn * a[..., 0] + cs * a[..., 1]], -1)
        return torch.where((b >= 0).unsqueeze(-1), w, a)

    L = (point(c["b2"], c["a2"]) - point(c["b1"], c["a1"])).norm(dim=-1)
    energy = (0.5 * c["k"] * (L - c["x0"]) ** 2).sum()
    want = -torch.autograd.grad(energy, p)[0]
    assert float((out["f64"] - want).abs().max()) <= 1e-12 * float(out["S"].max())


@pytest.mark.parametrize("name", FH.CASE_NAMES)
def test_no_case_decides_a_clamp_or_a_zero_length_within_rounding(name):
    c, ref = FH.case(name), FH.reference(name)
    B, nb = c["p"].shape[:2]
    assert c["kind"].shape == c["b1"].shape == c["limit"].shape and c["a1"].shape == c["kind"].shape + (2,)
    valid = ref["valid"]
    assert float(ref["gap"]["sat"][valid].min()) >= FH.MIN_GAP if bool(valid.any()) else True
    if name != "invalid":
        assert float(ref["gap"]["L"][valid].min()) >= FH.MIN_GAP
    for n in FH.LEAVES:
        assert bool(torch.isfinite(ref["grads"][n]).all()), n
    assert bool(torch.isfinite(ref["f64"]).all())


def test_the_cases_are_what_their_names_say():
    R = FH.reference
    assert FH.case("one")["kind"].shape == (1, 1) and FH.case("one")["b1"].item() == -1 and bool(R("one")["valid"].all())
    small = FH.case("small")
    assert small["kind"][0].tolist() == [1, 2, 3, 0] and R("small")["valid"][:, :3].all() and not R("small")["valid"][:, 3].any()
    assert [FH.case(n)["kind"].shape[1] for n in ("edge63", "edge64", "edge65", "e257", "full")] == [63, 64, 65, 257, 1024]
    assert FH.case("full")["p"].shape == (2, 64, 3)
    ob = R("one_body")
    assert bool(ob["valid"].all()) and bool(ob["touched"][:, 0].all()) and not bool(ob["touched"][:, 1].any())
    assert not bool(R("untouched")["touched"][:, 3:].any()) and bool(R("untouched")["touched"][:, :3].any())
    inv = R("invalid")
    assert inv["valid"][0].tolist() == [False] * 14 + [True, True] and not bool(inv["valid"][2].any())
    assert float(inv["gap"]["L"][0, 13]) == 0.0                              # L == 0 exactly
    sat = R("saturated")
    two = FH.case("saturated")["kind"] != 3
    assert bool(sat["sat"][:, 0::2][two[:, 0::2]].all()) and not bool(sat["sat"][:, 1::2].any())
    assert bool(torch.isinf(FH.case("saturated")["limit"]).any())
    ps = FH.case("per_scene")
    assert len({tuple(r) for r in ps["kind"].tolist()}) == 6 and len({tuple(r) for r in ps["b1"].tolist()}) == 6
    # a saturated element has no gradient at all, an invalid one neither
    for name in ("saturated", "invalid"):
        ref = R(name)
        dead = ~ref["valid"] | ref["sat"]
        for n in ("k", "c", "x0", "w0", "a1", "a2"):
            assert float(ref["grads"][n][dead].abs().max()) == 0.0, (name, n)


# ------------------------------------------------------------------------------------------------------------- ForceSet
def _set(**over):
    from lcp_physics_amd.physics.force_elements import ForceSet
    c = {n: FH.case("small")[n] for n in FH.ELEMENT_ARRAYS}
    c.update(over)
    return ForceSet(**c)


def test_force_set_validates_shapes_dtypes_and_the_limit():
    fs = _set()
    assert (fs.B, fs.E) == (5, 4)
    small = FH.case("small")
    with pytest.raises(ValueError):
        _set(k=small["k"][:, :3])
    with pytest.raises(ValueError):
        _set(a1=small["a1"][..., 0])
    with pytest.raises(ValueError):
        _set(b1=small["b1"].long())
    with pytest.raises(ValueError):
        _set(k=small["k"].float())
    for bad in (0.0, -1.0, float("nan")):
        lim = small["limit"].clone()
        lim[2, 1] = bad
        with pytest.raises(ValueError):
            _set(limit=lim)
    with pytest.raises(ValueError):
        _set(**{n: FH.case("small")[n][:, :0] for n in FH.ELEMENT_ARRAYS})


def test_from_list_and_concat_build_the_arrays_and_keep_the_graph():
    from lcp_physics_amd.physics.force_elements import DRAG, MOTOR, SPRING, ForceSet
    k = torch.tensor(40.0, dtype=F64, requires_grad=True)
    anchor = torch.tensor([0.5, 0.25], dtype=F64, requires_grad=True)
    per_scene = torch.tensor([1.0, 2.0, 3.0], dtype=F64)
    fs = ForceSet.from_list([("spring", 0, 1, anchor, (-0.5, 0.0), {"k": k, "c": 0.5, "rest": per_scene, "limit": 9.0}),
                             ("motor", -1, 2, {"kp": 30.0, "kd": 2.0, "target": 1.0, "rate": -1.0}),
                             ("drag", 1, {"lin": 0.1, "ang": 0.01})], 3)
    assert (fs.B, fs.E) == (3, 3)
    assert fs.kind.tolist() == [[SPRING, MOTOR, DRAG]] * 3 and fs.b1.tolist() == [[0, -1, 1]] * 3 and fs.b2.tolist() == [[1, 2, -1]] * 3
    assert fs.k[1].tolist() == [40.0, 30.0, 0.1] and fs.c[1].tolist() == [0.5, 2.0, 0.01]
    assert fs.x0[:, 0].tolist() == [1.0, 2.0, 3.0] and fs.x0[0, 1:].tolist() == [1.0, 0.0] and fs.w0[0].tolist() == [0.0, -1.0, 0.0]
    assert fs.limit[0].tolist() == [9.0, FH.INF, FH.INF]
    assert fs.a1[2].tolist() == [[0.5, 0.25], [0.0, 0.0], [0.0, 0.0]] and fs.a2[0, 0].tolist() == [-0.5, 0.0]
    moved = fs.to("cpu")
    (moved.k.sum() + moved.a1.sum()).backward()
    assert float(k.grad) == 3.0 and anchor.grad.tolist() == [3.0, 3.0]      # one spring in each of three scenes
    both = ForceSet.concat([fs, fs])
    assert both.E == 6 and both.kind[0].tolist() == [SPRING, MOTOR, DRAG] * 2 and both.k.requires_grad
    for bad in ([], [("spring", 0, 1, {"k": 1.0})], [("drag", 0, {"k": 1.0})], [("rope", 0, 1, {})]):
        with pytest.raises(ValueError):
            ForceSet.from_list(bad, 2)
    with pytest.raises(ValueError):
        ForceSet.concat([fs, ForceSet.from_list([("drag", 0, {"lin": 1.0})], 2)])
