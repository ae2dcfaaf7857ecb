"""CPU: the two link entries are exported and bound as the header declares them and refuse bad arguments before any launch; the
closed forms of the header's table (tests/links_host.py `closed_form`) are the autograd Jacobian of the position-level functions on
random poses; `LinkSet.from_list` keeps its books and refuses what it must; two world slots are the reference's revolute joint to the
world."""
import ctypes
import math
import os
import re

import pytest
import torch

from tests import links_host as LH

F64, F32, I32 = torch.float64, torch.float32, torch.int32
FWD, BWD = "lcp_link_jacobian_f64", "lcp_link_jacobian_backward_f64"


# ------------------------------------------------------------------------------------------------------------- the C ABI
def _ctype(decl):
    decl = decl.strip()
    return ctypes.c_void_p if "*" in decl else {"int": ctypes.c_int, "double": ctypes.c_double}[decl.split()[0]]


def test_the_library_exports_both_entries_and_their_ctypes_signatures_match_the_header():
    from lcp_physics_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "lcp_hip.h")).read()
    for name, nargs in ((FWD, 15), (BWD, 18)):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        declared = [_ctype(a) for a in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == declared and len(args) == nargs
        assert getattr(lib, name).argtypes == args


def _fake(n):
    return [ctypes.c_void_p(4096 * (k + 1)) for k in range(n)]


def test_bad_arguments_are_refused_before_any_launch_and_an_empty_batch_is_accepted():
    """Fake pointers: a call that launched would fault, one that is refused (or has nothing to do) never touches them."""
    from lcp_physics_amd import _lib
    lib = _lib.load()
    fwd = lambda sizes=(2, 3, 4, 1, 5), ins=None, base=ctypes.c_void_p(64), out=ctypes.c_void_p(128): getattr(lib, FWD)(
        *sizes, *(_fake(7) if ins is None else ins), base, out, None)
    bwd = lambda sizes=(2, 3, 4, 1, 5), ins=None, g=ctypes.c_void_p(64), outs=None: getattr(lib, BWD)(
        *sizes, *(_fake(7) if ins is None else ins), g, *(_fake(4) if outs is None else outs), None)
    for sizes in ((-1, 3, 4, 1, 5), (2, 0, 4, 1, 5), (2, 3, 0, 1, 0), (2, 3, 4, -1, 5), (2, 3, 4, 1, -1), (2, 3, 4, 1, 9)):
        assert fwd(sizes) == -1 and bwd(sizes) == -1, sizes                 # LCP_E_BADARG
    for sizes in ((2, 65, 4, 1, 5), (2, 3, 257, 1, 5), (2, 3, 4, 65537, 5)):
        assert fwd(sizes) == -2 and bwd(sizes) == -2, sizes                 # LCP_E_TOOLARGE
    for k in range(7):                                                      # the six link arrays, p
        ins = _fake(7)
        ins[k] = None
        assert fwd(ins=ins) == -1 and bwd(ins=ins) == -1, k
    assert fwd(out=None) == -1 and fwd(base=None) == -1 and bwd(g=None) == -1 and bwd(outs=[None] * 4) == -1
    assert fwd((0, 3, 4, 1, 5)) == 0 and bwd((0, 3, 4, 1, 5)) == 0           # B == 0: success without a launch
    assert fwd((2, 3, 4, 0, 0), base=None) == 0                              # no rows at all: nothing to write


# ------------------------------------------------------------------------------------------------------------- the mirror
@pytest.mark.parametrize("name", LH.CASE_NAMES)
def test_the_table_is_the_jacobian_of_the_position_level_functions(name):
    """Random poses: every entry of the closed forms within 1e-12 of the row's largest entry of the autograd Jacobian (two float64
    evaluations of a few products each), zeros where no link can write."""
    c, ref = LH.case(name), LH.reference(name)
    table = LH.closed_form(c)
    assert table.shape == ref["Je"].shape == (c["p"].shape[0], LH.el_of(c["kind"]), 3 * c["p"].shape[1])
    scale = ref["Je"].abs().amax(dim=2, keepdim=True).clamp(min=1.0)
    assert float(((table - ref["Je"]).abs() / scale).max()) < 1e-12
    assert float(ref["Je"][~ref["struct"]].abs().max() if (~ref["struct"]).any() else 0.0) == 0.0
    assert float(table[~ref["struct"]].abs().max() if (~ref["struct"]).any() else 0.0) == 0.0
    dead = ~ref["live"]
    assert float(ref["Je"][dead].abs().max() if dead.any() else 0.0) == 0.0
    for n in LH.LEAVES:
        assert bool(torch.isfinite(ref["grads"][n]).all()), n


def test_the_cases_are_the_ones_the_gpu_comparison_needs():
    shape = lambda n: (LH.case(n)["p"].shape[0], LH.case(n)["p"].shape[1], LH.case(n)["kind"].shape[1])
    assert [shape(n) for n in LH.CASE_NAMES[:6]] == [(1, 2, 1)] * 3 + [(3, 5, 7), (70, 3, 1), (2, 8, 70)]
    assert [int(LH.case(n)["kind"][0, 0]) for n in LH.CASE_NAMES[:3]] == [LH.DISTANCE, LH.SLOT, LH.PRISMATIC]
    m = LH.case("mixed")
    for b in range(3):
        named = torch.cat([m["first"][b], m["second"][b]]).tolist()
        assert max(named.count(k) for k in range(5)) >= 3 and named.count(4) == 0 and named.count(-1) == 2
    assert set(m["kind"][0].tolist()) == {1, 2, 3} and not torch.equal(m["first"][0], m["first"][1])
    inv, ref = LH.case("invalid"), LH.reference("invalid")
    assert LH.el_of(inv["kind"]) == 10 and int((~ref["live"]).sum()) == 2 * 7 and int(ref["live"].sum()) == 2 * 3
    assert float(ref["grads"]["p"][:, 2].abs().max()) == 0.0 and float(ref["grads"]["p"].abs().max()) > 0.0


def test_a_rod_and_a_slot_by_hand():
    """A body at (3, 0) turned by pi / 2 with its anchor (1, 0) - so at (3, 1) in the world - on a rod to the world point (3, 5): n is
    +y and the arm (0, 1) is parallel to it, so the row is (0, 0, -1).  The same anchor in a world slot along x (phi 0: t = +y)
    through (0, 1): the row is (cross((0, 1), (0, 1)), 0, 1) = (0, 0, 1)."""
    c = {"kind": torch.tensor([[LH.DISTANCE, LH.SLOT]], dtype=I32), "first": torch.zeros(1, 2, dtype=I32),
         "second": torch.full((1, 2), -1, dtype=I32), "a1": torch.tensor([[[1.0, 0.0], [1.0, 0.0]]], dtype=F64),
         "a2": torch.tensor([[[3.0, 5.0], [0.0, 1.0]]], dtype=F64), "phi": torch.zeros(1, 2, dtype=F64),
         "p": torch.tensor([[[math.pi / 2, 3.0, 0.0]]], dtype=F64)}
    want = torch.tensor([[[0.0, 0.0, -1.0], [0.0, 0.0, 1.0]]], dtype=F64)
    assert float((LH.jacobian(c) - want).abs().max()) < 1e-15 and float((LH.closed_form(c) - want).abs().max()) < 1e-15
    C, live = LH.constraints(c)
    assert bool(live.all()) and float((C - torch.tensor([[4.0, 0.0]], dtype=F64)).abs().max()) < 1e-15


# ------------------------------------------------------------------------------------------------------------- LinkSet
def _p0(nb=3):
    return torch.tensor([[0.3, 1.0, 2.0], [-0.5, 6.0, 1.0], [1.1, 4.0, 7.0]], dtype=F64)[:nb]


def test_from_list_keeps_its_books():
    from lcp_physics_amd.physics.links import DISTANCE, PRISMATIC, SLOT, LinkSet
    a = torch.tensor([0.5, -0.25], dtype=F64, requires_grad=True)
    ls = LinkSet.from_list([("distance", 0, 1, a, (0.0, 1.0)), ("slot", 1, None, (0.0, 0.0), (2.0, 3.0), 0.4),
                            ("prismatic", 2, 0, (1.0, 0.0), (0.0, 0.0), -0.7)], _p0(), B=4)
    assert (ls.B, ls.L, ls.e) == (4, 3, 4) and ls.kind[0].tolist() == [DISTANCE, SLOT, PRISMATIC]
    assert ls.first[3].tolist() == [0, 1, 2] and ls.second[3].tolist() == [1, -1, 0]                 # None: the world
    assert ls.kind.dtype == I32 and ls.a1.dtype == F64 and ls.a1.shape == (4, 3, 2) and ls.rest.shape == (4, 4)
    assert ls.phi[0].tolist() == [0.0, 0.4, -0.7] and ls.a2[1, 1].tolist() == [2.0, 3.0]
    assert ls.a1.requires_grad and not ls.rest.requires_grad                                          # values may be leaves
    ls.a1.sum().backward()
    assert a.grad.tolist() == [4.0, 4.0]
    # `rest`: the rod's length and the slider's relative angle at the creation pose; a slot's row has none
    p0 = _p0().unsqueeze(0).expand(4, -1, -1)
    c = {n: getattr(ls, n).detach() for n in LH.LINK_ARRAYS}
    C, _ = LH.constraints(dict(c, p=p0))
    assert float((ls.rest[:, 0] - C[:, 0]).abs().max()) < 1e-15 and float(ls.rest[0, 0]) > 1.0
    assert float(ls.rest[:, 1].abs().max()) == 0.0 and float(ls.rest[:, 2].abs().max()) == 0.0
    assert float((ls.rest[:, 3] - (1.1 - 0.3)).abs().max()) < 1e-15
    res = ls.residual(p0).detach()
    assert float(res[:, [0, 3]].abs().max()) == 0.0 and float((res - (C - ls.rest)).abs().max()) < 1e-15
    moved = p0.clone()
    moved[:, 0, 1] += 0.5
    assert float(ls.residual(moved).detach()[:, 0].abs().min()) > 1e-3
    both = LinkSet.concat([ls, ls])
    assert (both.L, both.e) == (6, 8) and both.rest.shape == (4, 8) and both.kind[0].tolist() == ls.kind[0].tolist() * 2
    per_scene = LinkSet.from_list([("slot", 0, None, torch.zeros(4, 2, dtype=F64), (0.0, 0.0), torch.arange(4, dtype=F64))], p0)
    assert per_scene.phi[:, 0].tolist() == [0.0, 1.0, 2.0, 3.0] and per_scene.B == 4


def test_from_list_refuses_what_it_must():
    from lcp_physics_amd.physics.links import LinkSet
    p0 = _p0()
    on_anchor = (p0[1, 1:] - p0[0, 1:]).tolist()                          # body 1's centre in world axes from body 0's ...
    c, s = math.cos(0.3), math.sin(0.3)
    local = (c * on_anchor[0] + s * on_anchor[1], -s * on_anchor[0] + c * on_anchor[1])               # ... and in body 0's frame
    with pytest.raises(ValueError, match="coincide"):
        LinkSet.from_list([("distance", 0, 1, local, (0.0, 0.0))], p0)
    assert LinkSet.from_list([("distance", 0, 1, local, (0.0, 0.0))], p0, check=False).e == 1
    with pytest.raises(ValueError, match="coincide"):
        LinkSet.from_list([("distance", 1, None, (0.0, 0.0), (6.0, 1.0))], p0)
    for bad in ([("hinge", 0, 1, (0.0, 0.0), (0.0, 0.0))], [("distance", 0, 1, (0.0, 0.0))], [("slot", 0, 1, (0.0, 0.0), (0.0, 0.0))],
                [("distance", 0, 0, (0.0, 0.0), (1.0, 0.0))], [("distance", 3, 0, (0.0, 0.0), (1.0, 0.0))],
                [("slot", 0, 5, (0.0, 0.0), (1.0, 0.0), 0.0)], []):
        with pytest.raises(ValueError):
            LinkSet.from_list(bad, p0)
    with pytest.raises(ValueError):
        LinkSet.from_list([("distance", 0, 1, (0.0, 0.0, 0.0), (1.0, 0.0))], p0)
    ls = LinkSet.from_list([("distance", 0, 1, (0.0, 0.0), (0.0, 0.0))], p0, B=2)
    with pytest.raises(ValueError):
        LinkSet(ls.kind, ls.first, ls.second, ls.a1, ls.a2, ls.phi.float(), ls.rest, ls.e)
    with pytest.raises(ValueError):
        LinkSet(ls.kind, ls.first, ls.second, ls.a1[:, :, :1], ls.a2, ls.phi, ls.rest, ls.e)
    with pytest.raises(ValueError):
        LinkSet.concat([ls, LinkSet.from_list([("distance", 0, 1, (0.0, 0.0), (0.0, 0.0))], p0, B=3)])
    with pytest.raises(RuntimeError, match="GPU"):                          # no CPU route
        ls.jacobian(p0.unsqueeze(0).expand(2, -1, -1).contiguous())


def test_two_world_slots_are_the_revolute_joint_to_the_world():
    """`first`'s anchor on the world point itself (d = 0), one slot with t = (1, 0) and one with t = (0, 1): the two rows of the
    reference's revolute joint to the world, [-pos1_y, 1, 0] and [pos1_x, 0, 1] (`JointSet.jacobian_torch`), at the creation pose and at
    poses turned about the pin.  t = R(rot_2) (-sin phi, cos phi) is (1, 0) at phi = -pi / 2 (the rule's own sign: +pi / 2 gives
    (-1, 0), the negated row) and (0, 1) at phi = 0; cos(pi / 2) = 6.1e-17 in float64 is the bound on the entries that are 0 there."""
    from lcp_physics_amd.physics.joints import JointSet
    from lcp_physics_amd.physics.links import LinkSet
    B = 5
    pin = torch.tensor([4.0, 9.0], dtype=F64)
    th0 = torch.linspace(-2.0, 2.5, B, dtype=F64)
    arm = torch.tensor([1.5, -2.0], dtype=F64)                            # the pin in the body's frame
    centre = lambda th: pin - torch.stack([torch.cos(th) * arm[0] - torch.sin(th) * arm[1], torch.sin(th) * arm[0] + torch.cos(th) * arm[1]], -1)
    p0 = torch.cat([th0.unsqueeze(-1), centre(th0)], -1).unsqueeze(1)                                # [B,1,3]
    js = JointSet.from_list([("joint", 0, None, tuple(pin.tolist()))], p0, B)
    ls = LinkSet.from_list([("slot", 0, None, arm, pin, -math.pi / 2), ("slot", 0, None, arm, pin, 0.0)], p0, B)
    assert float(ls.residual(p0).abs().max()) < 1e-14                     # the anchor sits on both lines
    for turn in (0.0, 0.7, -1.9):                                         # the joint's angle follows the body's (constraints.py:39-43)
        th = th0 + turn
        p = torch.cat([th.unsqueeze(-1), centre(th)], -1).unsqueeze(1)
        want = js.jacobian_torch(p, jrot1=js.jrot1 + turn)
        c = {n: getattr(ls, n) for n in LH.LINK_ARRAYS}
        got, table = LH.jacobian(dict(c, p=p)), LH.closed_form(dict(c, p=p))
        assert got.shape == want.shape == (B, 2, 3)
        assert float((got - want).abs().max()) < 1e-14 and float((table - want).abs().max()) < 1e-14
