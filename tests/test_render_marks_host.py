"""CPU: the float64 restatement of the drawing with marks and joint markers (tests/render_marks_host.py) checked on its own - against
render_host where there is nothing to add, against answers worked out by hand, its decision margins on every case the GPU tests use,
its gradients against central differences - and the host side of `lcp_render_marks_f64` / `lcp_render_marks_backward_f64`: symbols,
ctypes bindings, the refusals before any launch, `marks_of`."""
import ctypes
import math
import os

import pytest
import torch

from tests import render_host as RH
from tests import render_marks_host as MH

FWD, BWD = "lcp_render_marks_f64", "lcp_render_marks_backward_f64"
F64 = torch.float64


@pytest.mark.parametrize("name", RH.CASE_NAMES)
def test_without_marks_and_joints_it_is_render_host_exactly(name):
    c = RH.case(name)
    image, ids, margin = RH.render_host(c)
    for extra in ({}, dict(mark=torch.zeros(c["kind"].shape, dtype=torch.int32), mark_colors=torch.rand(*c["kind"].shape, c["colors"].shape[2]))):
        got = MH.render_marks_host(dict(c, **extra))
        assert torch.equal(got[0], image) and torch.equal(got[1], ids) and got[2] == margin


def _tiny(joints, sizes, nb=1, centre=(3.5, 2.75)):
    """5 x 7 pixels of one world unit, w = 1, black background, white markers on bodies that are not drawn (hulls of two vertices)."""
    cam = (5, 7, 0.0, 0.0, 1.0, 1.0)
    stick = [[0.0, 0.0], [1.0, 0.0]]
    c = RH._assemble([[("hull", (0.0,) + tuple(centre), stick, 0.0)] * nb], cam, 1, 0, False, 8, background=[0.0])
    c = MH._with_marks(c, [0] * nb, 0, joints=joints, sizes=sizes)
    c["joint_colors"] = torch.ones_like(c["joint_colors"])
    c["jr1"], c["jrot1"] = torch.zeros_like(c["jr1"]), torch.zeros_like(c["jrot1"])
    return c


def test_known_answers_of_a_segment_and_a_disc():
    """Pixel (i, j) is the world point (j + 1/2, i + 1/2); the markers' centre is (3.5, 2.75).
    The horizontal tick (3.5 -+ 2, 2.75) of width 1: alpha = clamp(1/2 - (dist - 1/2)) = clamp(1 - dist).
    The disc of radius 1.5: alpha = clamp(1/2 - (|x - c| - 3/2)) = clamp(2 - |x - c|)."""
    tick = MH.render_marks_host(_tiny([(MH.YCON, 0, -1, 0.0, 0.0)], (1.0, 1.5, 1.0, 2.0)))[0][0, 0]
    want = {(2, 3): 0.75, (3, 3): 0.25, (1, 3): 0.0, (2, 5): 0.75, (2, 1): 0.75, (3, 5): 0.25,
            (2, 6): max(0.0, 1.0 - math.hypot(1.0, 0.25)), (2, 0): max(0.0, 1.0 - math.hypot(1.0, 0.25)), (4, 3): 0.0}
    for (i, j), a in want.items():
        assert abs(float(tick[i, j]) - a) <= 1e-15, (i, j, float(tick[i, j]), a)
    post = MH.render_marks_host(_tiny([(MH.XCON, 0, -1, 0.0, 0.0)], (1.0, 1.5, 1.0, 2.0)))[0][0, 0]      # vertical: (3.5, 2.75 -+ 2)
    for (i, j), a in {(2, 3): 1.0, (2, 2): 0.0, (0, 3): 0.75, (4, 3): 1.0, (2, 4): 0.0}.items():      # (row 0 lies 1/4 beyond its end)
        assert abs(float(post[i, j]) - a) <= 1e-15, (i, j)
    disc = MH.render_marks_host(_tiny([(MH.JOINT, 0, -1, 0.0, 0.0)], (1.0, 1.5, 1.0, 2.0)))[0][0, 0]
    want = {(2, 3): 1.0, (2, 4): 2.0 - math.hypot(1.0, 0.25), (3, 4): 0.75, (4, 3): 0.25, (2, 5): 0.0, (0, 3): 0.0, (1, 3): 0.75}
    for (i, j), a in want.items():
        assert abs(float(disc[i, j]) - a) <= 1e-15, (i, j, float(disc[i, j]), a)
    # the ring of radius 2 and thickness 1/2 around the same point: cov(d) - cov(d + 1/2), d = |x - c| - 2
    ring = MH.render_marks_host(_tiny([(MH.ROTCON, 0, -1, 0.0, 0.0)], (0.5, 1.5, 1.0, 2.0)))[0][0, 0]
    cov = lambda d: min(max(0.5 - d, 0.0), 1.0)
    for (i, j) in ((2, 3), (2, 5), (4, 3), (3, 4), (0, 3)):
        d = math.hypot(j + 0.5 - 3.5, i + 0.5 - 2.75) - 2.0
        assert abs(float(ring[i, j]) - (cov(d) - cov(d + 0.5))) <= 1e-15, (i, j)


def test_a_segment_of_no_length_is_the_disc_of_half_its_width():
    """A FIXED joint between two bodies on the same point (width 1.6) against a JOINT's dot of radius 0.8 there: the same image and the
    same gradient of the point, finite (nothing is divided by |AB|^2 = 0)."""
    seg = RH.leaves(_tiny([(MH.FIXED, 0, 1, 0.0, 0.0)], (1.0, 0.8, 1.6, 2.0), nb=2, centre=(3.3, 2.6)))
    dot = RH.leaves(_tiny([(MH.JOINT, 0, -1, 0.0, 0.0)], (1.0, 0.8, 1.6, 2.0), nb=2, centre=(3.3, 2.6)))
    a, b = MH.render_marks_host(seg)[0], MH.render_marks_host(dot)[0]
    assert torch.equal(a, b) and float(a.detach().max()) > 0.5
    G = torch.randn(a.shape, generator=torch.Generator().manual_seed(1), dtype=F64)
    ga, gb = torch.autograd.grad((a * G).sum(), seg["p"])[0], torch.autograd.grad((b * G).sum(), dot["p"])[0]
    assert bool(torch.isfinite(ga).all()) and float(ga[0, 0].abs().max()) > 0.0
    assert torch.equal(ga[0, 0], gb[0, 0]) and float(ga[0, 1].abs().max()) == 0.0          # A carries the point, B nothing


@pytest.mark.parametrize("name", MH.CASE_NAMES)
def test_every_case_of_the_gpu_tests_has_its_decision_margin(name):
    ref = MH.reference(name)
    print(name, "margin %.3g" % ref["margin"])
    assert ref["margin"] > 1e-6
    assert bool(torch.isfinite(ref["image"]).all())
    for n, g in ref["grads"].items():
        assert bool(torch.isfinite(g).all()), n


def test_a_circles_image_depends_on_its_angle_with_a_spoke_and_not_without():
    G = torch.randn(1, 1, 19, 23, generator=torch.Generator().manual_seed(2), dtype=F64)
    grads = {}
    for mark in (MH.SPOKE, 0):
        c = MH.leaves(MH.spin_case(0.7, mark))
        image, _, margin = MH.render_marks_host(c)
        assert margin > 1e-6
        grads[mark] = torch.autograd.grad((image * G).sum(), c["p"])[0][0, 0]
    print("d<image, G>/d(rot, x, y) with a spoke", grads[MH.SPOKE].tolist(), "without", grads[0].tolist())
    assert abs(float(grads[MH.SPOKE][0])) > 1e-3 and float(grads[0][0]) == 0.0
    assert float(grads[0][1:].abs().min()) > 0.0


@pytest.mark.parametrize("name", ["marks3", "joints"])
def test_the_restatements_gradients_match_central_differences(name):
    """f = <image, G> along a random direction of all eight inputs: central differences with steps of 1e-6 against autograd (the
    margin, 1e-4, is far above what a step moves any distance: f is smooth between the two evaluations)."""
    base = MH.case(name)
    assert MH.reference(name)["margin"] > 2e-5
    c = MH.leaves({k: (v.to(F64) if k in ("colors", "mark_colors", "joint_colors") else v) for k, v in base.items()})
    names = [n for n in MH.GRAD_NAMES if c[n].numel()]
    gen = torch.Generator().manual_seed(7)
    G = torch.randn(MH.reference(name)["image"].shape, generator=gen, dtype=F64)
    f = lambda cc: (MH.render_marks_host(cc)[0] * G).sum()
    grads = dict(zip(names, torch.autograd.grad(f(c), [c[n] for n in names])))
    live = (torch.arange(8).reshape(1, 1, 8) < (base["nverts"] * (base["kind"] != 0)).unsqueeze(-1)).unsqueeze(-1).expand_as(base["verts_local"])
    scale = {n: 1.0 for n in names}
    scale["p"] = torch.tensor([1.0, 1.0, 1.0]) * (base["p"].abs() < 1e12).to(F64)      # (a step of 1e-6 is lost on 1e15)
    for trial in range(2):
        dirs = {n: torch.randn(c[n].shape, generator=gen, dtype=F64) * scale[n] for n in names}
        dirs["verts_local"] = dirs["verts_local"] * live
        if name == "joints":
            # a segment of no length is a kink (its parameter is 0 by convention; any length at all and it follows the pixel): the two
            # bodies on one point move together and the zero radius stays zero
            dirs["p"][:, 3, 1:] = dirs["p"][:, 2, 1:]
            dirs["radius"][:, 2] = 0.0
        eps = 1e-6
        moved = lambda s: {k: (v.detach() + s * eps * dirs[k] if k in dirs else v) for k, v in c.items()}
        fd = (f(moved(+1)) - f(moved(-1))).item() / (2 * eps)
        ad = float(sum((grads[n] * dirs[n]).sum() for n in names))
        print(name, trial, "central difference", fd, "autograd", ad, "difference", abs(fd - ad))
        assert abs(ad) > 1e-3
        assert abs(fd - ad) <= 1e-6 * max(1.0, abs(ad))


# -------------------------------------------------------------------------------------------------- the entries, without a GPU
def _fake(n, base=1):
    # non-NULL addresses that are never dereferenced: the argument and size checks come first
    return [ctypes.c_void_p(4096 * (k + base)) for k in range(n)]


def _call(lib, which, sizes=(4, 3, 8, 12, 19, 23, 3), ins=None, cam=(0.0, 0.0, 1.0, 1.0), marks=None, nj=2, joints=None, order=0,
          lengths=(1.0, 2.0, 2.0, 5.0), g=ctypes.c_void_p(8192 * 16), outs=None, ws=ctypes.c_void_p(8192 * 32)):
    marks = _fake(2, 20) if marks is None else marks
    joints = _fake(6, 30) if joints is None else joints
    head = (*sizes, *(_fake(7) if ins is None else ins), None, *cam, *marks, nj, *joints, order, *lengths)
    if which == FWD:
        return getattr(lib, FWD)(*head, *(_fake(2, 40) if outs is None else outs), None)
    return getattr(lib, BWD)(*head, g, *(_fake(8, 50) if outs is None else outs), ws, None)


def test_the_library_exports_both_entries_and_lib_binds_them():
    from lcp_physics_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "lcp_hip.h")).read()
    for name, nargs in ((FWD, 36), (BWD, 44)):
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        assert getattr(lib, name).argtypes == args
        assert "int %s(" % name in header


@pytest.mark.parametrize("which", [FWD, BWD])
def test_refusals_come_before_any_launch(which):
    from lcp_physics_amd import _lib
    lib = _lib.load()
    bad = lambda **kw: _call(lib, which, **kw) == -1          # LCP_E_BADARG
    for k in range(7):                                        # kind radius verts_local nverts p colors background
        ins = _fake(7)
        ins[k] = None
        assert bad(ins=ins), k
    assert bad(marks=[ctypes.c_void_p(4096), None])           # marks without their colours
    for k in range(6):                                        # jtype jb1 jb2 jr1 jrot1 joint_colors
        joints = _fake(6, 30)
        joints[k] = None
        assert bad(joints=joints), k
    assert bad(nj=-1) and bad(nj=65) and bad(order=2) and bad(order=-1)
    for k in range(4):                                        # line_w, dot_r, joint_w, joint_r
        for v in ((0.0, -1.0, float("nan")) if k in (0, 2) else (-1.0, float("nan"))):
            lengths = [1.0, 2.0, 2.0, 5.0]
            lengths[k] = v
            assert bad(lengths=lengths), (k, v)
    assert bad(sizes=(4, 65, 8, 12, 19, 23, 3)) and bad(sizes=(4, 3, 7, 12, 19, 23, 3)) and bad(sizes=(4, 3, 8, 1025, 19, 23, 3))
    assert bad(cam=(0.0, 0.0, 0.0, 1.0)) and bad(cam=(0.0, 0.0, 1.0, 0.0))
    if which == FWD:
        assert bad(outs=[None, None])
    else:
        assert bad(outs=[None] * 8) and bad(g=None)
        assert bad(ws=None)                                   # g_p with joints and no workspace


def test_marks_of_follows_the_references_choice_and_render_with_marks_has_no_cpu_fallback():
    from lcp_physics_amd.physics import render as R
    from lcp_physics_amd.physics.contacts import GeometryBatch
    shapes = [("circle", 2.0), ("rect", (3.0, 1.0)), ("hull", [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])]
    marks = R.marks_of(shapes)
    assert marks.dtype == torch.int32 and marks.tolist() == [R.SPOKE, R.DIAGONALS, R.CENTRE] == [MH.SPOKE, MH.DIAGONALS, MH.CENTRE]
    geom = GeometryBatch.from_shapes(shapes, B=2)
    with pytest.raises(RuntimeError, match="GPU"):
        R.render(geom, torch.zeros(2, 3, 3, dtype=F64), R.Camera(8, 8), torch.rand(3, 3), marks=marks)
