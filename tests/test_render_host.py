"""CPU: the float64 restatement of the drawing (tests/render_host.py) checked on its own - its gradients against central
differences, its hard mask against analytic areas, painter's order - and the host side of the two entry points
`lcp_render_f64` / `lcp_render_backward_f64`: symbols, ctypes bindings, the refusals before any launch, no CPU fallback."""
import ctypes
import math
import os

import pytest
import torch

from tests import render_host as RH

FWD, BWD = "lcp_render_f64", "lcp_render_backward_f64"
F64 = torch.float64


def _scene(bodies, cam, C=3, cap=8, seed=0):
    return RH._assemble([bodies], cam, C, seed, False, cap)


@pytest.mark.parametrize("which", ["p", "radius", "verts_local", "colors", "all"])
def test_the_restatements_gradients_match_central_differences(which):
    """f = <image, G> along a random direction of one input (or of all four): central differences with steps of 1e-6 against
    autograd.  The inputs' decision margin (5e-4) is far above the 1e-5 a step moves any distance, so no pixel changes branch
    between the two evaluations and f is smooth there: the error is the truncation, 1e-12 |f'''|, plus the rounding,
    1e-16 |f| / 1e-6 - bounded by 1e-6 max(1, |df|) with room."""
    base = RH.case("three")
    assert RH.reference("three")["margin"] > 1e-4
    c = RH.leaves({k: (v.to(F64) if k == "colors" else v) for k, v in base.items()})
    names = ("p", "radius", "verts_local", "colors") if which == "all" else (which,)
    gen = torch.Generator().manual_seed(7)
    G = torch.randn(3, 3, base["H"], base["W"], generator=gen, dtype=F64)
    f = lambda cc: (RH.render_host(cc)[0] * G).sum()
    grads = dict(zip(names, torch.autograd.grad(f(c), [c[n] for n in names])))
    live = (torch.arange(8).reshape(1, 1, 8) < base["nverts"].unsqueeze(-1)).unsqueeze(-1).expand(3, 3, 8, 2)
    assert float(grads["verts_local"][~live].abs().max()) == 0.0 if "verts_local" in grads else True
    for trial in range(2):
        dirs = {n: torch.randn(c[n].shape, generator=gen, dtype=F64) for n in names}
        if "verts_local" in dirs:
            dirs["verts_local"] = dirs["verts_local"] * live
        eps = 1e-6
        moved = lambda s: {k: (v.detach() + s * eps * dirs[k] if k in dirs else v) for k, v in c.items()}
        fd = (f(moved(+1)) - f(moved(-1))).item() / (2 * eps)
        ad = float(sum((grads[n] * dirs[n]).sum() for n in names))
        print(which, trial, "central difference", fd, "autograd", ad, "difference", abs(fd - ad))
        assert abs(ad) > 1e-3                                                   # (the direction does move the image)
        assert abs(fd - ad) <= 1e-6 * max(1.0, abs(ad))


@pytest.mark.parametrize("shape", ["circle", "rect"])
def test_the_hard_mask_has_the_analytic_area(shape):
    """Pixels with d <= 0 are the pixel centres inside the shape: |count / ppm^2 - area| <= perimeter sqrt(2) / ppm (every pixel
    that the count gets wrong is cut by the boundary, and those lie within half a pixel diagonal of it on either side)."""
    ppm = 1.7
    cam = (61, 67, -2.3, 1.9, ppm, 1.0 / ppm)
    if shape == "circle":
        r = 9.37
        bodies, area, perimeter = [("circle", (0.3, 17.13, 19.71), r, 0.0)], math.pi * r * r, 2 * math.pi * r
    else:
        a, b = 21.3, 11.9
        bodies, area, perimeter = [("hull", (0.47, 17.13, 19.71), RH._rect(a, b), 3.0)], a * b, 2 * (a + b)      # (outlined: the mask is filled)
    _, ids, _ = RH.render_host(_scene(bodies, cam))
    count = int((ids == 0).sum())
    print(shape, "count / ppm^2", count / ppm ** 2, "area", area, "bound", perimeter * math.sqrt(2) / ppm)
    assert abs(count / ppm ** 2 - area) <= perimeter * math.sqrt(2) / ppm
    assert int((ids == -1).sum()) == ids.numel() - count


def test_painters_order_on_overlapping_bodies():
    """Later over earlier (world.py:279-280): deep inside both of two filled bodies the image is the later body's colour and the
    mask its index; inside an outline's hole the earlier body shows through, but the mask still names the outlined body."""
    cam = (24, 24, 0.0, 0.0, 1.0, 1.0)
    a = ("hull", (0.1, 10.2, 11.3), RH._rect(14.0, 12.0), 0.0)
    b = ("circle", (0.0, 13.4, 12.6), 6.0, 0.0)
    ring = ("circle", (0.0, 13.4, 12.6), 6.0, 1.5)
    at = (12, 13)                                                                 # row, column: the world point (13.5, 12.5)
    for bodies, colour_of, top in (([a, b], 1, 1), ([b, a], 1, 1), ([a, ring], 0, 1), ([ring, a], 1, 1)):
        c = _scene(bodies, cam)
        image, ids, _ = RH.render_host(c)
        assert torch.equal(image[0, :, at[0], at[1]], c["colors"][0, colour_of].to(F64)), bodies
        assert int(ids[0, at[0], at[1]]) == top
    image, ids, _ = RH.render_host(_scene([a, b], cam))
    assert torch.equal(image[0, :, 0, 23], _scene([a, b], cam)["background"].to(F64)) and int(ids[0, 0, 23]) == -1


# -------------------------------------------------------------------------------------------------- the entries, without a GPU
def _fake(n):
    # non-NULL addresses that are never dereferenced: the argument and size checks come first
    return [ctypes.c_void_p(4096 * (k + 1)) for k in range(n)]


def _fwd(lib, sizes=(4, 3, 8, 12, 19, 23, 3), ins=None, thickness=None, cam=(0.0, 0.0, 1.0, 1.0), outs=None):
    return getattr(lib, FWD)(*sizes, *(_fake(7) if ins is None else ins), thickness, *cam, *(_fake(2) if outs is None else outs), None)


def _bwd(lib, sizes=(4, 3, 8, 12, 19, 23, 3), ins=None, thickness=None, cam=(0.0, 0.0, 1.0, 1.0), g=ctypes.c_void_p(8192 * 16), outs=None):
    return getattr(lib, BWD)(*sizes, *(_fake(7) if ins is None else ins), thickness, *cam, g, *(_fake(4) if outs is None else outs), None)


def test_the_library_exports_both_entries_and_lib_binds_them():
    from lcp_physics_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "lcp_hip.h")).read()
    for name, nargs in ((FWD, 22), (BWD, 25)):
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        assert getattr(lib, name).argtypes == args
        assert "int %s(" % name in header


def test_null_required_pointers_are_bad_arguments():
    from lcp_physics_amd import _lib
    lib = _lib.load()
    for k in range(7):                                             # kind radius verts_local nverts p colors background
        ins = _fake(7)
        ins[k] = None
        assert _fwd(lib, ins=ins) == -1 and _bwd(lib, ins=ins) == -1, k          # LCP_E_BADARG
    assert _fwd(lib, outs=[None, None]) == -1 and _bwd(lib, outs=[None] * 4) == -1          # nothing asked for
    assert _bwd(lib, g=None) == -1


@pytest.mark.parametrize("sizes,cam", [
    ((0, 3, 8, 12, 19, 23, 3), None), ((4, 0, 8, 12, 19, 23, 3), None), ((4, 65, 8, 12, 19, 23, 3), None),        # B, nb
    ((4, 3, 7, 12, 19, 23, 3), None), ((4, 3, 65, 12, 19, 23, 3), None),                                           # capacity
    ((4, 3, 8, -1, 19, 23, 3), None), ((4, 3, 8, 1025, 19, 23, 3), None),                                          # scene_verts_max
    ((4, 3, 8, 12, 0, 23, 3), None), ((4, 3, 8, 12, 19, 0, 3), None),                                              # H, W
    ((4, 3, 8, 12, 19, 23, 0), None), ((4, 3, 8, 12, 19, 23, 5), None),                                            # C
    ((4096, 3, 8, 12, 512, 512, 2), None), ((1, 3, 8, 12, 32768, 32768, 2), None),                                 # B C H W >= 2^31
    (None, (0.0, 0.0, 0.0, 1.0)), (None, (0.0, 0.0, -1.0, 1.0)), (None, (0.0, 0.0, float("nan"), 1.0)),            # ppm
    (None, (0.0, 0.0, 1.0, 0.0)), (None, (0.0, 0.0, 1.0, -2.0)), (None, (0.0, 0.0, 1.0, float("nan")))])           # w
def test_bad_sizes_and_cameras_are_refused_before_any_launch(sizes, cam):
    from lcp_physics_amd import _lib
    lib = _lib.load()
    kw = {}
    if sizes is not None:
        kw["sizes"] = sizes
    if cam is not None:
        kw["cam"] = cam
    assert _fwd(lib, **kw) == -1 and _bwd(lib, **kw) == -1


def test_render_has_no_cpu_fallback():
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.render import Camera, render, render_ids
    geom = GeometryBatch.from_shapes([("circle", 2.0), ("rect", (3.0, 1.0))], B=2)
    p = torch.zeros(2, 2, 3, dtype=F64)
    with pytest.raises(RuntimeError, match="GPU"):
        render(geom, p, Camera(8, 8), torch.rand(2, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        render_ids(geom, p, Camera(8, 8))
    with pytest.raises(ValueError):
        Camera(0, 8)
