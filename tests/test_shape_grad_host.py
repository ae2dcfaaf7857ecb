"""CPU: the host side of the shape gradient of the contact frame (lcp_contacts_shape.hip) - the symbol and its ctypes binding,
the refusals of `lcp_contact_frame_backward_shape_f64` before any launch, and a `GeometryBatch` that keeps the graph of a
learnable shape."""
import ctypes

import pytest
import torch

NAME = "lcp_contact_frame_backward_shape_f64"


def _fake(n):
    # non-NULL addresses that are never dereferenced: the argument and size checks come first
    return [ctypes.c_void_p(4096 * (k + 1)) for k in range(n)]


def _call(lib, nb=4, maxc=16, nvcap=8, vmax=32, ptrs=None, outs=None):
    ptrs = _fake(5) + [0.1] + _fake(6) if ptrs is None else ptrs          # kind radius verts nverts p | eps | count i1 i2 g_n g_p1 g_p2
    outs = _fake(2) if outs is None else outs
    return getattr(lib, NAME)(4, nb, maxc, nvcap, vmax, *ptrs, *outs, None)


def test_the_library_exports_the_entry_and_lib_binds_it():
    from lcp_physics_amd import _lib
    assert NAME in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == 20
    lib = _lib.load()
    assert getattr(lib, NAME).argtypes == args
    header = open(__import__("os").path.join(__import__("os").path.dirname(_lib._HERE), "include", "lcp_hip.h")).read()
    assert "int %s(" % NAME in header


def test_null_required_pointers_are_bad_arguments():
    from lcp_physics_amd import _lib
    lib = _lib.load()
    for k in range(12):
        if k == 5:
            continue                                                        # (eps)
        ptrs = _fake(5) + [0.1] + _fake(6)
        ptrs[k] = None
        assert _call(lib, ptrs=ptrs) == -1, k                               # LCP_E_BADARG
    assert _call(lib, outs=[None, None]) == -1                              # nothing asked for
    assert _call(lib, nb=0) == -1 and _call(lib, maxc=0) == -1 and _call(lib, vmax=-1) == -1


@pytest.mark.parametrize("nb,nvcap,vmax", [(65, 8, 64), (40, 7, 64), (40, 65, 64), (12, 16, 1025)])
def test_sizes_beyond_the_limits_are_refused_before_any_launch(nb, nvcap, vmax):
    from lcp_physics_amd import _lib
    lib = _lib.load()
    assert _call(lib, nb=nb, nvcap=nvcap, vmax=vmax) == -2                  # LCP_E_TOOLARGE
    assert _call(lib, nb=nb, nvcap=nvcap, vmax=vmax, outs=[None] + _fake(1)) == -2
    assert _call(lib, nb=nb, nvcap=nvcap, vmax=vmax, outs=_fake(1) + [None]) == -2


def test_lds_beyond_the_limit_is_refused():
    from lcp_physics_amd import _lib
    assert _call(_lib.load(), nb=64, maxc=4096, nvcap=64, vmax=1024) == -2


def test_geometry_batch_keeps_the_graph_of_a_learnable_shape():
    from lcp_physics_amd.physics.contacts import GeometryBatch
    rad = torch.tensor(20.0, dtype=torch.float64, requires_grad=True)
    tri = torch.tensor([[10.0, 0.0], [-5.0, 8.0], [-5.0, -8.0]], dtype=torch.float64, requires_grad=True)
    g = GeometryBatch.from_shapes([("circle", rad), ("hull", tri), ("rect", (4.0, 2.0)), ("circle", 3.0)], B=5)
    assert g.radius.requires_grad and g.verts_local.requires_grad
    assert g.radius[:, 0].tolist() == [20.0] * 5 and g.radius[:, 3].tolist() == [3.0] * 5
    assert torch.equal(g.verts_local[2, 1, :3].detach(), tri.detach()) and float(g.verts_local[:, 1, 3:].detach().abs().max()) == 0.0
    assert g.nverts.tolist() == [[0, 3, 4, 0]] * 5 and g.scene_verts_max == 7
    g2 = g.to("cpu")
    assert g2.radius.requires_grad and g2.verts_local.requires_grad
    (g2.radius.sum() + (g2.verts_local * 2.0).sum()).backward()
    assert float(rad.grad) == 5.0 and torch.equal(tri.grad, torch.full((3, 2), 10.0, dtype=torch.float64))
    # leaves handed over directly stay leaves
    r = torch.ones(2, 3, dtype=torch.float64, requires_grad=True)
    h = GeometryBatch(g.kind[:2, :3], r, torch.zeros(2, 3, 8, 2, dtype=torch.float64), g.nverts[:2, :3]).to("cpu")
    assert h.radius.requires_grad


def test_frame_function_keeps_its_positional_signature():
    import inspect
    from lcp_physics_amd.physics.contacts import ContactFrameFunction, contact_frame_backward_shape
    names = list(inspect.signature(ContactFrameFunction.forward).parameters)
    assert names == ["ctx", "p", "geom", "frame", "eps", "radius", "verts_local"]
    assert list(inspect.signature(contact_frame_backward_shape).parameters)[:7] == ["geom", "p", "cb", "g_n", "g_p1", "g_p2", "eps"]
