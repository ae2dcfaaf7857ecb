"""Device routing table: one call per kernel family and workspace layout, forward then backward.  Each forward must leave the
layout tag it has always left in the workspace trailer (the last 256 bytes of a workspace of exactly lcp_workspace_bytes), and each
backward must either return finite gradients or fail with the return code it has always given."""
import numpy as np
import pytest
import torch

DEV = "cuda"
B = 8


def _tag(ws):
    return int(ws[-256:-252].cpu().numpy().view(np.int32)[0])


def _finite(grads):
    vals = grads.values() if isinstance(grads, dict) else [g for g in grads if g is not None]
    return all(bool(torch.isfinite(g).all()) for g in vals)


def _backward(fn):
    """'finite', 'nan' or the error code name a backward ends with."""
    try:
        g = fn()
        torch.cuda.synchronize()
    except RuntimeError as err:
        for code in ("LCP_E_BADARG", "LCP_E_TOOLARGE", "LCP_E_LAUNCH"):
            if code in str(err):
                return code
        raise
    return "finite" if _finite(g) else "nan"


def _scene(kind):
    from lcp_physics_amd import scenes
    if kind == "stack":                                     # 3 bodies, 8 contacts, the pinned floor: four scenes per wave
        sc = scenes.make_stack_scenes(B=B, nbox=2, pts_per_interface=4, seed=7, dtype=torch.float32)
    elif kind == "joints6":                                 # the same with six general equality rows: the wave64 step
        sc = scenes.make_stack_scenes(B=B, nbox=2, pts_per_interface=4, seed=7, dtype=torch.float32)
        sc.Je = torch.randn(B, 6, 3 * sc.nb, generator=torch.Generator().manual_seed(3)).float()
    else:                                                   # BASELINE config 5: 11 bodies, 64 contacts
        sc = scenes.make_pile_scenes(B=B, seed=3, dtype=torch.float32)
    return sc.to(device=DEV)


def _buffers(sc):
    from lcp_physics_amd.physics.contacts import ContactBuffers
    cb = ContactBuffers(sc.B, sc.nb, sc.nc, DEV)
    cb.c_n, cb.c_p1, cb.c_p2, cb.c_i1, cb.c_i2 = sc.c_n, sc.c_p1, sc.c_p2, sc.c_i1, sc.c_i2
    return cb


def _fused(kind, compute="f64", path="auto", pinned=None):
    from lcp_physics_amd.physics.batched_world import fused_step, fused_step_backward
    sc = _scene(kind)
    out = fused_step(sc, compute=compute, path=path, pinned=pinned)
    torch.cuda.synchronize()
    dl = torch.randn(B, sc.nb, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    return _tag(out["ws"]), _backward(lambda: fused_step_backward(sc, out, dl, compute=compute))


def _counts(kind, compute="f64", path="auto", pinned=False):
    from lcp_physics_amd.physics.batched_world import solve_dynamics, solve_dynamics_backward
    sc = _scene(kind)
    cb, e = _buffers(sc), sc.Je.shape[1]
    cnt = torch.full((B,), sc.nc, dtype=torch.int32, device=DEV)
    out = solve_dynamics(B, sc.nb, sc.nc, e, cnt, sc.Mdiag, sc.v, sc.f, sc.rest, sc.fric, cb, sc.Je, sc.dt, compute=compute,
                         path=path, pinned=pinned)
    torch.cuda.synchronize()
    dl = torch.randn(B, sc.nb, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    return _tag(out["ws"]), _backward(lambda: solve_dynamics_backward(B, sc.nb, sc.nc, e, sc.Mdiag, sc.v, sc.f, sc.rest, sc.fric,
                                                                      cb, sc.Je, sc.dt, dl, out, compute=compute, want_Je=True))


def _poststab(kind, compute="f64", path="auto"):
    from lcp_physics_amd import _lib
    from lcp_physics_amd.physics.batched_world import post_stabilization, post_stabilization_backward
    sc = _scene(kind)
    cb, e = _buffers(sc), sc.Je.shape[1]
    cnt = torch.full((B,), sc.nc, dtype=torch.int32, device=DEV)
    _lib.set_path(path)
    try:
        out = post_stabilization(B, sc.nb, sc.nc, e, cnt, sc.Mdiag, sc.v, sc.rest, cb, sc.Je, compute=compute)
        torch.cuda.synchronize()
    finally:
        _lib.set_path("auto")
    dl = torch.randn(B, sc.nb, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    return _tag(out["ws"]), _backward(lambda: post_stabilization_backward(B, sc.nb, sc.nc, e, sc.Mdiag, sc.v, sc.rest, cb, sc.Je,
                                                                          dl, out, compute=compute, want_Je=True))


def _dense(kind, compute="f64", path="auto", io_f64=False, perturb_A=False, all_contact=False):
    from lcp_physics_amd.lcp import lcp_backward, lcp_solve
    from lcp_physics_amd.physics import assemble_contacts
    sc = _scene(kind)
    lcp = list(assemble_contacts(sc))
    if perturb_A:                                           # equality rows that do not pin the leading coordinates: class 3
        lcp[4] = lcp[4] + 0.01 * torch.rand(lcp[4].shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    if io_f64:
        lcp = [t.double() for t in lcp]
    sol = lcp_solve(*lcp, compute=compute, path=path)
    torch.cuda.synchronize()
    cot = torch.randn(B, lcp[0].shape[1], generator=torch.Generator().manual_seed(2)).to(DEV, lcp[0].dtype)
    return _tag(sol.ws), _backward(lambda: lcp_backward(sol, cot))


def _all_contact(kind, compute="f64", path="auto"):
    """The dense backward of a fused step (LCP_HINT_ALL_CONTACT) on the workspace the step left."""
    from lcp_physics_amd.physics.batched_world import fused_step, solution_of_step
    from lcp_physics_amd.physics import assemble_contacts
    from lcp_physics_amd.lcp import lcp_backward
    sc = _scene(kind)
    out = fused_step(sc, compute=compute, path=path)
    lcp = assemble_contacts(sc)
    torch.cuda.synchronize()
    sol = solution_of_step(sc, out, lcp[2], lcp[4], compute=compute)
    cot = torch.randn(B, lcp[0].shape[1], generator=torch.Generator().manual_seed(2)).to(DEV)
    return _tag(out["ws"]), _backward(lambda: lcp_backward(sol, cot))


# (case, call, tag the forward leaves, how the backward ends)
CASES = [
    ("step quad body", lambda: _fused("stack"), 4, "finite"),
    ("step quad contact space", lambda: _fused("stack", path="big"), 5, "finite"),
    ("step quad fp32", lambda: _fused("stack", compute="f32"), 5, "finite"),
    ("step quad forced", lambda: _fused("stack", path="quad"), 4, "finite"),
    ("step solo forced", lambda: _fused("stack", path="solo"), 4, "finite"),
    ("step quad unpinned", lambda: _fused("stack", pinned=False), 4, "finite"),
    ("step generic", lambda: _fused("stack", path="generic"), 9, "finite"),
    ("step primal forced", lambda: _fused("stack", path="primal"), 6, "finite"),
    ("step primal_wg forced", lambda: _fused("stack", path="primal_wg"), 13, "finite"),
    ("step primal pinned", lambda: _fused("pile"), 6, "finite"),
    ("step primal unpinned", lambda: _fused("pile", pinned=False), 6, "finite"),
    ("step big", lambda: _fused("pile", path="big"), 7, "finite"),
    ("step fp32 generic", lambda: _fused("pile", compute="f32"), 9, "finite"),
    ("step primal_wg pinned", lambda: _fused("pile", path="primal_wg"), 13, "finite"),
    ("step wave64", lambda: _fused("joints6", compute="f32"), 8, "LCP_E_TOOLARGE"),
    ("counts quad", lambda: _counts("stack", pinned=True), 4, "finite"),
    ("counts primal", lambda: _counts("pile", pinned=True), 6, "finite"),
    ("counts primal_wg", lambda: _counts("pile", path="primal_wg", pinned=True), 13, "finite"),
    ("counts wave64 sizes: generic", lambda: _counts("joints6", compute="f32"), 9, "LCP_E_TOOLARGE"),
    ("poststab quad", lambda: _poststab("stack"), 10, "finite"),
    ("poststab primal forced", lambda: _poststab("stack", path="primal"), 10, "finite"),
    ("poststab primal", lambda: _poststab("pile"), 10, "finite"),
    ("poststab generic", lambda: _poststab("stack", path="generic"), 11, "finite"),
    ("poststab fp32", lambda: _poststab("pile", compute="f32"), 11, "finite"),
    ("dense wave64 quad body", lambda: _dense("stack"), 12, "finite"),
    ("dense wave64 contact space", lambda: _dense("stack", path="big"), 1, "finite"),
    ("dense wave64 fp32", lambda: _dense("stack", compute="f32"), 1, "finite"),
    ("dense wave64 wave", lambda: _dense("joints6"), 1, "finite"),
    ("dense generic", lambda: _dense("stack", path="generic"), 3, "finite"),
    ("dense fp64 io", lambda: _dense("stack", io_f64=True), 1, "finite"),
    ("dense big primal class 4", lambda: _dense("pile"), 2, "finite"),
    ("dense big primal class 3", lambda: _dense("pile", perturb_A=True), 2, "finite"),
    ("dense big contact space", lambda: _dense("pile", path="big"), 2, "finite"),
    ("dense fp32 generic", lambda: _dense("pile", compute="f32"), 3, "finite"),
    ("dense fp64 io generic sizes", lambda: _dense("pile", io_f64=True), 3, "finite"),
    ("all-contact quad body", lambda: _all_contact("stack"), 4, "finite"),
    ("all-contact quad contact space", lambda: _all_contact("stack", path="big"), 5, "finite"),
    ("all-contact generic", lambda: _all_contact("stack", path="generic"), 9, "finite"),
    ("all-contact primal", lambda: _all_contact("pile"), 6, "LCP_E_TOOLARGE"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case,call,tag,bwd", CASES, ids=[c[0] for c in CASES])
def test_forward_tag_and_backward(case, call, tag, bwd):
    got_tag, got_bwd = call()
    print(case, "tag", got_tag, "backward", got_bwd)
    assert (got_tag, got_bwd) == (tag, bwd), case


@pytest.mark.gpu
def test_fused_step_backward_is_solve_dynamics_backward_on_the_same_record():
    """The two host entries of `lcp_step_backward_je_f32` on ONE forward record: every gradient, Je's included, bit for bit."""
    from lcp_physics_amd.physics.batched_world import fused_step, fused_step_backward, solve_dynamics_backward
    sc = _scene("stack")
    e = sc.Je.shape[1]
    out = fused_step(sc)
    dl = torch.randn(B, sc.nb, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    ga = fused_step_backward(sc, out, dl, want_Je=True)
    gb = solve_dynamics_backward(B, sc.nb, sc.nc, e, sc.Mdiag, sc.v, sc.f, sc.rest, sc.fric, _buffers(sc), sc.Je, sc.dt, dl, out,
                                 want_Je=True)
    torch.cuda.synchronize()
    assert e == 3 and sorted(ga) == sorted(gb) == sorted(("Mdiag", "v", "f", "rest", "fric", "c_n", "c_p1", "c_p2", "Je"))
    for k in ga:
        assert ga[k].shape == gb[k].shape and _finite({k: ga[k]})
        assert torch.equal(ga[k].view(torch.int32), gb[k].view(torch.int32)), k
