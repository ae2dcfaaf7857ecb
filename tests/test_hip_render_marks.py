"""GPU: the drawing with marks and joint markers on the device (lcp_render_marks.hip: `lcp_render_marks_f64`,
`lcp_render_marks_backward_f64`, through `lcp_physics_amd.physics.render`) against its float64 restatement on the CPU
(tests/render_marks_host.py).

The tolerances are those of tests/test_hip_render.py for the same arithmetic.  Every parity test first asserts the decision margin
of its inputs (> 1e-6; tests/test_render_marks_host.py checks the same condition without a GPU) and then compares EVERY pixel:
  image   |device - host| <= 1e-6 for colours in [0, 1]: the fp32 store rounds by at most 6e-8, fp64 reordering gives ~1e-12 / w
  ids     identical to `render_ids` (marks and markers do not change the mask) and to the restatement's
  grads   each of the eight tensors within 1e-9 max|g| of autograd's for a random fp32 cotangent, and bit-identical across two runs."""
import pytest
import torch

from tests import render_host as RH
from tests import render_marks_host as MH

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64


def _device(c, leaves=False):
    """(geom, p, cam, colors, kwargs of render) of a case of render_marks_host.py on the device; with `leaves` the eight
    differentiable inputs require grad (`kw["jrot1"]`, `kw["joints"].jr1`, `kw["mark_colors"]`, `kw["joint_colors"]` among them)."""
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.joints import JointSet
    from lcp_physics_amd.physics.render import Camera
    t = lambda k: c[k].to(DEV).contiguous()
    geom = GeometryBatch(t("kind"), t("radius"), t("verts_local"), t("nverts"), None, None)
    p, colors = t("p"), t("colors")
    kw = dict(background=t("background"), thickness=t("thickness"), edge_width=c["w"], marks=t("mark"), mark_colors=t("mark_colors"),
              marks_over=bool(c["order"]), mark_width=c["line_w"], dot_radius=c["dot_r"], joint_width=c["joint_w"], joint_radius=c["joint_r"])
    if c["jtype"].shape[1]:
        kw.update(joints=JointSet(t("jtype"), t("jb1"), t("jb2"), t("jr1"), t("jrot1").clone(), 0), jrot1=t("jrot1"), joint_colors=t("joint_colors"))
    if leaves:
        for x in (geom.radius, geom.verts_local, p, colors, kw["mark_colors"]):
            x.requires_grad_(True)
        if "joints" in kw:
            for x in (kw["joint_colors"], kw["jrot1"], kw["joints"].jr1):
                x.requires_grad_(True)
    cam = Camera(c["H"], c["W"], origin=(c["x0"], c["y0"]), pixels_per_meter=c["ppm"])
    return geom, p, cam, colors, kw


def _grads(geom, p, colors, kw):
    j = "joints" in kw
    return dict(p=p.grad, radius=geom.radius.grad, verts_local=geom.verts_local.grad, colors=colors.grad, mark_colors=kw["mark_colors"].grad,
                joint_colors=kw["joint_colors"].grad if j else None, jrot1=kw["jrot1"].grad if j else None,
                jr1=kw["joints"].jr1.grad if j else None)


@pytest.mark.parametrize("name", MH.CASE_NAMES)
def test_image_and_mask_match_the_restatement(name):
    from lcp_physics_amd.physics.render import render, render_ids
    c, ref = MH.case(name), MH.reference(name)
    assert ref["margin"] > 1e-6, ref["margin"]
    geom, p, cam, colors, kw = _device(c)
    ids = torch.full((3, c["H"], c["W"]), -7, dtype=torch.int32, device=DEV)
    image = render(geom, p, cam, colors, ids_out=ids, **kw)
    only_ids = render_ids(geom, p, cam)
    assert image.dtype == torch.float32 and image.shape == ref["image"].shape
    err = float((image.cpu().to(F64) - ref["image"]).abs().max())
    plain = render(geom, p, cam, colors, background=kw["background"], thickness=kw["thickness"], edge_width=kw["edge_width"])
    print(name, "margin %.3g" % ref["margin"], "image error %.3g" % err, "mask pixels that differ", int((ids.cpu() != ref["ids"]).sum()),
          "pixels the marks and markers change", int(((image - plain).abs().amax(1) > 1e-3).sum()))
    assert err <= 1e-6
    assert torch.equal(ids, only_ids) and torch.equal(ids.cpu(), ref["ids"])
    assert int(((image - plain).abs().amax(1) > 1e-3).sum()) > 0          # (they are in the picture)


@pytest.mark.parametrize("name", MH.CASE_NAMES)
def test_gradients_match_autograd_of_the_restatement_and_repeat_bitwise(name):
    from lcp_physics_amd.physics.render import render
    c, ref = MH.case(name), MH.reference(name)
    assert ref["margin"] > 1e-6, ref["margin"]
    g = ref["g_image"].to(DEV)
    runs = []
    for _ in range(2):
        geom, p, cam, colors, kw = _device(c, leaves=True)
        render(geom, p, cam, colors, **kw).backward(g)
        runs.append(_grads(geom, p, colors, kw))
    torch.cuda.synchronize()
    nj = c["jtype"].shape[1]
    bad = []
    for n, want in ref["grads"].items():
        if not want.numel():                                          # (a case without joints)
            assert nj == 0 and runs[0][n] is None
            continue
        got = runs[0][n].cpu()
        assert got.dtype == want.dtype and got.shape == want.shape, n
        scale = float(want.abs().max())
        err = float((got.to(F64) - want.to(F64)).abs().max())
        print(name, n, "max|g| %.3g" % scale, "error %.3g" % err, "relative %.3g" % (err / scale))
        assert scale > 0.0
        if not err <= 1e-9 * scale:
            bad.append((n, err / scale))
        assert torch.equal(runs[0][n].view(torch.uint8), runs[1][n].view(torch.uint8)), (n, "two runs differ")
    assert bad == []
    got = {n: (None if t is None else t.cpu()) for n, t in runs[0].items()}
    hull = c["kind"] != 0
    nv = c["nverts"] * hull
    pad = torch.arange(c["verts_local"].shape[2]).reshape(1, 1, -1) >= nv.unsqueeze(-1)
    assert float(got["verts_local"][pad].abs().max()) == 0.0 and float(got["radius"][hull].abs().max()) == 0.0
    m = c["mark"]
    undrawn = ~(((m == MH.SPOKE) & ~hull) | (m == MH.CENTRE) | ((m == MH.DIAGONALS) & hull & (nv == 4)))
    if undrawn.any():
        assert float(got["mark_colors"][undrawn].abs().max()) == 0.0
    if nj:
        other = c["jtype"] != MH.JOINT
        assert float(got["jrot1"][other].abs().max()) == 0.0 and float(got["jr1"][other].abs().max()) == 0.0
        gone = (c["jtype"] == MH.FIXED) & (c["jb2"] < 0)
        if gone.any():
            assert float(got["joint_colors"][gone].abs().max()) == 0.0


def _raw(lib, name, c, marks, g=None):
    """One call of a C entry on case `c` of render_host.py; `marks`: the arguments between the camera and the outputs."""
    from lcp_physics_amd import _lib
    t = {k: c[k].to(DEV).contiguous() for k in ("kind", "radius", "verts_local", "nverts", "p", "colors", "background", "thickness")}
    B, nb, cap = c["verts_local"].shape[:3]
    H, W, C = c["H"], c["W"], c["colors"].shape[2]
    P = _lib.ptr
    head = (B, nb, cap, int((c["nverts"] * (c["kind"] != 0)).sum(1).max()), H, W, C, P(t["kind"]), P(t["radius"]), P(t["verts_local"]),
            P(t["nverts"]), P(t["p"]), P(t["colors"]), P(t["background"]), P(t["thickness"]), c["x0"], c["y0"], c["ppm"], c["w"], *marks)
    dev = torch.device(DEV)
    if g is None:
        outs = [torch.full((B, C, H, W), -3.0, dtype=torch.float32, device=DEV), torch.full((B, H, W), -7, dtype=torch.int32, device=DEV)]
        rc = getattr(lib, name)(*head, *[P(o) for o in outs], _lib.stream_ptr(dev))
    else:
        outs = [torch.full(s, float("nan"), dtype=d, device=DEV) for s, d in (((B, nb, 3), F64), ((B, nb), F64), ((B, nb, cap, 2), F64),
                                                                               ((B, nb, C), torch.float32))]
        extra = [None] * 5 if marks else []
        rc = getattr(lib, name)(*head, P(g), *[P(o) for o in outs], *extra, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == 0, (name, rc)
    return outs


@pytest.mark.parametrize("name", ["three", "special", "nb64"])
def test_nothing_in_same_out(name):
    """The new C entries with mark = NULL and nj = 0 on the cases of the plain drawing: image and ids bitwise those of lcp_render_f64,
    the gradients within 1e-9 max|g| of lcp_render_backward_f64's."""
    from lcp_physics_amd import _lib
    lib = _lib.load()
    c = RH.case(name)
    none = (None, None, 0, None, None, None, None, None, None, 0, 1.0, 2.0, 2.0, 5.0)
    old, new = _raw(lib, "lcp_render_f64", c, ()), _raw(lib, "lcp_render_marks_f64", c, none)
    assert torch.equal(old[0].view(torch.int32), new[0].view(torch.int32)) and torch.equal(old[1], new[1])
    g = RH.reference(name)["g_image"].to(DEV)
    old, new = _raw(lib, "lcp_render_backward_f64", c, (), g), _raw(lib, "lcp_render_marks_backward_f64", c, none, g)
    for n, a, b in zip(("p", "radius", "verts_local", "colors"), old, new):
        scale, err = float(a.abs().max()), float((a.to(F64) - b.to(F64)).abs().max())
        print(name, n, "max|g| %.3g" % scale, "difference %.3g" % err)
        assert scale > 0.0 and err <= 1e-9 * scale, n


def test_render_without_marks_and_joints_takes_the_plain_entry():
    """`render` with neither `marks` nor `joints` is today's call: the bits of `lcp_render_f64`, and no new autograd node."""
    from lcp_physics_amd import _lib
    from lcp_physics_amd.physics.render import RenderFunction, render
    c = MH.case("marks3")
    geom, p, cam, colors, kw = _device(c)
    plain = {k: kw[k] for k in ("background", "thickness", "edge_width")}
    p.requires_grad_(True)
    image = render(geom, p, cam, colors, **plain)
    assert type(image.grad_fn).__name__.startswith(RenderFunction.__name__)
    want = _raw(_lib.load(), "lcp_render_f64", c, ())[0]
    assert torch.equal(image.detach(), want)


def test_only_the_gradients_that_are_needed_are_computed_and_shared_colours_sum_over_the_scenes():
    from lcp_physics_amd.physics.render import render
    c, ref = MH.case("limits"), MH.reference("limits")
    g = ref["g_image"].to(DEV)
    geom, p, cam, colors, kw = _device(c)
    assert not render(geom, p, cam, colors, **kw).requires_grad
    kw["jrot1"].requires_grad_(True)
    render(geom, p, cam, colors, **kw).backward(g)
    assert p.grad is None and geom.radius.grad is None and geom.verts_local.grad is None and colors.grad is None
    assert kw["mark_colors"].grad is None and kw["joint_colors"].grad is None and kw["joints"].jr1.grad is None
    want = ref["grads"]["jrot1"]
    assert float((kw["jrot1"].grad.cpu() - want).abs().max()) <= 1e-9 * float(want.abs().max())
    kw["jrot1"] = kw["jrot1"].detach()
    p.requires_grad_(True)
    render(geom, p, cam, colors, **kw).backward(g)
    want = ref["grads"]["p"]
    assert float((p.grad.cpu() - want).abs().max()) <= 1e-9 * float(want.abs().max())
    assert kw["joints"].jr1.grad is None and kw["mark_colors"].grad is None
    # [nb,C] / [nj,C] colours shared by the scenes: the fp32 sum of the three scenes' fp32 gradients (two roundings of 6e-8 relative
    # to the largest partial sum)
    shared = {n: kw[n][0].clone().requires_grad_(True) for n in ("mark_colors", "joint_colors")}
    render(geom, p.detach(), cam, colors, **dict(kw, **shared)).backward(g)
    for n, leaf in shared.items():
        want = ref["grads"][n].to(F64).sum(0)
        assert float((leaf.grad.cpu().to(F64) - want).abs().max()) <= 4 * 6e-8 * float(ref["grads"][n].abs().max()) * 3, n


def test_default_colours_are_the_references_and_need_three_channels():
    from lcp_physics_amd.physics.render import render
    geom, p, cam, colors, kw = _device(MH.case("joints"))             # C = 4
    blue = torch.tensor([0.0, 0.0, 1.0, 1.0], device=DEV).expand(3, 5, 4).contiguous()
    green = torch.tensor([0.0, 1.0, 0.0, 1.0], device=DEV).expand(3, 9, 4).contiguous()
    named = render(geom, p, cam, colors, **dict(kw, mark_colors=blue, joint_colors=green))
    assert torch.equal(render(geom, p, cam, colors, **dict(kw, mark_colors=None, joint_colors=None)), named)
    one = colors[..., :1].contiguous()
    with pytest.raises(ValueError):
        render(geom, p, cam, one, **dict(kw, background=kw["background"][:1].contiguous(), mark_colors=None, joint_colors=None))


def test_render_with_marks_into_out_replays_bitwise_from_a_graph():
    from lcp_physics_amd.physics.render import render
    c = MH.case("joints")
    geom, p, cam, colors, kw = _device(c)
    geom.verts_max()                                                  # (the one host read of the geometry, before the capture)
    eager = render(geom, p, cam, colors, **kw)
    out = torch.zeros_like(eager)
    ids = torch.zeros(3, c["H"], c["W"], dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        render(geom, p, cam, colors, out=out, ids_out=ids, **kw)                    # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        render(geom, p, cam, colors, out=out, ids_out=ids, **kw)
    for shift in (0.0, 3.25):
        p[:, :4, 1] += shift                                          # the graph reads the pose through the same pointer
        kw["jrot1"] += shift
        out.fill_(-1.0)
        ids.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
        again = render(geom, p, cam, colors, **kw)
        assert torch.equal(out, again) and (shift == 0.0) == torch.equal(out, eager)
    _, host_ids, margin = MH.render_marks_host(dict(c, p=p.cpu(), jrot1=kw["jrot1"].cpu()))
    assert margin > 1e-6 and torch.equal(ids.cpu(), host_ids)


def _world(B=4, joints=True, leaf=True):
    """A pendulum (a circle on a revolute joint) next to a free outlined ball on a floor that a TOTAL joint pins; the camera sees all."""
    from lcp_physics_amd.physics.bodies import BodyBatch
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.joints import JointSet
    from lcp_physics_amd.physics.render import Camera, marks_of
    shapes = [("rect", [500.0, 500.0], [900.0, 10.0]), ("circle", [340.0, 390.0], 20.0), ("circle", [560.0, 474.5], 20.0, {"vel": (0.0, 30.0, 0.0)})]
    bb = BodyBatch.from_list(shapes, B, g=100.0)
    p0 = bb.p0.detach().clone().requires_grad_(leaf)
    if joints:
        js = JointSet.from_list([("total", 0), ("joint", 1, None, (300.0, 340.0))], p0.detach())
        world = ContactWorld(bb.geom, p0, bb.v0, bb.Mdiag, bb.f_gravity, bb.rest, bb.fric, joints=js, dt=1.0 / 30, maxc=8)
    else:
        f = bb.f_gravity.clone()
        f[:, 0] = 0.0
        Je = torch.eye(3, 9, dtype=torch.float32, device=DEV).unsqueeze(0).repeat(B, 1, 1)
        world = ContactWorld(bb.geom, p0, bb.v0, bb.Mdiag, f, bb.rest, bb.fric, Je=Je, dt=1.0 / 30, maxc=8)
    cam = Camera(48, 80, origin=(269.3, 319.1), pixels_per_meter=0.25)
    colors = torch.tensor([[0.2, 0.3, 0.4], [0.9, 0.1, 0.2], [0.1, 0.8, 0.3]], dtype=torch.float32, device=DEV)
    thickness = torch.tensor([0.0, 6.0, 6.0], dtype=F64, device=DEV).expand(B, 3).contiguous()
    return world, p0, cam, colors, dict(thickness=thickness, marks=marks_of(shapes).to(DEV))


def test_world_render_draws_the_worlds_joints_and_a_pixel_loss_reaches_the_balls_spin():
    from lcp_physics_amd.physics.render import render
    world, p0, cam, colors, kw = _world()
    assert torch.equal(world.render(cam, colors, joints=True, **kw), render(world.geom, world.p, cam, colors, joints=world.joints, **kw))
    assert not torch.equal(world.render(cam, colors, joints=True, **kw), world.render(cam, colors, **kw))
    for _ in range(3):
        world.step(differentiable=True)
    assert world._jrot_ad is not None and world._jrot_ad.requires_grad
    image = world.render(cam, colors, joints=True, **kw)
    assert image.requires_grad
    assert torch.equal(image.detach(), render(world.geom, world.p.detach(), cam, colors, joints=world.joints, jrot1=world.joints.jrot1, **kw))
    weight = torch.randn(image.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    (image * weight).sum().backward()
    g = p0.grad.cpu()
    print("d loss / d p0 with marks and joints", g[0].tolist())
    assert bool(torch.isfinite(g).all()) and float(g[:, 2, 0].abs().min()) > 0.0          # every scene's ball: its angle moves the pixels
    assert float(g[:, 1].abs().min()) > 0.0                                                # and the pendulum
    # the same roll-out drawn without marks: the ball's angle is invisible
    world, p0, cam, colors, kw = _world()
    for _ in range(3):
        world.step(differentiable=True)
    (world.render(cam, colors, thickness=kw["thickness"]) * weight).sum().backward()
    g = p0.grad.cpu()
    print("d loss / d p0 without", g[0].tolist())
    assert bool(torch.isfinite(g).all()) and float(g[:, 2, 0].abs().max()) == 0.0 and float(g[:, 2, 1:].abs().min()) > 0.0


def test_joints_true_needs_a_jointset():
    from lcp_physics_amd.physics.render import FrameRecorder
    world, _, cam, colors, kw = _world(joints=False, leaf=False)
    with pytest.raises(ValueError):
        world.render(cam, colors, joints=True, **kw)
    with pytest.raises(ValueError):
        FrameRecorder(world, cam, colors, capacity=1, joints=True, **kw).record()
    assert world.render(cam, colors, **kw).shape == (4, 3, 48, 80)    # (marks alone need none)


def test_descent_on_a_circles_angle_follows_the_restatements_descent():
    """Ten fixed steps of gradient descent turning an outlined circle's spoke towards a target frame, on the device and on the
    restatement: the losses agree within 1e-6 relative at every iteration (the device image is fp32: 6e-8 per pixel of the ramp, against
    differences of order 1; the descent is stopped before it converges).  Without the spoke this gradient is identically zero."""
    from lcp_physics_amd.physics.render import render
    target = MH.render_marks_host(MH.spin_case(1.15, MH.SPOKE))[0].detach().to(torch.float32)
    lr, steps = 2.0, 10
    c = MH.spin_case(0.55, MH.SPOKE)
    turn = torch.tensor([1.0, 0.0, 0.0], dtype=F64)
    host_p, host_loss = c["p"].clone(), []
    for _ in range(steps):
        hp = host_p.clone().requires_grad_(True)
        image, _, margin = MH.render_marks_host(dict(c, p=hp))
        assert margin > 1e-6
        loss = ((image - target.to(F64)) ** 2).mean()
        loss.backward()
        host_loss.append(loss.item())
        host_p = host_p - lr * hp.grad * turn
    geom, p, cam, colors, kw = _device(c)
    tgt, dev_loss, turn = target.to(DEV).to(F64), [], turn.to(DEV)
    for _ in range(steps):
        dp = p.clone().requires_grad_(True)
        loss = ((render(geom, dp, cam, colors, **kw).to(F64) - tgt) ** 2).mean()
        loss.backward()
        dev_loss.append(loss.item())
        p = p - lr * dp.grad * turn
    rel = [abs(a - b) / b for a, b in zip(dev_loss, host_loss)]
    print("host losses", host_loss, "relative differences", rel, "angle", float(p[0, 0, 0]))
    assert host_loss[-1] < 0.7 * host_loss[0]                          # (it does descend)
    assert max(rel) <= 1e-6


def test_frame_recorder_records_the_marks_and_the_worlds_joints():
    from lcp_physics_amd.physics.render import FrameRecorder
    world, _, cam, colors, kw = _world(leaf=False)
    bg = torch.tensor([0.05, 0.1, 0.15], dtype=torch.float32, device=DEV)
    rec = FrameRecorder(world, cam, colors, capacity=2, background=bg, joints=True, marks_over=True, **kw)
    want = []
    for k in range(2):
        rec.record()
        want.append(torch.round(world.render(cam, colors, background=bg, joints=True, marks_over=True, **kw).clamp(0, 1) * 255).to(torch.uint8))
        world.step()
    frames = rec.frames()
    assert frames.shape == (2, 4, 3, 48, 80) and frames.dtype == torch.uint8 and frames.is_cuda
    assert torch.equal(frames, torch.stack(want)) and not torch.equal(frames[0], frames[1])
    bare = torch.round(world.render(cam, colors, background=bg, thickness=kw["thickness"]).clamp(0, 1) * 255).to(torch.uint8)
    assert not torch.equal(torch.stack(want)[1], bare)
