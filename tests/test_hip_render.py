"""GPU: the drawing on the device (lcp_render.hip: `lcp_render_f64`, `lcp_render_backward_f64`, through
`lcp_physics_amd.physics.render`) against its float64 restatement on the CPU (tests/render_host.py).

Every parity test first asserts the decision margin of its inputs (> 1e-6, see render_host.py) and then compares EVERY pixel:
  image   |device - host| <= 1e-6 for colours in [0, 1]: the fp32 store rounds by at most 6e-8, fp64 reordering gives ~1e-12 / w
  ids     identical
  grads   each tensor within 1e-9 max|g| of autograd's for a random fp32 cotangent (fp64 sums over at most ~1e4 terms; the fp32
          colour gradient is compared with autograd's fp32 gradient of the fp32 colours), and bit-identical across two runs."""
import numpy as np
import pytest
import torch

from tests import render_host as RH

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64


def _device(c, leaves=False):
    """(geom, p, cam, colors, kwargs of render) of a case on the device."""
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.render import Camera
    t = lambda k: c[k].to(DEV).contiguous()
    geom = GeometryBatch(t("kind"), t("radius"), t("verts_local"), t("nverts"), None, None)
    p, colors = t("p"), t("colors")
    if leaves:
        geom.radius.requires_grad_(True)
        geom.verts_local.requires_grad_(True)
        p.requires_grad_(True)
        colors.requires_grad_(True)
    cam = Camera(c["H"], c["W"], origin=(c["x0"], c["y0"]), pixels_per_meter=c["ppm"])
    return geom, p, cam, colors, dict(background=t("background"), thickness=t("thickness"), edge_width=c["w"])


@pytest.mark.parametrize("name", RH.CASE_NAMES)
def test_image_and_mask_match_the_restatement(name):
    from lcp_physics_amd.physics.render import render, render_ids
    c, ref = RH.case(name), RH.reference(name)
    assert ref["margin"] > 1e-6, ref["margin"]
    geom, p, cam, colors, kw = _device(c)
    ids = torch.full((3, c["H"], c["W"]), -7, dtype=torch.int32, device=DEV)
    image = render(geom, p, cam, colors, ids_out=ids, **kw)
    only_ids = render_ids(geom, p, cam)
    assert image.dtype == torch.float32 and image.shape == ref["image"].shape
    err = float((image.cpu().to(F64) - ref["image"]).abs().max())
    wrong = int((ids.cpu() != ref["ids"]).sum())
    print(name, "margin %.3g" % ref["margin"], "image error %.3g" % err, "mask pixels that differ", wrong)
    assert err <= 1e-6
    assert wrong == 0 and torch.equal(only_ids.cpu(), ref["ids"])
    if not c["per_scene_colors"]:                                     # [nb,C] colours are the [B,nb,C] ones expanded
        shared = render(geom, p, cam, colors[0], **kw)
        assert torch.equal(shared, image)


@pytest.mark.parametrize("name", RH.CASE_NAMES)
def test_gradients_match_autograd_of_the_restatement_and_repeat_bitwise(name):
    from lcp_physics_amd.physics.render import render
    c, ref = RH.case(name), RH.reference(name)
    assert ref["margin"] > 1e-6, ref["margin"]
    g = ref["g_image"].to(DEV)
    runs = []
    for _ in range(2):
        geom, p, cam, colors, kw = _device(c, leaves=True)
        render(geom, p, cam, colors, **kw).backward(g)
        runs.append(dict(p=p.grad, radius=geom.radius.grad, verts_local=geom.verts_local.grad, colors=colors.grad))
    torch.cuda.synchronize()
    bad = []
    for n, want in ref["grads"].items():
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
    hull = c["kind"] != 0
    pad = torch.arange(c["verts_local"].shape[2]).reshape(1, 1, -1) >= (c["nverts"] * hull).unsqueeze(-1)
    assert float(runs[0]["verts_local"].cpu()[pad].abs().max()) == 0.0 and float(runs[0]["radius"].cpu()[hull].abs().max() if hull.any() else 0.0) == 0.0


def test_only_the_gradients_that_are_needed_are_computed_and_shared_colours_sum_over_the_scenes():
    from lcp_physics_amd.physics.render import render
    c, ref = RH.case("three"), RH.reference("three")
    g = ref["g_image"].to(DEV)
    geom, p, cam, colors, kw = _device(c)
    assert not render(geom, p, cam, colors, **kw).requires_grad
    p.requires_grad_(True)
    render(geom, p, cam, colors, **kw).backward(g)
    assert geom.radius.grad is None and geom.verts_local.grad is None and colors.grad is None
    want = ref["grads"]["p"]
    assert float((p.grad.cpu() - want).abs().max()) <= 1e-9 * float(want.abs().max())
    shared = colors[0].clone().requires_grad_(True)
    render(geom, p.detach(), cam, shared, **kw).backward(g)
    # fp32 sum of the three scenes' fp32 gradients: two roundings of 6e-8 relative to the largest partial sum
    want = ref["grads"]["colors"].to(F64).sum(0)
    assert float((shared.grad.cpu().to(F64) - want).abs().max()) <= 4 * 6e-8 * float(ref["grads"]["colors"].abs().max()) * 3


def test_render_into_out_replays_bitwise_from_a_graph():
    from lcp_physics_amd.physics.render import render
    c = RH.case("special")
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
        p[:, 1:, 1] += shift                                          # the graph reads the pose through the same pointer
        out.fill_(-1.0)
        ids.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
        again = render(geom, p, cam, colors, **kw)
        assert torch.equal(out, again) and (shift == 0.0) == torch.equal(out, eager)
    _, host_ids, margin = RH.render_host(dict(c, p=p.cpu()))
    assert margin > 1e-6 and torch.equal(ids.cpu(), host_ids)


def _world(p0_leaf=False, B=4):
    """The ball / box / floor scene of the bodies fixture (tests/test_hip_bodies.py) as a ContactWorld, and a camera on the ball."""
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.render import Camera
    from tests.test_hip_bodies import _rollout_bodies, _rollout_fixture
    d = _rollout_fixture()
    t64 = lambda a: torch.tensor(a, dtype=F64)
    bb = _rollout_bodies(d, B, t64(float(d["ball_rad"])), t64(d["box_verts_raw"]), t64(float(d["mass"][0])), t64(float(d["mass"][1])))
    p0 = bb.p0.detach().clone().requires_grad_(p0_leaf)
    f = bb.f_gravity.clone()
    f[:, 0] = 0.0                                                     # the floor is held by Je and carries no gravity
    Je = torch.tensor(np.repeat(d["Je"][:1], B, axis=0), dtype=torch.float32, device=DEV)
    world = ContactWorld(bb.geom, p0, bb.v0, bb.Mdiag, f, bb.rest, bb.fric, Je=Je, dt=float(d["dt"]), maxc=8)
    ball = d["ball_pos"].reshape(-1)[-2:]
    ppm = 0.5
    cam = Camera(48, 80, origin=(float(ball[0]) - 40.3 / ppm, float(ball[1]) - 24.7 / ppm), pixels_per_meter=ppm)
    colors = torch.tensor([[0.2, 0.3, 0.4], [0.9, 0.1, 0.2], [0.1, 0.8, 0.3]], dtype=torch.float32, device=DEV)
    return world, p0, cam, colors


def test_world_render_is_render_of_the_worlds_state_and_a_pixel_loss_reaches_p0():
    from lcp_physics_amd.physics.render import render, render_ids
    world, p0, cam, colors = _world(p0_leaf=True)
    assert torch.equal(world.render(cam, colors), render(world.geom, world.p, cam, colors))
    seen = set(render_ids(world.geom, world.p, cam).unique().cpu().tolist())
    assert {1} <= seen, seen                                          # the ball is in the picture
    for _ in range(3):
        world.step(differentiable=True)
    image = world.render(cam, colors)
    assert image.requires_grad and torch.equal(image.detach(), render(world.geom, world.p.detach(), cam, colors))
    weight = torch.randn(image.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    (image * weight).sum().backward()
    g = p0.grad.cpu()
    print("d loss / d p0", g[0].tolist())
    assert bool(torch.isfinite(g).all()) and float(g[:, 1, 1:].abs().min()) > 0.0          # every scene's ball moves the pixels


def test_descent_on_a_pixel_loss_follows_the_restatements_descent():
    """Ten fixed steps of gradient descent moving a circle towards a target image, on the device and on the restatement: the losses
    agree within 1e-6 relative at every iteration (the device image is fp32: 6e-8 per
    pixel of the ramp, against differences of order 1; the descent is stopped well before it converges)."""
    from lcp_physics_amd.physics.render import render
    cam_t = (19, 23, -3.3, 2.1, 0.75, 1.7)
    white = dict(colors=torch.ones(1, 1, 1, dtype=torch.float32), background=torch.zeros(1, dtype=torch.float32))
    mk = lambda x, y: dict(RH._assemble([[("circle", (0.0, x, y), 4.5, 0.0)]], cam_t, 1, 11, False, 8), **white)
    target = RH.render_host(mk(14.1, 15.3))[0].to(torch.float32)
    lr, steps = 24.0, 10
    c = mk(9.37, 11.21)
    host_p, host_loss = c["p"].clone(), []
    for _ in range(steps):
        hp = host_p.clone().requires_grad_(True)
        loss = ((RH.render_host(dict(c, p=hp))[0] - target.to(F64)) ** 2).mean()
        loss.backward()
        host_loss.append(loss.item())
        host_p = host_p - lr * hp.grad
    geom, p, cam, colors, kw = _device(c)
    tgt, dev_loss = target.to(DEV).to(F64), []
    for _ in range(steps):
        dp = p.clone().requires_grad_(True)
        loss = ((render(geom, dp, cam, colors, **kw).to(F64) - tgt) ** 2).mean()
        loss.backward()
        dev_loss.append(loss.item())
        p = p - lr * dp.grad
    rel = [abs(a - b) / b for a, b in zip(dev_loss, host_loss)]
    print("host losses", host_loss, "relative differences", rel)
    assert host_loss[-1] < 0.7 * host_loss[0]                          # (it does descend)
    assert max(rel) <= 1e-6


def test_frame_recorder_keeps_uint8_frames_on_the_device_and_saves_png(tmp_path):
    from PIL import Image

    from lcp_physics_amd.physics.render import FrameRecorder
    world, _, cam, colors = _world()
    bg = torch.tensor([0.05, 0.1, 0.15], dtype=torch.float32, device=DEV)
    rec = FrameRecorder(world, cam, colors, capacity=3, background=bg)
    want = []
    for k in range(3):
        rec.record()
        want.append(torch.round(world.render(cam, colors, background=bg).clamp(0, 1) * 255).to(torch.uint8))
        world.step()
    frames = rec.frames()
    assert frames.shape == (3, 4, 3, 48, 80) and frames.dtype == torch.uint8 and frames.is_cuda
    assert torch.equal(frames, torch.stack(want)) and not torch.equal(frames[0], frames[2])
    with pytest.raises(RuntimeError):
        rec.record()                                                  # full
    paths = rec.save(str(tmp_path / "frames"), scene=2)
    assert len(paths) == 3
    for k, path in enumerate(paths):
        back = torch.tensor(np.array(Image.open(path))).permute(2, 0, 1)
        assert torch.equal(back, frames[k, 2].cpu())
