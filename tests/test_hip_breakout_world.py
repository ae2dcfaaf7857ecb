"""GPU: worlds from pixels (`lcp_physics_amd.physics.breakout`: extract_params -> make_world -> simulate_breakout) against the
three roll-outs of the unmodified reference in tests/golden/breakout.npz (tools/gen_breakout_golden.py: a bounce off a block, off
the paddle with a halved step, off a wall).  Five replicas of each roll-out run side by side in ONE batch of 15 scenes with
max_blocks = 8 (the frames hold 3, 5 and 4 blocks: every scene has absent slots).

Bounds, those tests/test_hip_fixed_dt.py holds the same machinery to at this pose scale: clocks to 1e-12, sub-step and contact
counts exactly, states within 2e-4 after every step, the gradient within 1e-4 relative."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import encoder_host as EH

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "breakout.npz")
REPLICAS, MAXB = 5, 8


@functools.lru_cache(None)
def _golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files if k.startswith("r_")}


def _rollout(differentiable):
    """The batch of 15 scenes stepped max(nsteps) times; returns the per-step records and, when differentiable, the speeds' grads."""
    from lcp_physics_amd.physics.breakout import extract_params, make_world, simulate_breakout, to_vector
    g = _golden()
    rep = lambda a: np.repeat(a, REPLICAS, axis=0)
    keys = rep(g["r_key"])
    frames = torch.from_numpy(EH.to_frame(keys, 3, np.random.default_rng(0))).to(DEV)
    params = extract_params(frames, max_blocks=MAXB)
    state0 = to_vector(params)
    bw = make_world(params, torch.from_numpy(rep(g["r_ball_vel"])).to(DEV))
    assert bw.world.nb == 7 + MAXB and bw.world.e == 3 * (5 + MAXB) and bw.world._pinned
    assert bw.present.sum(1).cpu().tolist() == rep(g["r_nblocks"]).tolist()
    pv = torch.from_numpy(rep(g["r_paddle_vel"])).to(DEV)
    vx, vy = pv[:, 0].clone().requires_grad_(differentiable), pv[:, 1].clone().requires_grad_(differentiable)
    actions = torch.from_numpy(rep(g["r_actions"])).to(DEV)
    nsteps = rep(g["r_nsteps"])
    steps, final = [], [None] * len(nsteps)
    for k in range(int(nsteps.max())):
        s = simulate_breakout(bw, actions[:, k], vx, vy, differentiable=differentiable)
        steps.append(dict(state=s.detach().cpu().numpy(), t=bw.world.t.cpu().numpy().copy(), nsub=bw.world.substeps.cpu().numpy().copy(),
                          nc=bw.world.contacts.count.cpu().numpy().copy()))
        for b in np.flatnonzero(nsteps == k + 1):
            final[b] = s[b]
    grad = None
    if differentiable:
        loss = sum((f[:4] ** 2).mean() for f in final)               # per scene: mean squared paddle (pos, dims) of its last step
        loss.backward()
        grad = torch.stack([vx.grad, vy.grad], dim=1).cpu().numpy()
        losses = np.array([float((f.detach()[:4] ** 2).mean()) for f in final])
        return state0.cpu().numpy(), steps, grad, losses
    return state0.cpu().numpy(), steps, None, None


def _compare(state0, steps):
    g = _golden()
    rep = lambda a: np.repeat(a, REPLICAS, axis=0)
    want, nsteps = rep(g["r_state"]), rep(g["r_nsteps"])
    assert np.array_equal(state0, want[:, 0]), "the state read off the frames"
    worst = 0.0
    for k, st in enumerate(steps):
        live = nsteps > k
        err = float(np.abs(st["state"][live] - want[live, k + 1]).max())
        worst = max(worst, err)
        assert np.abs(st["t"][live] - rep(g["r_t"])[live, k]).max() <= 1e-12, (k, st["t"])
        assert np.array_equal(st["nsub"][live], rep(g["r_nsub"])[live, k]), (k, st["nsub"].tolist())
        assert np.array_equal(st["nc"][live], rep(g["r_ncontacts"])[live, k]), (k, st["nc"].tolist())
        assert err <= 2e-4, (k, err)
    for b in range(0, len(nsteps), REPLICAS):                          # replicas of a scene are the same scene
        for st in steps:
            assert np.array_equal(st["state"][b:b + REPLICAS], np.repeat(st["state"][b:b + 1], REPLICAS, axis=0)), b
    return worst


def test_rollouts_match_the_reference_after_every_step():
    """Measured on an MI355X: worst |state - reference| 7.3e-07 over the 8 steps (bound 2e-4); clocks and counts exact."""
    state0, steps, _, _ = _rollout(False)
    worst = _compare(state0, steps)
    g = _golden()
    assert int(g["r_nsub"].max()) > 1                                  # (the halving is part of what is compared)
    print("breakout roll-outs: worst |state - reference| %.3e over %d steps (bound 2e-4)" % (worst, len(steps)))


def test_the_gradient_reaches_the_paddle_speeds():
    """d(mean squared state[:, :4] of the last step) / d(paddle_vel_x, paddle_vel_y) per scene against the reference's autograd,
    within 1e-4 relative to the larger component; the differentiable steps are held to the states' bounds too.
    Measured on an MI355X: worst relative gradient error 3.5e-08 (bound 1e-4), worst state error 7.3e-07, loss within 5.6e-10."""
    state0, steps, grad, losses = _rollout(True)
    worst = _compare(state0, steps)
    g = _golden()
    want, wl = np.repeat(g["r_grad"], REPLICAS, axis=0), np.repeat(g["r_loss"], REPLICAS)
    rel = np.abs(grad - want).max(axis=1) / np.abs(want).max(axis=1)
    print("breakout gradient: worst relative error %.3e (bound 1e-4), worst |state - reference| %.3e, loss error %.3e"
          % (float(rel.max()), worst, float(np.abs(losses - wl).max() / wl.max())))
    assert np.isfinite(grad).all() and float(rel.max()) <= 1e-4, (grad.tolist(), want.tolist())


def test_a_world_from_the_state_vector_is_the_world_from_the_params():
    """`make_world(to_vector(params))` - the form run_breakout.py:85-86 uses - finds the absent slots by their placeholder."""
    from lcp_physics_amd.physics.breakout import extract_params, make_world, to_vector
    g = _golden()
    frames = torch.from_numpy(EH.to_frame(g["r_key"], 3, np.random.default_rng(0))).to(DEV)
    params = extract_params(frames, max_blocks=MAXB)
    vel = torch.from_numpy(g["r_ball_vel"]).to(DEV)
    a, b = make_world(params, vel), make_world(to_vector(params), vel)
    assert a.present.sum(1).cpu().tolist() == g["r_nblocks"].tolist() and torch.equal(a.present, b.present)
    for x, y in ((a.world.p, b.world.p), (a.world.v, b.world.v), (a.dims, b.dims), (a.world.geom.no_contact, b.world.geom.no_contact),
                 (a.world.geom.verts_local, b.world.geom.verts_local), (a.world.contacts.count, b.world.contacts.count)):
        assert torch.equal(x, y)
    nc = a.world.geom.no_contact[0].bool()
    slot = a.blocks.start + int(g["r_nblocks"][0])                    # the first absent slot of scene 0: it collides with nothing
    assert bool(nc[slot].sum() == a.world.nb - 1) and not bool(nc[a.ball, a.paddle]) and not bool(nc[a.ball, a.blocks.start])
