"""CPU: tests/golden/fixed_dt.npz (the unmodified reference under `World.step(fixed_dt=True)`, physics/world.py:72-80;
tools/gen_fixed_dt_golden.py) is self-consistent, the CPU oracle chained by the same rule reproduces its sub-steps, and
`ContactWorld.step(fixed_dt=True)` has no route without a GPU."""
import os

import numpy as np
import pytest
import torch

from oracle import contacts_oracle as C
from oracle import ref_shim
from oracle import world_oracle as W
from tests.fixed_dt_io import GOLD, first_substep_of, load_fixed_dt
from tests.world_io import shapes_of

WORLDS, ROLLOUT = load_fixed_dt()


def test_fixture_is_small_and_complete():
    assert os.path.getsize(GOLD) <= os.path.getsize(os.path.join(os.path.dirname(GOLD), "shape_grad.npz"))
    assert len(WORLDS) == 10 and ROLLOUT["force0"].shape == (8, 3)
    # part (b): scenes that finish the same step at different sub-steps
    nsub = ROLLOUT["nsub"]
    assert nsub.shape == (8, int(ROLLOUT["nsteps"]))
    assert sorted(nsub.max(axis=1).tolist()) == [2, 3, 4, 4, 4, 5, 6, 7]
    assert any(len(set(nsub[:, k].tolist())) > 1 for k in range(nsub.shape[1]))
    assert np.abs(ROLLOUT["t"] - float(ROLLOUT["dt"]) * np.arange(1, nsub.shape[1] + 1)).max() < 1e-12


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_fixture_substeps_are_consistent(name):
    """world.py:75-78 restated on the recorded clocks: end_t = t + dt, every sub-step asks for exactly end_t - t (fp64), the clock
    only moves forward, the last sub-step of a step reaches end_t, and the dts the sub-steps used sum to the step."""
    rec = WORLDS[name]
    dt, first = float(rec["dt"]), first_substep_of(rec)
    assert first[-1] == len(rec["sub_dt"]) == len(rec["sub_t"]) == len(rec["sub_step"]) == len(rec["sub_f"])
    assert int(rec["nsub"].max()) > 1 and int(rec["nsub"].min()) >= 1
    for k in range(len(rec["nsub"])):
        t = float(rec["t"][k])
        end_t = t + dt
        for s in range(first[k], first[k + 1]):
            assert int(rec["sub_step"][s]) == k
            assert t < end_t and float(rec["sub_dt"][s]) == end_t - t, (name, k, s)
            assert t < float(rec["sub_t"][s]) <= t + float(rec["sub_dt"][s])
            t = float(rec["sub_t"][s])
        assert not t < end_t and t == float(rec["t"][k + 1]), (name, k)
        assert abs((float(rec["t"][k + 1]) - float(rec["t"][k])) - dt) < 1e-12
        assert float(rec["sub_dt"][first[k]:first[k + 1]].min()) >= 1e-3
    assert np.abs(rec["t"] - dt * np.arange(len(rec["t"]))).max() < 1e-12          # every scene is on the frame grid
    # f(t): `f` until the clock reaches t_switch, `f_off` from then on (forces.py:14-18)
    t_start = np.concatenate([[rec["t"][0]], rec["sub_t"][:-1]])
    for s in range(first[-1]):
        assert np.array_equal(rec["sub_f"][s], rec["f"] if t_start[s] < float(rec["t_switch"]) else rec["f_off"])


def _oracle_step_dt(rec, shapes, p, v, contacts, f, dt_k, joints, nocon):
    """`world_oracle.step_dt(dt_k)`.  It takes the non-strict floor as dt_k / 4, the reference as `self.dt / 4` (world.py:98: the WORLD's
    dt, also inside a sub-step), so for the non-strict record the same pieces are chained here with that floor."""
    kw = dict(eps=float(rec["eps"]), tol=float(rec["tol"]), no_contact=nocon)
    if bool(rec["strict"]):
        return W.step_dt(shapes, p, v, contacts, rec["Mdiag"], f, rec["rest"], rec["fric"], rec["Je"], dt_k, strict=True,
                         post_stab=bool(rec["post_stab"]), joints=joints, **kw)
    assert joints is None and not bool(rec["post_stab"])
    new_v = W.solve_dynamics(rec["Mdiag"], v, f, dt_k, contacts, rec["rest"], rec["fric"], rec["Je"])
    p_new, cs, dt_used, trials = W.move_and_find(shapes, p, new_v, dt_k, strict=False, dt_floor=float(rec["dt"]) / 4, **kw)
    return p_new, new_v, cs, dt_used, trials


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_world_oracle_chained_by_the_fixed_dt_rule_reproduces_the_substeps(name):
    """`while t < end_t: step_dt(end_t - t)` over oracle/world_oracle.py: the sub-step count of every step, every dt asked and every
    clock of the reference (to 1e-12, as tests/test_world_oracle.py holds the plain mode), contact counts, poses and velocities."""
    rec = WORLDS[name]
    shapes = shapes_of(rec)
    dt = float(rec["dt"])
    p, v, t = rec["p"][0].copy(), rec["v"][0].copy(), 0.0
    nocon = [tuple(x) for x in rec["no_contact"].tolist()]
    joints = {k: rec[k] for k in ("jtype", "jb1", "jb2", "jr1", "jrot1")} if any(int(x) in (1, 2) for x in rec["jtype"]) else None
    contacts = C.find_contacts(W.bodies_at(shapes, p), eps=float(rec["eps"]), no_contact=nocon)
    assert len(contacts) == int(rec["ncontacts"][0])
    p_atol = 2e-5 if bool(rec["post_stab"]) else 1e-6                    # (tests/test_world_oracle.py: the degenerate post-stabilisation LCP)
    s = 0
    for k in range(len(rec["nsub"])):
        end_t, n = t + dt, 0
        while t < end_t:
            dt_k = end_t - t
            assert n < 64, (name, k, "the chained oracle does not terminate")
            assert abs(dt_k - float(rec["sub_dt"][s])) < 1e-12, (name, k, n, "dt asked")
            f = rec["f"] if t < float(rec["t_switch"]) else rec["f_off"]
            out = _oracle_step_dt(rec, shapes, p, v, contacts, f, dt_k, joints, nocon)
            p, v, contacts, dt_used = out[:4]
            if joints is not None:
                joints = out[5]
            t += dt_used
            assert abs(t - float(rec["sub_t"][s])) < 1e-12, (name, k, n, "t")
            s += 1
            n += 1
        assert n == int(rec["nsub"][k]), (name, k, "sub-steps", n, int(rec["nsub"][k]))
        assert abs(t - float(rec["t"][k + 1])) < 1e-12
        assert len(contacts) == int(rec["ncontacts"][k + 1]), (name, k, "contact count")
        assert np.allclose(v, rec["v"][k + 1], atol=1e-6, rtol=1e-7), (name, k, "v", np.abs(v - rec["v"][k + 1]).max())
        assert np.allclose(p, rec["p"][k + 1], atol=p_atol, rtol=1e-9), (name, k, "p", np.abs(p - rec["p"][k + 1]).max())


@pytest.mark.skipif(not ref_shim.reference_available(), reason="needs the reference tree")
def test_one_scene_replayed_live_on_the_reference():
    """The generator's own recording of one scene, run again on the reference tree: counts, clocks and poses as committed."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_fixed_dt_golden.py")
    spec = importlib.util.spec_from_file_location("gen_fixed_dt_golden", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ref_shim.load_reference()
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        live = gen.record_world("stack3", gen.GW._scenes()["stack3"])
    finally:
        torch.set_default_dtype(old)
    rec = WORLDS["stack3"]
    for k in ("nsub", "ncontacts", "t", "sub_dt", "sub_t", "p", "v"):
        assert np.array_equal(live[k], rec[k]), k


def test_fixed_dt_has_no_route_without_a_gpu():
    """No fallback: the sub-step wrappers refuse CPU tensors, and so does `ContactWorld.step(fixed_dt=True)` before any work."""
    from lcp_physics_amd.physics import batched_world as bw
    from lcp_physics_amd.physics.contacts import GeometryBatch, move_and_find_contacts
    B, nb = 2, 3
    t = torch.zeros(B, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU"):
        bw.substep_begin(t, t + 1.0 / 30, torch.zeros(B, nb, 3), torch.zeros(B, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU"):
        bw.substep_commit(torch.ones(B, dtype=torch.int32), torch.zeros(B, nb, 3), torch.zeros(B, nb, 3))
    geom = GeometryBatch.from_shapes([("circle", 1.0)] * nb, B)
    with pytest.raises(RuntimeError, match="GPU"):
        move_and_find_contacts(geom, torch.zeros(B, nb, 3, dtype=torch.float64), torch.zeros(B, nb, 3), 1.0 / 30, dt_scene=t)
    world = object.__new__(bw.ContactWorld)                              # (a world cannot be BUILT on the CPU either: its first detection raises)
    world.t, world.dt = t, 1.0 / 30
    for kw in ({}, {"max_substeps": 4}, {"differentiable": True}):
        with pytest.raises(RuntimeError, match="GPU"):
            world.step(fixed_dt=True, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        bw.ContactWorld(geom, torch.zeros(B, nb, 3, dtype=torch.float64), torch.zeros(B, nb, 3), torch.ones(B, nb, 3), torch.zeros(B, nb, 3),
                        torch.zeros(B, nb), torch.zeros(B, nb))
