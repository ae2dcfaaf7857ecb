"""GPU: the contact report of lcp_report.hip (lcp_contact_report_f32; physics/contact_report.py; `ContactWorld(report=...)`) against the
host mirror tests/contact_report_host.py, which tests/test_contact_report_host.py checks on the CPU against the oracle's G and A.

(a) the raw entry on the named cases: floats within 2^-24 |ref| + 1e-12 S per entry (one float32 rounding plus the float64 sum: the
force elements' bound), integers exact.  (b) the identity M (v_new - v) - dt f = body_impulse + joint_impulse on worlds after one
step, within 4 * 2^-24 S per coordinate.  (c) the world's plumbing: plain, captured, recorded and fixed-interval steps."""
import pytest
import torch

from tests import contact_report_host as RH

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32, I32 = torch.float64, torch.float32, torch.int32
DT = 1.0 / 30
NAN = float("nan")


def _lib():
    from lcp_physics_amd import _lib as L
    return L


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(I32), b.contiguous().view(I32))


def _shapes(c):
    B, nb, _, _, P = RH.dims(c)
    return {"body_impulse": (B, nb, 3), "body_normal": (B, nb), "body_touching": (B, nb), "joint_impulse": (B, nb, 3),
            "pair_impulse": (B, P, 3), "pair_normal": (B, P), "pair_contacts": (B, P)}


def _call(c, min_impulse=0.0, absent=()):
    """The raw entry into outputs pre-filled with NaN / -1: the outputs (CPU) that were not `absent` (NULL)."""
    L = _lib()
    B, nb, maxc, e, P = RH.dims(c)
    dev = lambda t: None if t is None else t.to(DEV).contiguous()
    d = {k: dev(c[k]) for k in ("count", "active", "c_n", "c_p1", "c_p2", "c_i1", "c_i2", "z", "y", "Je", "first", "second")}
    outs = {}
    for n, sh in _shapes(c).items():
        if n not in absent:
            outs[n] = torch.full(sh, -1, dtype=I32, device=DEV) if n in RH.INTS else torch.full(sh, NAN, dtype=F32, device=DEV)
    ptr = lambda t: L.ptr(t) if t is not None and t.numel() else None
    rc = L.load().lcp_contact_report_f32(B, nb, maxc, e, P, *[ptr(d[k]) for k in ("count", "active", "c_n", "c_p1", "c_p2", "c_i1", "c_i2", "z")],
                                         ptr(d["y"]) if e else None, ptr(d["Je"]) if e else None, ptr(d["first"]), ptr(d["second"]),
                                         float(min_impulse), *[ptr(outs.get(n)) for n in RH.OUTPUTS], L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    return {n: t.cpu() for n, t in outs.items()}


def _against(got, ref, what):
    """Bound (a) on every output present in `got`; prints the largest ratio of error to bound."""
    ok, line = True, []
    for n in RH.OUTPUTS:
        if n not in got:
            continue
        if n in RH.INTS:
            same = torch.equal(got[n], ref[n])
            line.append("%s %s" % (n, "exact" if same else "DIFFERS"))
            ok = ok and same
        else:
            assert bool(torch.isfinite(got[n]).all()), (what, n, "not written everywhere")
            good, worst = RH.within_bound(got[n], ref, n)
            line.append("%s %.3f" % (n, worst))
            ok = ok and good
    print("%s: |got - ref| / (2^-24 |ref| + 1e-12 S):  %s" % (what, "   ".join(line)))
    return ok


# ------------------------------------------------------------------------------------------------------------- (a) the raw entry
@pytest.mark.parametrize("name", RH.CASE_NAMES)
def test_every_case_matches_the_mirror_at_both_thresholds(name):
    c = RH.case(name)
    assert _against(_call(c), RH.reference(name), name)
    thr = RH.some_zn(name)
    ref = RH.report_host(c, thr)
    assert int(ref["body_touching"].sum()) < int(RH.reference(name)["body_touching"].sum())
    assert _against(_call(c, thr), ref, "%s, min_impulse = %.6g" % (name, thr))


@pytest.mark.parametrize("name", ["small", "edge65", "ragged", "full"])
def test_each_optional_output_null_in_turn_gives_the_same_bits_elsewhere(name):
    c = RH.case(name)
    full, again = _call(c), _call(c)
    for n in RH.OUTPUTS:
        assert _bits(full[n], again[n]), n
    for gone in RH.OUTPUTS:
        part = _call(c, absent=(gone,))
        assert gone not in part
        for n in part:
            assert _bits(full[n], part[n]), (n, "without", gone)
    only = _call(c, absent=tuple(n for n in RH.OUTPUTS if n != "joint_impulse"))
    assert _bits(only["joint_impulse"], full["joint_impulse"])


def test_the_host_wrapper_returns_the_entrys_bits():
    from lcp_physics_amd.physics.contact_report import ContactReport, contact_report
    from lcp_physics_amd.physics.contacts import ContactBuffers
    from lcp_physics_amd.physics.proximity import PairSet
    for name in ("ragged", "nopairs", "nojoints"):
        c = RH.case(name)
        B, nb, maxc, e, P = RH.dims(c)
        frame = ContactBuffers(B, nb, maxc, torch.device(DEV))
        for k in ("c_n", "c_p1", "c_p2", "c_i1", "c_i2"):
            getattr(frame, k).copy_(c[k])
        dev = lambda t: None if t is None else t.to(DEV)
        pairs = PairSet(c["first"], c["second"], torch.ones(B, P, dtype=F64)).to(DEV) if P else None
        raw = _call(c, 0.25)
        rep = contact_report(frame, dev(c["z"]), count=dev(c["count"]), y=dev(c["y"]), Je=dev(c["Je"]), pairs=pairs, min_impulse=0.25,
                             active=dev(c["active"]))
        assert isinstance(rep, ContactReport) and rep.P == P
        for n in RH.OUTPUTS:
            assert _bits(getattr(rep, n).cpu(), raw[n]), (name, n)
        assert contact_report(frame, dev(c["z"]), count=dev(c["count"]), y=dev(c["y"]), Je=dev(c["Je"]), pairs=pairs, min_impulse=0.25,
                              active=dev(c["active"]), out=rep) is rep
        assert rep.to("cpu").body_impulse.device.type == "cpu"
        with pytest.raises(RuntimeError):
            contact_report(frame, c["z"])                                                  # a CPU tensor: no fallback


# ------------------------------------------------------------------------------------------------------------- worlds
B = 8


def _drop_world(nbox, maxc, B_=B, lift=None, **kw):
    """A pinned floor and `nbox` boxes resting on each other inside the detection margin.  `lift` = (gap, speed): the top box starts
    `gap` higher and falls at `speed`, so that the penetration test halves the step."""
    from lcp_physics_amd import scenes
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.contacts import GeometryBatch
    w = scenes.make_drop_world(B_, nbox=nbox, gap=(0.01, 0.02))
    if lift is not None:
        w["p"][:, nbox, 2] -= lift[0]
        w["v"][:, nbox, 2] = lift[1]
    w = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in w.items()}
    return ContactWorld(GeometryBatch.from_shapes(w["shapes"], B_).to(DEV), w["p"], w["v"], w["Mdiag"], w["f"], w["rest"], w["fric"],
                        Je=w["Je"], dt=DT, maxc=maxc, compute="f64", **kw)


def _joint_world(kind, **kw):
    """"chain": a pinned floor and two boxes side by side on it, hinged to each other, one of them pushed sideways.  "falling": two
    links hinged to the world and to each other, swinging under gravity, no contact."""
    from lcp_physics_amd import scenes
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.joints import JointSet
    if kind == "chain":
        shapes = [("rect", scenes.FLOOR_DIMS), ("rect", (40.0, 40.0)), ("rect", (40.0, 40.0))]
        y = 500.0 - scenes.FLOOR_DIMS[1] / 2 - 0.02 - 20.0
        p0 = torch.tensor([[0.0, 500.0, 500.0], [0.0, 470.0, y], [0.0, 530.0, y]], dtype=F64)
        joints = [("total", 0), ("joint", 1, 2, (500.0, y))]
        dims = torch.tensor([scenes.FLOOR_DIMS, (40.0, 40.0), (40.0, 40.0)], dtype=F64)
        v0 = torch.tensor([[0.0, 0.0, 0.0], [0.0, 6.0, 0.0], [0.0, 0.0, 0.0]], dtype=F32)
        grav = torch.tensor([0.0, 1.0, 1.0], dtype=F64)
        nocon = None
    else:
        shapes = [("rect", (20.0, 60.0)), ("rect", (20.0, 60.0))]
        p0 = torch.tensor([[0.0, 300.0, 50.0], [0.0, 300.0, 100.0]], dtype=F64)
        joints = [("joint", 0, None, (300.0, 30.0)), ("joint", 1, 0, (300.0, 75.0))]
        dims = torch.tensor([(20.0, 60.0), (20.0, 60.0)], dtype=F64)
        v0 = torch.tensor([[0.5, 8.0, 0.0], [-0.3, 0.0, 4.0]], dtype=F32)
        grav = torch.tensor([1.0, 1.0], dtype=F64)
        nocon = torch.ones(B, 2, 2, dtype=torch.uint8) - torch.eye(2, dtype=torch.uint8)
    nb = len(shapes)
    mass = 0.5 + torch.arange(B * nb, dtype=F64).reshape(B, nb) / (B * nb)                 # (the scenes differ)
    Mdiag = scenes._rect_mdiag(mass, dims[:, 0].unsqueeze(0), dims[:, 1].unsqueeze(0))
    f = torch.zeros(B, nb, 3, dtype=F64)
    f[:, :, 2] = mass * grav * scenes.GRAVITY
    geom = GeometryBatch.from_shapes(shapes, B)
    if nocon is not None:
        geom.no_contact = nocon
    js = JointSet.from_list(joints, p0, B=B).to(DEV)
    rep = lambda t: t.unsqueeze(0).repeat(B, 1, 1).to(DEV)
    half = torch.full((B, nb), 0.5, dtype=F32, device=DEV)
    return ContactWorld(geom.to(DEV), rep(p0), rep(v0), Mdiag.to(DEV), f.to(DEV), half, half, joints=js, dt=DT, maxc=8, compute="f64", **kw)


def _before(world):
    """What the next solve will consume, as CPU copies: the records, their counts, the joint Jacobian, the velocities, the forces."""
    cb = world.contacts
    s = {k: getattr(cb, k).detach().cpu().clone() for k in ("c_n", "c_p1", "c_p2", "c_i1", "c_i2", "count")}
    s["Je"] = None if world.Je is None else world.Je.detach().cpu().clone()
    s["v"], s["f"] = world.v.detach().cpu().clone(), world._forces().detach().cpu().clone()
    return s


def _mirror_case(world, s, out, pairs=None, count=None, active=None):
    y = out.get("y")
    return {"nb": world.nb, "c_n": s["c_n"], "c_p1": s["c_p1"], "c_p2": s["c_p2"], "c_i1": s["c_i1"], "c_i2": s["c_i2"],
            "z": out["z"].detach().cpu(), "count": s["count"] if count is None else count, "active": active,
            "y": None if y is None else y.detach().cpu(), "Je": s["Je"], "first": None if pairs is None else pairs.first.cpu(),
            "second": None if pairs is None else pairs.second.cpu()}


def _report_cpu(world):
    return {n: getattr(world.report, n).detach().cpu().clone() for n in RH.OUTPUTS}


IDENTITY_WORLDS = {"four boxes on a pinned floor": lambda: _drop_world(4, 16, report=True),
                   "12 bodies, more than 16 contacts": lambda: _drop_world(11, 32, report=True),
                   "a hinged chain resting on a floor": lambda: _joint_world("chain", report=True),
                   "falling hinged links, no contact": lambda: _joint_world("falling", report=True)}


@pytest.mark.parametrize("name", sorted(IDENTITY_WORLDS))
def test_the_identity_on_worlds_after_one_step(name):
    """|Mdiag (v_new - v) - dt f - body_impulse - joint_impulse| <= 4 * 2^-24 S per coordinate, S the sum of the magnitudes of every
    term: u is formed in fp32 by the kernels (two roundings), v_new, z and y are rounded once at their stores, the report once - each at
    most 2^-24 of a term of S - and the fp64 solve's own residual is below one of them
    (tests/test_contact_report_host.py::test_the_identity_holds_on_the_oracles_fp64_solves).  The terms of S are those of G^T z row by
    row: the two friction multipliers of a record are rounded separately and count separately (with their difference in S instead, a
    resting stack's x coordinates, whose S is then of order 1e-2, sit at 400 times 2^-24 S from those roundings alone).
    Measured on an MI355X, largest |residual| / (2^-24 S): four boxes 0.84, 12 bodies with 22 contacts 0.68, the hinged pair on a floor
    0.97, falling hinged links 0.61."""
    world = IDENTITY_WORLDS[name]()
    s = _before(world)
    out = world.step()
    torch.cuda.synchronize()
    ref = RH.report_host(_mirror_case(world, s, out))
    rep = _report_cpu(world)
    M, v, v_new, f = world.Mdiag.cpu().double(), s["v"].double(), world.v.cpu().double(), s["f"].double()
    res = M * v_new - M * v - DT * f - rep["body_impulse"].double() - rep["joint_impulse"].double()
    S = (M * v_new).abs() + (M * v).abs() + (DT * f).abs() + ref["S_body_impulse"] + ref["S_joint_impulse"]
    ratio = float((res.abs() / (2.0 ** -24 * S).clamp(min=1e-300)).max())
    print("%s: contacts %s, largest |residual| / (2^-24 S) = %.3f (bound 4), largest |contact| %.3g, |joint| %.3g, iters %s"
          % (name, s["count"].tolist(), ratio, float(rep["body_impulse"].abs().max()), float(rep["joint_impulse"].abs().max()),
             out["iters"].cpu().tolist()))
    if "no contact" in name:
        assert int(s["count"].sum()) == 0 and float(rep["body_impulse"].abs().max()) == 0.0
    else:
        assert int(s["count"].min()) > (16 if "12 bodies" in name else 0) and float(rep["body_impulse"].abs().max()) > 0.0
    if "hinged" in name:
        assert float(rep["joint_impulse"].abs().max()) > 0.0
    assert _against(rep, ref, name)                                                        # and the report is the mirror's
    assert bool((res.abs() <= 4.0 * 2.0 ** -24 * S).all()), ratio


# ------------------------------------------------------------------------------------------------------------- (c) plumbing
def _pairs(nb):
    from lcp_physics_amd.physics.proximity import PairSet
    return PairSet.all_pairs(nb, B).to(DEV)


def test_plain_and_recorded_steps_fill_the_report():
    for differentiable in (False, True):
        world = _drop_world(4, 16, report=_pairs(5), report_min_impulse=0.5)
        for k in range(2):
            s = _before(world)
            out = world.step(differentiable=differentiable)
        torch.cuda.synchronize()
        ref = RH.report_host(_mirror_case(world, s, out, pairs=world._report_pairs), 0.5)
        rep = _report_cpu(world)
        assert int(rep["pair_contacts"].sum()) > 0 and int(rep["body_touching"].sum()) > 0
        assert not any(getattr(world.report, n).requires_grad for n in RH.OUTPUTS)
        assert _against(rep, ref, "step(differentiable=%s)" % differentiable)


def test_a_captured_run_equals_the_eager_steps_bit_for_bit():
    """run(3, graph=True) (two warm-up steps and one eager: nothing is replayed yet) and run(6, graph=True) (two captured steps,
    replayed twice) against the same number of eager steps; the eager world's last report against the mirror."""
    for n in (3, 6):
        wg, we = _drop_world(4, 16, report=_pairs(5)), _drop_world(4, 16, report=_pairs(5))
        wg.run(n, graph=True)
        for k in range(n):
            s = _before(we)
            out = we.step()
        torch.cuda.synchronize()
        assert len(wg._graphs) == (1 if n == 6 else 0)
        rg, re_ = _report_cpu(wg), _report_cpu(we)
        for name in RH.OUTPUTS:
            assert _bits(rg[name], re_[name]), (n, name)
        assert _bits(wg.p.cpu(), we.p.cpu()) and _bits(wg.v.cpu(), we.v.cpu())
        assert float(re_["body_impulse"].abs().max()) > 0.0
        assert _against(re_, RH.report_host(_mirror_case(we, s, out, pairs=we._report_pairs)), "after %d steps" % n)


def test_a_fixed_interval_step_sums_its_sub_steps(monkeypatch):
    """A scene whose top box falls into the stack, so that the penetration test halves the step: every sub-step's launch is recorded
    (its own frame, z, y, Je, counts and active scenes) and mirrored; the impulses are the sum, the counts the largest.  The bound is
    (a) for every sub-step's launch, summed, plus one float32 rounding of the running sum per in-place addition."""
    from lcp_physics_amd.physics import contact_report as CR
    calls = []
    real = CR.contact_report

    def spy(frame, z, count=None, y=None, Je=None, pairs=None, min_impulse=0.0, active=None, out=None):
        cp = lambda t: None if t is None else t.detach().cpu().clone()
        calls.append({"c_n": cp(frame.c_n), "c_p1": cp(frame.c_p1), "c_p2": cp(frame.c_p2), "c_i1": cp(frame.c_i1), "c_i2": cp(frame.c_i2),
                      "z": cp(z), "count": cp(count), "active": cp(active), "y": cp(y), "Je": cp(Je), "first": cp(pairs.first),
                      "second": cp(pairs.second), "min_impulse": min_impulse})
        return real(frame, z, count=count, y=y, Je=Je, pairs=pairs, min_impulse=min_impulse, active=active, out=out)

    monkeypatch.setattr(CR, "contact_report", spy)
    world = _drop_world(3, 16, lift=(3.0, 200.0), report=_pairs(4), report_min_impulse=0.25)
    world.step(fixed_dt=True)
    torch.cuda.synchronize()
    nsub = world.substeps.cpu()
    assert int(nsub.max()) > 1 and len(calls) == int(nsub.max()), nsub.tolist()
    assert any(int((c["active"] == 0).sum()) > 0 for c in calls) or int(nsub.min()) == int(nsub.max())
    refs = [RH.report_host(dict(c, nb=world.nb), c["min_impulse"]) for c in calls]
    rep = _report_cpu(world)
    for n in RH.OUTPUTS:
        if n in RH.INTS:
            assert torch.equal(rep[n], torch.stack([r[n] for r in refs]).max(0).values), n
            continue
        total, bound, running = 0.0, 0.0, None
        for k, r in enumerate(refs):
            bound = bound + 2.0 ** -24 * r[n].abs() + 1e-12 * r["S_" + n]
            running = r[n] if running is None else running + r[n]
            if k:
                bound = bound + 2.0 ** -24 * running.abs()
        err = (rep[n].double() - running).abs()
        print("fixed_dt %s: %d sub-steps, largest |got - sum| / bound %.3f" % (n, len(refs), float((err / bound.clamp(min=1e-300)).max())))
        assert bool((err <= bound).all()), n
    assert float(rep["body_impulse"].abs().max()) > 0.0


def test_a_captured_fixed_interval_run_equals_the_eager_steps_bit_for_bit():
    """K sub-steps per step, the in-place folding captured with them."""
    wg, we = (_drop_world(3, 16, lift=(3.0, 200.0), report=_pairs(4)) for _ in range(2))
    wg.run(4, graph=True, fixed_dt=True, max_substeps=4)
    for _ in range(4):
        we.step(fixed_dt=True, max_substeps=4)
    torch.cuda.synchronize()
    assert len(wg._graphs) == 1
    for n in RH.OUTPUTS:
        assert _bits(getattr(wg.report, n).cpu(), getattr(we.report, n).cpu()), n


def test_a_world_without_a_report_is_the_same_world():
    plain, reporting = _drop_world(4, 16), _drop_world(4, 16, report=True)
    assert plain.report is None and reporting.report.P == 0
    for _ in range(5):
        plain.step()
        reporting.step()
    torch.cuda.synchronize()
    assert _bits(plain.p.cpu(), reporting.p.cpu()) and _bits(plain.v.cpu(), reporting.v.cpu()) and torch.equal(plain.t, reporting.t)
    with pytest.raises(ValueError):
        from lcp_physics_amd.physics.proximity import PairSet
        _drop_world(4, 16, report=PairSet.all_pairs(5, B + 1).to(DEV))


def test_a_breakout_ball_that_reaches_a_block_is_reported_for_exactly_that_block():
    """The golden roll-outs of tests/test_hip_breakout_world.py (a bounce off a block, off the paddle, off a wall), stepped plainly: in a
    step whose consumed records name the ball and a block and which turns the ball, `pair_contacts` is positive for exactly the named
    blocks; in every other step no block is reported."""
    import numpy as np
    from lcp_physics_amd.physics.breakout import extract_params, make_world
    from lcp_physics_amd.physics.proximity import PairSet
    from tests import encoder_host as EH
    from tests.test_hip_breakout_world import MAXB, _golden
    g = _golden()
    nscenes = len(g["r_key"])
    frames = torch.from_numpy(EH.to_frame(g["r_key"], 3, np.random.default_rng(0))).to(DEV)
    params = extract_params(frames, max_blocks=MAXB)
    ball, blocks = 5 + MAXB, list(range(5, 5 + MAXB))
    bw = make_world(params, torch.from_numpy(g["r_ball_vel"]).to(DEV), report=PairSet.between([ball], blocks, nscenes).to(DEV))
    world = bw.world
    assert bw.ball == ball and world.report.P == MAXB
    hits = 0
    for _ in range(int(g["r_nsteps"].max())):
        s = _before(world)
        world.step()
        torch.cuda.synchronize()
        got = world.report.pair_contacts.cpu() > 0
        turned = (world.v.cpu()[:, ball] != s["v"][:, ball]).any(1)
        for b in range(nscenes):
            n = min(int(s["count"][b]), world.maxc)
            i1, i2 = s["c_i1"][b, :n].tolist(), s["c_i2"][b, :n].tolist()
            named = {(j if i == ball else i) for i, j in zip(i1, i2) if ball in (i, j)} & set(blocks)
            want = torch.tensor([blk in named and bool(turned[b]) for blk in blocks])
            assert torch.equal(got[b], want), (b, got[b].tolist(), sorted(named), bool(turned[b]))
            hits += int(want.sum())
    assert hits >= 1
