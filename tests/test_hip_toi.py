"""GPU: the time-of-impact query of lcp_toi.hip (lcp_time_of_impact_f64, lcp_time_of_impact_backward_f64; physics/impact.py) against
the host mirror tests/toi_host.py, which tests/test_toi_host.py checks on the CPU, and the worlds that clip their steps with it
(`ContactWorld(ccd=...)`).

Bounds.  A HIT of either side lies where margin <= d <= margin + tol, an interval of length tol / |ddot| in time to first order: the
two times differ by at most 2 tol / |ddot| (+ 1e-12 horizon for the rounding of the times).  The existing distance kernel at
p + toi v must find the pair in that band, give or take 1e-9 of the coordinates' scale S (the tolerance of the proximity tests).  The
normal is compared with the mirror's AT THE KERNEL'S toi, within 1e-9; the gradients with the mirror's implicit gradient at the kernel's
own toi, within 1e-8 of each output's largest entry - the rule of the proximity backward.  Pairs the mirror cannot decide (`excluded`:
grazing within 1e-6, or a tied feature at toi; at most 2 % of a case, asserted on the CPU) are left out of the comparisons of status,
normal and gradient."""
import itertools

import pytest
import torch

from tests import toi_host as TH

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32, I32 = torch.float64, torch.float32, torch.int32
SCENE = ("kind", "radius", "verts_local", "nverts", "p", "v")
PAIRS = ("pair_first", "pair_second")
FWD_OUTS = (("toi", F64, ()), ("status", I32, ()), ("normal", F64, (2,)), ("first_toi", F64, None), ("first_pair", I32, None))
BWD_OUTS = ("p", "v", "radius", "verts_local", "margin")
NAN = float("nan")


def _lib():
    from lcp_physics_amd import _lib as L
    return L


def _absmax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _sizes(c):
    B, nb, cap = c["verts_local"].shape[:3]
    nv = torch.where(c["kind"] != 0, c["nverts"].clamp(0, cap), torch.zeros_like(c["nverts"]))
    return [B, nb, cap, c.get("svm", int(nv.sum(1).max())), c["pair_first"].shape[1]]


def _inputs(c):
    d = {k: c[k].to(DEV).contiguous() for k in SCENE + PAIRS + ("margin", "horizon")}
    return d, _sizes(c) + [_lib().ptr(d[k]) for k in SCENE + PAIRS]


def _filled(shape, dtype):
    return torch.full(shape, NAN if dtype == F64 else -77, dtype=dtype, device=DEV)


def _forward(c, want=None, rc=0):
    """The raw entry into outputs pre-filled with NaN / -77: dict of CPU tensors; `want`: the names asked for (the others NULL)."""
    L = _lib()
    d, args = _inputs(c)
    B, P = c["pair_first"].shape
    outs = {n: _filled((B,) if tail is None else (B, P) + tail, dt) for n, dt, tail in FWD_OUTS if want is None or n in want}
    got = L.load().lcp_time_of_impact_f64(*args, L.ptr(d["margin"]), L.ptr(d["horizon"]), c["tol"], c["max_iter"],
                                          *[L.ptr(outs.get(n)) for n, _, _ in FWD_OUTS], L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert got == rc
    return {n: o.cpu() for n, o in outs.items()}


def _backward(c, toi, status, g_toi, want=None):
    """The raw entry: the gradients keyed as toi_host.LEAVES (CPU)."""
    L = _lib()
    d, args = _inputs(c)
    t, s, g = (x.to(DEV).contiguous() for x in (toi, status, g_toi))
    outs = {n: _filled(tuple(c[n].shape), F64) for n in BWD_OUTS if want is None or n in want}
    rc = L.load().lcp_time_of_impact_backward_f64(*args, L.ptr(t), L.ptr(s), L.ptr(g), *[L.ptr(outs.get(n)) for n in BWD_OUTS],
                                                  L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    return {n: o.cpu() for n, o in outs.items()}


_FWD = {}


def _fwd(name):
    if name not in _FWD:
        _FWD[name] = _forward(TH.case(name))
    return _FWD[name]


def _g_toi(c, ref):
    g = torch.randn(c["pair_first"].shape, generator=torch.Generator().manual_seed(7), dtype=F64)
    return torch.where(ref["excluded"], torch.zeros_like(g), g)


# ------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("name", TH.CASE_NAMES)
def test_forward_matches_the_mirror(name):
    c, ref, out = TH.case(name), TH.reference(name), _fwd(name)
    toi, status, normal = out["toi"], out["status"], out["normal"]
    B, P = status.shape
    keep = ~ref["excluded"]
    assert int(ref["excluded"].sum()) <= 0.02 * B * P
    assert not bool(torch.isnan(toi).any()) and bool(torch.isfinite(normal).all()) and bool(((status >= 0) & (status <= 3)).all())
    print("%s: status counts kernel %s mirror %s" % (name, torch.bincount(status.flatten().long(), minlength=4).tolist(),
                                                     torch.bincount(ref["status"].flatten().long(), minlength=4).tolist()))
    assert torch.equal(status[keep], ref["status"][keep])
    hz = c["horizon"].reshape(B, 1).expand(B, P)
    miss, touching, hit = status == TH.MISS, status == TH.TOUCHING, (status == TH.HIT) & keep
    assert torch.equal(toi[miss].view(torch.int64), hz.clamp(min=0.0)[miss].contiguous().view(torch.int64))      # horizon's bits
    assert _absmax(toi[touching]) == 0.0
    assert _absmax(normal[miss | (status == TH.UNCONVERGED)]) == 0.0
    if bool(hit.any()):
        bound = 2 * c["tol"] / ref["ddot"].abs() + 1e-12 * hz
        err = (toi - ref["toi"]).abs()
        print("%s: |toi - mirror| at most %.3g of its bound, over %d hits" % (name, float((err / bound)[hit].max()), int(hit.sum())))
        assert bool((err <= bound)[hit].all())
    unc = (status == TH.UNCONVERGED) & keep
    assert bool((toi[unc] <= ref["root"][unc]).all())                                     # a true lower bound
    # the normal against the mirror's at the kernel's own toi
    seen, worst = {}, 0.0
    for b, r in ((status == TH.HIT) | touching).logical_and(keep).nonzero().tolist():
        k1, k2 = int(c["pair_first"][b, r]), int(c["pair_second"][b, r])
        key = (b, k1, k2, float(toi[b, r]))
        if key not in seen:
            seen[key] = TH.evaluate(c, b, k1, k2, key[3])
        _, n, tied = seen[key]
        if not tied:
            worst = max(worst, float((normal[b, r] - n).abs().max()))
    print("%s: |normal - mirror at the same toi| %.3g" % (name, worst))
    assert worst <= 1e-9
    # first_toi / first_pair: the reduction of the kernel's own toi and status, bit for bit
    cand = (status == TH.HIT) | (status == TH.UNCONVERGED)
    masked = torch.where(cand, toi, torch.full_like(toi, float("inf")))
    best = masked.min(1).values
    pair = torch.where(cand & (masked == best.unsqueeze(1)), torch.arange(P).expand(B, P), torch.full((B, P), P)).min(1).values
    none = ~cand.any(1)
    want_t = torch.where(none, c["horizon"].clamp(min=0.0), best)
    want_p = torch.where(none, torch.full_like(pair, -1), pair).to(I32)
    assert torch.equal(out["first_toi"].view(torch.int64), want_t.view(torch.int64)) and torch.equal(out["first_pair"], want_p)


@pytest.mark.parametrize("name", TH.CASE_NAMES)
def test_the_distance_kernel_finds_every_hit_within_tol_of_its_margin(name):
    """Every HIT as a two-body scene at p + toi v through lcp_pair_distance_f64: margin - 1e-9 S <= dist <= margin + tol + 1e-9 S."""
    c, out = TH.case(name), _fwd(name)
    idx = (out["status"] == TH.HIT).nonzero()
    if idx.numel() == 0:
        return
    b, r = idx[:, 0], idx[:, 1]
    k = torch.stack([c["pair_first"][b, r], c["pair_second"][b, r]], 1).long()
    bb = b.unsqueeze(1)
    pose = c["p"][bb, k] + out["toi"][b, r].reshape(-1, 1, 1) * c["v"][bb, k].double()
    N, cap = len(b), c["verts_local"].shape[2]
    L = _lib()
    dev = lambda t: t.to(DEV).contiguous()
    ins = [dev(c["kind"][bb, k]), dev(c["radius"][bb, k]), dev(c["verts_local"][bb, k]), dev(c["nverts"][bb, k]), dev(pose),
           torch.zeros(N, 1, dtype=I32, device=DEV), torch.ones(N, 1, dtype=I32, device=DEV),
           torch.full((N, 1), float("inf"), dtype=F64, device=DEV)]
    dist = torch.full((N, 1), NAN, dtype=F64, device=DEV)
    rc = L.load().lcp_pair_distance_f64(N, 2, cap, 2 * cap, 1, *[L.ptr(t) for t in ins], L.ptr(dist), None, None, None,
                                        L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    gap = dist.cpu()[:, 0] - c["margin"][b, r]
    S = TH.scale(c)
    print("%s: %d hits, d - margin in [%.3g, %.3g], tol %.3g, S %.3g" % (name, N, float(gap.min()), float(gap.max()), c["tol"], S))
    assert float(gap.min()) >= -1e-9 * S and float(gap.max()) <= c["tol"] + 1e-9 * S


# ------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("name", TH.CASE_NAMES)
def test_backward_matches_the_mirrors_implicit_gradient_at_the_kernels_toi(name):
    c, ref, out = TH.case(name), TH.reference(name), _fwd(name)
    g = _g_toi(c, ref)
    got = _backward(c, out["toi"], out["status"], g)
    want = TH.gradients(c, out["toi"], out["status"], g)
    for k in BWD_OUTS:
        assert bool(torch.isfinite(got[k]).all()), k                                      # written, everywhere
    hull = c["kind"] != 0
    cap = c["verts_local"].shape[2]
    pad = torch.arange(cap).reshape(1, 1, cap) >= (c["nverts"] * hull).unsqueeze(2)
    assert _absmax(got["radius"][hull]) == 0.0 and _absmax(got["verts_local"][pad]) == 0.0
    live = want["live"]
    assert _absmax(got["margin"][~live & ~ref["excluded"]]) == 0.0                        # exactly 0 on pairs that are not live
    touched = torch.zeros(c["kind"].shape, dtype=torch.bool)
    for b, r in (live | ref["excluded"]).nonzero().tolist():
        touched[b, int(c["pair_first"][b, r])] = touched[b, int(c["pair_second"][b, r])] = True
    for k in ("p", "v", "radius", "verts_local"):
        assert _absmax(got[k][~touched]) == 0.0, k                                        # ... and on the bodies of none that is
    for k in BWD_OUTS:
        err, scale = float((got[k] - want[k]).abs().max()), float(want[k].abs().max())
        print("%s %s: |difference| %.3g of %.3g (%d live pairs)" % (name, k, err, scale, int(live.sum())))
        assert err <= 1e-8 * scale, k
    if name in ("mixed", "boxes", "rod"):
        assert int(live.sum()) > 0 and float(want["p"].abs().max()) > 0


@pytest.mark.parametrize("name", ["mixed", "edges257"])
def test_two_runs_give_the_same_bits_with_every_subset_of_outputs(name):
    c, ref, full = TH.case(name), TH.reference(name), _fwd(name)
    g = _g_toi(c, ref)
    bits = lambda t: t.view(torch.int64) if t.dtype == F64 else t
    names = [n for n, _, _ in FWD_OUTS]
    for k in range(1, len(names) + 1):
        for want in itertools.combinations(names, k):
            part = _forward(c, want=want)
            assert set(part) == set(want)
            for n in want:
                assert torch.equal(bits(part[n]), bits(full[n])), (want, n)
    whole = _backward(c, full["toi"], full["status"], g)
    for k in range(1, len(BWD_OUTS) + 1):
        for want in itertools.combinations(BWD_OUTS, k):
            part = _backward(c, full["toi"], full["status"], g, want=want)
            for n in want:
                assert torch.equal(bits(part[n]), bits(whole[n])), (want, n)


def test_the_cull_and_bodies_at_rest():
    """A horizon so short that every pair's bounding circles are too far apart to close: all MISS with the horizon's bits, the same
    with the cull's condition true and the advancement's first step deciding (v = 0: a_k = 0)."""
    c = TH.case("mixed")
    B, P = c["pair_first"].shape
    short = dict(c, horizon=torch.full((B,), 1e-5, dtype=F64))
    out = _forward(short)
    assert bool((out["status"] == TH.MISS).all()) and bool((out["toi"] == 1e-5).all()) and bool((out["first_pair"] == -1).all())
    assert bool((out["first_toi"] == 1e-5).all())
    rest = _forward(dict(c, v=torch.zeros_like(c["v"])))
    assert bool((rest["status"] == TH.MISS).all()) and torch.equal(rest["toi"], c["horizon"].reshape(B, 1).expand(B, P))
    # no result depends on the cull: one evaluation is all a pair needs where the cull's condition holds, so max_iter = 1 says MISS too
    one = _forward(dict(short, max_iter=1))
    assert bool((one["status"] == TH.MISS).all())
    nan = _forward(dict(c, horizon=torch.tensor([NAN, -1.0, 2.0], dtype=F64)))
    assert bool((nan["status"][:2] == TH.MISS).all()) and _absmax(nan["toi"][:2]) == 0.0 and bool((nan["first_toi"][:2] == 0.0).all())
    assert torch.equal(nan["toi"][2], _fwd("mixed")["toi"][2])


# ------------------------------------------------------------------------------------------------------------- the autograd surface
def _geom(c, leaves=False):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.proximity import PairSet
    t = lambda k: c[k].to(DEV).contiguous()
    lf = (lambda k: t(k).requires_grad_(True)) if leaves else t
    geom = GeometryBatch(t("kind"), lf("radius"), lf("verts_local"), t("nverts"), None, _sizes(c)[3])
    pairs = PairSet(t("pair_first"), t("pair_second"), torch.full(c["pair_first"].shape, float("inf"), dtype=F64, device=DEV))
    return geom, lf("p"), lf("v"), pairs


def test_time_of_impact_returns_the_entrys_bits_and_its_backward_the_entrys_gradients():
    from lcp_physics_amd.physics import impact
    assert (impact.MISS, impact.HIT, impact.TOUCHING, impact.UNCONVERGED) == (0, 1, 2, 3)
    c, ref, raw = TH.case("mixed"), TH.reference("mixed"), _fwd("mixed")
    geom, p, v, pairs = _geom(c, leaves=True)
    margin = c["margin"].to(DEV).requires_grad_(True)
    toi, status, normal = impact.time_of_impact(geom, p, v, pairs, c["horizon"].to(DEV), margin=margin, normals=True)
    assert torch.equal(toi.detach().cpu(), raw["toi"]) and torch.equal(status.cpu(), raw["status"]) and torch.equal(normal.cpu(), raw["normal"])
    assert toi.requires_grad and not status.requires_grad and not normal.requires_grad
    g = _g_toi(c, ref)
    toi.backward(g.to(DEV))
    want = _backward(c, raw["toi"], raw["status"], g)
    for k, t in zip(BWD_OUTS, (p, v, geom.radius, geom.verts_local, margin)):
        assert t.grad.dtype == t.dtype and torch.equal(t.grad.cpu().double(), want[k] if k != "v" else want[k].float().double()), k
    # a number for the horizon and the margin, two outputs, only what requires grad is asked for
    geom2, p2, v2, pairs2 = _geom(dict(c, margin=torch.zeros_like(c["margin"])))
    v2 = v2.double().requires_grad_(True)                                                 # another dtype: rounded, the gradient cast back
    res = impact.time_of_impact(geom2, p2, v2, pairs2, 2.0)
    assert len(res) == 2 and torch.equal(res[0].detach().cpu(), _forward(dict(c, margin=torch.zeros_like(c["margin"])))["toi"])
    res[0].sum().backward()
    assert v2.grad.dtype == F64 and bool(torch.isfinite(v2.grad).all()) and float(v2.grad.abs().max()) > 0 and geom2.radius.grad is None


def _gradcheck_case():
    """2 scenes x 3 bodies (a circle, a rect, a pentagon), the three pairs in both orders; the circle flies at the rect, the rect and
    the pentagon close on each other while they turn: every HIT far from grazing and from a tie."""
    import numpy as np
    rng = np.random.default_rng(5)
    bodies, vel = [], []
    for b in range(2):
        bodies.append([("circle", (0.2, 0.0, 3.0 + b), 4.0), ("hull", (0.35 + 0.1 * b, 40.0, 0.0), TH._rect(14.0, 10.0)),
                       ("hull", (0.8, 80.0, 8.0), TH._hull(rng, 5, 9.0, 8.0))])
        vel.append([(0.5, 12.0 + b, 0.5), (0.3, 0.0, 0.0), (-0.4, -14.0, -1.0)])
    c = TH._assemble(bodies, 8)
    return TH._finish(c, vel, [[(0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0)]] * 2, 4.0, margin=0.1, tol=1e-12, max_iter=256)


def test_gradcheck_at_two_scenes_of_three_bodies():
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.impact import time_of_impact
    from lcp_physics_amd.physics.proximity import PairSet
    c = _gradcheck_case()
    hits = 0
    for b in range(2):
        for r in range(6):
            a = TH.advance(c, b, r)
            if a["status"] == TH.HIT:
                hits += 1
                _, gm = TH.brute(c, b, r)
                assert not a["tied"] and gm < -0.5                                        # away from grazing and from a tie
    assert hits >= 8
    t = lambda k: c[k].to(DEV).contiguous()
    ins = [t("p").requires_grad_(True), t("v").double().requires_grad_(True), t("radius").requires_grad_(True),
           t("verts_local").requires_grad_(True), t("margin").requires_grad_(True)]
    pairs = PairSet(t("pair_first"), t("pair_second"), torch.full((2, 6), float("inf"), dtype=F64, device=DEV))

    def fn(p, v, radius, verts_local, margin):
        geom = GeometryBatch(t("kind"), radius, verts_local, t("nverts"), None, _sizes(c)[3])
        return time_of_impact(geom, p, v, pairs, 4.0, margin=margin, tol=1e-12, max_iter=256)[0]

    # v is rounded to float32 inside, so a step of 1e-6 on it is lost: gradcheck takes the other four inputs ...
    assert torch.autograd.gradcheck(lambda p, r, vl, m: fn(p, ins[1].detach(), r, vl, m), [ins[0]] + ins[2:], eps=1e-6, atol=1e-6, rtol=1e-6,
                                    nondet_tol=0.0)
    # ... and v gets central differences at steps that float32 holds exactly on these velocities (2^-8 and 2^-9), extrapolated once:
    # what is left is of the order (toi h)^4 = 1e-8 of the higher derivatives, which the lever arms of 10 units put at up to 100 times
    # the first - 1e-5 relative covers it; the gradient itself is held to 1e-8 against the mirror above
    toi = fn(*ins)
    g_v, = torch.autograd.grad(toi.sum(), ins[1])
    v0 = ins[1].detach()
    total = lambda v: float(fn(ins[0].detach(), v, ins[2].detach(), ins[3].detach(), ins[4].detach()).sum())
    worst = 0.0
    for b, k, q in itertools.product(range(2), range(3), range(3)):
        fd = []
        for h in (2.0 ** -8, 2.0 ** -9):
            d = torch.zeros_like(v0)
            d[b, k, q] = h
            fd.append((total(v0 + d) - total(v0 - d)) / (2 * h))
        rich = (4 * fd[1] - fd[0]) / 3
        worst = max(worst, abs(rich - float(g_v[b, k, q])) / max(1.0, float(g_v.abs().max())))
    print("d toi / d v against extrapolated central differences: %.3g of %.3g" % (worst, float(g_v.abs().max())))
    assert worst <= 1e-5


# ------------------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_are_refused_before_any_launch():
    L = _lib()
    lib, c = L.load(), TH.case("mixed")
    d, args = _inputs(c)
    B, P = c["pair_first"].shape
    toi = torch.full((B, P), NAN, dtype=F64, device=DEV)
    st = torch.ones(B, P, dtype=I32, device=DEV)
    g = torch.zeros(B, P, dtype=F64, device=DEV)
    g_p = torch.full(c["p"].shape, NAN, dtype=F64, device=DEV)
    stream = L.stream_ptr(torch.device(DEV))
    m, h = L.ptr(d["margin"]), L.ptr(d["horizon"])
    fwd = lambda a, out=True, m=m, h=h, tol=1e-6, it=64: lib.lcp_time_of_impact_f64(*a, m, h, tol, it, L.ptr(toi) if out else None, None, None,
                                                                                   None, None, stream)
    toi0 = torch.zeros(B, P, dtype=F64, device=DEV)
    bwd = lambda a, out=True, t=L.ptr(toi0), s=L.ptr(st), gg=L.ptr(g): lib.lcp_time_of_impact_backward_f64(
        *a, t, s, gg, L.ptr(g_p) if out else None, None, None, None, None, stream)
    with_size = lambda k, v: args[:k] + [v] + args[k + 1:]
    bad = [with_size(0, -1), with_size(4, 0), with_size(4, 1025), with_size(1, 0), with_size(1, 65), with_size(2, 7), with_size(2, 65),
           with_size(3, -1), with_size(3, 1025)] + [with_size(k, None) for k in range(5, 13)]     # sizes; every array NULL in turn
    for a in bad:
        assert fwd(a) == -1 and bwd(a) == -1
    assert fwd(args, out=False) == -1 and bwd(args, out=False) == -1                      # no output
    assert fwd(args, m=None) == -1 and fwd(args, h=None) == -1
    assert fwd(args, tol=0.0) == -1 and fwd(args, tol=-1.0) == -1 and fwd(args, tol=NAN) == -1 and fwd(args, it=0) == -1 and fwd(args, it=1025) == -1
    assert bwd(args, t=None) == -1 and bwd(args, s=None) == -1 and bwd(args, gg=None) == -1
    assert fwd(with_size(0, 0)) == 0 and bwd(with_size(0, 0)) == 0                        # B = 0: success, no launch
    torch.cuda.synchronize()
    assert bool(torch.isnan(toi).all()) and bool(torch.isnan(g_p).all())                  # nothing was written
    assert fwd(args, it=1024) == 0 and bwd(args) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(toi).any()) and not bool(torch.isnan(g_p).any())


def test_host_side_refusals_and_no_synchronisation():
    from lcp_physics_amd.physics.impact import time_of_impact
    from lcp_physics_amd.physics.proximity import PairSet
    c = TH.case("mixed")
    geom, p, v, pairs = _geom(c)
    for kw, match in ((dict(tol=0.0), "tol"), (dict(max_iter=0), "max_iter"), (dict(max_iter=1025), "max_iter"), (dict(margin=-1.0), "margin"),
                      (dict(margin=torch.zeros(3, 4, dtype=F64, device=DEV)), "margin")):
        with pytest.raises(ValueError, match=match):
            time_of_impact(geom, p, v, pairs, 2.0, **kw)
    with pytest.raises(ValueError, match="horizon"):
        time_of_impact(geom, p, v, pairs, torch.ones(2, dtype=F64, device=DEV))
    with pytest.raises(ValueError, match="shape"):
        time_of_impact(geom, p, v[:, :4], pairs, 2.0)
    with pytest.raises(ValueError, match="scenes"):
        time_of_impact(geom, p, v, PairSet(pairs.first[:2], pairs.second[:2], pairs.max_dist[:2]), 2.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        time_of_impact(geom, p.cpu(), v, pairs, 2.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        time_of_impact(geom, p, v.cpu(), pairs, 2.0)
    # no call synchronises: a stream capture would refuse one
    hz, mg = c["horizon"].to(DEV), c["margin"].to(DEV)
    time_of_impact(geom, p, v, pairs, hz, margin=mg)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        toi, status = time_of_impact(geom, p, v, pairs, hz, margin=mg)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(toi.cpu(), _fwd("mixed")["toi"]) and torch.equal(status.cpu(), _fwd("mixed")["status"])


# ------------------------------------------------------------------------------------------------------------- worlds that clip their steps
WB, WDT, WVX = 4, 1.0 / 30, 1800.0


def _wall_world(**kw):
    """Body 0: a wall 10 x 200 at x = 50, pinned by a constant Je; body 1: a ball of radius 1 at x = 0 flying at it with 1800 units/s
    (scaled per scene) - 60 units a step against a wall 10 thick.  No forces."""
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.contacts import GeometryBatch
    geom = GeometryBatch.from_shapes([("rect", (10.0, 200.0)), ("circle", 1.0)], WB).to(DEV)
    p0 = torch.tensor([[0.0, 50.0, 0.0], [0.0, 0.0, 0.0]], dtype=F64, device=DEV).repeat(WB, 1, 1)
    speed = WVX * (1.0 + 0.05 * torch.arange(WB, dtype=F32, device=DEV))
    v0 = torch.zeros(WB, 2, 3, dtype=F32, device=DEV)
    v0[:, 1, 1] = speed
    Mdiag = torch.tensor([[500.0, 10.0, 10.0], [0.5, 1.0, 1.0]], dtype=F32, device=DEV).repeat(WB, 1, 1)
    Je = torch.zeros(WB, 3, 6, dtype=F32, device=DEV)
    for q in range(3):
        Je[:, q, q] = 1.0
    half = torch.zeros(WB, 2, dtype=F32, device=DEV) + 0.5
    v_in = kw.pop("v0", v0)
    return ContactWorld(geom, p0, v_in, Mdiag, torch.zeros(WB, 2, 3, device=DEV), half, half, Je=Je, dt=WDT, maxc=4, **kw), speed.double().cpu()


def _ball_pairs():
    from lcp_physics_amd.physics.proximity import PairSet
    return PairSet.between([1], [0], WB).to(DEV)


def test_without_ccd_the_ball_goes_through_the_wall():
    """Today's behaviour, stated: the end pose overlaps nothing, the move is accepted, no contact record was ever made."""
    world, _ = _wall_world()
    world.step()
    assert float(world.p[:, 1, 1].min()) > 56.0 and int(world.contacts.count.sum()) == 0
    toi, status = world.time_to_contact(_ball_pairs())                                    # (beyond the wall and leaving: a MISS)
    assert bool((status == 0).all()) and bool((toi == WDT).all())


def test_with_ccd_the_step_ends_at_first_touch():
    pairs = _ball_pairs()
    world, speed = _wall_world(ccd=pairs)
    margin, tol = world.eps / 2, 1e-6
    toi, status = world.time_to_contact(pairs, margin=margin)
    assert bool((status == 1).all())
    world.step()
    dt_used = world.contacts.dt_used.cpu()
    want = (44.0 - margin) / speed
    print("dt_used", dt_used.tolist(), "(44 - margin) / v_x", want.tolist())
    assert bool(((dt_used - want).abs() <= tol / speed).all()) and torch.equal(dt_used, toi[:, 0].cpu())
    assert bool((world.contacts.count >= 1).all())                                        # a circle - wall record exists
    i1, i2 = world.contacts.c_i1[:, 0].cpu(), world.contacts.c_i2[:, 0].cpu()
    assert bool(((i1 + i2) == 1).all())
    t = dt_used.clone()
    assert torch.equal(world.t.cpu(), t)
    for _ in range(5):
        world.step()
        t = t + world.contacts.dt_used.cpu()
        assert float((world.p[:, 1, 1] + 1.0).max()) <= 45.0 + tol
    assert float((world.t.cpu() - t).abs().max()) <= 1e-15 and bool(torch.isfinite(world.p).all())


def test_with_ccd_a_fixed_interval_step_makes_up_the_remainder():
    world, _ = _wall_world(ccd=_ball_pairs())
    world.step(fixed_dt=True)
    assert torch.equal(world.t.cpu(), torch.full((WB,), WDT, dtype=F64)) and world.substeps.tolist() == [2] * WB
    assert float((world.p[:, 1, 1] + 1.0).max()) <= 45.0 + 1e-6 and bool((world.p[:, 1, 1] < 44.0).all())     # it bounced or stopped


def test_with_ccd_a_captured_run_equals_eager_steps():
    eager, _ = _wall_world(ccd=_ball_pairs())
    for _ in range(6):
        eager.step()
    replay, _ = _wall_world(ccd=_ball_pairs())
    replay.run(6, graph=True)
    torch.cuda.synchronize()
    for a, b in ((eager.p, replay.p), (eager.v, replay.v), (eager.t, replay.t)):
        assert torch.equal(a, b)
    assert float((replay.p[:, 1, 1] + 1.0).max()) <= 45.0 + 1e-6


def test_with_ccd_a_differentiable_roll_out_reaches_v0():
    v0 = torch.zeros(WB, 2, 3, dtype=F32, device=DEV)
    v0[:, 1, 1] = WVX
    v0[:, 1, 2] = 30.0
    v0.requires_grad_(True)
    world, _ = _wall_world(ccd=_ball_pairs(), v0=v0)
    for _ in range(3):
        world.step(differentiable=True)
    assert float((world.p[:, 1, 1] + 1.0).max()) <= 45.0 + 1e-6
    toi, _ = world.time_to_contact(_ball_pairs(), horizon=1.0)
    assert toi.requires_grad or not world.v.requires_grad
    world.p[:, 1, 1:].sum().backward()
    assert v0.grad is not None and bool(torch.isfinite(v0.grad).all()) and float(v0.grad.abs().max()) > 0


def test_ccd_true_is_all_pairs_and_its_refusals():
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.contacts import GeometryBatch
    a, _ = _wall_world(ccd=True)
    b, _ = _wall_world(ccd=_ball_pairs())
    assert a._ccd.pairs.first.tolist() == [[0]] * WB and a._ccd.pairs.second.tolist() == [[1]] * WB
    for _ in range(4):
        a.step()
        b.step()
    assert torch.equal(a.p, b.p) and torch.equal(a.v, b.v) and torch.equal(a.t, b.t)
    with pytest.raises(ValueError, match="ccd"):
        _wall_world(ccd_margin=0.01)
    nb = 46
    geom = GeometryBatch.from_shapes([("circle", 1.0)] * nb, 1).to(DEV)
    p = torch.zeros(1, nb, 3, dtype=F64, device=DEV)
    p[0, :, 1] = 10.0 * torch.arange(nb, dtype=F64, device=DEV)
    z = torch.zeros(1, nb, 3, dtype=F32, device=DEV)
    with pytest.raises(ValueError, match="45"):
        ContactWorld(geom, p, z, z + 1.0, z, z[..., 0], z[..., 0], Je=None, maxc=4, ccd=True)


def test_ccd_true_leaves_out_the_pairs_of_no_contact():
    from lcp_physics_amd.physics.contacts import GeometryBatch
    world, _ = _wall_world()
    g = world.geom
    nc = torch.zeros(WB, 2, 2, dtype=torch.uint8, device=DEV)
    nc[1:, 0, 1] = 1
    nc[1:, 1, 0] = 1
    world.geom = GeometryBatch(g.kind, g.radius, g.verts_local, g.nverts, nc, g.verts_max())
    pairs = world._ccd_all_pairs()
    assert pairs.second.tolist() == [[1]] + [[0]] * (WB - 1) and pairs.first.tolist() == [[0]] * WB
    toi, status = world.time_to_contact(pairs)
    assert status[:, 0].tolist() == [1] + [0] * (WB - 1)


def test_a_world_without_ccd_is_what_it_was():
    """A four-box stack over 20 steps: a world built with ccd=None gives the bits of a world built without the argument, and the
    query itself changes nothing in either."""
    from lcp_physics_amd.physics.batched_world import ContactWorld
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.proximity import PairSet

    def build(**kw):
        B = 4
        geom = GeometryBatch.from_shapes([("rect", (400.0, 10.0))] + [("rect", (30.0, 20.0))] * 3, B).to(DEV)
        p0 = torch.tensor([[0.0, 200.0, 300.0]] + [[0.0, 200.0 + 2.0 * k, 300.0 - 15.05 - 20.05 * k] for k in range(3)], dtype=F64, device=DEV)
        p0 = p0.repeat(B, 1, 1)
        p0[:, 1:, 1] += torch.arange(B, dtype=F64, device=DEV).reshape(B, 1)
        Mdiag = torch.tensor([[1e4, 10.0, 10.0]] + [[60.0, 1.0, 1.0]] * 3, dtype=F32, device=DEV).repeat(B, 1, 1)
        f = torch.zeros(B, 4, 3, dtype=F32, device=DEV)
        f[:, 1:, 2] = 100.0
        Je = torch.zeros(B, 3, 12, dtype=F32, device=DEV)
        for q in range(3):
            Je[:, q, q] = 1.0
        half = torch.zeros(B, 4, dtype=F32, device=DEV) + 0.5
        return ContactWorld(geom, p0, torch.zeros(B, 4, 3, device=DEV), Mdiag, f, half, half, Je=Je, dt=WDT, maxc=16, **kw)

    plain, same = build(), build(ccd=None)
    assert plain._ccd is None and same._ccd is None
    pairs = PairSet.all_pairs(4, 4).to(DEV)
    for k in range(20):
        plain.step()
        same.step()
        if k % 5 == 0:
            same.time_to_contact(pairs)
    for a, b in ((plain.p, same.p), (plain.v, same.v), (plain.t, same.t), (plain.contacts.count, same.contacts.count)):
        assert torch.equal(a, b)
    assert int(plain.contacts.count.sum()) > 0
