"""The force elements of lcp_forces.hip (include/lcp_hip.h, "force elements") restated as plain float64 torch operations on the CPU: the
yardstick of tests/test_hip_force_elements.py, checked on its own by tests/test_force_elements_host.py.  Autograd gives the gradients.

`forces_host(case)` returns
    f64   [B,nb,3]  the unrounded sum: f_base plus every element's wrench on the body
    S     [B,nb,3]  the sum of the magnitudes of the terms that enter each entry, |f_base| included
    gap   two [B,E] arrays: `sat`, | |s| - limit | / limit of the unclamped tension or torque (inf where limit is inf or the element
          has no clamp), and `L`, a spring's length (inf for everything else)
    valid [B,E] the elements that are evaluated at all, raw [B,E] the unclamped tension / torque, sat [B,E] the clamped ones
A saturated element enters f64 detached: it has no gradient with respect to anything.

The seeded case table `CASES` is generated once per process; `case(name)` hands out its tensors (do not modify them) and
`reference(name)` the mirror's outputs with the gradients of sum(f64 * g_f) to every leaf."""
import torch

F64, F32, I32 = torch.float64, torch.float32, torch.int32
INF = float("inf")
LEAVES = ("p", "v", "k", "c", "x0", "w0", "a1", "a2")                    # the backward's outputs, in the C entry's order
ELEMENT_ARRAYS = ("kind", "b1", "b2", "a1", "a2", "k", "c", "x0", "w0", "limit")
CASE_NAMES = ("one", "small", "edge63", "edge64", "edge65", "e257", "full", "one_body", "untouched", "invalid", "saturated", "per_scene")
MIN_GAP = 1e-6


def _cross(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def _perp(a):
    return torch.stack([-a[..., 1], a[..., 0]], -1)


def _gather(state, b):
    """state [B,nb,3] at the body indices b [B,E] (clamped: the caller masks what is not a body)."""
    B, E = b.shape
    idx = b.clamp(0, state.shape[1] - 1).long().unsqueeze(-1).expand(B, E, 3)
    return state.gather(1, idx)


def _end(b, a, p, v):
    """Anchor `a` [B,E,2] on body `b` [B,E] (-1: a world point at rest): r, P, V [B,E,2] and rot, w [B,E]."""
    body = (b >= 0).unsqueeze(-1)
    st, vel = _gather(p, b), _gather(v, b)
    rot, w = st[..., 0], vel[..., 0]
    cs, sn = torch.cos(rot), torch.sin(rot)
    r = torch.stack([cs * a[..., 0] - sn * a[..., 1], sn * a[..., 0] + cs * a[..., 1]], -1)          # utils.py:105-112
    r = torch.where(body, r, torch.zeros_like(r))
    P = torch.where(body, st[..., 1:] + r, a)
    V = torch.where(body, vel[..., 1:] + w.unsqueeze(-1) * _perp(r), torch.zeros_like(r))
    return r, P, V, torch.where(b >= 0, rot, torch.zeros_like(rot)), torch.where(b >= 0, w, torch.zeros_like(w))


def _clamp(raw, limit):
    sat = raw.abs() >= limit
    finite = torch.where(torch.isinf(limit), torch.ones_like(limit), limit)
    return torch.where(sat, torch.sign(raw) * finite, raw), sat


def forces_host(c, leaves=None):
    """The rule of the header for case `c`; `leaves`: tensors to use in place of c's (float64, possibly requiring grad).  Runs on
    whatever device the tensors live on (the closure route of the world tests evaluates it on the GPU)."""
    t = dict(c)
    t.update(leaves or {})
    p, v = t["p"].to(F64), t["v"].to(F64)
    kind, b1, b2, limit = c["kind"], c["b1"], c["b2"], c["limit"]
    k, cc, x0, w0, a1, a2 = (t[n].to(F64) for n in ("k", "c", "x0", "w0", "a1", "a2"))
    B, nb = p.shape[:2]
    E = kind.shape[1]
    inside = lambda b: (b >= -1) & (b < nb)
    two_ended = inside(b1) & inside(b2) & (b1 != b2)
    # ---- spring
    r1, P1, V1, rot1, w1 = _end(b1, a1, p, v)
    r2, P2, V2, rot2, w2 = _end(b2, a2, p, v)
    d = P2 - P1
    dd = (d * d).sum(-1)
    has_len = dd > 0
    L = torch.sqrt(torch.where(has_len, dd, torch.ones_like(dd)))
    u = d / L.unsqueeze(-1)
    Ldot = (u * (V2 - V1)).sum(-1)
    s_raw = k * (L - x0) + cc * Ldot
    s, s_sat = _clamp(s_raw, limit)
    F = s.unsqueeze(-1) * u
    spring = (kind == 1) & two_ended & has_len
    ws1 = torch.cat([_cross(r1, F).unsqueeze(-1), F], -1)
    ws2 = torch.cat([_cross(r2, -F).unsqueeze(-1), -F], -1)
    # ---- motor
    tau_raw = k * (x0 - (rot2 - rot1)) + cc * (w0 - (w2 - w1))
    tau, t_sat = _clamp(tau_raw, limit)
    motor = (kind == 2) & two_ended
    zero = torch.zeros_like(tau)
    wm1, wm2 = torch.stack([-tau, zero, zero], -1), torch.stack([tau, zero, zero], -1)
    # ---- drag
    drag = (kind == 3) & (b1 >= 0) & (b1 < nb)
    vel = _gather(v, b1)
    wd1 = torch.stack([-cc * vel[..., 0], -k * vel[..., 1], -k * vel[..., 2]], -1)
    # ---- what each end receives
    pick = lambda m, x: torch.where(m.unsqueeze(-1), x, torch.zeros_like(x))
    W1 = pick(spring, ws1) + pick(motor, wm1) + pick(drag, wd1)
    W2 = pick(spring, ws2) + pick(motor, wm2)
    sat = (spring & s_sat) | (motor & t_sat)
    W1 = torch.where(sat.unsqueeze(-1), W1.detach(), W1)
    W2 = torch.where(sat.unsqueeze(-1), W2.detach(), W2)
    valid = spring | motor | drag
    m1 = (valid & (b1 >= 0)).unsqueeze(-1)
    m2 = ((spring | motor) & (b2 >= 0)).unsqueeze(-1)
    base = t.get("f_base")
    base = torch.zeros(B, nb, 3, dtype=F64, device=p.device) if base is None else base.to(F64)
    offs = (torch.arange(B, device=p.device) * nb).unsqueeze(1)
    i1 = (offs + b1.clamp(0, nb - 1).long()).reshape(-1)
    i2 = (offs + b2.clamp(0, nb - 1).long()).reshape(-1)
    T1, T2 = pick(m1.squeeze(-1), W1).reshape(-1, 3), pick(m2.squeeze(-1), W2).reshape(-1, 3)
    flat = torch.zeros(B * nb, 3, dtype=F64, device=p.device)
    f64 = base + flat.index_add(0, i1, T1).index_add(0, i2, T2).reshape(B, nb, 3)
    S = base.detach().abs() + flat.index_add(0, i1, T1.detach().abs()).index_add(0, i2, T2.detach().abs()).reshape(B, nb, 3)
    touched = flat[:, 0].index_add(0, i1, m1.reshape(-1).to(F64)).index_add(0, i2, m2.reshape(-1).to(F64)).reshape(B, nb) > 0
    raw = torch.where(spring, s_raw, torch.where(motor, tau_raw, torch.zeros_like(s_raw))).detach()
    clamped = (spring | motor) & torch.isfinite(limit)
    gap_sat = torch.where(clamped, (raw.abs() - limit).abs() / limit, torch.full_like(raw, INF))
    gap_L = torch.where((kind == 1) & two_ended, torch.sqrt(dd.detach()), torch.full_like(raw, INF))
    return {"f64": f64, "S": S, "gap": {"sat": gap_sat, "L": gap_L}, "valid": valid, "raw": raw, "sat": sat, "touched": touched}


# ------------------------------------------------------------------------------------------------------------- the cases
def _random(seed, B, nb, E, kinds=(1, 2, 3), world=0.25, limit=INF):
    """A seeded case: kinds drawn from `kinds` per element and scene, spring / motor ends two different members of {world, bodies}
    (the world with probability about `world` per end), drag on a body; coordinates of order 10, stiffness of order 10."""
    g = torch.Generator().manual_seed(seed)
    U = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=F64)
    kind = torch.tensor(kinds, dtype=I32)[torch.randint(0, len(kinds), (B, E), generator=g)]
    body = lambda: torch.randint(0, nb, (B, E), generator=g)
    i1 = torch.where(torch.rand(B, E, generator=g) < world, torch.zeros(B, E, dtype=torch.long), 1 + body())
    i2 = (i1 + 1 + body()) % (nb + 1)                                       # (never i1: both in [0, nb], 0 the world)
    b1, b2 = (i1 - 1).to(I32), (i2 - 1).to(I32)
    b1 = torch.where(kind == 3, body().to(I32), b1)
    anchor = lambda b: torch.where((b >= 0).unsqueeze(-1), U(-1.5, 1.5, B, E, 2), U(-10.0, 10.0, B, E, 2))
    spring = kind == 1
    c = {"kind": kind, "b1": b1, "b2": b2, "a1": anchor(b1), "a2": anchor(b2),
         "k": U(5.0, 50.0, B, E), "c": U(0.1, 2.0, B, E),
         "x0": torch.where(spring, U(0.5, 3.0, B, E), U(-1.0, 1.0, B, E)), "w0": U(-1.0, 1.0, B, E),
         "limit": torch.full((B, E), float(limit), dtype=F64),
         "p": torch.cat([U(-3.0, 3.0, B, nb, 1), U(-10.0, 10.0, B, nb, 2)], -1),
         "v": (2.0 * torch.randn(B, nb, 3, generator=g)).to(F32),
         "f_base": torch.randn(B, nb, 3, generator=g).to(F32),
         "g_f": torch.randn(B, nb, 3, generator=g).to(F32)}
    return c


def _set(c, scene, e, kind, b1, b2):
    c["kind"][scene, e], c["b1"][scene, e], c["b2"][scene, e] = kind, b1, b2


def _build():
    C = {}
    one = _random(1, 1, 1, 1, kinds=(1,))
    _set(one, 0, 0, 1, -1, 0)                                               # a world-anchored spring
    one["a1"][0, 0] = torch.tensor([3.0, -4.0], dtype=F64)
    C["one"] = one
    small = _random(2, 5, 3, 4)
    for s in range(5):                                                      # all kinds plus a kind-0 slot
        _set(small, s, 0, 1, 0, 1)
        _set(small, s, 1, 2, -1, 2)
        _set(small, s, 2, 3, 1, -1)
        _set(small, s, 3, 0, 0, 1)
    small["limit"][:, 1] = 1e4
    C["small"] = small
    C["edge63"] = _random(3, 3, 5, 63)                                      # one wavefront per scene, a lane short
    C["edge64"] = _random(4, 3, 64, 64)                                     # exactly a wavefront of elements and of bodies
    C["edge65"] = _random(5, 3, 33, 65)                                     # the first size on a wider group
    C["e257"] = _random(6, 2, 9, 257)                                       # past 256 lanes: the element loop strides
    C["full"] = _random(7, 2, 64, 1024)
    ob = _random(8, 2, 2, 1024, world=0.0)                                  # every element on body 0: the longest owned sum
    flip = torch.rand(2, 1024, generator=torch.Generator().manual_seed(80)) < 0.5
    ob["b1"] = torch.where(flip | (ob["kind"] == 3), torch.zeros_like(ob["b1"]), torch.full_like(ob["b1"], -1))
    ob["b2"] = torch.where(ob["b1"] == 0, torch.full_like(ob["b2"], -1), torch.zeros_like(ob["b2"]))
    ob["a1"] = torch.where((ob["b1"] < 0).unsqueeze(-1), ob["a1"] * 6.0, ob["a1"])
    ob["a2"] = torch.where((ob["b2"] < 0).unsqueeze(-1), ob["a2"] * 6.0, ob["a2"])
    C["one_body"] = ob
    un = _random(9, 3, 8, 5, world=0.3)                                     # bodies 3.. have no element
    un["b1"] = torch.where(un["b1"] >= 0, un["b1"] % 3, un["b1"])
    un["b2"] = torch.where(un["b2"] >= 0, (un["b1"].clamp(min=0) + 1 + un["b2"] % 2) % 3, un["b2"])
    C["untouched"] = un
    inv = _random(10, 3, 4, 16)
    nb = 4
    forms = [(0, 0, 1), (7, 0, 1), (-1, 0, 1), (1, nb, 1), (1, 0, nb), (1, -2, 1), (2, 1, -5), (2, 2, 2), (1, 1, 1), (1, -1, -1),
             (2, -1, -1), (3, -1, 0), (3, nb, 0)]
    for s in range(3):
        for e, (kd, i, j) in enumerate(forms):
            _set(inv, s, e, kd, i, j)
    for s in range(2):                                                      # L == 0 exactly: a world anchor at the centre of a body
        _set(inv, s, 13, 1, -1, 2)                                          # whose own anchor is its centre
        inv["a1"][s, 13] = inv["p"][s, 2, 1:]
        inv["a2"][s, 13] = 0.0
        _set(inv, s, 14, 1, 0, 3)                                           # (valid ones among them)
        _set(inv, s, 15, 3, 1, 99)                                          # (a drag's b2 is ignored)
    for e in (13, 14, 15):                                                  # scene 2: nothing valid at all
        _set(inv, 2, e, 0, 0, 1)
    C["invalid"] = inv
    sat = _random(11, 3, 6, 40)
    raw = forces_host(sat)["raw"].abs()
    e = torch.arange(40).unsqueeze(0).expand(3, 40)
    sat["limit"] = torch.where(e % 2 == 0, 0.5 * raw + 1e-3, torch.where(e % 4 == 1, torch.full_like(raw, INF), 2.0 * raw + 1.0))
    C["saturated"] = sat
    C["per_scene"] = _random(12, 6, 5, 7, kinds=(0, 1, 1, 2, 3), world=0.3)
    return C


_CASES, _REFS = {}, {}


def case(name):
    if not _CASES:
        _CASES.update(_build())
    return _CASES[name]


def reference(name):
    """The mirror's outputs for case `name` and `grads`: d sum(f64 * g_f) / d leaf for every leaf of LEAVES (float64)."""
    if name not in _REFS:
        c = case(name)
        leaves = {n: c[n].to(F64).clone().requires_grad_(True) for n in LEAVES}
        out = forces_host(c, leaves)
        grads = torch.autograd.grad((out["f64"] * c["g_f"].to(F64)).sum(), [leaves[n] for n in LEAVES], allow_unused=True)
        out = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
        out["grads"] = {n: (torch.zeros_like(leaves[n]) if g is None else g).detach() for n, g in zip(LEAVES, grads)}
        _REFS[name] = out
    return _REFS[name]
