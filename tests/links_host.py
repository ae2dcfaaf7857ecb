"""The mechanism links of lcp_links.hip (include/lcp_hip.h, "mechanism links") restated as plain float64 torch operations on the CPU: the
yardstick of tests/test_hip_links.py, checked on its own by tests/test_links_host.py.

The mirror knows the POSITION-level functions only: `constraints(c)` is C(p) per row, and `jacobian(c)` differentiates it with autograd,
so it shares no formula with the kernel's closed forms (`closed_form(c)` restates the header's table for tests/test_links_host.py, which
compares the two).  The gradients of sum(Je * gJe) to the pose, the anchors and the angles are autograd through that Jacobian.

The seeded case table is generated once per process; `case(name)` hands out its tensors (do not modify them) and `reference(name)` the
mirror's Jacobian `Je` [B,el,3nb] f64 (link rows only), the mask `struct` of the entries a link can fill, and `grads`."""
import math

import torch

F64, F32, I32 = torch.float64, torch.float32, torch.int32
NONE, DISTANCE, SLOT, PRISMATIC = 0, 1, 2, 3
ROWS = {NONE: 0, DISTANCE: 1, SLOT: 1, PRISMATIC: 2}
LINK_ARRAYS = ("kind", "first", "second", "a1", "a2", "phi")
LEAVES = ("p", "a1", "a2", "phi")                                        # the backward's outputs, in the C entry's order
COINCIDENT = 1e-12
# (B, nb, L) = (1,2,1) of each kind; (3,5,7) mixed; (70,3,1) and (2,8,70) cross a wavefront whichever way lanes are grouped
CASE_NAMES = ("one_distance", "one_slot", "one_prismatic", "mixed", "many_scenes", "many_links", "invalid")


def _rot(th, a):
    c, s = torch.cos(th), torch.sin(th)
    return torch.stack([c * a[..., 0] - s * a[..., 1], s * a[..., 0] + c * a[..., 1]], -1)


def el_of(kind):
    """The rows of scene 0's kinds."""
    return sum(ROWS.get(int(k), 0) for k in kind[0].tolist())


def valid_links(c):
    """[B,L]: the links whose indices the kernel accepts (the others keep their rows, all zero)."""
    nb = c["p"].shape[1]
    f, s = c["first"], c["second"]
    return (f >= 0) & (f < nb) & (s >= -1) & (s < nb) & (f != s)


def constraints(c, leaves=None):
    """C(p) per row [B,el] (constants left out: they drop out of the Jacobian), and [B,el] `live`: the rows that are not zeroed (an
    invalid link's, a rod's between coincident anchors)."""
    p, a1, a2, phi = leaves if leaves is not None else (c["p"], c["a1"], c["a2"], c["phi"])
    B, nb = p.shape[0], p.shape[1]
    ok = valid_links(c)
    ar = torch.arange(B).unsqueeze(1)
    b1, b2 = c["first"].long().clamp(0, nb - 1), c["second"].long().clamp(0, nb - 1)
    world = (c["second"] < 0)
    p1, p2 = p[ar, b1], p[ar, b2]
    w1 = p1[..., 1:] + _rot(p1[..., 0], a1)
    rot2 = torch.where(world, torch.zeros_like(p2[..., 0]), p2[..., 0])
    w2 = torch.where(world.unsqueeze(-1), a2, p2[..., 1:] + _rot(rot2, a2))
    far = ((w2 - w1) ** 2).sum(-1).detach().sqrt() >= COINCIDENT
    dist = torch.where(far.unsqueeze(-1), w2 - w1, torch.ones_like(w1)).norm(dim=-1)                          # (no sqrt'(0) in the graph)
    th = rot2 + phi
    slot = (torch.stack([-torch.sin(th), torch.cos(th)], -1) * (w1 - w2)).sum(-1)
    ang = p1[..., 0] - rot2
    cols, live = [], []
    for l, k in enumerate(int(x) for x in c["kind"][0].tolist()):
        if k == DISTANCE:
            cols.append(dist[:, l]); live.append(ok[:, l] & far[:, l])
        elif k in (SLOT, PRISMATIC):
            cols.append(slot[:, l]); live.append(ok[:, l])
            if k == PRISMATIC:
                cols.append(ang[:, l]); live.append(ok[:, l])
    if not cols:
        return p.new_zeros(B, 0), torch.zeros(B, 0, dtype=torch.bool)
    live = torch.stack(live, 1)
    return torch.stack(cols, 1) * live.to(F64), live


def jacobian(c, leaves=None, create_graph=False):
    """Je [B,el,3nb] f64 = dC/dp by autograd, row by row (scenes do not interact: the gradient of a row's sum over the batch)."""
    if leaves is None:
        leaves = (c["p"].clone().requires_grad_(True), c["a1"], c["a2"], c["phi"])
    p = leaves[0]
    C, _ = constraints(c, leaves)
    B, nb = p.shape[0], p.shape[1]
    rows = []
    for r in range(C.shape[1]):
        (g,) = torch.autograd.grad(C[:, r].sum(), p, create_graph=create_graph, retain_graph=True, allow_unused=True)
        rows.append(torch.zeros_like(p) if g is None else g)
    return torch.stack(rows, 1).reshape(B, len(rows), 3 * nb) if rows else p.new_zeros(B, 0, 3 * nb)


def structure(c):
    """[B,el,3nb] bool: the six columns each row's link may fill (everything else is a structural zero)."""
    B, nb = c["p"].shape[0], c["p"].shape[1]
    el = el_of(c["kind"])
    m = torch.zeros(B, el, nb, dtype=torch.bool)
    ok = valid_links(c)
    row = 0
    for l, k in enumerate(int(x) for x in c["kind"][0].tolist()):
        for q in range(ROWS.get(k, 0)):
            for b in range(B):
                if ok[b, l]:
                    m[b, row + q, int(c["first"][b, l])] = True
                    if int(c["second"][b, l]) >= 0:
                        m[b, row + q, int(c["second"][b, l])] = True
        row += ROWS.get(k, 0)
    return m.unsqueeze(-1).expand(B, el, nb, 3).reshape(B, el, 3 * nb)


def closed_form(c):
    """The table of include/lcp_hip.h, entry by entry, [B,el,3nb] f64 - what the kernel computes; compared with `jacobian` on the CPU."""
    p, a1, a2, phi = c["p"], c["a1"], c["a2"], c["phi"]
    B, nb = p.shape[0], p.shape[1]
    cross = lambda a, b: a[0] * b[1] - a[1] * b[0]
    Je = torch.zeros(B, el_of(c["kind"]), 3 * nb, dtype=F64)
    ok = valid_links(c)
    for b in range(B):
        row = 0
        for l, k in enumerate(int(x) for x in c["kind"][0].tolist()):
            n_rows = ROWS.get(k, 0)
            if n_rows and bool(ok[b, l]):
                i, j = int(c["first"][b, l]), int(c["second"][b, l])
                r1 = _rot(p[b, i, 0], a1[b, l])
                w1 = p[b, i, 1:] + r1
                r2 = _rot(p[b, j, 0], a2[b, l]) if j >= 0 else torch.zeros(2, dtype=F64)
                w2 = p[b, j, 1:] + r2 if j >= 0 else a2[b, l]
                rot2 = p[b, j, 0] if j >= 0 else torch.zeros((), dtype=F64)
                if k == DISTANCE:
                    d = w2 - w1
                    if float(d.norm()) >= COINCIDENT:
                        n = d / d.norm()
                        Je[b, row, 3 * i:3 * i + 3] = torch.stack([-cross(r1, n), -n[0], -n[1]])
                        if j >= 0:
                            Je[b, row, 3 * j:3 * j + 3] = torch.stack([cross(r2, n), n[0], n[1]])
                else:
                    t = _rot(rot2, torch.stack([-torch.sin(phi[b, l]), torch.cos(phi[b, l])]))
                    d = w1 - w2
                    Je[b, row, 3 * i:3 * i + 3] = torch.stack([cross(r1, t), t[0], t[1]])
                    if j >= 0:
                        Je[b, row, 3 * j:3 * j + 3] = torch.stack([-cross(r2 + d, t), -t[0], -t[1]])
                    if k == PRISMATIC:
                        Je[b, row + 1, 3 * i] = 1.0
                        if j >= 0:
                            Je[b, row + 1, 3 * j] = -1.0
            row += n_rows
    return Je


# ----------------------------------------------------------------------------------------------------------------- cases
def _random_case(seed, B, nb, links, per_scene=False):
    """`links`: [(kind, first, second)] shared by all scenes; `per_scene`: scene s turns the indices of bodies 0 .. nb - 2 by s (the
    last body, and the world, stay)."""
    g = torch.Generator().manual_seed(seed)
    L = len(links)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=F64)
    p = torch.cat([6.0 * rnd(B, nb, 1) - 3.0, 40.0 * rnd(B, nb, 2) - 20.0], -1)
    col = lambda k: torch.tensor([ln[k] for ln in links], dtype=I32).reshape(1, L).repeat(B, 1)
    kind, first, second = col(0), col(1), col(2)
    if per_scene:
        turn = lambda b: torch.where((b >= 0) & (b < nb - 1), (b + torch.arange(B, dtype=I32).unsqueeze(1)) % (nb - 1), b)
        first, second = turn(first), turn(second)
    c = dict(kind=kind, first=first.contiguous(), second=second.contiguous(), a1=4.0 * rnd(B, L, 2) - 2.0, a2=4.0 * rnd(B, L, 2) - 2.0,
             phi=2.0 * math.pi * rnd(B, L) - math.pi, p=p)
    c["g_Je"] = torch.randn(B, el_of(kind), 3 * nb, generator=g, dtype=F64).to(F32)
    return c


def _build():
    cases = {"one_distance": _random_case(11, 1, 2, [(DISTANCE, 0, 1)]),
             "one_slot": _random_case(12, 1, 2, [(SLOT, 1, 0)]),
             "one_prismatic": _random_case(13, 1, 2, [(PRISMATIC, 0, 1)])}
    # body 1 carries three links, body 4 none, two links end in the world; every scene names other bodies
    cases["mixed"] = _random_case(14, 3, 5, [(DISTANCE, 0, 1), (SLOT, 1, -1), (PRISMATIC, 2, 1), (DISTANCE, 3, -1), (SLOT, 2, 3),
                                             (PRISMATIC, 0, 3), (DISTANCE, 2, 0)], per_scene=True)
    cases["many_scenes"] = _random_case(15, 70, 3, [(PRISMATIC, 2, 0)])
    kinds = (DISTANCE, SLOT, PRISMATIC)
    cases["many_links"] = _random_case(16, 2, 8, [(kinds[l % 3], l % 8, (l * 3 + 1) % 8 if l % 5 else -1) for l in range(70)])
    # kind 0 (no rows), an unknown kind (no rows), indices out of range and first == second (zero rows), a rod between coincident
    # anchors (a zero row) - between live links; no live link names body 2
    inv = _random_case(17, 2, 4, [(DISTANCE, 0, 1), (NONE, 0, 1), (SLOT, 7, 1), (PRISMATIC, 1, 1), (DISTANCE, 1, -1), (9, 0, 1),
                                  (SLOT, 0, -2), (PRISMATIC, -1, 0), (DISTANCE, 3, 0), (SLOT, 3, 1)])
    inv["a2"][:, 4] = inv["p"][:, 1, 1:] + _rot(inv["p"][:, 1, 0], inv["a1"][:, 4])      # link 4: the world point is body 1's anchor
    cases["invalid"] = inv
    return cases


_CASES, _REFS = None, {}


def case(name):
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES[name]


def reference(name):
    """dict(Je [B,el,3nb] f64, struct [B,el,3nb] bool, live [B,el] bool, grads {p, a1, a2, phi} of sum(Je * g_Je))."""
    if name not in _REFS:
        c = case(name)
        leaves = tuple(c[n].clone().requires_grad_(True) for n in LEAVES)
        Je = jacobian(c, leaves, create_graph=True)
        _, live = constraints(c)
        loss = (Je * c["g_Je"].double()).sum()
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
        _REFS[name] = dict(Je=Je.detach(), struct=structure(c), live=live,
                           grads={n: (torch.zeros_like(c[n]) if g is None else g.detach()) for n, g in zip(LEAVES, grads)})
    return _REFS[name]
