"""The contact report of lcp_report.hip (include/lcp_hip.h, "contact reports") restated as plain float64 torch operations on the CPU: the
yardstick of tests/test_hip_contact_report.py, checked on its own by tests/test_contact_report_host.py.

`report_host(case, min_impulse=0.0)` returns, for every float output `name` of the entry, `name` (the unrounded float64 sum) and
`S_name` (the sum of the magnitudes of the terms that enter each entry - for the impulses the terms of G^T z row by row, so the two
friction multipliers of a record count separately, not their difference), and the two integer outputs.  A case is a dict of CPU tensors
    c_n, c_p1, c_p2 [B,maxc,2] f32, c_i1, c_i2 [B,maxc] i32, z [B,4 maxc] f32, count [B] i32 | None, active [B] i32 | None,
    y [B,e] f32 | None, Je [B,e,3 nb] f32 | None, first, second [B,P] i32 | None, nb
The seeded table is generated once per process; `case(name)` hands out its tensors (do not modify them), `reference(name)` the mirror's
outputs at min_impulse = 0."""
import torch

F64, F32, I32 = torch.float64, torch.float32, torch.int32
FLOATS = ("body_impulse", "body_normal", "joint_impulse", "pair_impulse", "pair_normal")
INTS = ("body_touching", "pair_contacts")
OUTPUTS = ("body_impulse", "body_normal", "body_touching", "joint_impulse", "pair_impulse", "pair_normal", "pair_contacts")
CASE_NAMES = ("small", "edge65", "bodies64", "full", "ragged", "invalid", "nojoints", "nopairs")


def dims(c):
    """(B, nb, maxc, e, P) of a case."""
    B, maxc = c["c_i1"].shape
    return B, c["nb"], maxc, (0 if c["Je"] is None or c["y"] is None else c["Je"].shape[1]), (0 if c["first"] is None else c["first"].shape[1])


def record_impulses(c):
    """Per record: zn [B,maxc], the impulse j [B,maxc,2], the torque on either body t1, t2 [B,maxc], `live` [B,maxc], the records
    the report reads (the first min(count, maxc) of an active scene), and A1, A2 [B,maxc,3], the magnitudes of the three rows' terms
    (|zn| |Jc| + (|z_f1| + |z_f2|) |Jf|) in what either body receives."""
    B, nb, maxc, _, _ = dims(c)
    z = c["z"].to(F64)
    zn = z[:, :maxc]
    fr = z[:, maxc:3 * maxc].reshape(B, maxc, 2)
    zt = fr[..., 0] - fr[..., 1]
    n, p1, p2 = c["c_n"].to(F64), c["c_p1"].to(F64), c["c_p2"].to(F64)
    d = torch.stack([n[..., 1], -n[..., 0]], -1)                              # left_orthogonal (utils.py:99-102)
    j = zn.unsqueeze(-1) * n + zt.unsqueeze(-1) * d
    cross = lambda a, b: a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]        # cross_2d (utils.py:93-96)
    count = torch.full((B,), maxc, dtype=torch.long) if c["count"] is None else c["count"].long().clamp(0, maxc)
    live = torch.arange(maxc).unsqueeze(0) < count.unsqueeze(1)
    if c["active"] is not None:
        live = live & (c["active"] != 0).unsqueeze(1)
    zf = fr.abs().sum(-1)
    mags = lambda p: torch.cat([(zn.abs() * cross(p, n).abs() + zf * cross(p, d).abs()).unsqueeze(-1),
                                zn.abs().unsqueeze(-1) * n.abs() + zf.unsqueeze(-1) * d.abs()], -1)
    return zn, j, cross(p1, j), -cross(p2, j), live, mags(p1), mags(p2)


def report_host(c, min_impulse=0.0):
    B, nb, maxc, e, P = dims(c)
    zn, j, t1, t2, live, A1, A2 = record_impulses(c)
    i1, i2 = c["c_i1"].long(), c["c_i2"].long()
    W1 = torch.cat([t1.unsqueeze(-1), j], -1)                                 # what body i1 receives: (cross(p1, j), j)
    W2 = torch.cat([t2.unsqueeze(-1), -j], -1)                                # what body i2 receives: (-cross(p2, j), -j)
    pushing = zn > float(min_impulse)
    out = {}

    def collect(on1, on2, stem):
        """on1 / on2 [B,maxc,K]: record c gives W1 / W2 to slot k."""
        a, b = on1.to(F64), on2.to(F64)
        imp = torch.einsum("bck,bcq->bkq", a, W1) + torch.einsum("bck,bcq->bkq", b, W2)
        S = torch.einsum("bck,bcq->bkq", a, A1) + torch.einsum("bck,bcq->bkq", b, A2)
        named = on1 | on2
        out[stem + "_impulse"], out["S_" + stem + "_impulse"] = imp, S
        out[stem + "_normal"] = torch.einsum("bck,bc->bk", named.to(F64), zn)
        out["S_" + stem + "_normal"] = torch.einsum("bck,bc->bk", named.to(F64), zn.abs())
        return (named & pushing.unsqueeze(-1)).sum(1).to(I32)

    bodies = torch.arange(nb).reshape(1, 1, nb)
    lv = live.unsqueeze(-1)
    out["body_touching"] = collect((i1.unsqueeze(-1) == bodies) & lv, (i2.unsqueeze(-1) == bodies) & lv, "body")
    if P:
        f, s = c["first"].long().unsqueeze(1), c["second"].long().unsqueeze(1)           # [B,1,P]
        good = (f != s) & (f >= 0) & (f < nb) & (s >= 0) & (s < nb)
        a1, a2 = i1.unsqueeze(-1), i2.unsqueeze(-1)
        out["pair_contacts"] = collect((a1 == f) & (a2 == s) & good & lv, (a1 == s) & (a2 == f) & good & lv, "pair")
    else:
        out["pair_impulse"], out["S_pair_impulse"] = torch.zeros(B, 0, 3, dtype=F64), torch.zeros(B, 0, 3, dtype=F64)
        out["pair_normal"], out["S_pair_normal"] = torch.zeros(B, 0, dtype=F64), torch.zeros(B, 0, dtype=F64)
        out["pair_contacts"] = torch.zeros(B, 0, dtype=I32)
    if e:
        terms = c["Je"].to(F64) * c["y"].to(F64).unsqueeze(-1)                           # [B,e,3 nb]
        if c["active"] is not None:
            terms = terms * (c["active"] != 0).to(F64).reshape(B, 1, 1)
        out["joint_impulse"], out["S_joint_impulse"] = terms.sum(1).reshape(B, nb, 3), terms.abs().sum(1).reshape(B, nb, 3)
    else:
        out["joint_impulse"], out["S_joint_impulse"] = torch.zeros(B, nb, 3, dtype=F64), torch.zeros(B, nb, 3, dtype=F64)
    return out


def within_bound(got, ref, name):
    """|got - ref| <= 2^-24 |ref| + 1e-12 S per entry: one float32 rounding plus the float64 sum (the force elements' bound).  Returns
    (ok, the largest ratio of error to bound)."""
    err = (got.to(F64) - ref[name]).abs()
    bound = 2.0 ** -24 * ref[name].abs() + 1e-12 * ref["S_" + name]
    ok = bool((err <= bound).all())
    worst = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    return ok, worst


# ------------------------------------------------------------------------------------------------------------- the cases
def _random(seed, B, nb, maxc, P, e, counts=True):
    """A seeded case: unit normals, arms of order 1, z >= 0, the two bodies of a record different members of [0, nb), pairs drawn at
    random (first != second), counts in [0, maxc]."""
    g = torch.Generator().manual_seed(seed)
    U = lambda lo, hi, *shape: (lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=F64))
    ang = U(0.0, 6.283185307179586, B, maxc)
    i1 = torch.randint(0, nb, (B, maxc), generator=g)
    i2 = (i1 + 1 + torch.randint(0, max(nb - 1, 1), (B, maxc), generator=g)) % nb
    z = torch.cat([U(0.0, 5.0, B, maxc), U(0.0, 2.0, B, 2 * maxc), U(0.0, 1.0, B, maxc)], 1)
    c = {"nb": nb, "c_n": torch.stack([torch.cos(ang), torch.sin(ang)], -1).to(F32), "c_p1": U(-2.0, 2.0, B, maxc, 2).to(F32),
         "c_p2": U(-2.0, 2.0, B, maxc, 2).to(F32), "c_i1": i1.to(I32), "c_i2": i2.to(I32), "z": z.to(F32),
         "count": torch.randint(0, maxc + 1, (B,), generator=g).to(I32) if counts else None, "active": None,
         "y": None, "Je": None, "first": None, "second": None}
    if e:
        c["y"] = (3.0 * torch.randn(B, e, generator=g, dtype=F64)).to(F32)
        c["Je"] = torch.randn(B, e, 3 * nb, generator=g, dtype=F64).to(F32)
    if P:
        f = torch.randint(0, nb, (B, P), generator=g)
        c["first"] = f.to(I32)
        c["second"] = ((f + 1 + torch.randint(0, max(nb - 1, 1), (B, P), generator=g)) % nb).to(I32)
    return c


def _build():
    C = {}
    C["small"] = _random(1, 5, 3, 4, 3, 3, counts=False)                      # several scenes per wavefront, a ragged last workgroup
    C["edge65"] = _random(2, 3, 5, 65, 10, 2)                                 # the first size on 128 lanes
    C["edge65"]["count"][0] = 65
    C["bodies64"] = _random(3, 3, 64, 16, 40, 5)                              # the most bodies
    C["bodies64"]["count"][0] = 16
    C["full"] = _random(4, 2, 64, 1024, 1024, 24)                             # the largest LDS
    C["full"]["count"] = torch.tensor([1024, 777], dtype=I32)
    rag = _random(5, 8, 6, 12, 15, 4)                                         # truncated and inactive scenes
    rag["count"] = torch.tensor([0, 1, 5, 12, 13, 15, 7, 3], dtype=I32)
    rag["active"] = torch.tensor([1, 1, 0, 1, 1, 7, 0, 1], dtype=I32)
    C["ragged"] = rag
    inv = _random(6, 3, 4, 8, 8, 2, counts=False)
    nb = 4
    inv["c_i1"][:, 0], inv["c_i2"][:, 1] = -1, -1                             # one side outside [0, nb): the other still receives
    inv["c_i1"][:, 2], inv["c_i2"][:, 3] = nb, nb
    inv["c_i1"][:, 4], inv["c_i2"][:, 4] = -1, nb                             # both sides outside: nothing at all
    for q, (f, s) in enumerate([(1, 1), (-1, 2), (2, -1), (nb, 0), (0, nb), (0, 1), (1, 0), (2, 3)]):
        inv["first"][:, q], inv["second"][:, q] = f, s
    inv["c_i1"][:, 5], inv["c_i2"][:, 5] = 0, 1                               # (records between the valid pairs, either way round)
    inv["c_i1"][:, 6], inv["c_i2"][:, 6] = 1, 0
    inv["c_i1"][:, 7], inv["c_i2"][:, 7] = 3, 2
    C["invalid"] = inv
    C["nojoints"] = _random(7, 3, 4, 8, 6, 0)
    C["nopairs"] = _random(8, 3, 4, 8, 0, 3)
    return C


_CASES, _REFS = {}, {}


def case(name):
    if not _CASES:
        _CASES.update(_build())
    return _CASES[name]


def reference(name):
    if name not in _REFS:
        _REFS[name] = report_host(case(name))
    return _REFS[name]


def some_zn(name):
    """One of the case's own normal multipliers (a live record's): the threshold the strict comparison is tested at."""
    c = case(name)
    zn, live = record_impulses(c)[0], record_impulses(c)[4]
    vals = zn[live]
    return float(vals.sort().values[vals.numel() // 2])
