"""Contact reports: which bodies touch and how hard - the impulses of a solve per body, per body pair and per joint.

Every solve writes the contact multipliers `z` and the joint multipliers `y`.  At a solution (lcp/solvers/pdipm.py:82-85 with the LCP of
physics/engines.py:31-32,52-76)

    M (v_new - v) - dt f  =  G^T z  +  Je^T y

the first term the contact impulse on every body coordinate, the second the joint impulse.  ONE launch of `lcp_contact_report_f32`
(lcp_report.hip; include/lcp_hip.h, "contact reports", has the rule) turns `z`, `y` and the records the solve consumed into

    rep = contact_report(world.contacts, out["z"], count=world.contacts.count, y=out["y"], Je=world.Je, pairs=PairSet.all_pairs(nb, B).to(dev))
    rep.body_impulse  [B,nb,3] f32   (torque, x, y) the body receives from all its contacts
    rep.body_normal   [B,nb]   f32   the sum of the normal multipliers of the records that name the body
    rep.body_touching [B,nb]   i32   how many of them exceed `min_impulse`
    rep.joint_impulse [B,nb,3] f32   Je^T y
    rep.pair_impulse  [B,P,3]  f32   what `first` receives from `second`, the torque about `first`'s centre
    rep.pair_normal   [B,P]    f32, rep.pair_contacts [B,P] i32

The records a solve consumed are overwritten by the detection that follows it, so a world reports from inside its step:
`ContactWorld(..., report=True | PairSet)` fills the persistent `world.report` once per step.  An impulse divided by `world.dt` is the
mean force over the step.  No CPU fallback.

No gradient is defined: every backward solves with the right-hand side (dl_dx, 0, 0, 0), and a cotangent on `z` or `y` would reach into
every solver family.  What a loss usually needs is there already: the body-space net constraint impulse `Mdiag (v_new - v) - dt f` is
differentiable through recorded steps, and equals `body_impulse + joint_impulse`.
"""
from dataclasses import dataclass, fields

import torch

from .. import _lib

MAX_PAIRS = 1024
_INTS = ("body_touching", "pair_contacts")


@dataclass
class ContactReport:
    """The seven tensors of a report (module docstring); `P` is 0 for a report without pairs."""
    body_impulse: torch.Tensor
    body_normal: torch.Tensor
    body_touching: torch.Tensor
    joint_impulse: torch.Tensor
    pair_impulse: torch.Tensor
    pair_normal: torch.Tensor
    pair_contacts: torch.Tensor

    @staticmethod
    def zeros(B, nb, P, device):
        """A report of zeros for B scenes of nb bodies and P pairs."""
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        i = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
        return ContactReport(f(B, nb, 3), f(B, nb), i(B, nb), f(B, nb, 3), f(B, P, 3), f(B, P), i(B, P))

    @property
    def P(self):
        return self.pair_normal.shape[1]

    def to(self, device):
        return ContactReport(*[getattr(self, f.name).to(device) for f in fields(self)])

    def zero_(self):
        for f in fields(self):
            getattr(self, f.name).zero_()
        return self

    def accumulate_(self, other):
        """Fold another report of the same interval in, in place: the impulses add, the counts keep the larger."""
        for f in fields(self):
            mine, theirs = getattr(self, f.name), getattr(other, f.name)
            if f.name in _INTS:
                torch.maximum(mine, theirs, out=mine)
            else:
                mine.add_(theirs)
        return self


def contact_report(frame, z, count=None, y=None, Je=None, pairs=None, min_impulse=0.0, active=None, out=None):
    """The report of one solve.  `frame`: the `contacts.ContactBuffers` the solve consumed; `z` [B,4 maxc] f32 and `y` [B,e] f32 its
    multipliers, `Je` [B,e,3 nb] f32 its joint Jacobian (`y` or `Je` None: no joint impulse).  `count` [B] i32: the records of every
    scene (None: all `maxc`, the fused step); `active` [B] i32: scenes with 0 report nothing (None: all active).  `pairs`: a
    `proximity.PairSet`, of which only `first` and `second` are read (None: no pair part).  `min_impulse`: the threshold of the two
    counts.  `out`: the `ContactReport` to write (every element is overwritten).  The tensors carry no gradient."""
    B, maxc = frame.c_i1.shape
    nb = frame.p_out.shape[1] if out is None else out.body_normal.shape[1]
    dev = z.device
    for name in ("c_n", "c_p1", "c_p2"):
        _lib.require_gpu_tensor(getattr(frame, name), name, torch.float32)
    for name in ("c_i1", "c_i2"):
        _lib.require_gpu_tensor(getattr(frame, name), name, torch.int32)
    _lib.require_gpu_tensor(z, "z", torch.float32)
    if tuple(z.shape) != (B, 4 * maxc):
        raise ValueError("z must be [%d,%d] (got %s)" % (B, 4 * maxc, tuple(z.shape)))
    for name, t in (("count", count), ("active", active)):
        if t is not None and tuple(_lib.require_gpu_tensor(t, name, torch.int32).shape) != (B,):
            raise ValueError("%s must be [%d] (got %s)" % (name, B, tuple(t.shape)))
    e = 0
    if y is not None and Je is not None and Je.numel():
        e = Je.shape[1]
        _lib.require_gpu_tensor(y, "y", torch.float32)
        _lib.require_gpu_tensor(Je, "Je", torch.float32)
        if tuple(Je.shape) != (B, e, 3 * nb) or tuple(y.shape) != (B, e):
            raise ValueError("Je must be [%d,e,%d] and y [%d,e] (got %s and %s)" % (B, 3 * nb, B, tuple(Je.shape), tuple(y.shape)))
    P = 0
    if pairs is not None:
        P = pairs.first.shape[1]
        _lib.require_gpu_tensor(pairs.first, "pairs.first", torch.int32)
        _lib.require_gpu_tensor(pairs.second, "pairs.second", torch.int32)
        if tuple(pairs.first.shape) != (B, P) or tuple(pairs.second.shape) != (B, P):
            raise ValueError("pairs are for %s scenes x pairs, the frame has %d scenes" % (tuple(pairs.first.shape), B))
    if out is None:
        out = ContactReport.zeros(B, nb, P, dev)
    for f in fields(out):
        t = _lib.require_gpu_tensor(getattr(out, f.name), "out." + f.name, torch.int32 if f.name in _INTS else torch.float32)
        if t.shape[0] != B or t.shape[1] != (P if f.name.startswith("pair") else nb):
            raise ValueError("out.%s is %s: not a report of %d scenes, %d bodies, %d pairs" % (f.name, tuple(t.shape), B, nb, P))
    ptr = _lib.ptr
    pair_ptr = lambda t: ptr(t) if P else None
    with _lib.on_device(dev):
        rc = _lib.load().lcp_contact_report_f32(
            B, nb, maxc, e, P, ptr(count), ptr(active), ptr(frame.c_n), ptr(frame.c_p1), ptr(frame.c_p2), ptr(frame.c_i1),
            ptr(frame.c_i2), ptr(z), ptr(y) if e else None, ptr(Je) if e else None,
            pair_ptr(pairs.first if P else None), pair_ptr(pairs.second if P else None), float(min_impulse),
            ptr(out.body_impulse), ptr(out.body_normal), ptr(out.body_touching), ptr(out.joint_impulse),
            pair_ptr(out.pair_impulse), pair_ptr(out.pair_normal), pair_ptr(out.pair_contacts), _lib.stream_ptr(dev))
    _lib.check(rc, "lcp_contact_report_f32")
    return out
