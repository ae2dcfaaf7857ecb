"""Mechanism links on the device: rods, slots and sliders between bodies as equality rows of the step, differentiable.

The reference holds a scene together with a revolute `Joint`, a `FixedJoint` and the world-axis constraints (`physics/constraints.py`);
a rod of fixed length between two anchors, a pin riding in a slot of another body or a slider cannot be built from them, and a stiff
spring is no substitute (`ForceSet` couples explicitly: `dt sqrt(k / m) < 2`).  A `LinkSet` adds those three as rows of `Je`.  Anchors
and axes are stored in the bodies' frames, so a link's rows are a pure function of the pose - there is no state to advance.  ONE launch
of `lcp_link_jacobian_f64` (lcp_links.hip) writes the base rows (a constant `Je`, or a `JointSet`'s) and the link rows of every scene
into one matrix, and ONE launch of `lcp_link_jacobian_backward_f64` is the backward to the pose, the anchors and the angles:

    ls = LinkSet.from_list([("distance", 1, None, (0.0, 0.0), (50.0, 80.0)),          # a rod from body 1's centre to a world point
                            ("slot", 2, 1, (0.0, 0.0), (0.0, 0.0), 0.3),              # body 2's centre rides a line fixed in body 1
                            ("prismatic", 3, None, (0.0, 0.0), (10.0, 20.0), 0.0)],   # a slider on a world rail
                           p0, B).to(dev)
    world = ContactWorld(geom, p, v, Mdiag, f, rest, fric, links=ls)         # alone, with a constant Je, or with a JointSet
    Je = link_jacobian(ls, world.p)                                          # [B,e,3nb] float32, differentiable

Every link is a position-level function C(p) and its rows are dC/dp (include/lcp_hip.h, "mechanism links", has the table).  The
constraint is enforced at VELOCITY level (`Je v_new = 0`), as the reference's joints are: the position drifts the way a revolute
`Joint`'s does and is corrected by nothing beyond what `post_stab` already does - `LinkSet.residual(p)` measures it.  Closed loops whose
rows are linearly dependent are not detected: the solvers do not pivot.  No CPU fallback.
"""
from dataclasses import dataclass, fields

import torch

from .. import _lib

NONE, DISTANCE, SLOT, PRISMATIC = 0, 1, 2, 3
ROWS = {NONE: 0, DISTANCE: 1, SLOT: 1, PRISMATIC: 2}
_NAMES = {"distance": DISTANCE, "slot": SLOT, "prismatic": PRISMATIC}
MAX_LINKS = 256
COINCIDENT = 1e-12                                         # a rod between anchors closer than this has no direction
_INTS = ("kind", "first", "second")
_LEAVES = ("a1", "a2", "phi")                              # the parameters with a gradient, in the kernel's order


def _rot(th, a):
    """R(th) a for th [...] and a [...,2]."""
    c, s = torch.cos(th), torch.sin(th)
    return torch.stack([c * a[..., 0] - s * a[..., 1], s * a[..., 0] + c * a[..., 1]], -1)


@dataclass
class LinkSet:
    """The links of B scenes, L per scene: `kind`, `first`, `second` [B,L] int32 (`second` -1: the world); `a1`, `a2` [B,L,2] f64
    (anchors in the bodies' frames; the world's is a world point); `phi` [B,L] f64 (the angle of a slot's line in `second`'s frame:
    the line runs along R(rot_2) (cos phi, sin phi)); `rest` [B,e] f64, per row what `residual` subtracts - a rod's length and a
    slider's relative angle, measured at the creation pose; `e` the rows, those of scene 0's kinds (one kind list for all scenes)."""
    kind: torch.Tensor
    first: torch.Tensor
    second: torch.Tensor
    a1: torch.Tensor
    a2: torch.Tensor
    phi: torch.Tensor
    rest: torch.Tensor
    e: int

    def __post_init__(self):
        if self.kind.dim() != 2:
            raise ValueError("links.kind must be [B,L] (got %s)" % (tuple(self.kind.shape),))
        B, L = self.kind.shape
        want = {"a1": (B, L, 2), "a2": (B, L, 2), "rest": (B, self.e)}
        for f in fields(self):
            if f.name == "e":
                continue
            t = getattr(self, f.name)
            if tuple(t.shape) != want.get(f.name, (B, L)):
                raise ValueError("links.%s must be %s (got %s)" % (f.name, want.get(f.name, (B, L)), tuple(t.shape)))
            dt = torch.int32 if f.name in _INTS else torch.float64
            if t.dtype != dt:
                raise ValueError("links.%s must be %s (got %s)" % (f.name, dt, t.dtype))
        if L < 1 or L > MAX_LINKS:
            raise ValueError("1 to %d links per scene (got %d)" % (MAX_LINKS, L))

    @property
    def B(self):
        return self.kind.shape[0]

    @property
    def L(self):
        return self.kind.shape[1]

    def to(self, device):
        """The set on `device`.  The float arrays move through autograd: what required grad still leads back to its leaf."""
        return LinkSet(*[getattr(self, f.name).to(device).contiguous() for f in fields(self) if f.name != "e"], self.e)

    @staticmethod
    def from_list(links, p0, B=1, check=True):
        """`links`: a list of
            ("distance", b1, b2_or_None, anchor1, anchor2)
            ("slot", b1, b2_or_None, anchor1, anchor2, phi)
            ("prismatic", b1, b2_or_None, anchor1, anchor2, phi)
        the same in all B scenes; `p0` [nb,3] (or [B,nb,3]) the poses the links are created at (only `rest` is measured there).  Anchors
        are in the bodies' frames; with `None` for the second body the second anchor is a world point.  Anchors and angles are numbers or
        tensors (anchors [2] or [B,2], angles 0-dim or [B]); a tensor that requires grad stays connected.  `check`: coincident rod
        anchors, equal bodies and indices outside `p0` are refused here, on the host."""
        p0 = torch.as_tensor(p0, dtype=torch.float64)
        if p0.dim() == 2:
            p0 = p0.unsqueeze(0).expand(int(B), -1, -1)
        B, nb = p0.shape[0], p0.shape[1]
        if not links:
            raise ValueError("a LinkSet needs at least one link")

        def col(x, tail=()):
            t = torch.as_tensor(x, dtype=torch.float64) if not isinstance(x, torch.Tensor) else x.to(torch.float64)
            if tuple(t.shape) == tuple(tail):
                t = t.unsqueeze(0).expand((B,) + tuple(tail))
            if tuple(t.shape) != (B,) + tuple(tail):
                raise ValueError("a value must be a number, a tensor of shape %s or one per scene (got %s)" % (tuple(tail), tuple(t.shape)))
            return t.to(p0.device)

        kinds, firsts, seconds, a1s, a2s, phis = [], [], [], [], [], []
        for ln in links:
            what = ln[0]
            if what not in _NAMES or len(ln) != (5 if what == "distance" else 6):
                raise ValueError("not a link: %r (kinds: %s)" % (ln, ", ".join(_NAMES)))
            b1, b2 = int(ln[1]), -1 if ln[2] is None else int(ln[2])
            if check and (not 0 <= b1 < nb or not -1 <= b2 < nb or b1 == b2):
                raise ValueError("%r: the first body must be one of the %d bodies, the second another one or None" % (ln, nb))
            kinds.append(_NAMES[what]); firsts.append(b1); seconds.append(b2)
            a1s.append(col(ln[3], (2,))); a2s.append(col(ln[4], (2,)))
            phis.append(col(0.0 if what == "distance" else ln[5]))
        ints = lambda xs: torch.tensor(xs, dtype=torch.int32, device=p0.device).reshape(1, -1).expand(B, -1).contiguous()
        kind, first, second = ints(kinds), ints(firsts), ints(seconds)
        a1, a2, phi = torch.stack(a1s, 1).contiguous(), torch.stack(a2s, 1).contiguous(), torch.stack(phis, 1).contiguous()
        e = sum(ROWS[k] for k in kinds)
        with torch.no_grad():
            rest = torch.zeros(B, e, dtype=torch.float64, device=p0.device)
            ls = LinkSet(kind, first, second, a1, a2, phi, rest, e)
            C = ls.residual(p0)                                            # (with rest 0: the functions themselves)
            row = 0
            for l, k in enumerate(kinds):
                if k == DISTANCE:
                    if check and bool((C[:, row] < COINCIDENT).any()):
                        raise ValueError("%r: the two anchors coincide at the creation pose - a rod needs a direction" % (links[l],))
                    rest[:, row] = C[:, row]
                elif k == PRISMATIC:
                    rest[:, row + 1] = C[:, row + 1]
                row += ROWS[k]
        return ls

    @staticmethod
    def concat(sets):
        """The links of several sets of the same B, one after the other."""
        sets = list(sets)
        if not sets or any(s.B != sets[0].B for s in sets):
            raise ValueError("concat needs sets of the same number of scenes")
        cat = lambda n: torch.cat([getattr(s, n) for s in sets], 1).contiguous()
        return LinkSet(*[cat(f.name) for f in fields(LinkSet) if f.name != "e"], sum(s.e for s in sets))

    def _kinds(self):
        """Scene 0's kinds as a list (one device read, then cached: the kinds never change)."""
        k = self.__dict__.get("_kind_list")
        if k is None:
            k = self.__dict__["_kind_list"] = [int(x) for x in self.kind[0].tolist()]
        return k

    def residual(self, p):
        """C(p) per row, [B,e] float64, minus `rest`: how far the pose `p` [B,nb,3] is from the positions the links were created at - a
        rod's length error, a slider's relative angle; a slot's row is the distance of `first`'s anchor from the line through `second`'s
        (`rest` 0).  Plain torch on `p`'s device, differentiable; a diagnostic - the step holds `Je v = 0` and nothing pulls C back."""
        B = p.shape[0]
        ar = torch.arange(B, device=p.device).unsqueeze(1)
        b1, b2 = self.first.long(), self.second.long()
        world = (b2 < 0).unsqueeze(-1)
        p1, p2 = p[ar, b1], p[ar, b2.clamp_min(0)]
        w1 = p1[..., 1:] + _rot(p1[..., 0], self.a1)
        rot2 = torch.where(world[..., 0], torch.zeros_like(p2[..., 0]), p2[..., 0])
        w2 = torch.where(world, self.a2, p2[..., 1:] + _rot(rot2, self.a2))
        th = rot2 + self.phi
        t = torch.stack([-torch.sin(th), torch.cos(th)], -1)
        dist = (w2 - w1).norm(dim=-1)
        slot = (t * (w1 - w2)).sum(-1)
        ang = p1[..., 0] - rot2
        cols = []
        for l, k in enumerate(self._kinds()):
            if k == DISTANCE:
                cols.append(dist[:, l])
            elif k in (SLOT, PRISMATIC):
                cols.append(slot[:, l])
                if k == PRISMATIC:
                    cols.append(ang[:, l])
        C = torch.stack(cols, 1) if cols else p.new_zeros(B, 0)
        return C - self.rest

    def _check(self, p, leaves=None):
        a1, a2, phi = leaves if leaves is not None else (self.a1, self.a2, self.phi)
        _lib.require_gpu_tensor(p, "p", torch.float64)
        if p.dim() != 3 or p.shape[0] != self.B or p.shape[2] != 3:
            raise ValueError("p must be [%d,nb,3] (got %s)" % (self.B, tuple(p.shape)))
        for n in _INTS:
            _lib.require_gpu_tensor(getattr(self, n), "links." + n, torch.int32)
        for n, t in zip(_LEAVES, (a1, a2, phi)):
            _lib.require_gpu_tensor(t, "links." + n, torch.float64)
        P = _lib.ptr
        return (P(self.kind), P(self.first), P(self.second), P(a1), P(a2), P(phi), P(p))

    def jacobian(self, p, Je_base=None, out=None, _leaves=None):
        """Je [B, e0 + e, 3nb] float32 at pose `p` [B,nb,3] float64: the rows of `Je_base` [B,e0,3nb] float32 (None: none), then the
        links' - one launch, no autograd (`link_jacobian` is the differentiable call).  `out`: the tensor to write (the plain step's
        persistent buffer; it must not be `Je_base`)."""
        ptrs = self._check(p, _leaves)
        B, nb = p.shape[0], p.shape[1]
        e0 = 0
        if Je_base is not None and Je_base.numel():
            _lib.require_gpu_tensor(Je_base, "Je_base", torch.float32)
            if Je_base.dim() != 3 or Je_base.shape[0] != B or Je_base.shape[2] != 3 * nb:
                raise ValueError("Je_base must be [%d,e0,%d] (got %s)" % (B, 3 * nb, tuple(Je_base.shape)))
            e0 = Je_base.shape[1]
        else:
            Je_base = None
        if out is None:
            out = torch.empty(B, e0 + self.e, 3 * nb, dtype=torch.float32, device=p.device)
        else:
            _lib.require_gpu_tensor(out, "out", torch.float32)
            if tuple(out.shape) != (B, e0 + self.e, 3 * nb):
                raise ValueError("out must be %s (got %s)" % ((B, e0 + self.e, 3 * nb), tuple(out.shape)))
            if Je_base is not None and out.data_ptr() == Je_base.data_ptr():
                raise ValueError("out must not be Je_base")
        with _lib.on_device(p.device):
            rc = _lib.load().lcp_link_jacobian_f64(B, nb, self.L, e0, self.e, *ptrs, _lib.ptr(Je_base), _lib.ptr(out),
                                                   _lib.stream_ptr(p.device))
        _lib.check(rc, "lcp_link_jacobian_f64")
        return out

    def jacobian_backward(self, p, gJe, want=(True, True, True, True), _leaves=None):
        """(g_p [B,nb,3], g_a1, g_a2 [B,L,2], g_phi [B,L]) float64 from d(loss)/dJe [B, e0 + e, 3nb]: the backward of the LINK rows of
        `jacobian()` at pose `p` - one launch of `lcp_link_jacobian_backward_f64`; `want`: which of the four to compute (None for the
        rest).  The cotangent of the base rows is `gJe[:, :e0]`, the caller's slice."""
        ptrs = self._check(p, _leaves)
        B, nb = p.shape[0], p.shape[1]
        gJe = _lib.require_gpu_tensor(gJe.to(torch.float32).contiguous(), "gJe", torch.float32)
        if gJe.dim() != 3 or gJe.shape[0] != B or gJe.shape[1] < self.e or gJe.shape[2] != 3 * nb:
            raise ValueError("gJe must be [%d, e0 + %d, %d] (got %s)" % (B, self.e, 3 * nb, tuple(gJe.shape)))
        shapes = ((B, nb, 3), (B, self.L, 2), (B, self.L, 2), (B, self.L))
        outs = [torch.empty(s, dtype=torch.float64, device=p.device) if w else None for s, w in zip(shapes, want)]
        if any(o is not None for o in outs):
            with _lib.on_device(p.device):
                rc = _lib.load().lcp_link_jacobian_backward_f64(B, nb, self.L, gJe.shape[1] - self.e, self.e, *ptrs, _lib.ptr(gJe),
                                                                *[_lib.ptr(o) for o in outs], _lib.stream_ptr(p.device))
            _lib.check(rc, "lcp_link_jacobian_backward_f64")
        return tuple(outs)


class _LinkJacobianFn(torch.autograd.Function):
    """Je = the combined matrix the kernel computed at pose `p` (`LinkSet.jacobian`; its values, `Je_value` - a tensor that belongs to
    the step), with the gradient of the links' rows: backward = one launch of `lcp_link_jacobian_backward_f64`, which is asked only for
    the gradients autograd needs; the base rows of the cotangent are handed on to `Je_base`'s own node."""

    @staticmethod
    def forward(ctx, p, a1, a2, phi, Je_base, links, Je_value):
        ctx.links = links
        ctx.e0 = Je_value.shape[1] - links.e
        ctx.save_for_backward(p, a1, a2, phi)
        return Je_value.detach()

    @staticmethod
    def backward(ctx, gJe):
        p, a1, a2, phi = ctx.saved_tensors
        need = ctx.needs_input_grad
        g = ctx.links.jacobian_backward(p, gJe, want=need[:4], _leaves=(a1, a2, phi))
        g_base = gJe[:, :ctx.e0] if (need[4] and ctx.e0) else None
        return g[0], g[1], g[2], g[3], g_base, None, None


def link_jacobian(links, p, Je_base=None):
    """The equality rows of B scenes `[B, e0 + e, 3nb]` float32 at pose `p` [B,nb,3] f64: `Je_base`'s rows (None: none), then the rows
    of `links`.  Differentiable with respect to `p`, `Je_base` and the links' `a1`, `a2`, `phi`."""
    a1, a2, phi = links.a1, links.a2, links.phi
    det = lambda t: None if t is None else t.detach()
    value = links.jacobian(p.detach(), det(Je_base), _leaves=(a1.detach(), a2.detach(), phi.detach()))
    if Je_base is not None and not Je_base.numel():
        Je_base = None
    return _LinkJacobianFn.apply(p, a1, a2, phi, Je_base, links, value)
