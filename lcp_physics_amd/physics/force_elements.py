"""Force elements on the device: springs / dampers, PD motors and viscous drag as a function of the state, differentiable.

`f` and `force_fn(t)` know the clock and nothing else; a tether between two bodies, a servo on a joint or drag depend on the pose and
the velocities.  ONE launch of `lcp_force_elements_f64` (lcp_forces.hip) evaluates the `E` elements of every scene and adds their
wrenches onto a base force, and ONE launch of `lcp_force_elements_backward_f64` is the backward to the pose, the velocities, the
base force and the elements' parameters:

    els = ForceSet.from_list([("spring", 0, 1, (0.5, 0.0), (-0.5, 0.0), {"k": 40.0, "c": 0.5, "rest": 2.0}),
                              ("motor", -1, 2, {"kp": 30.0, "kd": 2.0, "target": 1.0, "limit": 50.0}),
                              ("drag", 1, {"lin": 0.1, "ang": 0.01})], B).to(dev)
    world = ContactWorld(geom, p, v, Mdiag, f, rest, fric, elements=els)       # every step evaluates them at its starting state
    f_now = element_forces(els, world.p, world.v, f_base=world.f)              # [B,nb,3] float32 (torque, fx, fy)

Conventions (include/lcp_hip.h, "force elements", has the rule): a spring acts between the anchors `a1` on `b1` and `a2` on `b2`, given
in the bodies' frames; a body index of -1 is the world, whose anchor is a world point at rest.  A motor drives `b2` against the base
`b1` towards the relative angle `x0` and rate `w0`.  `limit` clamps the spring's tension or the motor's torque; a clamped element has
no gradient, and neither has an invalid one (equal or out-of-range indices).  For drag, `k` is the linear and `c` the angular
coefficient.  No CPU fallback.
"""
from dataclasses import dataclass, fields

import torch

from .. import _lib

INF = float("inf")
MAX_ELEMENTS = 1024
NONE, SPRING, MOTOR, DRAG = 0, 1, 2, 3
_FLOATS = ("a1", "a2", "k", "c", "x0", "w0", "limit")
_LEAVES = ("k", "c", "x0", "w0", "a1", "a2")                # the parameters with a gradient, in the kernel's order


@dataclass
class ForceSet:
    """The force elements of B scenes, E per scene: `kind`, `b1`, `b2` [B,E] int32; `a1`, `a2` [B,E,2] f64; `k`, `c`, `x0`, `w0`,
    `limit` [B,E] f64 (`limit` positive, +inf allowed: checked here, once)."""
    kind: torch.Tensor
    b1: torch.Tensor
    b2: torch.Tensor
    a1: torch.Tensor
    a2: torch.Tensor
    k: torch.Tensor
    c: torch.Tensor
    x0: torch.Tensor
    w0: torch.Tensor
    limit: torch.Tensor

    def __post_init__(self):
        if self.kind.dim() != 2:
            raise ValueError("elements.kind must be [B,E] (got %s)" % (tuple(self.kind.shape),))
        B, E = self.kind.shape
        for f in fields(self):
            t = getattr(self, f.name)
            want = (B, E, 2) if f.name in ("a1", "a2") else (B, E)
            if tuple(t.shape) != want:
                raise ValueError("elements.%s must be %s (got %s)" % (f.name, want, tuple(t.shape)))
            dt = torch.float64 if f.name in _FLOATS else torch.int32
            if t.dtype != dt:
                raise ValueError("elements.%s must be %s (got %s)" % (f.name, dt, t.dtype))
        if E < 1 or E > MAX_ELEMENTS:
            raise ValueError("1 to %d elements per scene (got %d)" % (MAX_ELEMENTS, E))
        if not bool((self.limit > 0).all()):                              # (a NaN fails too)
            raise ValueError("elements.limit must be positive")

    @property
    def B(self):
        return self.kind.shape[0]

    @property
    def E(self):
        return self.kind.shape[1]

    def to(self, device):
        """The set on `device`.  The float arrays move through autograd: what required grad still leads back to its leaf."""
        return ForceSet(*[getattr(self, f.name).to(device).contiguous() for f in fields(self)])

    @staticmethod
    def from_list(elements, B):
        """`elements`: a list of
            ("spring", b1, b2, a1, a2, {"k": ..., "c": 0, "rest": 0, "limit": inf})
            ("motor", base, body, {"kp": ..., "kd": 0, "target": 0, "rate": 0, "limit": inf})
            ("drag", body, {"lin": 0, "ang": 0})
        the same in all B scenes.  Values are numbers or tensors (0-dim or [B]; anchors [2] or [B,2]); a tensor that requires grad
        stays connected.  CPU tensors unless the values say otherwise; `.to(device)` moves them."""
        B = int(B)
        if not elements:
            raise ValueError("a ForceSet needs at least one element")

        def col(x, tail=()):
            t = torch.as_tensor(x, dtype=torch.float64) if not isinstance(x, torch.Tensor) else x.to(torch.float64)
            if t.dim() == len(tail):
                t = t.unsqueeze(0).expand((B,) + tuple(tail))
            if tuple(t.shape) != (B,) + tuple(tail):
                raise ValueError("a value must be a number, a tensor of shape %s or one per scene (got %s)" % (tuple(tail), tuple(t.shape)))
            return t

        def known(opts, names, what):
            bad = set(opts) - set(names)
            if bad:
                raise ValueError("%s: unknown option(s) %s (known: %s)" % (what, sorted(bad), ", ".join(names)))

        rows = {n: [] for n in ("kind", "b1", "b2") + _FLOATS}
        zero2 = (0.0, 0.0)
        for el in elements:
            what = el[0]
            if what == "spring" and len(el) == 6:
                _, b1, b2, a1, a2, o = el
                known(o, ("k", "c", "rest", "limit"), what)
                vals = (SPRING, b1, b2, a1, a2, o.get("k", 0.0), o.get("c", 0.0), o.get("rest", 0.0), 0.0, o.get("limit", INF))
            elif what == "motor" and len(el) == 4:
                _, b1, b2, o = el
                known(o, ("kp", "kd", "target", "rate", "limit"), what)
                vals = (MOTOR, b1, b2, zero2, zero2, o.get("kp", 0.0), o.get("kd", 0.0), o.get("target", 0.0), o.get("rate", 0.0),
                        o.get("limit", INF))
            elif what == "drag" and len(el) == 3:
                _, b1, o = el
                known(o, ("lin", "ang"), what)
                vals = (DRAG, b1, -1, zero2, zero2, o.get("lin", 0.0), o.get("ang", 0.0), 0.0, 0.0, INF)
            else:
                raise ValueError("not a force element: %r" % (el,))
            for n, x in zip(rows, vals):
                rows[n].append(x)
        dev = next((x.device for n in _FLOATS for x in rows[n] if isinstance(x, torch.Tensor)), torch.device("cpu"))
        ints = lambda n: torch.tensor([int(x) for x in rows[n]], dtype=torch.int32, device=dev).reshape(1, -1).expand(B, -1).contiguous()
        flt = lambda n: torch.stack([col(x, (2,) if n in ("a1", "a2") else ()).to(dev) for x in rows[n]], 1).contiguous()
        return ForceSet(ints("kind"), ints("b1"), ints("b2"), *[flt(n) for n in _FLOATS])

    @staticmethod
    def concat(sets):
        """The elements of several sets of the same B, one after the other."""
        sets = list(sets)
        if not sets or any(s.B != sets[0].B for s in sets):
            raise ValueError("concat needs sets of the same number of scenes")
        return ForceSet(*[torch.cat([getattr(s, f.name) for s in sets], 1).contiguous() for f in fields(ForceSet)])


def _inputs(els, nb, p, v, k, c, x0, w0, a1, a2):
    """The arguments both entries share."""
    P = _lib.ptr
    return (els.B, nb, els.E, P(els.kind), P(els.b1), P(els.b2), P(a1), P(a2), P(k), P(c), P(x0), P(w0), P(els.limit), P(p), P(v))


def _forward(els, p, v, f_base, k, c, x0, w0, a1, a2, out):
    dev = p.device
    with _lib.on_device(dev):
        rc = _lib.load().lcp_force_elements_f64(*_inputs(els, p.shape[1], p, v, k, c, x0, w0, a1, a2), _lib.ptr(f_base), _lib.ptr(out),
                                                _lib.stream_ptr(dev))
    _lib.check(rc, "lcp_force_elements_f64")
    return out


class ForceElementsFunction(torch.autograd.Function):
    """(p, v, f_base, k, c, x0, w0, a1, a2) -> f [B,nb,3] float32: one launch each way.  The backward asks the kernel only for the
    gradients autograd needs (NULL for the rest) and evaluates every element again from the saved INPUTS; the gradient of `f_base` is
    the incoming one, the gradient of `v` is cast to `v`'s dtype."""

    @staticmethod
    def forward(ctx, p, v, f_base, k, c, x0, w0, a1, a2, els):
        v32 = v.to(torch.float32).contiguous()
        out = torch.empty(p.shape, dtype=torch.float32, device=p.device)
        _forward(els, p, v32, f_base, k, c, x0, w0, a1, a2, out)
        ctx.els, ctx.v_dtype = els, v.dtype
        ctx.save_for_backward(p, v32, k, c, x0, w0, a1, a2)
        return out

    @staticmethod
    def backward(ctx, g_f):
        p, v32, k, c, x0, w0, a1, a2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        dev = p.device
        shapes = (p, p) + (k, c, x0, w0, a1, a2)                         # g_p, g_v [B,nb,3]; the parameters' own shapes
        wanted = (need[0], need[1]) + tuple(need[3:9])
        outs = [torch.empty(t.shape, dtype=torch.float64, device=dev) if w else None for t, w in zip(shapes, wanted)]
        g_base = g_f if need[2] else None
        if any(o is not None for o in outs):
            g32 = g_f.to(torch.float32).contiguous()
            with _lib.on_device(dev):
                rc = _lib.load().lcp_force_elements_backward_f64(*_inputs(ctx.els, p.shape[1], p, v32, k, c, x0, w0, a1, a2),
                                                                 _lib.ptr(g32), *[_lib.ptr(o) for o in outs], _lib.stream_ptr(dev))
            _lib.check(rc, "lcp_force_elements_backward_f64")
            if outs[1] is not None:
                outs[1] = outs[1].to(ctx.v_dtype)
        return (outs[0], outs[1], g_base, *outs[2:], None)


def element_forces(elements, p, v, f_base=None, out=None):
    """The forces of B scenes `[B,nb,3]` float32 (torque, fx, fy): `f_base` (default 0) plus the wrenches of `elements` at pose `p`
    [B,nb,3] f64 and velocity `v` [B,nb,3] (float32, the world's dtype; anything else is rounded to it).  Differentiable with respect
    to `p`, `v`, `f_base` and the float arrays of `elements` except `limit`.  `out`: the tensor to write (no autograd then: the plain
    step's persistent buffer; it may be `f_base`)."""
    _lib.require_gpu_tensor(p, "p", torch.float64)
    if tuple(p.shape) != (elements.B, p.shape[1], 3):
        raise ValueError("p must be [%d,nb,3] (got %s)" % (elements.B, tuple(p.shape)))
    if tuple(v.shape) != tuple(p.shape):
        raise ValueError("v must have p's shape %s (got %s)" % (tuple(p.shape), tuple(v.shape)))
    for n in ("kind", "b1", "b2"):
        _lib.require_gpu_tensor(getattr(elements, n), "elements." + n, torch.int32)
    for n in _FLOATS:
        _lib.require_gpu_tensor(getattr(elements, n), "elements." + n, torch.float64)
    if f_base is not None:
        if tuple(f_base.shape) != tuple(p.shape):
            raise ValueError("f_base must have p's shape %s (got %s)" % (tuple(p.shape), tuple(f_base.shape)))
        _lib.require_gpu_tensor(f_base, "f_base", torch.float32)
    leaves = [getattr(elements, n) for n in _LEAVES]
    if out is not None:
        _lib.require_gpu_tensor(out, "out", torch.float32)
        if tuple(out.shape) != tuple(p.shape):
            raise ValueError("out must have p's shape %s (got %s)" % (tuple(p.shape), tuple(out.shape)))
        return _forward(elements, p, _lib.require_gpu_tensor(v, "v", torch.float32), f_base, *leaves, out)
    return ForceElementsFunction.apply(p, v, f_base, *leaves, elements)
