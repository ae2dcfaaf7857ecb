"""Continuous collision on the device: the time of impact of body pairs along the engine's own move, differentiable.

A step accepts a move when its END pose does not penetrate, so a body that travels more than an obstacle's thickness in one `dt` lands
beyond it without a contact record.  The proximity queries say how far apart a pair is now; this query says WHEN it will touch, should
every body keep moving by `p + t v`.  ONE launch of `lcp_time_of_impact_f64` (lcp_toi.hip, conservative advancement on the distance
rule of the proximity queries) answers the `P` pairs of every scene, and ONE launch of `lcp_time_of_impact_backward_f64` is the
backward of the times (a single evaluation at the pose of impact):

    pairs = PairSet.between([ball], walls, world.B).to(dev)
    toi, status = world.time_to_contact(pairs, horizon=1.0)          # [B,P] f64, [B,P] int32; part of the graph after differentiable steps
    toi[status == HIT].sum().backward()

    world = ContactWorld(..., ccd=pairs)                             # or ccd=True: no step moves past a first touch

Conventions (include/lcp_hip.h, "time of impact", has the rule and the proof that no iterate passes the first touch): a pair that does
not come within `margin + tol` before `horizon` is a MISS and returns `horizon`; a pair within `margin + tol` at `t = 0` is TOUCHING
and returns 0; a HIT returns a time at which `margin <= dist <= margin + tol`, no later than the first touch; a pair that needs more
than `max_iter` evaluations is UNCONVERGED and returns a true lower bound.  Only a HIT that is closing has a gradient.  A `PairSet`'s
`max_dist` is not consulted.  No CPU fallback.
"""
import torch

from .. import _lib
from .render import _geometry

MISS, HIT, TOUCHING, UNCONVERGED = 0, 1, 2, 3
MAX_ITER_LIMIT = 1024


class _Launch:
    """The arguments both entries share, resolved once: sizes, the device pointers of the constant inputs, the scalars."""

    def __init__(self, geom, pairs, tol, max_iter):
        tol, max_iter = float(tol), int(max_iter)
        if not tol > 0:
            raise ValueError("tol must be positive (got %r)" % (tol,))
        if max_iter < 1 or max_iter > MAX_ITER_LIMIT:
            raise ValueError("max_iter must be 1 to %d (got %d)" % (MAX_ITER_LIMIT, max_iter))
        if pairs.B != geom.B:
            raise ValueError("pairs are for %d scenes, the geometry for %d" % (pairs.B, geom.B))
        self.sizes = (geom.B, geom.nb, geom.nvcap, geom.verts_max(), pairs.P)
        self.kind, self.nverts = geom.kind, geom.nverts
        self.first = _lib.require_gpu_tensor(pairs.first, "pairs.first", torch.int32)
        self.second = _lib.require_gpu_tensor(pairs.second, "pairs.second", torch.int32)
        self.tol, self.max_iter = tol, max_iter

    def inputs(self, radius, verts_local, p, v32):
        P = _lib.ptr
        return (*self.sizes, P(self.kind), P(radius), P(verts_local), P(self.nverts), P(p), P(v32), P(self.first), P(self.second))

    def forward(self, radius, verts_local, p, v32, margin, horizon, toi=None, status=None, normal=None, first_toi=None, first_pair=None):
        """The raw entry: every output a tensor to write or None."""
        P = _lib.ptr
        dev = p.device
        with _lib.on_device(dev):
            rc = _lib.load().lcp_time_of_impact_f64(*self.inputs(radius, verts_local, p, v32), P(margin), P(horizon), self.tol,
                                                    self.max_iter, P(toi), P(status), P(normal), P(first_toi), P(first_pair),
                                                    _lib.stream_ptr(dev))
        _lib.check(rc, "lcp_time_of_impact_f64")


def _per_scene(horizon, B, dev):
    """`horizon` as [B] f64 on the device: a number or a tensor."""
    if isinstance(horizon, torch.Tensor):
        if tuple(horizon.shape) != (B,):
            raise ValueError("horizon must be a number or [B] = [%d] (got %s)" % (B, tuple(horizon.shape)))
        return _lib.require_gpu_tensor(horizon.detach(), "horizon", torch.float64)
    return torch.full((B,), float(horizon), dtype=torch.float64, device=dev)


def _per_pair(margin, B, P, dev):
    """`margin` as [B,P] f64 on the device: a number (checked here) or a tensor (the caller's to keep >= 0: no synchronisation)."""
    if isinstance(margin, torch.Tensor):
        if tuple(margin.shape) != (B, P):
            raise ValueError("margin must be a number or [B,P] = %s (got %s)" % ((B, P), tuple(margin.shape)))
        _lib.require_gpu_tensor(margin.detach(), "margin", torch.float64)
        return margin
    if not float(margin) >= 0:
        raise ValueError("margin must not be negative (got %r)" % (margin,))
    return torch.full((B, P), float(margin), dtype=torch.float64, device=dev)


class TimeOfImpactFunction(torch.autograd.Function):
    """(p, v, radius, verts_local, margin) -> toi [B,P] f64, status [B,P] int32[, normal [B,P,2] f64]: one launch each way.  Only `toi`
    is differentiable; the backward asks the kernel only for the gradients autograd needs (NULL for the rest) and evaluates every
    live pair once, at the forward's own `toi`.  The gradient of `v` is cast to `v`'s dtype."""

    @staticmethod
    def forward(ctx, p, v, radius, verts_local, margin, horizon, launch, normals):
        dev = p.device
        B, P = launch.sizes[0], launch.sizes[4]
        v32 = v.to(torch.float32).contiguous()
        toi = torch.empty(B, P, dtype=torch.float64, device=dev)
        status = torch.empty(B, P, dtype=torch.int32, device=dev)
        normal = torch.empty(B, P, 2, dtype=torch.float64, device=dev) if normals else None
        launch.forward(radius, verts_local, p, v32, margin, horizon, toi=toi, status=status, normal=normal)
        ctx.launch, ctx.v_dtype = launch, v.dtype
        ctx.save_for_backward(p, v32, radius, verts_local, toi, status)
        ctx.mark_non_differentiable(status)
        if normals:
            ctx.mark_non_differentiable(normal)
            return toi, status, normal
        return toi, status

    @staticmethod
    def backward(ctx, g_toi, *_):
        p, v32, radius, verts_local, toi, status = ctx.saved_tensors
        dev = p.device
        shapes = (p, p, radius, verts_local, toi)                          # g_p, g_v, g_radius, g_verts_local, g_margin
        outs = [torch.empty(t.shape, dtype=torch.float64, device=dev) if need else None for t, need in zip(shapes, ctx.needs_input_grad[:5])]
        if all(o is None for o in outs):
            return (None,) * 8
        g_toi = g_toi.to(torch.float64).contiguous()
        P = _lib.ptr
        with _lib.on_device(dev):
            rc = _lib.load().lcp_time_of_impact_backward_f64(*ctx.launch.inputs(radius, verts_local, p, v32), P(toi), P(status), P(g_toi),
                                                             *[P(o) for o in outs], _lib.stream_ptr(dev))
        _lib.check(rc, "lcp_time_of_impact_backward_f64")
        if outs[1] is not None:
            outs[1] = outs[1].to(ctx.v_dtype)
        return (*outs, None, None, None)


def _checked(geom, p, v, pairs, horizon, margin, tol, max_iter):
    _geometry(geom, p)
    if tuple(v.shape) != tuple(p.shape):
        raise ValueError("v must have p's shape %s (got %s)" % (tuple(p.shape), tuple(v.shape)))
    if not v.is_cuda:
        raise RuntimeError("v must live on a GPU (got %s); the HIP path has no CPU fallback" % (v.device,))
    launch = _Launch(geom, pairs, tol, max_iter)
    return launch, _per_scene(horizon, geom.B, p.device), _per_pair(margin, geom.B, pairs.P, p.device)


def time_of_impact(geom, p, v, pairs, horizon, margin=0.0, tol=1e-6, max_iter=64, normals=False):
    """When the body pairs of B scenes first come within `margin` of each other along `p + t v`, `0 <= t <= horizon`:
    `(toi [B,P] f64, status [B,P] int32)`, with `normals=True` also the unit normal [B,P,2] f64 from the first body towards the second
    at `toi` (zeros unless HIT or TOUCHING).  `toi` is differentiable with respect to `p` [B,nb,3] f64, `v` [B,nb,3] (float32, the
    world's dtype; anything else is rounded to it), `geom.radius`, `geom.verts_local` and `margin` when it is a tensor.  `horizon`: a
    number or [B] f64; `margin`: a number or [B,P] f64, not negative; `tol`: the distance within which a pair counts as touching;
    `max_iter`: the evaluations of the distance a pair may take (1 to 1024)."""
    launch, horizon, margin = _checked(geom, p, v, pairs, horizon, margin, tol, max_iter)
    return TimeOfImpactFunction.apply(p, v, geom.radius, geom.verts_local, margin, horizon, launch, bool(normals))


class FirstImpact:
    """The per-scene part of the query into persistent buffers, for a world that clips its steps: `first_toi [B]` f64 (the smallest
    `toi` of the HIT or UNCONVERGED pairs, else `horizon`), `first_pair [B]` int32 and `dt_scene [B]` f64 = min(horizon, first_toi).
    One launch and one elementwise minimum per call, through the same pointers every time: a captured graph replays them."""

    def __init__(self, geom, pairs, margin, tol=1e-6, max_iter=64):
        dev = pairs.first.device
        self.geom, self.pairs = geom, pairs
        self.launch = _Launch(geom, pairs, tol, max_iter)
        self.margin = _per_pair(margin, geom.B, pairs.P, dev).detach().contiguous()
        self.first_toi = torch.zeros(geom.B, dtype=torch.float64, device=dev)
        self.first_pair = torch.full((geom.B,), -1, dtype=torch.int32, device=dev)
        self.dt_scene = torch.zeros(geom.B, dtype=torch.float64, device=dev)
        self._horizon = torch.zeros(geom.B, dtype=torch.float64, device=dev)

    def __call__(self, p, v, horizon):
        """`horizon`: a number or [B] f64 (copied into the query's own buffer).  Returns `dt_scene`."""
        geom = self.geom
        r, vl, pd = _geometry(geom, p)
        v32 = _lib.require_gpu_tensor(v.detach(), "v", torch.float32)
        if isinstance(horizon, torch.Tensor):
            self._horizon.copy_(horizon)
        else:
            self._horizon.fill_(float(horizon))
        self.launch.forward(r, vl, pd, v32, self.margin, self._horizon, first_toi=self.first_toi, first_pair=self.first_pair)
        return torch.minimum(self._horizon, self.first_toi, out=self.dt_scene)
