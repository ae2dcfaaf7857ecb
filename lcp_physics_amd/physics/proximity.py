"""Proximity queries on the device: the signed distance between body pairs, differentiable.

The contact list knows a pair only once it is within `eps` of touching; a planner or a learner needs the distance before that - for a
collision-avoidance cost, a "ball towards paddle" shaping term, a clearance constraint.  ONE launch of `lcp_pair_distance_f64`
(lcp_proximity.hip) answers the `P` pairs of every scene, and ONE launch of `lcp_pair_distance_backward_f64` is the backward of the
distances, so a loss on clearances reaches the pose, the radii and the hull vertices - and, through
`ContactWorld.step(differentiable=True)`, everything upstream:

    pairs = PairSet.all_pairs(world.geom.nb, world.B, max_dist=50.0).to(dev)
    dist = world.clearance(pairs)                    # [B,P] f64; part of the roll-out's graph after differentiable steps
    torch.relu(5.0 - dist).sum().backward()

Conventions (include/lcp_hip.h, "proximity queries", has the rule): `dist` is negative when the bodies overlap and equals minus the
contact list's largest penetration where the pair has a record; the normal points from the first body towards the second; a pair at
`max_dist` or beyond returns `max_dist` (and zeros for the normal and the witness points) and has no gradient, and so does a pair
that is no pair (equal or out-of-range indices, a hull of fewer than three vertices).  `no_contact` is not consulted.  No CPU
fallback.
"""
from dataclasses import dataclass

import torch

from .. import _lib
from .render import _geometry

INF = float("inf")
MAX_PAIRS = 1024


@dataclass
class PairSet:
    """The body pairs of B scenes, P per scene: `first [B,P]` and `second [B,P]` int32 (body 1 and body 2), `max_dist [B,P]` f64 (the
    cutoff, positive, +inf allowed: checked here, once)."""
    first: torch.Tensor
    second: torch.Tensor
    max_dist: torch.Tensor

    def __post_init__(self):
        if self.first.dim() != 2:
            raise ValueError("pairs.first must be [B,P] (got %s)" % (tuple(self.first.shape),))
        B, P = self.first.shape
        for name in ("second", "max_dist"):
            if tuple(getattr(self, name).shape) != (B, P):
                raise ValueError("pairs.%s must be %s (got %s)" % (name, (B, P), tuple(getattr(self, name).shape)))
        if P < 1 or P > MAX_PAIRS:
            raise ValueError("1 to %d pairs per scene (got %d)" % (MAX_PAIRS, P))
        if not bool((self.max_dist > 0).all()):                        # (a NaN fails too)
            raise ValueError("pairs.max_dist must be positive")

    @property
    def B(self):
        return self.first.shape[0]

    @property
    def P(self):
        return self.first.shape[1]

    def to(self, device):
        mv = lambda t: t.to(device).contiguous()
        return PairSet(mv(self.first), mv(self.second), mv(self.max_dist))

    @staticmethod
    def _of(first, second, B, max_dist):
        if len(first) > MAX_PAIRS:
            raise ValueError("%d pairs: more than %d a call - query them in several sets" % (len(first), MAX_PAIRS))
        rep = lambda idx: torch.tensor(idx, dtype=torch.int32).reshape(1, -1).expand(B, len(idx)).contiguous()
        return PairSet(rep(first), rep(second), torch.full((B, len(first)), float(max_dist), dtype=torch.float64))

    @staticmethod
    def all_pairs(nb, B, max_dist=INF):
        """Every pair i < j of `nb` bodies in the contact list's pair order (i outer, j inner), the same in all B scenes.  CPU tensors;
        `.to(device)` moves them."""
        nb = int(nb)
        if nb < 2:
            raise ValueError("pairs need at least two bodies")
        if nb * (nb - 1) // 2 > MAX_PAIRS:
            raise ValueError("%d bodies have %d pairs, more than %d a call - query them in several sets" % (nb, nb * (nb - 1) // 2, MAX_PAIRS))
        idx = [(i, j) for i in range(nb) for j in range(i + 1, nb)]
        return PairSet._of([i for i, _ in idx], [j for _, j in idx], B, max_dist)

    @staticmethod
    def between(firsts, seconds, B, max_dist=INF):
        """The product of two index lists: every body of `firsts` against every body of `seconds` (firsts outer), the same in all B
        scenes."""
        firsts, seconds = [int(i) for i in firsts], [int(j) for j in seconds]
        if not firsts or not seconds:
            raise ValueError("pairs need a body on either side")
        return PairSet._of([i for i in firsts for _ in seconds], [j for _ in firsts for j in seconds], B, max_dist)


class _Launch:
    """The arguments both entries share, resolved once: sizes and the device pointers of the constant inputs."""

    def __init__(self, geom, pairs):
        self.sizes = (geom.B, geom.nb, geom.nvcap, geom.verts_max(), pairs.P)
        self.kind, self.nverts = geom.kind, geom.nverts
        self.first = _lib.require_gpu_tensor(pairs.first, "pairs.first", torch.int32)
        self.second = _lib.require_gpu_tensor(pairs.second, "pairs.second", torch.int32)
        self.max_dist = _lib.require_gpu_tensor(pairs.max_dist, "pairs.max_dist", torch.float64)

    def inputs(self, radius, verts_local, p):
        P = _lib.ptr
        return (*self.sizes, P(self.kind), P(radius), P(verts_local), P(self.nverts), P(p), P(self.first), P(self.second),
                P(self.max_dist))


class PairDistanceFunction(torch.autograd.Function):
    """(p, radius, verts_local) -> dist [B,P] f64[, normal, w1, w2 [B,P,2] f64]: one launch each way.  Only `dist` is differentiable;
    the backward asks the kernel only for the gradients autograd needs (NULL for the rest) and recomputes every pair from the saved
    INPUTS."""

    @staticmethod
    def forward(ctx, p, radius, verts_local, launch, witnesses):
        lib = _lib.load()
        dev = p.device
        B, P = launch.sizes[0], launch.sizes[4]
        dist = torch.empty(B, P, dtype=torch.float64, device=dev)
        extra = [torch.empty(B, P, 2, dtype=torch.float64, device=dev) if witnesses else None for _ in range(3)]
        with _lib.on_device(dev):
            rc = lib.lcp_pair_distance_f64(*launch.inputs(radius, verts_local, p), _lib.ptr(dist), *[_lib.ptr(t) for t in extra],
                                           _lib.stream_ptr(dev))
        _lib.check(rc, "lcp_pair_distance_f64")
        ctx.launch = launch
        ctx.save_for_backward(p, radius, verts_local)
        if witnesses:
            ctx.mark_non_differentiable(*extra)
            return (dist, *extra)
        return dist

    @staticmethod
    def backward(ctx, g_dist, *_):
        saved = ctx.saved_tensors
        lib = _lib.load()
        dev = saved[0].device
        outs = [torch.empty(t.shape, dtype=t.dtype, device=dev) if need else None for t, need in zip(saved, ctx.needs_input_grad[:3])]
        if all(o is None for o in outs):
            return (None,) * 5
        p, radius, verts_local = saved
        g_dist = g_dist.to(torch.float64).contiguous()
        with _lib.on_device(dev):
            rc = lib.lcp_pair_distance_backward_f64(*ctx.launch.inputs(radius, verts_local, p), _lib.ptr(g_dist),
                                                    *[_lib.ptr(o) for o in outs], _lib.stream_ptr(dev))
        _lib.check(rc, "lcp_pair_distance_backward_f64")
        return (*outs, None, None)


def pair_distances(geom, p, pairs, witnesses=False):
    """The signed distances of the body pairs of B scenes: `dist [B,P]` f64, differentiable with respect to `p` [B,nb,3] f64,
    `geom.radius` and `geom.verts_local`.  With `witnesses=True`: `(dist, normal, w1, w2)`, the unit normal from the first body towards
    the second and the witness points on either surface, each [B,P,2] f64 in the world frame and without gradient."""
    _geometry(geom, p)
    if pairs.B != geom.B:
        raise ValueError("pairs are for %d scenes, the geometry for %d" % (pairs.B, geom.B))
    launch = _Launch(geom, pairs)
    return PairDistanceFunction.apply(p, geom.radius, geom.verts_local, launch, bool(witnesses))
