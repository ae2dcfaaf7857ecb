"""Overlap queries on the device: the area of the intersection of body pairs, differentiable.

`pair_distances` answers an overlapping pair with the penetration depth of one feature pair, which is only piecewise smooth and says
nothing about how much of a body lies inside another; `render` gives the overlap as a pixel count at the cost of a frame.  The area of
the intersection of two convex shapes is C1 in the pose, zero where the bodies are apart and grows smoothly from the first
touch - a goal-region reward ("which fraction of the box is inside the zone?"), IoU against a target polygon without rasterising, a
trigger that is sized rather than binary.  ONE launch of `lcp_pair_overlap_f64` (lcp_overlap.hip) answers the `P` pairs of every scene
and ONE launch of `lcp_pair_overlap_backward_f64` is its backward, so a loss on areas reaches the pose, the radii and the hull vertices
- and, through `ContactWorld.step(differentiable=True)`, everything upstream:

    zone = PairSet.between([box], [goal], world.B).to(dev)          # the goal: a body that geom.no_contact keeps out of collisions
    area = world.overlap(zone)                                       # [B,1] f64; part of the roll-out's graph after differentiable steps
    (1.0 - area / body_areas(world.geom)[:, box:box + 1]).sum().backward()

Conventions (include/lcp_hip.h, "overlap queries", has the rule): the pairs are a `proximity.PairSet`, whose `max_dist` is not
consulted - an area needs no cutoff; a pair that is no pair (equal or out-of-range indices, a hull of fewer than three vertices) has
area 0 and no gradient, and so has every pair that does not overlap.  `no_contact` is not consulted.  No CPU fallback for the kernel
entry; `body_areas` is plain torch and works anywhere.
"""
import math

import torch

from .. import _lib
from .render import _geometry


class _Launch:
    """The arguments both entries share, resolved once: sizes and the device pointers of the constant inputs."""

    def __init__(self, geom, pairs):
        self.sizes = (geom.B, geom.nb, geom.nvcap, geom.verts_max(), pairs.P)
        self.kind, self.nverts = geom.kind, geom.nverts
        self.first = _lib.require_gpu_tensor(pairs.first, "pairs.first", torch.int32)
        self.second = _lib.require_gpu_tensor(pairs.second, "pairs.second", torch.int32)

    def inputs(self, radius, verts_local, p):
        P = _lib.ptr
        return (*self.sizes, P(self.kind), P(radius), P(verts_local), P(self.nverts), P(p), P(self.first), P(self.second))


class PairOverlapFunction(torch.autograd.Function):
    """(p, radius, verts_local) -> area [B,P] f64: one launch each way.  The backward asks the kernel only for the gradients autograd
    needs (NULL for the rest) and recomputes every pair from the saved INPUTS."""

    @staticmethod
    def forward(ctx, p, radius, verts_local, launch):
        lib = _lib.load()
        dev = p.device
        area = torch.empty(launch.sizes[0], launch.sizes[4], dtype=torch.float64, device=dev)
        with _lib.on_device(dev):
            rc = lib.lcp_pair_overlap_f64(*launch.inputs(radius, verts_local, p), _lib.ptr(area), _lib.stream_ptr(dev))
        _lib.check(rc, "lcp_pair_overlap_f64")
        ctx.launch = launch
        ctx.save_for_backward(p, radius, verts_local)
        return area

    @staticmethod
    def backward(ctx, g_area):
        saved = ctx.saved_tensors
        lib = _lib.load()
        dev = saved[0].device
        outs = [torch.empty(t.shape, dtype=t.dtype, device=dev) if need else None for t, need in zip(saved, ctx.needs_input_grad[:3])]
        if all(o is None for o in outs):
            return (None,) * 4
        p, radius, verts_local = saved
        g_area = g_area.to(torch.float64).contiguous()
        with _lib.on_device(dev):
            rc = lib.lcp_pair_overlap_backward_f64(*ctx.launch.inputs(radius, verts_local, p), _lib.ptr(g_area),
                                                   *[_lib.ptr(o) for o in outs], _lib.stream_ptr(dev))
        _lib.check(rc, "lcp_pair_overlap_backward_f64")
        return (*outs, None)


def body_areas(geom):
    """The area of every body, `[B,nb]` f64: pi r^2 of a circle, the shoelace formula over the first `nverts` vertices of a hull.  Plain
    torch: differentiable with respect to `geom.radius` and `geom.verts_local` by autograd, on any device."""
    v, cap = geom.verts_local, geom.verts_local.shape[2]
    hull = geom.kind != 0
    n = torch.where(hull, geom.nverts.clamp(0, cap), torch.zeros_like(geom.nverts)).long().unsqueeze(-1)
    ar = torch.arange(cap, device=v.device).expand(*n.shape[:2], cap)
    nxt = torch.where(ar + 1 >= n, torch.zeros_like(ar), ar + 1)
    x, y = v[..., 0], v[..., 1]
    xn, yn = torch.gather(x, 2, nxt), torch.gather(y, 2, nxt)
    cr = torch.where(ar < n, x * yn - xn * y, torch.zeros_like(x))                       # (slots >= nverts: never used)
    return torch.where(hull, 0.5 * cr.sum(-1), math.pi * geom.radius * geom.radius)


def iou_of(area, a1, a2):
    """area / (a1 + a2 - area), 0 where the union is empty."""
    union = a1 + a2 - area
    live = union > 0
    return torch.where(live, area / torch.where(live, union, torch.ones_like(union)), torch.zeros_like(area))


def pair_overlaps(geom, p, pairs, iou=False):
    """The intersection areas of the body pairs of B scenes: `area [B,P]` f64, differentiable with respect to `p` [B,nb,3] f64,
    `geom.radius` and `geom.verts_local`.  With `iou=True`: `(area, area / (A1 + A2 - area))`, the union from `body_areas`; an invalid
    pair gives 0."""
    _geometry(geom, p)
    if pairs.B != geom.B:
        raise ValueError("pairs are for %d scenes, the geometry for %d" % (pairs.B, geom.B))
    area = PairOverlapFunction.apply(p, geom.radius, geom.verts_local, _Launch(geom, pairs))
    if not iou:
        return area
    own = body_areas(geom)
    nb = geom.nb
    f, s = pairs.first.long(), pairs.second.long()
    valid = (f != s) & (f >= 0) & (f < nb) & (s >= 0) & (s < nb)
    a1, a2 = torch.gather(own, 1, f.clamp(0, nb - 1)), torch.gather(own, 1, s.clamp(0, nb - 1))
    return area, torch.where(valid, iou_of(area, a1, a2), torch.zeros_like(area))
