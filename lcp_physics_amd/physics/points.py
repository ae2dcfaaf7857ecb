"""Point probes on the device: the signed distance from query points to the scene, differentiable.

How far is this point from the scene, and from which body?  A goal-reaching loss ("the distance from the target to body 3's surface"),
a fingertip or whisker mounted on a body, a collision cost for planned waypoints, a small signed-distance map used as an observation,
picking ("which body is under this point").  ONE launch of `lcp_point_distance_f64` (lcp_points.hip) answers the `N` points of every
scene, and ONE launch of `lcp_point_distance_backward_f64` is the backward of the distances, so a loss on them reaches the pose, the
radii, the hull vertices and the points' own coordinates - and, through `ContactWorld.step(differentiable=True)`, everything upstream:

    tips = PointSet.on_body(body=0, xy=[(12.0, 0.0), (0.0, 12.0)], B=world.B).to(dev)
    dist, body = world.probe(tips)                   # [B,2] f64 and int32; part of the roll-out's graph after differentiable steps
    torch.relu(5.0 - dist).sum().backward()

Conventions (include/lcp_hip.h, "point probes", has the rule): a point is given in the frame of the body it is mounted on (`body =
-1`: the world frame) and never tests its own mounting body; `target = -1` tests every body, `target = k` body k alone; the distance
is negative inside a body; a point with nothing within `max_dist` is void: it returns `max_dist`, `body = -1`, a zero normal and has
no gradient.  No CPU fallback.
"""
import math
from dataclasses import dataclass

import torch

from .. import _lib
from .render import Camera, _geometry


@dataclass
class PointSet:
    """The query points of B scenes, N per scene: `body [B,N]` int32 (the mounting body; -1: the world frame), `xy [B,N,2]` f64 in
    the mounting frame, `target [B,N]` int32 (-1: every body; k: body k alone), `max_dist [B,N]` f64 (the cutoff, positive, +inf
    allowed: checked here, once).  `xy` may require grad."""
    body: torch.Tensor
    xy: torch.Tensor
    target: torch.Tensor
    max_dist: torch.Tensor

    def __post_init__(self):
        if self.body.dim() != 2:
            raise ValueError("points.body must be [B,N] (got %s)" % (tuple(self.body.shape),))
        B, N = self.body.shape
        for name, shape in (("xy", (B, N, 2)), ("target", (B, N)), ("max_dist", (B, N))):
            if tuple(getattr(self, name).shape) != shape:
                raise ValueError("points.%s must be %s (got %s)" % (name, shape, tuple(getattr(self, name).shape)))
        if N < 1 or N > 1024:
            raise ValueError("1 to 1024 points per scene (got %d)" % N)
        if not bool((self.max_dist > 0).all()):                       # (a NaN fails too)
            raise ValueError("points.max_dist must be positive")

    @property
    def B(self):
        return self.body.shape[0]

    @property
    def N(self):
        return self.body.shape[1]

    def to(self, device):
        mv = lambda t: t.to(device).contiguous()                      # (differentiable: a graph on xy survives)
        return PointSet(mv(self.body), mv(self.xy), mv(self.target), mv(self.max_dist))

    @staticmethod
    def _uniform(body, xy, B, target, max_dist):
        xy = torch.as_tensor(xy, dtype=torch.float64).reshape(-1, 2)
        N = xy.shape[0]
        full = lambda v, dt_: torch.full((B, N), v, dtype=dt_)
        return PointSet(full(int(body), torch.int32), xy.unsqueeze(0).expand(B, N, 2).contiguous(), full(int(target), torch.int32),
                        full(float(max_dist), torch.float64))

    @staticmethod
    def on_body(body, xy, B, target=-1, max_dist=math.inf):
        """The points `xy` (a list of (x, y) in the body's frame) mounted on body `body` of every scene.  CPU tensors; `.to(device)`
        moves them."""
        return PointSet._uniform(body, xy, B, target, max_dist)

    @staticmethod
    def world(xy, B, target=-1, max_dist=math.inf):
        """The world-frame points `xy` (a list of (x, y)), the same in every scene."""
        return PointSet._uniform(-1, xy, B, target, max_dist)

    @staticmethod
    def grid(cam_or_extent, h=None, w=None, B=1, target=-1, max_dist=math.inf):
        """`h * w <= 1024` world-frame points in rows, point `i * w + j` at the centre of cell (i, j).  With a `render.Camera`: its
        pixel centres (x0 + (j + 1/2) / ppm, y0 + (i + 1/2) / ppm), `h` and `w` defaulting to the camera's, so that
        `dist.reshape(B, h, w)` is a signed-distance map aligned with `render_ids`.  With an extent `(x0, y0, x1, y1)`: the centres of
        `h` x `w` equal cells that tile it."""
        if isinstance(cam_or_extent, Camera):
            h = cam_or_extent.height if h is None else h
            w = cam_or_extent.width if w is None else w
            x0, y0 = (float(v) for v in cam_or_extent.origin)
            ppm = float(cam_or_extent.pixels_per_meter)
            dx = dy = None
        else:
            if h is None or w is None:
                raise ValueError("a grid over an extent needs h and w")
            x0, y0, x1, y1 = (float(v) for v in cam_or_extent)
            dx, dy = x1 - x0, y1 - y0
        h, w = int(h), int(w)
        if h < 1 or w < 1 or h * w > 1024:
            raise ValueError("a grid has 1 to 1024 points (got %d x %d)" % (h, w))
        j, i = torch.arange(w, dtype=torch.float64) + 0.5, torch.arange(h, dtype=torch.float64) + 0.5
        x, y = (x0 + j / ppm, y0 + i / ppm) if dx is None else (x0 + j * (dx / w), y0 + i * (dy / h))
        xy = torch.stack([x.reshape(1, w).expand(h, w), y.reshape(h, 1).expand(h, w)], -1)
        return PointSet._uniform(-1, xy, B, target, max_dist)


class _Launch:
    """The arguments both entries share, resolved once: sizes and the device pointers of the constant inputs."""

    def __init__(self, geom, points):
        self.sizes = (geom.B, geom.nb, geom.nvcap, geom.verts_max(), points.N)
        self.kind, self.nverts = geom.kind, geom.nverts
        self.body = _lib.require_gpu_tensor(points.body, "points.body", torch.int32)
        self.target = _lib.require_gpu_tensor(points.target, "points.target", torch.int32)
        self.max_dist = _lib.require_gpu_tensor(points.max_dist, "points.max_dist", torch.float64)

    def inputs(self, radius, verts_local, p, xy):
        P = _lib.ptr
        return (*self.sizes, P(self.kind), P(radius), P(verts_local), P(self.nverts), P(p), P(self.body), P(xy), P(self.target),
                P(self.max_dist))


class PointDistanceFunction(torch.autograd.Function):
    """(p, radius, verts_local, xy) -> dist [B,N] f64, body [B,N] i32[, normal [B,N,2] f64]: one launch each way.  Only `dist` is
    differentiable; the backward asks the kernel only for the gradients autograd needs (NULL for the rest) and recomputes the
    selections from the saved INPUTS."""

    @staticmethod
    def forward(ctx, p, radius, verts_local, xy, launch, normals):
        lib = _lib.load()
        dev = p.device
        B, N = launch.sizes[0], launch.sizes[4]
        dist = torch.empty(B, N, dtype=torch.float64, device=dev)
        body = torch.empty(B, N, dtype=torch.int32, device=dev)
        normal = torch.empty(B, N, 2, dtype=torch.float64, device=dev) if normals else None
        with _lib.on_device(dev):
            rc = lib.lcp_point_distance_f64(*launch.inputs(radius, verts_local, p, xy), _lib.ptr(dist), _lib.ptr(body),
                                            _lib.ptr(normal), _lib.stream_ptr(dev))
        _lib.check(rc, "lcp_point_distance_f64")
        ctx.launch = launch
        ctx.save_for_backward(p, radius, verts_local, xy)
        ctx.mark_non_differentiable(body)
        if normals:
            ctx.mark_non_differentiable(normal)
            return dist, body, normal
        return dist, body

    @staticmethod
    def backward(ctx, g_dist, *_):
        saved = ctx.saved_tensors
        lib = _lib.load()
        dev = saved[0].device
        outs = [torch.empty(t.shape, dtype=t.dtype, device=dev) if need else None for t, need in zip(saved, ctx.needs_input_grad[:4])]
        if all(o is None for o in outs):
            return (None,) * 6
        p, radius, verts_local, xy = saved
        g_dist = g_dist.to(torch.float64).contiguous()
        with _lib.on_device(dev):
            rc = lib.lcp_point_distance_backward_f64(*ctx.launch.inputs(radius, verts_local, p, xy), _lib.ptr(g_dist),
                                                     *[_lib.ptr(o) for o in outs], _lib.stream_ptr(dev))
        _lib.check(rc, "lcp_point_distance_backward_f64")
        return (*outs, None, None)


def point_distances(geom, p, points, normals=False):
    """The signed distances from the query points of B scenes to their bodies: `dist [B,N]` f64 (differentiable with respect to `p`
    [B,nb,3] f64, `geom.radius`, `geom.verts_local` and `points.xy`), `body [B,N]` int32 (the nearest body, -1: a void point) and,
    with `normals=True`, `normal [B,N,2]` f64 (d(dist)/dx in the world frame; 0 for a void point and at a circle's centre).  `body`
    and `normal` carry no gradient."""
    _geometry(geom, p)
    if points.B != geom.B:
        raise ValueError("points are for %d scenes, the geometry for %d" % (points.B, geom.B))
    _lib.require_gpu_tensor(points.xy.detach(), "points.xy", torch.float64)
    launch = _Launch(geom, points)
    return PointDistanceFunction.apply(p, geom.radius, geom.verts_local, points.xy, launch, bool(normals))
