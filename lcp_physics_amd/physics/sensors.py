"""Range sensors on the device: rays cast against every scene's geometry, differentiable.

An agent that sits inside a scene observes it through a fan of rays mounted on a body, each returning the distance to the first
surface it meets.  ONE launch of `lcp_cast_rays_f64` (lcp_sensors.hip) casts the `R` rays of every scene, and ONE launch of
`lcp_cast_rays_backward_f64` is the backward of the distances, so a loss on range readings reaches the pose, the radii, the hull
vertices and the rays' own mounting - and, through `ContactWorld.step(differentiable=True)`, everything upstream:

    rays = RaySet.fan(body=0, n=32, fov=math.pi / 2, max_range=200.0, B=world.B).to(dev)
    dist, hit = world.sense(rays)                    # [B,32] f64 and int32; part of the roll-out's graph after differentiable steps
    ((dist - target) ** 2).mean().backward()

Conventions (include/lcp_hip.h, "range sensors", has the rule): a ray starts at `origin` and points along `angle`, both in the frame
of the body it is mounted on (`body = -1`: the world frame); it never tests its own mounting body; a ray that meets nothing within
`range` returns `range` and `hit = -1`; an origin inside a body returns 0.  No CPU fallback.
"""
from dataclasses import dataclass

import torch

from .. import _lib
from .render import _geometry


@dataclass
class RaySet:
    """The rays of B scenes, R per scene: `body [B,R]` int32 (the mounting body; -1: the world frame), `origin [B,R,2]` f64 and
    `angle [B,R]` f64 in the mounting frame, `range [B,R]` f64 (the maximum range, positive: checked here, once).  `origin` and
    `angle` may require grad."""
    body: torch.Tensor
    origin: torch.Tensor
    angle: torch.Tensor
    range: torch.Tensor

    def __post_init__(self):
        B, R = self.body.shape
        for name, shape in (("origin", (B, R, 2)), ("angle", (B, R)), ("range", (B, R))):
            if tuple(getattr(self, name).shape) != shape:
                raise ValueError("rays.%s must be %s (got %s)" % (name, shape, tuple(getattr(self, name).shape)))
        if R < 1 or R > 1024:
            raise ValueError("1 to 1024 rays per scene (got %d)" % R)
        if not bool((self.range > 0).all()):                          # (a NaN fails too)
            raise ValueError("rays.range must be positive")

    @property
    def B(self):
        return self.body.shape[0]

    @property
    def R(self):
        return self.body.shape[1]

    def to(self, device):
        mv = lambda t: t.to(device).contiguous()                      # (differentiable: a graph on origin / angle survives)
        return RaySet(mv(self.body), mv(self.origin), mv(self.angle), mv(self.range))

    @staticmethod
    def fan(body, n, fov, max_range, B, origin=(0.0, 0.0), centre=0.0):
        """`n` rays spread evenly over the angle `fov` about `centre`, all starting at `origin`, mounted on body `body` of every
        scene (-1: the world frame).  n == 1: the one ray along `centre`.  CPU tensors; `.to(device)` moves them."""
        n = int(n)
        if n < 1:
            raise ValueError("a fan needs at least one ray")
        steps = torch.linspace(-0.5, 0.5, n, dtype=torch.float64) if n > 1 else torch.zeros(1, dtype=torch.float64)
        angle = (float(centre) + float(fov) * steps).reshape(1, n).expand(B, n).contiguous()
        org = torch.tensor([float(origin[0]), float(origin[1])], dtype=torch.float64).reshape(1, 1, 2).expand(B, n, 2).contiguous()
        return RaySet(torch.full((B, n), int(body), dtype=torch.int32), org, angle,
                      torch.full((B, n), float(max_range), dtype=torch.float64))


class _Launch:
    """The arguments both entries share, resolved once: sizes and the device pointers of the constant inputs."""

    def __init__(self, geom, rays):
        self.sizes = (geom.B, geom.nb, geom.nvcap, geom.verts_max(), rays.R)
        self.kind, self.nverts = geom.kind, geom.nverts
        self.body = _lib.require_gpu_tensor(rays.body, "rays.body", torch.int32)
        self.range = _lib.require_gpu_tensor(rays.range, "rays.range", torch.float64)

    def inputs(self, radius, verts_local, p, origin, angle):
        P = _lib.ptr
        return (*self.sizes, P(self.kind), P(radius), P(verts_local), P(self.nverts), P(p), P(self.body), P(origin), P(angle),
                P(self.range))


class CastRaysFunction(torch.autograd.Function):
    """(p, radius, verts_local, origin, angle) -> dist [B,R] f64, hit [B,R] i32[, normal [B,R,2] f64]: one launch each way.  Only
    `dist` is differentiable; the backward asks the kernel only for the gradients autograd needs (NULL for the rest) and recomputes
    the hits from the saved INPUTS."""

    @staticmethod
    def forward(ctx, p, radius, verts_local, origin, angle, launch, normals):
        lib = _lib.load()
        dev = p.device
        B, R = launch.sizes[0], launch.sizes[4]
        dist = torch.empty(B, R, dtype=torch.float64, device=dev)
        hit = torch.empty(B, R, dtype=torch.int32, device=dev)
        normal = torch.empty(B, R, 2, dtype=torch.float64, device=dev) if normals else None
        with _lib.on_device(dev):
            rc = lib.lcp_cast_rays_f64(*launch.inputs(radius, verts_local, p, origin, angle), _lib.ptr(dist), _lib.ptr(hit),
                                       _lib.ptr(normal), _lib.stream_ptr(dev))
        _lib.check(rc, "lcp_cast_rays_f64")
        ctx.launch = launch
        ctx.save_for_backward(p, radius, verts_local, origin, angle)
        ctx.mark_non_differentiable(hit)
        if normals:
            ctx.mark_non_differentiable(normal)
            return dist, hit, normal
        return dist, hit

    @staticmethod
    def backward(ctx, g_dist, *_):
        saved = ctx.saved_tensors
        lib = _lib.load()
        dev = saved[0].device
        outs = [torch.empty(t.shape, dtype=t.dtype, device=dev) if need else None for t, need in zip(saved, ctx.needs_input_grad[:5])]
        if all(o is None for o in outs):
            return (None,) * 7
        p, radius, verts_local, origin, angle = saved
        g_dist = g_dist.to(torch.float64).contiguous()
        with _lib.on_device(dev):
            rc = lib.lcp_cast_rays_backward_f64(*ctx.launch.inputs(radius, verts_local, p, origin, angle), _lib.ptr(g_dist),
                                                *[_lib.ptr(o) for o in outs], _lib.stream_ptr(dev))
        _lib.check(rc, "lcp_cast_rays_backward_f64")
        return (*outs, None, None)


def cast_rays(geom, p, rays, normals=False):
    """The range readings of B scenes: `dist [B,R]` f64 (differentiable with respect to `p` [B,nb,3] f64, `geom.radius`,
    `geom.verts_local`, `rays.origin` and `rays.angle`), `hit [B,R]` int32 (the body each ray meets first, -1: none within its range)
    and, with `normals=True`, `normal [B,R,2]` f64 (the surface normal at the hit; 0 for a miss and for an origin inside a body).
    `hit` and `normal` carry no gradient."""
    _geometry(geom, p)
    if rays.B != geom.B:
        raise ValueError("rays are for %d scenes, the geometry for %d" % (rays.B, geom.B))
    _lib.require_gpu_tensor(rays.origin.detach(), "rays.origin", torch.float64)
    _lib.require_gpu_tensor(rays.angle.detach(), "rays.angle", torch.float64)
    launch = _Launch(geom, rays)
    return CastRaysFunction.apply(p, geom.radius, geom.verts_local, rays.origin, rays.angle, launch, bool(normals))
